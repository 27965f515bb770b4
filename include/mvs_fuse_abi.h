/* mvs_fuse_abi.h -- fusing the filtered depth maps of a scan into one coloured point cloud on the device.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, mvs_image_format, the common rules --
 * caller-owned device memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).
 *
 * mvs_fuse_points is the last step of the reference's filter_depth (eval.py:745-758): of every reference view r it keeps
 * the pixels whose final mask is set, in order, with the colour of the view's image:
 *
 *     vertexs.append(xyz_world[r][final[r].reshape(-1)])                       eval.py:753
 *     vertex_colors.append((ref_img[1::4, 1::4, :][final[r]] * 255).astype(np.uint8))   eval.py:755-759
 *     np.concatenate(vertexs), np.concatenate(vertex_colors)                   eval.py:757-758
 *
 * Inputs (DEVICE pointers):
 *     xyz_world  double [R][h*w][3]  as mvs_filter_depth writes it
 *     masks      uint8  [R][3][h][w] as mvs_filter_depth writes it; plane 2 (final) selects, any byte != 0
 *     images     uint8, MVS_IMG_U8_HWC [V][4h][4w][3] or MVS_IMG_U8_CHW [V][3][4h][4w]: the decoded pixels
 *     ref_idx    int32  [R]          image of reference view r
 * Outputs (DEVICE pointers):
 *     xyz_out    float  [capacity][3]
 *     rgb_out    uint8  [capacity][3]
 *     counts_out int32  [R+1]        points of each view, then the total
 *
 * Order: view-major in r, row-major in the pixel index within a view, i.e. exactly
 *     np.concatenate([xyz_world[r][final[r].reshape(-1)] for r in range(R)]).
 * Coordinates: the float64 coordinate converted to float32 with round-to-nearest-even, which is what numpy stores when
 *     the reference's PLY writer assigns into its '<f4' fields.  Infinities stay; a NaN stays a NaN, its payload is
 *     NOT specified.
 * Colour: pixel (y, x) of view r takes image ref_idx[r] at (4y+1, 4x+1), i.e. img[1::4, 1::4].  The reference computes
 *     uint8(float32(u) / 255 * 255) with truncation, which is the identity on all 256 values of u
 *     (tests/test_scan_fusion_host.py pins that), so the bytes are copied.
 * Counts: counts_out is always exact, whatever the capacity.
 * Capacity: if the total exceeds `capacity`, the first `capacity` points are written, in order, and no element of
 *     xyz_out / rgb_out at or beyond `capacity` is touched.  Elements between the total and `capacity` are not written
 *     either.  xyz_out / rgb_out may be NULL only when capacity is 0.
 * Out-of-range views: a ref_idx[r] outside [0, V) contributes no point and counts_out[r] = 0; nothing is read for it.
 *
 * Three launches, ordered by the stream alone: (1) every block counts the selected pixels of one tile of
 * MVS_FUSE_TILE consecutive pixels of one view (wave ballot + popcount); (2) one block of MVS_FUSE_SCAN_WIDTH
 * threads turns the tile counts into exclusive offsets, MVS_FUSE_SCAN_WIDTH tiles per pass with a running carry, and
 * writes counts_out; (3) every block ranks the selected pixels of its tile and writes them.  No block waits for
 * another and there are no atomics: the same inputs give the same bytes on every run and every stream.  The grids of (1)
 * and (3) are capped at 2^24 - 1 blocks (a HIP launch has fewer than 2^32 threads) and a block takes every 2^24 - 1-th
 * tile, so any R*h*w < 2^31 launches; below 2^24 tiles that is one tile per block.
 *
 * Workspace: mvs_query_fuse_workspace(R, h, w) = 4 * (R * ceil(h*w / MVS_FUSE_TILE) + 1) bytes, 4-byte aligned.
 *
 * Refusals (nothing is enqueued): a NULL pointer -> MVS_ERR_NULL; R, h, w or V < 1, R*h*w >= 2^31 or capacity < 0 ->
 * MVS_ERR_BAD_SHAPE; an image format other than the two uint8 ones -> MVS_ERR_BAD_DTYPE; a workspace that is too
 * small or not 4-byte aligned -> MVS_ERR_WORKSPACE. */
#ifndef MVS_FUSE_ABI_H
#define MVS_FUSE_ABI_H

#include "mvs_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_FUSE_TILE 1024        /* pixels of one view that one block counts / scatters */
#define MVS_FUSE_SCAN_WIDTH 1024  /* tile counts the scan kernel covers in one pass */

int mvs_query_fuse_workspace(int R, int h, int w, size_t* bytes);
int mvs_fuse_points(const double* xyz_world, const unsigned char* masks, const void* images, int image_format,
                    const int* ref_idx, int V, int R, int h, int w, long long capacity, float* xyz_out,
                    unsigned char* rgb_out, int* counts_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_FUSE_ABI_H */
