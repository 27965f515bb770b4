/* mvs_cloud_abi.h -- cropping a fused point cloud to a box and voxel-downsampling it on the device.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).
 *
 * mvs_cloud_downsample is the last step of the reference's eval path for the bin-picking datasets (eval.py:831-840):
 *
 *     pcd = pcd.crop(bbox2)                                   eval.py:832   (bbox2: get_o3d_frame_bbox, eval.py:159-217)
 *     pcd = pcd.voxel_down_sample(voxel_size=dwn_smpl)        eval.py:837
 *     pcd.scale(0.01, (0,0,0))                                eval.py:839
 *
 * with Open3D's documented behaviour restated below; Open3D itself is no dependency.
 *
 * Inputs:
 *     xyz        DEVICE, [P][3], float (MVS_CLOUD_F32: what mvs_fuse_points writes) or double (MVS_CLOUD_F64: what the
 *                reference hands Open3D)
 *     rgb        DEVICE, uint8 [P][3]
 *     box_min, box_max  HOST, double [3]; read before the call returns
 * Outputs (DEVICE pointers):
 *     xyz_out    float     [capacity][3]
 *     rgb_out    uint8     [capacity][3]
 *     counts_out long long [2]          kept (in-box) points, occupied voxels
 *
 * Crop: point i is kept iff box_min[a] <= p[a] <= box_max[a] for a = 0, 1, 2, both ends inclusive, compared on the input
 *     value converted to double.  NaN and +-inf therefore fall out.
 * Grid: m[a] = the minimum of the kept points' coordinate a (so the grid depends on the data, as Open3D's does);
 *     vmin = m - 0.5 * voxel_size; idx[a] = floor((p[a] - vmin[a]) / voxel_size), every operation in IEEE double,
 *     nothing contracted.  The assignment of points to voxels is exactly that of this fp64 restatement.
 * Grid size: n[a] = floor((box_max[a] - box_min[a]) / voxel_size + 0.5) + 2.  Since m >= box_min, the largest index is
 *     at most n[a] - 2; the spare plane absorbs a rounding of the quotient at the very top.  No index is ever clamped.
 * Output: one point per occupied voxel, in ascending (iz, iy, ix), i.e. ascending (iz * n[1] + iy) * n[0] + ix.
 *     Open3D's own order is that of a hash map and unspecified: this order is this library's.
 * Coordinates: float32(mean * scale), mean = the arithmetic mean of the voxel's points.  The mean is accumulated in
 *     integers -- per point and axis round(((p - corner) / voxel_size) * 2^32), corner = vmin + idx * voxel_size, added
 *     with 64-bit integer atomics -- so it does not depend on the order the points arrive in: the same inputs give the
 *     same bytes on every run and every stream.  mean = corner + (sum / count) * voxel_size * 2^-32 in double.  Against
 *     the exact mean that is off by at most voxel_size * 2^-33 (the fixed-point step) plus a few roundings of 2^-53.
 * Colour: per channel (2 * sum + count) / (2 * count) in integers: the mean of the bytes rounded half up, exact for
 *     any count below 2^31.
 * Counts: both are always exact, whatever the capacity.
 * Capacity: as in mvs_fuse_points.  The first `capacity` voxels, in order, are written; no element of xyz_out / rgb_out
 *     at or beyond `capacity` is touched, nor any between the number of voxels and `capacity`.  xyz_out / rgb_out may be
 *     NULL only when capacity is 0.  With no kept point both counts are 0 and nothing else is written.
 *
 * Launches, ordered by the stream alone: (1) every block takes the per-axis minimum and the number of its
 * MVS_CLOUD_CHUNK points that lie in the box; (2) one block merges those partial results into vmin and counts_out[0];
 * (3) the grid is zeroed; (4) every kept point adds itself to its voxel's record (a 32-bit count, three 64-bit byte
 * sums, three 64-bit fixed-point sums) with integer atomics; (5) every block counts the occupied voxels of one tile of
 * MVS_CLOUD_TILE consecutive voxels; (6) one block of MVS_CLOUD_SCAN_WIDTH threads turns the tile counts into exclusive
 * offsets, with a running carry, and writes counts_out[1]; (7) every block ranks the occupied voxels of its tile and
 * writes them.  No block waits for another and no floating-point value is ever added atomically.
 *
 * Workspace, with cells = n[0] * n[1] * n[2]:
 *     mvs_query_cloud_workspace = 64 + MVS_CLOUD_RECORD * cells + 32 * ceil(P / MVS_CLOUD_CHUNK)
 *                                 + 8 * ceil((ceil(cells / MVS_CLOUD_TILE) + 1) / 2) bytes, 8-byte aligned.
 *
 * Refusals (decided before the first HIP call; nothing is enqueued): a NULL pointer -> MVS_ERR_NULL; P < 0, P >= 2^31,
 * capacity < 0, a voxel_size that is not finite or <= 0, a scale that is not finite, a box bound that is not finite,
 * box_min[a] > box_max[a], or cells >= 2^31 -> MVS_ERR_BAD_SHAPE; an xyz_dtype other than the two above ->
 * MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE.  P == 0 is legal and
 * gives two zero counts.
 *
 * A cloud without a bounding box would need a sort- or hash-based grid and is not served: a caller without a bin passes
 * the bounds it wants kept. */
#ifndef MVS_CLOUD_ABI_H
#define MVS_CLOUD_ABI_H

#include "mvs_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_CLOUD_F32 0 /* xyz is float  [P][3] */
#define MVS_CLOUD_F64 1 /* xyz is double [P][3] */

#define MVS_CLOUD_CHUNK 1024      /* points one block of the crop + minimum pass covers */
#define MVS_CLOUD_TILE 1024       /* voxels one block counts / emits */
#define MVS_CLOUD_SCAN_WIDTH 1024 /* tile counts the scan kernel covers in one pass */
#define MVS_CLOUD_RECORD 64       /* bytes of one voxel's record in the workspace */

int mvs_query_cloud_workspace(long long P, const double box_min[3], const double box_max[3], double voxel_size, size_t* bytes);
int mvs_cloud_downsample(const void* xyz, int xyz_dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, const unsigned char* rgb,
                         long long P, const double box_min[3], const double box_max[3], double voxel_size, double scale,
                         long long capacity, float* xyz_out, unsigned char* rgb_out, long long* counts_out /* [2] */,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_CLOUD_ABI_H */
