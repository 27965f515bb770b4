/* mvs_normals_abi.h -- point normals of a fused cloud on the device, and a voxel downsample that carries them.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).  Refusals are decided on the host before the first HIP call.
 *
 * mvs_cloud_normals is the reference's pcd.estimate_normals() (eval.py:817, before the crop and the voxel filter of
 * eval.py:832-837, which carry a cloud's normals along), with Open3D's documented behaviour restated below and its
 * unspecified parts -- the sign, above all -- specified.  Open3D itself is no dependency and nothing here was compared
 * against it.
 *
 * ---- mvs_cloud_normals -------------------------------------------------------------------------------------------
 * Inputs:
 *     xyz          DEVICE, [P][3], float (MVS_CLOUD_F32) or double (MVS_CLOUD_F64)
 *     box_min, box_max  HOST, double [3]: the search box; read before the call returns
 *     cell         edge of the search grid's cells; any admissible value gives the same output bytes
 *     knn          3 <= knn <= MVS_NORMALS_KNN_MAX
 *     view_starts  DEVICE, long long [R+1]: the exclusive prefix of the per-view point counts (non-decreasing)
 *     centres      DEVICE, double [R][3]: the camera centres.  R == 0 <=> both pointers are NULL.
 * Outputs (DEVICE pointers):
 *     normals_out  float     [P][3]    every element is written
 *     nbr_out      int32     [P][knn]  or NULL; every element is written
 *     counts_out   long long [3]
 *
 * Every operation below is in IEEE double on the inputs converted to double, one operation at a time, nothing contracted.
 *
 * Members: point i is a member iff box_min[a] <= p[a] <= box_max[a] for a = 0, 1, 2, both ends inclusive.  NaN and
 *     +-inf fall out.  Only members get a normal and only members are neighbours.  M = the number of members.
 * Neighbours: the neighbours of member i are the m = min(knn, M) members j with the smallest (d2, j), compared
 *     lexicographically, d2 = (dx*dx + dy*dy) + dz*dz with d = p[j] - p[i].  Point i itself is among them (d2 = 0), as in
 *     Open3D's KD-tree query of a point of the tree; exact duplicates and lattice ties are decided by the index.  The
 *     neighbour set is exactly that of this restatement.
 * Covariance: mean[a] = (sum of the neighbours' p[a]) / m; C[a][b] = (sum of (p[a] - mean[a]) * (p[b] - mean[b])) / m;
 *     both sums run over the neighbours in ascending (d2, j), starting from 0.  (Open3D accumulates raw cumulants; the
 *     centred form loses nothing to cancellation.)
 * Normal: a unit eigenvector of the smallest eigenvalue of C, found by 8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2)
 *     in double; of equal smallest diagonal entries the lowest axis is taken.  m < 3 gives (0, 0, 1).  A C whose entries
 *     are all zero (all neighbours coincide), and a zero or non-finite eigenvector, give (0, 0, 1): all as in Open3D.
 * Sign: with R > 0 point i belongs to the view r with view_starts[r] <= i < view_starts[r+1], and its normal n is
 *     negated iff (n[0]*c[0] + n[1]*c[1]) + n[2]*c[2] < 0 with c = centres[r] - p: Open3D's
 *     orient_normals_towards_camera_location, per view.  A point in no view's range, and every point when R == 0, takes
 *     the sign that makes its component of largest magnitude positive (the lowest axis wins ties).  The (0, 0, 1) of the
 *     degenerate cases is signed by the same rules.
 * Outputs: normals_out[i] = float32(n), (0, 0, 0) for a non-member.  nbr_out[i], if given: the m neighbour indices in
 *     ascending (d2, j), then -1 up to knn; all -1 for a non-member.
 *     counts_out[0] = M.
 *     counts_out[1] = the members with an estimated normal: those with m >= 3, i.e. M if M >= 3, else 0.
 *     counts_out[2] = the members that a point outside the box could have served better: m < knn, or
 *         d2 of the last neighbour > f*f, f = the smallest of p[a] - box_min[a] and box_max[a] - p[a] over the axes.  They
 *         are still computed from members only; a caller who wants the whole cloud's answer grows the box until this is 0.
 * Determinism: the neighbour sets are exact and every sum has a fixed order, so the same inputs give the same bytes on
 *     every run, on every stream and for every admissible `cell`.  No floating-point value is added atomically.
 *
 * Search grid: n[a] = floor((box_max[a] - box_min[a]) / cell) + 1 cells per axis, the cell of a member is
 *     floor((p[a] - box_min[a]) / cell) (rounding is monotonic, so it is at most n[a] - 1), linear index
 *     (iz * n[1] + iy) * n[0] + ix.  Launches, ordered by the stream alone: (1) counts_out and the cell counters are
 *     zeroed; (2) one thread per point: non-members get their zeros and -1s, members count themselves into their cell with
 *     integer atomics; (3) three launches turn the cell counts into exclusive offsets (tile sums of MVS_NORMALS_TILE
 *     cells, one block scanning the sums with a running carry, tiles scanned in place); (4) one thread per member
 *     claims a slot of its cell's range and writes its index and its point there -- the order inside a cell is whatever
 *     the atomics gave and does not matter; (5) one wave per member searches Chebyshev rings of cells around the member's
 *     own, keeping the best 64 candidates sorted by (d2, j) one per lane, until the knn-th is nearer than the nearest
 *     face of the examined block of cells less cell / 1000 (which covers the rounding of the cell index many times over),
 *     or the grid is exhausted; then mean, covariance, eigenvector, sign and counts.  The grid of (5) is capped at 2^24 - 1
 *     blocks of 32 members (a HIP launch has fewer than 2^32 threads) and the kernel loops over the rest, so every
 *     P < 2^31 launches.
 *
 * Workspace, with cells = n[0] * n[1] * n[2]:
 *     mvs_query_normals_workspace = 24 * P + 8 * ceil(P / 2) + 8 * ceil(cells / 2)
 *                                   + 8 * ceil((ceil(cells / MVS_NORMALS_TILE) + 1) / 2) bytes, 8-byte aligned.
 *
 * Refusals: a NULL required pointer (nbr_out may be NULL; view_starts and centres must be NULL iff R == 0) ->
 * MVS_ERR_NULL; P < 0, P >= 2^31, R < 0, knn outside [3, MVS_NORMALS_KNN_MAX], a cell that is not finite or <= 0, a box
 * bound that is not finite, box_min[a] > box_max[a], or cells >= 2^31 -> MVS_ERR_BAD_SHAPE; an xyz_dtype other than the
 * two -> MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE.  P == 0 is legal
 * and gives three zero counts.
 *
 * ---- mvs_cloud_downsample_normals --------------------------------------------------------------------------------
 * mvs_cloud_downsample (mvs_cloud_abi.h) with two more arguments: normals, DEVICE float [P][3], and normals_out, DEVICE
 * float [capacity][3].  xyz_out, rgb_out and counts_out are byte for byte what mvs_cloud_downsample gives on the same
 * inputs, with the same order, capacity rules and refusals (normals must not be NULL; normals_out may be NULL only when
 * capacity is 0).  normals_out[j] = float32((sum / count) * 2^-30) in double, where sum[a] adds, per point of the voxel,
 * rint(clamp(n[a], -1, 1) * 2^30) (ties to even; NaN counts as 0) with 64-bit integer atomics: the mean of the voxel's
 * normals to within 2^-31, independent of the order of the points, and below 2^31 points the sum cannot overflow.  The
 * mean is not renormalised (Open3D: "call NormalizeNormals afterwards if necessary").
 * Workspace: mvs_query_cloud_normals_downsample_workspace = mvs_query_cloud_workspace + 24 * cells of THAT grid
 * (mvs_cloud_abi.h: n[a] = floor((box_max[a] - box_min[a]) / voxel_size + 0.5) + 2), 8-byte aligned. */
#ifndef MVS_NORMALS_ABI_H
#define MVS_NORMALS_ABI_H

#include "mvs_abi.h"
#include "mvs_cloud_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_NORMALS_KNN_MAX 64  /* one candidate per lane of a wave */
#define MVS_NORMALS_TILE 1024   /* cells one block sums / scans */

int mvs_query_normals_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes);
int mvs_cloud_normals(const void* xyz, int xyz_dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, long long P,
                      const double box_min[3], const double box_max[3], double cell, int knn,
                      const long long* view_starts /* [R+1] */, const double* centres /* [R][3] */, int R,
                      float* normals_out, int* nbr_out, long long* counts_out /* [3] */, void* workspace,
                      size_t workspace_bytes, void* stream);

int mvs_query_cloud_normals_downsample_workspace(long long P, const double box_min[3], const double box_max[3],
                                                 double voxel_size, size_t* bytes);
int mvs_cloud_downsample_normals(const void* xyz, int xyz_dtype, const unsigned char* rgb, const float* normals, long long P,
                                 const double box_min[3], const double box_max[3], double voxel_size, double scale,
                                 long long capacity, float* xyz_out, unsigned char* rgb_out, float* normals_out,
                                 long long* counts_out /* [2] */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_NORMALS_ABI_H */
