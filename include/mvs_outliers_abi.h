/* mvs_outliers_abi.h -- statistical outlier removal on a fused cloud, on the device.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).  Refusals are decided on the host before the first HIP call.
 *
 * mvs_cloud_outliers is the reference's pcd.remove_statistical_outlier(nb_neighbors=20, std_ratio=2.0) (eval.py:495,
 * between the crop and the voxel filter; the reference drops the call's result, so the cloud it shows is unfiltered -- the
 * intent is plain).  Open3D's RemoveStatisticalOutliers is restated below: the mean distance to the nb_neighbors nearest
 * points (the point itself among them), the mean and the sample standard deviation of those over the valid points, a
 * point kept iff its mean distance is below mean + std_ratio * std.  What Open3D leaves to its implementation -- the order
 * of ties, the order of every sum, the cases of fewer than two valid points -- is specified here.  Open3D itself is no
 * dependency and nothing here was compared against it.
 *
 * Inputs:
 *     xyz           DEVICE, [P][3], float (MVS_CLOUD_F32) or double (MVS_CLOUD_F64)
 *     box_min, box_max  HOST, double [3]: the crop box; read before the call returns
 *     cell          edge of the search grid's cells; any admissible value gives the same output bytes
 *     nb_neighbors  2 <= nb_neighbors <= MVS_NORMALS_KNN_MAX
 *     std_ratio     finite, > 0
 * Outputs (DEVICE pointers):
 *     dist_out        double        [P]     every element is written
 *     keep_out        unsigned char [P]     every element is written, 0 or 1
 *     xyz_masked_out  [P][3] of xyz's dtype, or NULL; every element is written.  It must not alias xyz.
 *     counts_out      long long     [3]     M, n_valid, kept
 *     stats_out       double        [3]     mean, std, threshold
 *
 * Every operation below is in IEEE double on the inputs converted to double, one operation at a time, nothing contracted.
 *
 * Members: exactly the members of mvs_cloud_normals (mvs_normals_abi.h): point i is a member iff
 *     box_min[a] <= p[a] <= box_max[a] for a = 0, 1, 2, both ends inclusive.  NaN and +-inf fall out.  The box is the crop
 *     (the reference crops first), so only members are neighbours.  M = the number of members.
 * Neighbours: those of mvs_cloud_normals with knn = nb_neighbors: the m = min(nb_neighbors, M) members j with the
 *     smallest (d2, j), compared lexicographically, d2 = (dx*dx + dy*dy) + dz*dz with d = p[j] - p[i].  Point i itself is
 *     among them (d2 = 0), as in Open3D's KD-tree query of a point of the tree.
 * Mean distance: dist[i] = (sum of sqrt(d2) over the neighbours in ascending (d2, j), starting from 0.0) / m, sqrt
 *     correctly rounded.  dist_out[i] = dist[i], and -1.0 for a non-member (Open3D's marker).
 * Valid points: point i is valid iff it is a member and dist[i] > 0.  A member whose neighbours all coincide with it is
 *     not valid and is never kept, as in Open3D.  n_valid = their number.
 * Sums: x[i] = dist[i] if i is valid, else +0.0, for i = 0 .. P-1 in point-index order: the sums depend neither on `cell`
 *     nor on the order inside a grid cell.  S(x) is the balanced pairwise sum: pad x with +0.0 to a power of two, then,
 *     level by level from bit 0 upward, add the elements whose indices differ in that bit (x[2k] + x[2k+1], and so on).
 *     Adding +0.0 to a non-negative value is exact and floating-point addition commutes, so any split into aligned
 *     power-of-two blocks, with an xor butterfly inside a wave, gives these bits.
 * Statistics: mean = S(x) / n_valid.  y[i] = (x[i] - mean) * (x[i] - mean) if i is valid, else +0.0.
 *     std = sqrt(S(y) / (n_valid - 1)).  threshold = mean + std_ratio * std: a product, then a sum.
 *     n_valid == 0 gives mean = std = threshold = 0; n_valid == 1 gives std = 0 (so threshold = mean, and nothing is kept).
 * Keep: keep_out[i] = 1 iff i is valid and dist[i] < threshold, else 0.
 * Masked points: xyz_masked_out[i], if given, holds the three input values bit for bit where keep_out[i] is 1, and three
 *     canonical quiet NaNs (0x7FC00000 / 0x7FF8000000000000) elsewhere.  NaN points fall out of mvs_cloud_downsample,
 *     mvs_cloud_downsample_normals and mvs_cloud_normals by their own definitions, so the filtered cloud feeds them with P,
 *     the colours and the normals unchanged.
 * counts_out = M, n_valid, kept (the number of ones in keep_out); stats_out = mean, std, threshold.
 * P == 0 is legal: the three counts and the three statistics are zero.
 * Determinism: the neighbour sets are exact and every sum has a fixed order, so the same inputs give the same bytes on
 *     every run, on every stream and for every admissible `cell`.  No floating-point value is added atomically; integer
 *     atomics serve the counts and the cell bookkeeping only.
 *
 * Launches, ordered by the stream alone (no block waits for another): the search grid of mvs_cloud_normals over the box,
 *     its classify pass writing -1.0, 0 and the NaNs for non-members; one wave per member runs the same ring search and
 *     sums the m square roots in order (that grid is capped at 2^24 - 1 blocks and the kernel loops, as in
 *     mvs_cloud_normals); S(x) by blocks of MVS_OUTLIERS_BLOCK consecutive elements, the kernel relaunched on
 *     the partial sums until one is left (at most four launches below 2^31 points); a one-thread kernel forms the mean;
 *     S(y) likewise, y formed on load; a one-thread kernel forms std and threshold and writes stats_out; one thread per
 *     point marks.
 *
 * Workspace: mvs_query_outliers_workspace = mvs_query_normals_workspace(P, box_min, box_max, cell)
 *                                           + 8 * (L_1 + L_2 + ... ) + MVS_OUTLIERS_SCALARS bytes, 8-byte aligned,
 *     with L_0 = P and L_{k+1} = ceil(L_k / MVS_OUTLIERS_BLOCK) down to the first L_k == 1 (nothing for P <= 1): the
 *     partial sums of every level of the tree, and a fixed block for the scalars between the passes.
 *
 * Refusals: a NULL xyz, box_min, box_max, dist_out, keep_out, counts_out, stats_out or workspace (xyz_masked_out may be
 * NULL) -> MVS_ERR_NULL; P < 0, P >= 2^31, nb_neighbors outside [2, MVS_NORMALS_KNN_MAX], a std_ratio that is not finite
 * or <= 0, a cell that is not finite or <= 0, a box bound that is not finite, box_min[a] > box_max[a], or 2^31 cells or
 * more (n[a] = floor((box_max[a] - box_min[a]) / cell) + 1 per axis) -> MVS_ERR_BAD_SHAPE; an xyz_dtype other than the
 * two -> MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE. */
#ifndef MVS_OUTLIERS_ABI_H
#define MVS_OUTLIERS_ABI_H

#include "mvs_abi.h"
#include "mvs_cloud_abi.h"
#include "mvs_normals_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_OUTLIERS_BLOCK 1024   /* consecutive elements one block of the tree sums */
#define MVS_OUTLIERS_SCALARS 64   /* bytes of the scalar block */

int mvs_query_outliers_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes);
int mvs_cloud_outliers(const void* xyz, int xyz_dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, long long P,
                       const double box_min[3], const double box_max[3], double cell, int nb_neighbors, double std_ratio,
                       double* dist_out, unsigned char* keep_out, void* xyz_masked_out, long long* counts_out /* [3] */,
                       double* stats_out /* [3] */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_OUTLIERS_ABI_H */
