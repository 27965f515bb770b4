/* mvs_distance_abi.h -- the distance from every point of one cloud to the nearest point of another, on the device.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).  Refusals are decided on the host before the first HIP call.
 *
 * mvs_cloud_distance is one direction of the measure every MVSNet is judged by: with the reconstruction as the query and
 * the ground truth as the reference it gives the accuracy, the other way round the completeness; precision, recall and
 * the F-score at a threshold follow from the counts.  The reference project leaves this to DTU's MATLAB code; the
 * definition below is that code's nearest-neighbour distance alone.  DTU's observability mask, its ground-plane filter
 * and its point reduction (reducePts) are not part of it: they are mvs_cloud_select and mvs_cloud_reduce
 * (mvs_reduce_abi.h), which turn the filtered-out queries into the NaN rows this entry point leaves uncounted;
 * nothing here was compared against the MATLAB code or real DTU files.
 *
 * Inputs:
 *     ref_xyz       DEVICE, [P][3], float (MVS_CLOUD_F32) or double (MVS_CLOUD_F64): the cloud that is searched
 *     query_xyz     DEVICE, [N][3], float or double: the points whose distances are wanted.  It may alias ref_xyz.
 *     box_min, box_max  HOST, double [3]: the box of the reference cloud; read before the call returns
 *     cell          edge of the search grid's cells; any admissible value gives the same output bytes
 *     max_dist      >= 0, may be +inf: a nearest point farther than this counts as none
 *     thresholds    HOST, double [T], 0 <= T <= MVS_DISTANCE_THRESHOLDS_MAX, each finite and >= 0; read before the call
 *                   returns; may be NULL when T == 0
 * Outputs (DEVICE pointers):
 *     dist_out      double    [N]      every element is written
 *     idx_out       int       [N]      or NULL; every element is written
 *     counts_out    long long [2 + T]  n_counted, n_within, below[0 .. T-1]
 *     stats_out     double    [2]      S(x), mean
 * Both inputs are only read.
 *
 * Every operation below is in IEEE double on the inputs converted to double, one operation at a time, nothing contracted.
 *
 * Members: exactly the members of mvs_cloud_normals (mvs_normals_abi.h): reference point j is a member iff
 *     box_min[a] <= r[j][a] <= box_max[a] for a = 0, 1, 2, both ends inclusive.  NaN and +-inf fall out.  M = the number
 *     of members.  A reference point outside the box is never found, however near it lies.
 * Counted queries: query i is counted iff its three coordinates are finite.  It may lie anywhere, inside or outside the
 *     box.  A query that is not counted gets dist_out[i] = -1.0 and idx_out[i] = -1 (the marker of mvs_cloud_outliers).
 * Nearest: for a counted query, d2(j) = (dx*dx + dy*dy) + dz*dz with d = r[j] - q[i].  The nearest is the member with
 *     the smallest (d2, j), compared lexicographically, among the members whose d2 is finite (a d2 that overflowed is no
 *     distance).  If there is none (M == 0), or its d2 > max_dist * max_dist (one product), then dist_out[i] = +inf and
 *     idx_out[i] = -1.  Otherwise dist_out[i] = sqrt(d2), correctly rounded, idx_out[i] = j, and the query is WITHIN.
 *     A d2 equal to the product is within; max_dist == 0 leaves the coincident points only.
 * Counts: counts_out[0] = n_counted, counts_out[1] = n_within, counts_out[2 + t] = the number of within queries with
 *     dist_out[i] < thresholds[t], strictly.
 * Statistics: x[i] = dist_out[i] if query i is within, else +0.0, for i = 0 .. N-1 in query-index order.  S(x) is the
 *     balanced pairwise sum of mvs_outliers_abi.h, over the same tree of MVS_OUTLIERS_BLOCK-element blocks.
 *     stats_out[0] = S(x), stats_out[1] = S(x) / n_within, or 0 when n_within == 0.
 * Empty inputs: N == 0 and P == 0 are legal.  With N == 0 all counts and both statistics are zero; with P == 0 every
 *     counted query gets +inf, so n_within, the below counts and both statistics are zero.  ref_xyz is not read when
 *     P == 0, nor query_xyz, dist_out and idx_out when N == 0; they must still not be NULL.
 * Determinism: the nearest member is exact and the sum has a fixed order, so the same inputs give the same bytes on every
 *     run, on every stream and for every admissible `cell`.  No floating-point value is added atomically; integer atomics
 *     serve the counts and the cell bookkeeping only.
 *
 * Launches, ordered by the stream alone (no block waits for another): the search grid of mvs_cloud_normals over the box
 *     and the reference cloud; one wave per query walks the rings of cells around the query's cell -- the cell nearest to
 *     it when it lies outside the box -- each lane keeping the best of the candidates it loads, one ballot per ring and one
 *     minimum over the wave at the end, until no unexamined cell can hold a nearer member or one within max_dist; a query
 *     farther than max_dist from the box is answered without reading a cell (the grid of this launch is capped at 2^24 - 1
 *     blocks of 32 queries, a HIP launch having fewer than 2^32 threads, and the kernel loops over the rest); one thread per query counts, with one ballot
 *     and one integer atomic per wave and count; S(x) as in mvs_cloud_outliers; a one-thread kernel forms the mean.
 *
 * Workspace: mvs_query_distance_workspace = mvs_query_normals_workspace(P, box_min, box_max, cell)
 *                                           + 8 * (L_1 + L_2 + ... ) + MVS_DISTANCE_SCALARS bytes, 8-byte aligned,
 *     with L_0 = N and L_{k+1} = ceil(L_k / MVS_OUTLIERS_BLOCK) down to the first L_k == 1 (nothing for N <= 1), as in
 *     mvs_outliers_abi.h but over the queries.
 *
 * Refusals: a NULL ref_xyz, query_xyz, box_min, box_max, dist_out, counts_out, stats_out or workspace, or a NULL
 * thresholds with T > 0 (idx_out may be NULL) -> MVS_ERR_NULL; P or N outside [0, 2^31), T outside
 * [0, MVS_DISTANCE_THRESHOLDS_MAX], a max_dist or a threshold that is NaN or negative, a threshold that is not finite, a
 * cell that is not finite or <= 0, a box bound that is not finite, box_min[a] > box_max[a], or 2^31 cells or more
 * (n[a] = floor((box_max[a] - box_min[a]) / cell) + 1 per axis) -> MVS_ERR_BAD_SHAPE; a dtype other than the two ->
 * MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE. */
#ifndef MVS_DISTANCE_ABI_H
#define MVS_DISTANCE_ABI_H

#include "mvs_abi.h"
#include "mvs_cloud_abi.h"
#include "mvs_normals_abi.h"
#include "mvs_outliers_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_DISTANCE_THRESHOLDS_MAX 8   /* the most thresholds one call counts */
#define MVS_DISTANCE_SCALARS 64         /* bytes of the scalar block */

int mvs_query_distance_workspace(long long P, long long N, const double box_min[3], const double box_max[3], double cell,
                                 size_t* bytes);
int mvs_cloud_distance(const void* ref_xyz, int ref_dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, long long P,
                       const void* query_xyz, int query_dtype, long long N,
                       const double box_min[3], const double box_max[3], double cell,
                       double max_dist, const double* thresholds /* HOST [T] */, int T,
                       double* dist_out /* [N] */, int* idx_out /* [N] or NULL */,
                       long long* counts_out /* [2 + T] */, double* stats_out /* [2] */,
                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_DISTANCE_ABI_H */
