/* ext/mvs_register_abi.h -- the rigid registration of one cloud onto another (ICP), on the device.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).  Refusals are decided on the host before the first HIP call.
 * The header lives in include/ext/ until the contract tables of the test suite can be extended; then it moves to include/.
 *
 * mvs_cloud_register moves the SOURCE cloud onto the TARGET cloud: it iterates "find the nearest target point of every
 * transformed source point, then take the rigid motion that brings these pairs closest", with the semantics of Open3D's
 * registration_icp (point-to-point and point-to-plane estimation, its fitness, its inlier_rmse and its convergence
 * test).  Nothing here was compared against Open3D itself.
 *
 * Inputs:
 *     target_xyz      DEVICE, [P][3], float (MVS_CLOUD_F32) or double (MVS_CLOUD_F64): the fixed cloud, searched
 *     target_normals  DEVICE, [P][3] of target_dtype, or NULL.  With normals the step is point-to-plane, without
 *                     point-to-point.  Their sign does not matter (they enter as n * n products only); their length does.
 *     source_xyz      DEVICE, [N][3], float or double: the cloud that is moved.  It may alias target_xyz.
 *     box_min, box_max  HOST, double [3]: the box of the target cloud; read before the call returns
 *     cell            edge of the search grid's cells; any admissible value gives the same output bytes
 *     max_dist        >= 0, may be +inf: a nearest point farther than this is no correspondence
 *     init            HOST, double [16], row-major 4 x 4, or NULL = identity; read before the call returns.  Its last row
 *                     must be 0 0 0 1; its upper 3 x 3 block is taken as it is (nobody checks that it is a rotation)
 *     max_iterations  0 <= max_iterations <= MVS_REGISTER_ITERATIONS_MAX
 *     rel_fitness, rel_rmse   >= 0: the convergence criteria.  ABSOLUTE differences, as in Open3D despite the names
 * Outputs (DEVICE pointers):
 *     transform_out   double    [16]   row-major T: x -> R x + t maps the source onto the target
 *     counts_out      long long [4]    n_counted, n_inliers, iterations run, stop reason (MVS_REGISTER_STOP_*)
 *     stats_out       double    [2]    fitness, inlier_rmse -- of Evaluate(transform_out)
 *     history_out     double    [max_iterations + 1][MVS_REGISTER_HISTORY] or NULL: row k = T_k (16), fitness_k, rmse_k,
 *                     n_inliers_k.  Rows after the last evaluation are filled with bytes 0xFF (a NaN)
 *     system_out      double    [max_iterations][MVS_REGISTER_TERMS] or NULL: row k = the reduced sums step k solved from.
 *                     Rows of steps that were not taken are filled with bytes 0xFF
 *     idx_out         int       [N] or NULL: the correspondences of the last evaluation, -1 where there is none
 * All inputs are only read.
 *
 * Every operation below is in IEEE double on the inputs converted to double, one operation at a time, nothing contracted
 * (sin, cos and sqrt are the device library's).
 *
 * Members: exactly the members of mvs_cloud_normals / mvs_cloud_distance: target point j is a member iff
 *     box_min[a] <= q[j][a] <= box_max[a] for a = 0, 1, 2, both ends inclusive.
 * Counted sources: source i is counted iff its three coordinates are finite.  NaN rows, such as mvs_cloud_select writes,
 *     drop out: this is how one cluster of a cloud is registered.
 *
 * Evaluate(T), T = [R t; 0 0 0 1]: for each counted source p,
 *     s[a] = ((R[a][0]*p[0] + R[a][1]*p[1]) + R[a][2]*p[2]) + t[a]
 *     its correspondence is the nearest member of s by mvs_distance_abi.h's rule: d2(j) = (dx*dx + dy*dy) + dz*dz with
 *     d = q[j] - s, the smallest (d2, j) lexicographically among the finite d2, kept iff d2 <= max_dist * max_dist (one
 *     product).  An s that is not finite has no correspondence.  A source with a correspondence is an INLIER.
 *     Per source a vector of MVS_REGISTER_TERMS terms, all +0.0 unless stated:
 *         term 0 = 1.0 if counted; term 1 = 1.0 if inlier; term 2 = d2 if inlier; for an inlier further
 *         point-to-point, with o[a] = 0.5 * (box_min[a] + box_max[a]), s' = s - o, q' = q[j] - o:
 *             terms 3..5 = s'; 6..8 = q'; 9 + 3*a + b = s'[a] * q'[b]
 *         point-to-plane, with n = the normal of q[j], only if its three components are finite:
 *             e = s - q[j];  r = (e[0]*n[0] + e[1]*n[1]) + e[2]*n[2]
 *             J = (s[1]*n[2] - s[2]*n[1],  s[2]*n[0] - s[0]*n[2],  s[0]*n[1] - s[1]*n[0],  n[0], n[1], n[2])
 *             terms 3..23 = J[a] * J[b] for a <= b, row by row (a = 0: b = 0..5, then a = 1: b = 1..5, ...);
 *             24..29 = J[a] * r;  30 = r * r
 *     Each term is summed over i = 0 .. N-1 in source order by the balanced pairwise sum below.
 *     n_counted = sum 0, n_inliers = sum 1 (sums of ones are exact), fitness = n_inliers / n_counted (0 if none),
 *     inlier_rmse = sqrt(sum 2 / n_inliers) (0 if none).
 * The sum of a term: level 0 sums each MVS_REGISTER_GROUP consecutive sources, every later level each
 *     MVS_REGISTER_FANIN consecutive partial sums, until one is left; past the end +0.0.  Within a group an xor butterfly
 *     in index order, bit 0 first: v[i] + v[i ^ 1], then ^ 2, ... (the pairing of mvs_outliers_abi.h's S).
 *
 * The loop, from T_0 = init, for k = 0, 1, ...: Evaluate(T_k), history row k, then the first that applies:
 *     k > 0 and |fitness_k - fitness_{k-1}| < rel_fitness and |rmse_k - rmse_{k-1}| < rel_rmse -> MVS_REGISTER_STOP_CONVERGED
 *     k == max_iterations                                            -> MVS_REGISTER_STOP_MAX_ITERATIONS
 *     step k (below) is degenerate                                   -> MVS_REGISTER_STOP_DEGENERATE
 *     else system row k, T_{k+1} = dT * T_k (the 4 x 4 product, c[i][j] = ((a[i][0]*b[0][j] + a[i][1]*b[1][j]) +
 *     a[i][2]*b[2][j]) + a[i][3]*b[3][j] for i < 3; the last row is 0 0 0 1).
 *     At the stop transform_out = T_k, stats_out = (fitness_k, rmse_k), counts_out = (n_counted, n_inliers_k, k, reason).
 *     max_iterations == 0 evaluates init only.
 * Step k, point-to-plane: A = the symmetric 6 x 6 matrix of terms 3..23, b = terms 24..29; A x = -b is solved by LDL^T
 *     without pivoting (csrc/cloud_register_solve.h: d[j] = A[j][j] - sum_{m<j} L[j][m]^2 d[m], ...); x = (alpha, beta,
 *     gamma, t).  dT is Open3D's TransformVector6dToMatrix4d: rotation Rz(gamma) Ry(beta) Rx(alpha), translation t.
 *     Degenerate: n_inliers < 6, a sum that is not finite, a pivot d[j] that is not > 0 or not finite, a dT that is not finite.
 * Step k, point-to-point: with n = n_inliers, S[a][b] = term(9 + 3a + b) - term(3 + a) * term(6 + b) / n (the
 *     cross-covariance, times n), the rotation is Horn's: the unit quaternion that is the eigenvector of the largest
 *     eigenvalue of the symmetric 4 x 4 matrix N(S), found by MVS_REGISTER_JACOBI_SWEEPS cyclic Jacobi sweeps
 *     (csrc/cloud_register_solve.h states the order); it is a proper rotation whatever S is (the "determinant fix" of
 *     Kabsch / Umeyama is never needed), no scale.  t = (mq + o) - R (ms + o) with ms = terms 3..5 / n, mq = terms 6..8 / n.
 *     Degenerate: n_inliers < 3, a sum that is not finite, a dT that is not finite.
 *
 * Empty inputs: N == 0 and P == 0 are legal: there are no inliers, so the stop is DEGENERATE at k = 0 (MAX_ITERATIONS when
 *     max_iterations == 0) and transform_out = init.  target_xyz is not read when P == 0, nor source_xyz and idx_out when
 *     N == 0; they must still not be NULL.
 * Determinism: the nearest member is exact and every sum has a fixed shape that depends on N alone, so the same inputs
 *     give the same bytes of every output on every run, on every stream and for every admissible `cell`.  No
 *     floating-point value is added atomically; integer atomics serve the cell bookkeeping of the grid only.
 *
 * Launches, ordered by the stream alone; the host takes no part in the loop: the search grid of mvs_cloud_normals over
 *     the box and the target, built once; then max_iterations + 1 times: one kernel that transforms the sources, finds
 *     each one's nearest member (one wave per source, the search of mvs_cloud_distance), forms the terms and sums each
 *     group; the levels of the sum tree; a one-thread kernel that evaluates, tests the stop and solves.  A device word
 *     set at the stop makes every later kernel return at entry.
 *
 * Workspace: mvs_query_register_workspace = mvs_query_normals_workspace(P, box_min, box_max, cell)
 *                + 8 * MVS_REGISTER_TERMS * (L_0 + L_1 + ... ) + MVS_REGISTER_SCALARS bytes, 8-byte aligned, with
 *     L_0 = ceil(N / MVS_REGISTER_GROUP), L_{k+1} = ceil(L_k / MVS_REGISTER_FANIN) down to and including the first
 *     L_k == 1 (nothing for N == 0).  It does not depend on max_iterations, which is checked all the same.
 *
 * Refusals: a NULL target_xyz, source_xyz, box_min, box_max, transform_out, counts_out, stats_out or workspace (init,
 * target_normals, history_out, system_out and idx_out may be NULL) -> MVS_ERR_NULL; P or N outside [0, 2^31),
 * max_iterations outside [0, MVS_REGISTER_ITERATIONS_MAX], a max_dist, rel_fitness or rel_rmse that is NaN or negative,
 * an init with an entry that is not finite or a last row other than 0 0 0 1, a cell that is not finite or <= 0, a box
 * bound that is not finite, box_min[a] > box_max[a], or 2^31 cells or more -> MVS_ERR_BAD_SHAPE; a dtype other than the
 * two -> MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE. */
#ifndef MVS_REGISTER_ABI_H
#define MVS_REGISTER_ABI_H

#include "mvs_abi.h"
#include "mvs_cloud_abi.h"
#include "mvs_normals_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_REGISTER_ITERATIONS_MAX 1000  /* the most iterations one call enqueues */
#define MVS_REGISTER_TERMS 31             /* doubles of one term vector, and of one system_out row */
#define MVS_REGISTER_HISTORY 19           /* doubles of one history_out row */
#define MVS_REGISTER_GROUP 32             /* sources one level-0 partial sum covers */
#define MVS_REGISTER_FANIN 256            /* partial sums one partial sum of a later level covers */
#define MVS_REGISTER_JACOBI_SWEEPS 10     /* cyclic sweeps over the 4 x 4 matrix of the point-to-point step */
#define MVS_REGISTER_SCALARS 512          /* bytes of the scalar block */
#define MVS_REGISTER_STOP_CONVERGED 1
#define MVS_REGISTER_STOP_MAX_ITERATIONS 2
#define MVS_REGISTER_STOP_DEGENERATE 3

int mvs_query_register_workspace(long long P, long long N, const double box_min[3], const double box_max[3], double cell,
                                 int max_iterations, size_t* bytes);
int mvs_cloud_register(const void* target_xyz, int target_dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, long long P,
                       const void* target_normals /* DEVICE [P][3] of target_dtype, or NULL */,
                       const void* source_xyz, int source_dtype, long long N,
                       const double box_min[3], const double box_max[3], double cell, double max_dist,
                       const double* init /* HOST [16], row-major, or NULL = identity */,
                       int max_iterations, double rel_fitness, double rel_rmse,
                       double* transform_out /* [16] */, long long* counts_out /* [4] */, double* stats_out /* [2] */,
                       double* history_out /* [max_iterations + 1][MVS_REGISTER_HISTORY] or NULL */,
                       double* system_out /* [max_iterations][MVS_REGISTER_TERMS] or NULL */,
                       int* idx_out /* [N] or NULL */,
                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_REGISTER_ABI_H */
