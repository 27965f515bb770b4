/* ext/mvs_planes_abi.h -- the dominant planes of a cloud (RANSAC plane segmentation, applied repeatedly), on the device.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).  Refusals are decided on the host before the first HIP call.
 * The header lives in include/ext/ until the contract tables of the test suite can be extended; then it moves to include/.
 *
 * mvs_cloud_planes takes the supporting planes out of a cloud: round after round it draws K candidate planes through three
 * of the points that have no plane yet, counts for each how many of those points lie within `dist` of it, refits the best
 * one to its inliers by least squares and gives the points within `dist` of the refitted plane that plane's number.  It
 * is what Open3D's segment_plane does when it is called again on the rest, with the sampling, the fit and the stop
 * stated below.  Nothing here was compared against Open3D itself.
 *
 * Inputs:
 *     xyz             DEVICE, [P][3], float (MVS_CLOUD_F32) or double (MVS_CLOUD_F64); only read
 *     box_min, box_max  HOST, double [3]; read before the call returns
 *     dist            t, finite and >= 0: a point belongs to a plane iff it lies within t of it
 *     num_candidates  K, 1 <= K <= MVS_PLANES_CANDIDATES_MAX
 *     max_planes      1 <= max_planes <= MVS_PLANES_MAX: the most rounds that are run
 *     min_inliers     >= 3: a round whose best candidate counts fewer stops the call
 *     seed            of the keys
 *     toward          HOST, double [3], or NULL: the side every plane's normal is turned to; read before the call returns
 * Outputs (DEVICE pointers):
 *     planes_out      double    [max_planes][4]  (n0, n1, n2, d) of plane r: ((n0*x + n1*y) + n2*z) + d = 0, |n| = 1
 *     rounds_out      long long [max_planes][4]  M_r, the winner c*, its count, the final inliers of plane r
 *     counts_out      long long [4]              members, planes found, points on planes, stop reason (MVS_PLANES_STOP_*)
 *     labels_out      int       [P]              -2: not a member, -1: on no plane, else the plane's number
 *     cand_counts_out int       [max_planes][K]  or NULL: count[c] of every round
 *     sums_out        double    [max_planes][MVS_PLANES_SUMS]  or NULL: the nine sums the fit of round r starts from
 * Rows of planes_out, rounds_out, cand_counts_out and sums_out that belong to rounds which did not run to the end are
 * filled with bytes 0xFF (a NaN, a -1); of the round that stops the call, rounds_out holds what was known at the stop
 * (M_r for EXHAUSTED; M_r, c* and its count, and cand_counts_out's row, for NO_PLANE).
 *
 * Every operation below is in IEEE double on the inputs converted to double, one operation at a time, nothing contracted
 * (sqrt and the divisions are the device library's).
 *
 * Members: exactly the members of mvs_cloud_normals: point i is a member iff box_min[a] <= p[i][a] <= box_max[a] for
 *     a = 0, 1, 2, both ends inclusive.  NaN and +-inf fall out.  o[a] = 0.5 * (box_min[a] + box_max[a]); q = p - o.
 * Key: key(seed, i) is the (i+1)-th output of SplitMix64 started at `seed` (the hash of mvs_reduce_abi.h), modulo 2^64:
 *         z = seed + (i + 1) * 0x9E3779B97F4A7C15
 *         z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *         z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *         key = z ^ (z >> 31)
 *     Seed 0 gives 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F for i = 0, 1, 2.
 * Round r = 0, 1, ...: the active members A_r are the members with no plane yet, in index order; M_r is their number.
 *     M_r < 3 -> stop MVS_PLANES_STOP_EXHAUSTED.
 * Candidate c = 0 .. K-1: ranks k_j = key(seed, 3 * (r * K + c) + j) mod M_r for j = 0, 1, 2; q^j = q[A_r[k_j]];
 *         a = q^1 - q^0, b = q^2 - q^0
 *         n = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
 *         nn = (n0*n0 + n1*n1) + n2*n2
 *         d0 = (n0*q^0_0 + n1*q^0_1) + n2*q^0_2
 *         thr = (t*t) * nn
 *     The candidate is void if two of its ranks are equal, if nn is not > 0, or if nn or thr is not finite.
 * Count: count[c] = the number of i in A_r with s*s <= thr, s = ((n0*q0 + n1*q1) + n2*q2) - d0 with q = q[i]; 0 for a void
 *     candidate.  No square root and no division: the counts are integers any IEEE restatement reproduces.
 * Winner: c* = the smallest c with the largest count.  count[c*] < min_inliers -> stop MVS_PLANES_STOP_NO_PLANE.
 * Fit: over the winner's inliers (the i counted in count[c*]) nine sums, in this order: q0, q1, q2, q0*q0, q0*q1, q0*q2,
 *     q1*q1, q1*q2, q2*q2.  Each is summed over i = 0 .. P-1 in index order, +0.0 for every i that is no inlier, by the
 *     balanced pairwise sum of mvs_register_abi.h: level 0 sums each MVS_PLANES_GROUP consecutive points, every later
 *     level each MVS_PLANES_FANIN consecutive partial sums, until one is left; past the end +0.0; within a group an xor
 *     butterfly in index order, bit 0 first.  The shape depends on P alone.  They are sums_out[r].
 *     With m = count[c*]: mean[a] = sum_a / m; C[a][b] = sum_ab / m - mean[a] * mean[b].  The normal is a unit eigenvector
 *     of the smallest eigenvalue of C by the MVS_PLANES_JACOBI_SWEEPS cyclic Jacobi sweeps over (0,1), (0,2), (1,2) of
 *     mvs_normals_abi.h (csrc/cloud_planes_fit.h states every operation); of equal smallest diagonal entries the lowest
 *     axis is taken; v / sqrt((v0*v0 + v1*v1) + v2*v2).
 * Sign: the component of largest magnitude is made positive (the lowest axis wins a tie);
 *     d = -((n0*c0 + n1*c1) + n2*c2) with c = mean + o; then, with `toward`, n and d are negated iff
 *     ((n0*toward[0] + n1*toward[1]) + n2*toward[2]) + d < 0.
 *     If a mean, an entry of C, the eigenvector's length or d is not finite, or the length is 0, the plane is the
 *     candidate's own: n / sqrt(nn) through c = q^0 + o, signed by the same rules.
 * Final inliers: point i of A_r gets label r iff fabs(((n0*x + n1*y) + n2*z) + d) <= t, on p itself: the expression of
 *     mvs_cloud_select, so labels_out is a function of planes_out, and a plane can be handed to mvs_cloud_select.
 * Stop: after round max_planes - 1 -> MVS_PLANES_STOP_MAX_PLANES.  counts_out = (members, rounds that gave a plane, the
 *     sum of their final inliers, the reason).
 *
 * Empty input: P == 0 is legal and stops EXHAUSTED with zero counts.  xyz and labels_out are not touched; they must still
 *     not be NULL.
 * Determinism: the counts are integers, every sum has a fixed shape, and a round reads only what the rounds before it
 *     decided: the same inputs give the same bytes of every output on every run and stream.  No floating-point value is
 *     added atomically; integer atomics add the per-block counts.
 *
 * Launches, ordered by the stream alone; the host takes no part in the loop and no block waits for another: one thread
 *     per point marks the members; then per round the active members are counted per tile of MVS_PLANES_TILE points,
 *     the tile counts are scanned by one block, the active members' q are written in rank order, one thread per
 *     candidate forms it, the count kernel tests every candidate against every active member (a tile of points in
 *     registers, the candidates through loads that are uniform across the wave, one integer per candidate and block
 *     added at the end), one block picks the winner, the levels of the sum tree, a one-thread fit, one block per tile
 *     labels and counts.  A device word set at the stop makes every later kernel of a round return at entry.
 *
 * Workspace, with T = ceil(P / MVS_PLANES_TILE), K64 = 64 * ceil(K / 64), L_0 = ceil(P / MVS_PLANES_GROUP),
 *     L_{k+1} = ceil(L_k / MVS_PLANES_FANIN) down to and including the first L_k == 1 (nothing for P == 0):
 *     mvs_query_planes_workspace = 24 * P + 8 * ceil((T + 1) / 2) + 68 * K64 + 8 * MVS_PLANES_SUMS * (L_0 + L_1 + ...)
 *                                  + MVS_PLANES_SCALARS bytes, 8-byte aligned.  It does not depend on max_planes.
 *
 * Refusals: a NULL xyz, box_min, box_max, planes_out, rounds_out, counts_out, labels_out or workspace (toward,
 * cand_counts_out and sums_out may be NULL) -> MVS_ERR_NULL; P outside [0, 2^31), num_candidates outside
 * [1, MVS_PLANES_CANDIDATES_MAX], max_planes outside [1, MVS_PLANES_MAX], min_inliers < 3, a dist that is NaN, negative
 * or infinite, a toward or a box bound that is not finite, box_min[a] > box_max[a] -> MVS_ERR_BAD_SHAPE; a dtype other
 * than the two -> MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE. */
#ifndef MVS_PLANES_ABI_H
#define MVS_PLANES_ABI_H

#include "mvs_abi.h"
#include "mvs_cloud_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_PLANES_CANDIDATES_MAX 8192  /* K: a block's K integer counters fit in 32 KB of LDS */
#define MVS_PLANES_MAX 64               /* the most rounds one call enqueues */
#define MVS_PLANES_SUMS 9               /* doubles of one sums_out row */
#define MVS_PLANES_TILE 1024            /* points one block ranks, and tests per trip */
#define MVS_PLANES_GROUP 256            /* points one level-0 partial sum covers */
#define MVS_PLANES_FANIN 256            /* partial sums one partial sum of a later level covers */
#define MVS_PLANES_JACOBI_SWEEPS 8      /* cyclic sweeps over the 3 x 3 covariance */
#define MVS_PLANES_SCALARS 512          /* bytes of the scalar block */
#define MVS_PLANES_STOP_MAX_PLANES 1
#define MVS_PLANES_STOP_NO_PLANE 2
#define MVS_PLANES_STOP_EXHAUSTED 3

int mvs_query_planes_workspace(long long P, int num_candidates, int max_planes, size_t* bytes);
int mvs_cloud_planes(const void* xyz, int dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, long long P,
                     const double box_min[3], const double box_max[3], double dist, int num_candidates, int max_planes,
                     long long min_inliers, unsigned long long seed, const double* toward /* HOST [3] or NULL */,
                     double* planes_out /* [max_planes][4] */, long long* rounds_out /* [max_planes][4] */,
                     long long* counts_out /* [4] */, int* labels_out /* [P] */,
                     int* cand_counts_out /* [max_planes][num_candidates] or NULL */,
                     double* sums_out /* [max_planes][MVS_PLANES_SUMS] or NULL */,
                     void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_PLANES_ABI_H */
