/* mvs_reduce_abi.h -- the three steps DTU's evaluation applies to a cloud before it measures distances, on the device:
 * the point reduction (reducePts), the observability mask and the ground-plane filter.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).  Refusals are decided on the host before the first HIP call.
 *
 * mvs_cloud_reduce thins a cloud so that no two kept points lie within min_dist of each other: DTU's reducePts_haa, a
 * greedy pass over the points in a random order, with the order given by a stated hash instead of MATLAB's randperm.
 * mvs_cloud_select is the two per-point filters: is the point's voxel set in the observability mask, and does the point
 * lie above the ground plane.  Together with mvs_cloud_distance (mvs_distance_abi.h) they are DTU's evaluation of one
 * scan.  What is still not DTU's: randperm is replaced by the hash, so the individual kept points differ from those of
 * any MATLAB run while their distribution is the same; nothing here was compared against the MATLAB code or real DTU
 * files; the per-scan tables are not built.
 *
 * ---- mvs_cloud_reduce
 * Inputs:
 *     xyz           DEVICE, [P][3], float (MVS_CLOUD_F32) or double (MVS_CLOUD_F64); only read
 *     box_min, box_max  HOST, double [3]: the box of the cloud; read before the call returns
 *     cell          edge of the search grid's cells; any admissible value gives the same output bytes
 *     min_dist      finite, >= 0
 *     seed          of the keys
 *     max_rounds    1 .. MVS_REDUCE_ROUNDS_MAX: the most rounds that are run
 * Outputs (DEVICE pointers):
 *     keep_out      unsigned char [P]  1 where the point is kept, else 0; every element is written
 *     counts_out    long long     [4]  members, kept, undecided, rounds
 *
 * Every operation below is in IEEE double on the inputs converted to double, one operation at a time, nothing contracted.
 *
 * Members: exactly the members of mvs_cloud_normals (mvs_normals_abi.h): point i is a member iff
 *     box_min[a] <= p[i][a] <= box_max[a] for a = 0, 1, 2, both ends inclusive.  NaN and +-inf fall out.  A non-member
 *     gets keep_out[i] = 0.
 * Key: h(i) is the (i+1)-th output of SplitMix64 started at `seed`, all modulo 2^64:
 *         z = seed + (i + 1) * 0x9E3779B97F4A7C15
 *         z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *         z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *         h = z ^ (z >> 31)
 *     Seed 0 gives 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F for i = 0, 1, 2.  Members are ordered by
 *     (h(i), i), compared lexicographically.
 * Near: members i != j are near iff d2 = (dx*dx + dy*dy) + dz*dz <= min_dist * min_dist (one product), d = p[j] - p[i].
 *     The bound is inclusive, like MATLAB's rangesearch; exact duplicates are near, also at min_dist == 0.
 * Result: visit the members in key order and keep a member iff no member kept before it is near.  That is reducePts_haa
 *     with its randperm replaced by the hash.
 * Rounds: how it is computed, and part of the contract.  After round 0 every member is undecided.  In round k >= 1 take
 *     a member i still undecided after round k-1 and let E(i) be the near members with a smaller key.  If some member of
 *     E(i) was kept after round k-1, i is removed.  Otherwise, if all of E(i) were removed after round k-1 (or E(i) is
 *     empty), i is kept.  Otherwise i stays undecided.  A round reads only what earlier rounds decided.  `rounds` is the
 *     smaller of max_rounds and the first k after which nobody is undecided; it is 0 with no members.
 * Counts: counts_out = {members, kept, undecided, rounds}.  A member still undecided after max_rounds gets
 *     keep_out[i] = 0 and is counted in `undecided`; the mask is the greedy result iff undecided == 0.
 * Determinism: because a round reads only earlier rounds, all four counts and the mask are functions of the input
 *     alone: the same bytes on every run, on every stream and for every admissible `cell`.  No floating-point value is
 *     added atomically; integer atomics serve the counts and the cell bookkeeping only.
 * Empty input: P == 0 is legal: the four counts are zero.  xyz and keep_out are not touched; they must still not be NULL.
 *
 * Launches, ordered by the stream alone (no block waits for another, no cooperative or persistent grid): the search grid
 *     of mvs_cloud_normals over the box and the cloud; max_rounds round launches, each over the members in the grid's
 *     cell-sorted order with one 32-bit state word per member (0 = undecided, else round << 1 | kept; a word written in
 *     round k reads as undecided in round k), each adding its still-undecided count into its own counter and returning at
 *     once when the previous counter is zero; one launch that writes keep_out and the counts.  The candidates of a member
 *     are the cells that [p - min_dist, p + min_dist] touches, pulled out by the slack of the grid.  A round launch with
 *     16 lanes per member (the test hook's form) is capped at 2^24 - 1 blocks, a HIP launch having fewer than 2^32
 *     threads, and loops over the rest; with one lane per member it never needs more than 2^23.
 *
 * Workspace: mvs_query_reduce_workspace = mvs_query_normals_workspace(P, box_min, box_max, cell)
 *                                         + 8 * ceil(P / 2)                     the state words
 *                                         + 8 * (MVS_REDUCE_ROUNDS_MAX + 2)     members, one counter per round, one spare
 *     bytes, 8-byte aligned.
 *
 * Refusals: a NULL xyz, box_min, box_max, keep_out, counts_out or workspace -> MVS_ERR_NULL; P outside [0, 2^31), a
 * min_dist that is NaN, negative or not finite, max_rounds outside [1, MVS_REDUCE_ROUNDS_MAX], a cell that is not finite
 * or <= 0, a box bound that is not finite, box_min[a] > box_max[a], or 2^31 cells or more
 * (n[a] = floor((box_max[a] - box_min[a]) / cell) + 1 per axis) -> MVS_ERR_BAD_SHAPE; a dtype other than the two ->
 * MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE.
 *
 * ---- mvs_cloud_select
 * Inputs:
 *     xyz           DEVICE, [P][3], float or double; only read
 *     obs_mask      DEVICE, unsigned char [n[0]][n[1]][n[2]], or NULL: no observability test.  Only read
 *     n, origin     HOST, int [3] and double [3]: the mask's shape and the centre of voxel (0, 0, 0); read before the call
 *                   returns; may be NULL when obs_mask is
 *     res           the voxels' edge, finite and > 0 (checked with or without a mask)
 *     plane         HOST, double [4], or NULL: no plane test; read before the call returns
 * Outputs (DEVICE pointers):
 *     keep_out      unsigned char [P]  every element is written
 *     counts_out    long long     [3]  finite, observed, kept
 * One thread per point, in double on the inputs converted to double, nothing contracted.  A point with a non-finite
 * coordinate gets 0 and is counted nowhere.
 * Observed, when obs_mask is not NULL: g[a] = mround((p[a] - origin[a]) / res) with
 *     mround(x) = x < 0 ? -floor(-x + 0.5) : floor(x + 0.5) -- MATLAB's round, half away from zero; DTU's 1-based
 *     round(q / Res + 1) is the same cell.  The point is observed iff 0 <= g[a] < n[a] on all three axes, compared in
 *     double before any conversion to integer, and obs_mask[(g[0] * n[1] + g[1]) * n[2] + g[2]] != 0.  Without a mask
 *     every finite point is observed.
 * Above the plane, when plane is not NULL: ((plane[0] * x + plane[1] * y) + plane[2] * z) + plane[3] > 0, strictly: DTU's
 *     P' * [Q; 1] > 0.
 * keep is the conjunction of the tests that were asked for; counts_out = {finite points, observed ones, kept ones}.
 * P == 0 is legal: three zero counts; xyz and keep_out are not touched.
 *
 * Refusals: a NULL xyz, keep_out or counts_out, or a mask with a NULL n or origin -> MVS_ERR_NULL; P outside [0, 2^31),
 * with a mask an n[a] < 1 or n[0] * n[1] * n[2] >= 2^31 or a non-finite origin, a res that is not finite or <= 0, a
 * non-finite plane number -> MVS_ERR_BAD_SHAPE; a dtype other than the two -> MVS_ERR_BAD_DTYPE. */
#ifndef MVS_REDUCE_ABI_H
#define MVS_REDUCE_ABI_H

#include "mvs_abi.h"
#include "mvs_cloud_abi.h"
#include "mvs_normals_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_REDUCE_ROUNDS_MAX 256       /* the most rounds one call runs */

int mvs_query_reduce_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes);
int mvs_cloud_reduce(const void* xyz, int dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, long long P,
                     const double box_min[3], const double box_max[3], double cell,
                     double min_dist, unsigned long long seed, int max_rounds,
                     unsigned char* keep_out /* [P] */, long long* counts_out /* [4] */,
                     void* workspace, size_t workspace_bytes, void* stream);
int mvs_cloud_select(const void* xyz, int dtype, long long P,
                     const unsigned char* obs_mask /* DEVICE [n0][n1][n2] or NULL */, const int n[3],
                     const double origin[3], double res, const double* plane /* HOST [4] or NULL */,
                     unsigned char* keep_out /* [P] */, long long* counts_out /* [3] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_REDUCE_ABI_H */
