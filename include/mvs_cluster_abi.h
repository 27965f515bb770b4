/* mvs_cluster_abi.h -- the density-connected components of a cloud inside a box (DBSCAN), on the device, and the mask
 * that drops the small ones: what a planner takes from a fused cloud, and the remedy for the small dense blobs of wrong
 * depth that a k-NN distance test (mvs_cloud_outliers) cannot see because their neighbours are each other.
 *
 * An addition within ABI version 2 of libmvs_hip.so (mvs_abi.h: status codes, the common rules -- caller-owned device
 * memory, work enqueued on `stream`, no device allocation, no synchronisation, a status code plus
 * mvs_last_error_string(), never aborts).  Refusals are decided on the host before the first HIP call.
 *
 * Inputs:
 *     xyz           DEVICE, [P][3], float (MVS_CLOUD_F32) or double (MVS_CLOUD_F64); only read
 *     box_min, box_max  HOST, double [3]: the box of the cloud; read before the call returns
 *     cell          edge of the search grid's cells; any admissible value gives the same output bytes
 *     eps           finite, >= 0: the neighbourhood radius
 *     min_points    >= 1: the neighbours, itself counted, that make a member a core member
 *     min_size      >= 1: the smallest cluster that is kept
 * Outputs (DEVICE pointers):
 *     labels_out    int           [P]  the cluster number, -1 for noise, -2 for a non-member; every element is written
 *     keep_out      unsigned char [P]  1 where the point belongs to a cluster of at least min_size points, else 0; every
 *                                      element is written
 *     counts_out    long long     [7]  members, core, border, noise, clusters, kept points, size of the largest cluster
 *
 * Every operation below is in IEEE double on the inputs converted to double, one operation at a time, nothing contracted.
 *
 * Members: exactly the members of mvs_cloud_normals (mvs_normals_abi.h): point i is a member iff
 *     box_min[a] <= p[i][a] <= box_max[a] for a = 0, 1, 2, both ends inclusive.  NaN and +-inf fall out.  A non-member
 *     gets labels_out[i] = -2 and keep_out[i] = 0.
 * Neighbours: members i and j are neighbours iff d2 = (dx*dx + dy*dy) + dz*dz <= eps * eps (one product), d = p[j] - p[i].
 *     The bound is inclusive, as in mvs_cloud_reduce's "near" and scikit-learn's radius_neighbors.  A member is its own
 *     neighbour; exact duplicates are neighbours, also at eps == 0.
 * Core: a member with at least min_points neighbours, itself counted.
 * Clusters: the connected components of the graph on the core members whose edges are the neighbour pairs.  The number
 *     of a cluster is the count of clusters whose smallest core index is smaller than its own: numbers run from 0 to
 *     clusters - 1 in the order of the clusters' smallest core indices.  A core member's label is its cluster's number.
 * Border: a member that is not core but has a core neighbour.  Its label is the smallest cluster number among its core
 *     neighbours.
 * Noise: any other member: label -1.
 * Keep: keep_out[i] = 1 iff labels_out[i] >= 0 and the size of that cluster, core and border members counted, is
 *     >= min_size.  min_size = 1 drops the noise only.
 * Counts: counts_out = {members, core, border, noise, clusters, kept points, size of the largest cluster (0 without one)}.
 * Empty input: P == 0 is legal: seven zeros.  xyz, labels_out and keep_out are not touched; they must still not be NULL.
 *
 * These are the labels of the sequential DBSCAN of the libraries (scikit-learn's DBSCAN, Open3D's cluster_dbscan), which
 *     visits the points in index order: an unlabelled core point starts the next cluster and the cluster is expanded
 *     completely -- every core point density-reachable from it, and every still unlabelled neighbour of those -- before
 *     the visit goes on.  The argument: (1) the core points a cluster's expansion reaches are exactly one connected
 *     component of the core graph, whatever the order inside the expansion.  (2) A component is discovered at its
 *     smallest core index s: no earlier start could have reached it (it would be the same component, started at a core
 *     index below s), and a non-core point never starts a cluster; so clusters are started in ascending order of their
 *     smallest core index, which is the numbering above.  (3) A border point b is labelled by the first expansion that
 *     touches it and never relabelled.  Every cluster with a core neighbour of b touches b during its own expansion, and
 *     the expansions happen one after the other in ascending cluster number, so b keeps the smallest number among its
 *     core neighbours' clusters.  (4) A member without a core neighbour is touched by no expansion: noise.
 *     Checked on the host against scikit-learn's DBSCAN(algorithm="kd_tree") on seeded clouds (tests/cluster_ref.py,
 *     tests/test_cloud_cluster_host.py); never compared with Open3D, which is not a dependency.
 *
 * Determinism: members, neighbours and core are per-point predicates; the components of a graph, their smallest indices,
 *     a minimum over a set of neighbours and the sizes are functions of those.  So labels, mask and counts are functions
 *     of the input alone: the same bytes on every run, on every stream and for every admissible `cell`.  No
 *     floating-point value is added atomically; integer atomics serve the cell bookkeeping, the counts, the size
 *     histogram and the parent words below.
 *
 * Launches, ordered by the stream alone (no block waits for another, no cooperative or persistent grid):
 *     the search grid of mvs_cloud_normals over the box and the cloud, its classify launch also writing parent[i] = i,
 *         labels_out[i] = -2 for the non-members and keep_out[i] = 0;
 *     core: one thread per member in the grid's cell-sorted order walks the cells that [p - eps, p + eps] touches, pulled
 *         out by the slack of the grid, counts neighbours and stops at min_points;
 *     union: one thread per core member i unites i with every core neighbour of a smaller index in a lock-free
 *         union-find (csrc/cloud_unionfind.h) of one 32-bit parent word per point, indexed by the ORIGINAL point index;
 *     flatten: one launch in which every core member reads its root into its own parent word and the roots of each tile
 *         of 1024 indices are counted; one single-block scan of the tile counts; one launch that ranks the roots: the
 *         rank of a root among the roots in index order is the number of its cluster;
 *     label: one thread per member: a core member takes the number of its root, any other the smallest number among its
 *         core neighbours or -1, written to labels_out; each label >= 0 adds 1 to the integer histogram of the sizes;
 *     finish: one thread per point: keep_out from the histogram, the counts.
 * The union-find.  The invariant: EVERY VALUE EVER STORED IN parent[i] IS <= i.  It holds at the start (parent[i] = i),
 *     and there are two stores.  `find` halves a path: it replaces parent[x] = p by the g = parent[p] it has read, by a
 *     compare-and-swap that expects p; g <= p <= x by the invariant on the two words read.  `union` hangs a root under
 *     another: it finds the two roots, and if they differ swaps parent[larger] from `larger` (it still is a root) to
 *     `smaller`, which is below it.  Consequences: (a) a find path strictly decreases -- the next node is a value stored
 *     in a parent word of the current one, below it unless it is the root -- so it ends within i steps whatever other
 *     threads store meanwhile, and never leaves [0, i]; (b) a parent word only ever decreases (both stores replace a
 *     value by a smaller one), so every failed compare-and-swap means that some word has decreased since it was read;
 *     the words are bounded below by 0, so all retries together are bounded by the sum of the indices: a retry ends
 *     when its own swap succeeds or the two roots are equal, and is no wait on another block; (c) a word always names a
 *     point of the same set (halving moves a pointer to an ancestor, a union only writes a root), and a union never
 *     separates what was united, so at quiescence two core members have the same root iff a path of neighbour pairs joins
 *     them; (d) the root of a set is the only member whose word names itself, every other word names a smaller index of
 *     the set, so the root is the set's smallest index, independent of the schedule: the quantity the numbering needs.
 *
 * Workspace: mvs_query_cluster_workspace = mvs_query_normals_workspace(P, box_min, box_max, cell)
 *                                          + 8 * ceil(P / 2) * 4                      parent, core flag, number of a root,
 *                                                                                     size histogram: one word each per point
 *                                          + 8 * ceil((ceil(P / 1024) + 1) / 2)       the roots of each tile, and their sum
 *                                          + 8 * MVS_CLUSTER_COUNTERS                 members, core, border, noise, spare
 *     bytes, 8-byte aligned.
 *
 * Refusals: a NULL xyz, box_min, box_max, labels_out, keep_out, counts_out or workspace -> MVS_ERR_NULL; P outside
 * [0, 2^31), an eps that is NaN, negative or not finite, min_points < 1, min_size < 1, a cell that is not finite or <= 0,
 * a box bound that is not finite, box_min[a] > box_max[a], or 2^31 cells or more
 * (n[a] = floor((box_max[a] - box_min[a]) / cell) + 1 per axis) -> MVS_ERR_BAD_SHAPE; a dtype other than the two ->
 * MVS_ERR_BAD_DTYPE; a workspace that is too small or not 8-byte aligned -> MVS_ERR_WORKSPACE. */
#ifndef MVS_CLUSTER_ABI_H
#define MVS_CLUSTER_ABI_H

#include "mvs_abi.h"
#include "mvs_cloud_abi.h"
#include "mvs_normals_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_CLUSTER_COUNTERS 8          /* 8-byte counters behind the per-point words */

int mvs_query_cluster_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes);
int mvs_cloud_cluster(const void* xyz, int dtype /* MVS_CLOUD_F32 | MVS_CLOUD_F64 */, long long P,
                      const double box_min[3], const double box_max[3], double cell,
                      double eps, int min_points, int min_size,
                      int* labels_out /* [P] */, unsigned char* keep_out /* [P] */, long long* counts_out /* [7] */,
                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_CLUSTER_ABI_H */
