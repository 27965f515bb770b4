// cloud_cluster.hip -- the density-connected components of a cloud inside a box (DBSCAN) and the mask that drops the small
// ones, as include/mvs_cluster_abi.h defines them: the labels of the libraries' sequential traversal in index order,
// computed by a parallel rule (the header argues why they are the same).
//
// The cell grid is cloud_knn.h's (shared with the normals, the outliers, the distance and the reduction); the members
// are worked on in its cell-sorted slot order, so the candidates of a member are contiguous runs of sxyz, and they are
// the cells that [p - eps, p + eps] touches, as in cloud_reduce.hip.  Everything per point -- the parent word, the core
// flag, the number of a root, the size histogram -- is indexed by the ORIGINAL point index.  Launches:
//   hipMemsetAsync           counts_out; the core flags, the sizes and the counters; the grid's cell counters
//   cluster_classify_kernel  one thread per point: parent[i] = i, keep_out = 0, labels_out = -2 for a non-member; a
//                            member is counted into its cell and into counters[0]
//   the grid's three scans and its scatter (knn_build_finish)
//   cluster_core_kernel      one thread per member: counts the neighbours, itself among them, and stops at min_points;
//                            core[i] = 1, the core members of a wave counted into counters[1]
//   cluster_union_kernel     one thread per core member i: uf_union(i, j) for every core neighbour j < i (the pair is
//                            the larger index's to unite) whose parent word does not already name what i's names.
//                            cloud_unionfind.h: a retry ends when its own swap succeeds or the roots are equal, which
//                            is no wait on another block
//   cluster_flatten_kernel   one block per tile of kCloudTile indices: a core member reads its root into its own parent
//                            word; the roots of the tile (core, parent[i] == i) are counted -> tiles[block]
//   cluster_scan_kernel      one block: exclusive scan of the tile counts with a running carry; tiles[n] = clusters
//   cluster_number_kernel    one block per tile: number[i] of a root = its rank among the roots in index order
//   cluster_label_kernel     one thread per member: a core member takes number[parent[i]], any other the smallest
//                            number[parent[j]] over its core neighbours j, or -1; labels_out; sizes[label] grows by the
//                            wave's members of that label, one integer atomic per distinct label of the wave; the
//                            border and noise members of a wave are counted into counters[2] and [3]
//   cluster_finish_kernel    one thread per point: keep_out from sizes[label] >= min_size, the kept count, the largest
//                            size by an integer maximum, thread 0 the other counts
// The flatten, scan and number launches are cloud_common.h's tile_count, tile_scan_exclusive and tile_ranks around this
// file's flag.  No floating-point atomics.  Compiled with -ffp-contract=off: d2, eps * eps and the cell index are the
// header's fp64 restatement.
#include "mvs_cluster_abi.h"
#include "cloud_knn.h"
#include "cloud_unionfind.h"

namespace mvs {

constexpr int kClusterCounters = MVS_CLUSTER_COUNTERS;      // members, core, border, noise, spare (8-byte slots)
static_assert(kClusterCounters >= 4, "four counters are used");

struct ClusterParams {
    KnnGrid G;
    unsigned* parent;              // [P], by point: the union-find; every value stored in parent[i] is <= i
    int* core;                     // [P], by point: 1 for a core member
    int* number;                   // [P], by point: the cluster number of a root; read at roots only
    int* sizes;                    // [P], by cluster number
    int* tiles;                    // [n_tiles + 1]: the roots of each tile of kCloudTile indices, then their scan
    long long* counters;           // [kClusterCounters]: members, core, border, noise
    double eps2;                   // eps * eps
    double reach;                  // how far a neighbour's coordinate can lie from the member's, see cluster_walk
    int min_points, min_size;
    int n_tiles;                   // ceil(P / kCloudTile)
    int* labels_out;
    unsigned char* keep_out;
    long long* counts_out;
};

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) cluster_classify_kernel(ClusterParams C) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const bool member = knn_classify<T>(C.G, i, &C.counters[0]);
    if (i < C.G.P) {
        C.parent[i] = (unsigned)i;
        C.keep_out[i] = 0;
        if (!member) C.labels_out[i] = -2;
    }
}

// The neighbours of the member in slot s, itself included: visit(j, idx) for every slot j with d2 <= eps2, idx its point
// index, until visit returns false.  The cells a neighbour j of the member at p can lie in: d2 <= eps2 bounds each
// |p[j][a] - p[a]| by eps * (1 + 2^-51), or by 2^-511 where the square underflowed; `reach` is
// eps * (1 + 2^-48) + 2^-500 + G.slack, so fl(p[a] - reach) <= p[j][a] <= fl(p[a] + reach) as real numbers.  knn_cell is a
// monotone function of the coordinate, so j's cell lies between the cells of those two bounds on every axis, whatever
// the cell size (the argument of cloud_reduce.hip's round kernel).  The clamps and the index test cannot bite, see knn_take.
template <typename Visit>
__device__ __forceinline__ void cluster_walk(const ClusterParams& C, int s, Visit visit) {
    const KnnGrid& G = C.G;
    double p[3], lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = G.sxyz[(size_t)s * 3 + a];
        lo[a] = p[a] - C.reach;
        hi[a] = p[a] + C.reach;
    }
    int c0[3], c1[3];
    knn_cell(G, lo, c0);
    knn_cell(G, hi, c1);
    for (int z = c0[2]; z <= c1[2]; ++z) {
        for (int y = c0[1]; y <= c1[1]; ++y) {
            const int line = knn_linear(G, 0, y, z);
            int a = knn_begin(G, line + c0[0]), b = G.cells_end[line + c1[0]];
            a = a < 0 ? 0 : a;
            b = b > G.P ? G.P : b;
            for (int j = a; j < b; ++j) {
                const double* q = G.sxyz + (size_t)j * 3;
                const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 <= C.eps2)) continue;
                const int idx = G.sidx[j];
                if (idx < 0 || idx >= G.P) continue;
                if (!visit(j, idx)) return;
            }
        }
    }
}

// the point index of the member in slot s of this thread, or -1: beyond the members (or an index the scatter cannot write)
__device__ __forceinline__ int cluster_slot_point(const ClusterParams& C, long long s) {
    if (s >= knn_members(C.G)) return -1;
    const int i = C.G.sidx[s];
    return i >= 0 && i < C.G.P ? i : -1;
}

__global__ void __launch_bounds__(kCloudThreads) cluster_core_kernel(ClusterParams C) {
    const long long s = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const int i = cluster_slot_point(C, s);
    bool core = false;
    if (i >= 0) {
        int found = 0;
        cluster_walk(C, (int)s, [&](int, int) { return ++found < C.min_points; });
        core = found >= C.min_points;
        if (core) C.core[i] = 1;
    }
    const int count = __popcll(__ballot(core));
    if ((threadIdx.x & 63) == 0 && count)
        __hip_atomic_fetch_add(&C.counters[1], (long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kCloudThreads) cluster_union_kernel(ClusterParams C) {
    const long long s = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const int i = cluster_slot_point(C, s);
    if (i < 0 || !C.core[i]) return;
    // Two words that name the same point belong to one set (a word always names a point of its own set): such a pair needs
    // no union, and in a dense cloud that is nearly every pair once the first few have been united.  It only skips work
    unsigned mine = uf_load(&C.parent[i]);
    cluster_walk(C, (int)s, [&](int, int j) {
        if (j < i && C.core[j] && uf_load(&C.parent[j]) != mine) {
            uf_union(C.parent, (unsigned)i, (unsigned)j);
            mine = uf_load(&C.parent[i]);
        }
        return true;
    });
}

// element (pass, wave, lane) of this block's tile of point indices
__device__ __forceinline__ long long cluster_tile_point(int pass) {
    return (long long)blockIdx.x * kCloudTile + pass * kCloudThreads + threadIdx.x;
}
// is point i the root of a cluster?  Nobody unites any more: a root is a core member whose word names itself
__device__ __forceinline__ bool cluster_is_root(const ClusterParams& C, long long i) {
    return i < C.G.P && C.core[i] && C.parent[i] == (unsigned)i;
}

__global__ void __launch_bounds__(kCloudThreads) cluster_flatten_kernel(ClusterParams C) {
#pragma unroll
    for (int k = 0; k < kCloudPasses; ++k) {
        const long long i = cluster_tile_point(k);
        // a store of the root into the member's own word: below what it held, and a root's word is not written
        if (i < C.G.P && C.core[i]) {
            const unsigned r = uf_root(C.parent, (unsigned)i);
            if (r != (unsigned)i) __hip_atomic_store(&C.parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const int n = tile_count<kCloudPasses, kCloudThreads>([&](int k) { return cluster_is_root(C, cluster_tile_point(k)); });
    if (threadIdx.x == 0) C.tiles[blockIdx.x] = n;
}

__global__ void __launch_bounds__(kCloudScanWidth) cluster_scan_kernel(ClusterParams C) {
    const int carry = tile_scan_exclusive<kCloudScanWidth>(C.tiles, C.n_tiles);
    if (threadIdx.x == 0) C.tiles[C.n_tiles] = carry;       // the clusters
}

__global__ void __launch_bounds__(kCloudThreads) cluster_number_kernel(ClusterParams C) {
    const int tile_base = C.tiles[blockIdx.x];
    tile_ranks<kCloudPasses, kCloudThreads>([&](int k) { return cluster_is_root(C, cluster_tile_point(k)); },
                                            [&](int k, int rank, bool set) {
                                                if (set) C.number[cluster_tile_point(k)] = tile_base + rank;
                                            });
}

// the number of the cluster of core member j after the flatten launch: its word names its root.  The clamp cannot bite
// (a root's number is below the clusters, which are at most P); it keeps the histogram's index inside the buffer
__device__ __forceinline__ int cluster_of(const ClusterParams& C, int j) {
    const unsigned r = C.parent[j];
    const int c = C.number[r <= (unsigned)j ? r : (unsigned)j];
    return c < 0 ? 0 : c >= C.G.P ? C.G.P - 1 : c;
}

__global__ void __launch_bounds__(kCloudThreads) cluster_label_kernel(ClusterParams C) {
    const long long s = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const int i = cluster_slot_point(C, s);
    bool border = false, noise = false;
    int label = -1;
    if (i >= 0) {
        label = INT_MAX;
        if (C.core[i]) {
            label = cluster_of(C, i);
        } else {
            cluster_walk(C, (int)s, [&](int, int j) {
                if (C.core[j]) {
                    const int c = cluster_of(C, j);
                    label = c < label ? c : label;
                }
                return label != 0;         // nothing is below 0
            });
            border = label != INT_MAX;
            noise = !border;
        }
        label = noise ? -1 : label;
        C.labels_out[i] = label;
    }
    // The histogram, one atomic per distinct label of the wave: a scan is mostly one cluster, and a word that every thread
    // adds 1 to is a queue.  Every lane of the wave is here; `src` is wave-uniform
    unsigned long long todo = __ballot(label >= 0);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        const int l = lane_int(label, src);
        const unsigned long long same = __ballot(label == l);
        if ((int)(threadIdx.x & 63) == src)
            __hip_atomic_fetch_add(&C.sizes[l], __popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        todo &= ~same;
    }
    const bool first = (threadIdx.x & 63) == 0;
    int count = __popcll(__ballot(border));
    if (first && count) __hip_atomic_fetch_add(&C.counters[2], (long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    count = __popcll(__ballot(noise));
    if (first && count) __hip_atomic_fetch_add(&C.counters[3], (long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kCloudThreads) cluster_finish_kernel(ClusterParams C) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const int clusters = C.tiles[C.n_tiles] < C.G.P ? C.tiles[C.n_tiles] : C.G.P;
    bool kept = false;
    if (i < C.G.P) {
        const int label = C.labels_out[i];
        kept = label >= 0 && label < C.G.P && C.sizes[label] >= C.min_size;
        if (kept) C.keep_out[i] = 1;
        // thread c < clusters speaks for cluster c: the largest size
        if (i < clusters)
            __hip_atomic_fetch_max(&C.counts_out[6], (long long)C.sizes[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int count = __popcll(__ballot(kept));
    if ((threadIdx.x & 63) == 0 && count)
        __hip_atomic_fetch_add(&C.counts_out[5], (long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (i == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) C.counts_out[k] = C.counters[k];
        C.counts_out[4] = clusters;
    }
}

// behind the grid's knn_workspace(P, cells): four words per point, the root tiles, the counters
static long long cluster_tiles(long long P) { return cloud_blocks(kLaunchRowTile, P); }      // P / 1024 <= 2^21: never capped
static size_t cluster_words(long long P) { return 8 * (size_t)((P + 1) / 2); }      // one 32-bit word per point, 8-byte aligned
static size_t cluster_tail(long long P) {
    return 4 * cluster_words(P) + 8 * (size_t)((cluster_tiles(P) + 2) / 2) + 8 * (size_t)kClusterCounters;
}
static size_t cluster_workspace(long long P, long long cells) { return knn_workspace(P, cells) + cluster_tail(P); }

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_cluster_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes) {
    return grid_query("mvs_query_cluster_workspace", kCellGrid, P, box_min, box_max, cell, bytes, cluster_workspace);
}

int mvs_cloud_cluster(const void* xyz, int dtype, long long P, const double box_min[3], const double box_max[3], double cell,
                      double eps, int min_points, int min_size, int* labels_out, unsigned char* keep_out,
                      long long* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!xyz || !box_min || !box_max || !labels_out || !keep_out || !counts_out || !workspace)
        return fail(MVS_ERR_NULL, "mvs_cloud_cluster: NULL argument");
    int n[3];
    long long cells;
    if (int rc = grid_check("mvs_cloud_cluster", kCellGrid, P, box_min, box_max, cell, n, &cells)) return rc;
    if (!(eps >= 0.0) || !std::isfinite(eps))         // also NaN
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_cluster: eps = %g (need a finite eps >= 0)", eps);
    if (min_points < 1) return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_cluster: min_points = %d (need min_points >= 1)", min_points);
    if (min_size < 1) return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_cluster: min_size = %d (need min_size >= 1)", min_size);
    if (int rc = check_xyz_dtype("mvs_cloud_cluster", dtype)) return rc;
    if (int rc = check_workspace8("mvs_cloud_cluster", workspace, workspace_bytes, cluster_workspace(P, cells))) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(hipMemsetAsync(counts_out, 0, 7 * sizeof(long long), s), "zeroing the counts")) return rc;
    if (P == 0) return MVS_OK;
    ClusterParams C{};
    knn_bind(C.G, xyz, P, box_min, box_max, cell, 1, n, cells, workspace);
    char* tail = static_cast<char*>(workspace) + knn_workspace(P, cells);
    const size_t words = cluster_words(P);
    C.parent = reinterpret_cast<unsigned*>(tail);
    C.number = reinterpret_cast<int*>(tail + words);
    C.core = reinterpret_cast<int*>(tail + 2 * words);
    C.sizes = reinterpret_cast<int*>(tail + 3 * words);
    C.tiles = reinterpret_cast<int*>(tail + 4 * words);
    C.counters = reinterpret_cast<long long*>(tail + cluster_tail(P) - 8 * (size_t)kClusterCounters);
    C.eps2 = eps * eps;
    C.reach = ((eps + eps * 0x1p-48) + 0x1p-500) + C.G.slack;
    C.min_points = min_points;
    C.min_size = min_size;
    C.n_tiles = (int)cluster_tiles(P);
    C.labels_out = labels_out;
    C.keep_out = keep_out;
    C.counts_out = counts_out;
    // the core flags, the sizes, the tiles and the counters start at zero; parent and number are written before they are read
    if (int rc = check_hip(hipMemsetAsync(C.core, 0, cluster_tail(P) - 2 * words, s), "zeroing the flags, the sizes and the counters"))
        return rc;
    if (int rc = knn_build_begin(C.G, s)) return rc;
    const bool f64 = dtype == MVS_CLOUD_F64;
    const int blocks = knn_point_blocks(C.G);
    if (f64) cluster_classify_kernel<double><<<blocks, kCloudThreads, 0, s>>>(C);
    else cluster_classify_kernel<float><<<blocks, kCloudThreads, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cluster_classify_kernel")) return rc;
    if (int rc = knn_build_finish(C.G, f64, s)) return rc;
    cluster_core_kernel<<<blocks, kCloudThreads, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cluster_core_kernel")) return rc;
    cluster_union_kernel<<<blocks, kCloudThreads, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cluster_union_kernel")) return rc;
    cluster_flatten_kernel<<<C.n_tiles, kCloudThreads, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cluster_flatten_kernel")) return rc;
    cluster_scan_kernel<<<1, kCloudScanWidth, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cluster_scan_kernel")) return rc;
    cluster_number_kernel<<<C.n_tiles, kCloudThreads, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cluster_number_kernel")) return rc;
    cluster_label_kernel<<<blocks, kCloudThreads, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cluster_label_kernel")) return rc;
    cluster_finish_kernel<<<blocks, kCloudThreads, 0, s>>>(C);
    return check_hip(hipGetLastError(), "cluster_finish_kernel");
}

}  // extern "C"
