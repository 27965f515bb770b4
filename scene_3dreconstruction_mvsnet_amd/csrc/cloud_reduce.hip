// cloud_reduce.hip -- DTU's point reduction (reducePts with a stated hash for its random order), its observability mask
// and its ground-plane filter, as include/mvs_reduce_abi.h defines them.
//
// mvs_cloud_reduce.  The greedy thinning in key order is the lexicographically-first maximal independent set of the
// "near" graph, and that set is the fixed point of the header's synchronous rule, so every launch is ordered by the
// stream alone.  The cell grid is cloud_knn.h's (shared with the normals, the outliers and the distance); the members
// are worked on in its cell-sorted slot order, so the candidates of a member are contiguous runs of sxyz.  Launches:
//   hipMemsetAsync           counts_out; the counters and the state words; the grid's cell counters
//   reduce_classify_kernel   one thread per point: keep_out = 0, a member is counted into its cell and into counters[0]
//   the grid's three scans and its scatter (knn_build_finish)
//   reduce_round_kernel      max_rounds launches, round k = 1 ..: returns at once when counters[k - 1] == 0.  kLanes lanes
//                            per member (1, or kKnnGroup = 16 sharing each span of candidates) walk the rows of the cells
//                            that [p - min_dist, p + min_dist] touches; a near member with a smaller key that an EARLIER
//                            round kept removes the member, one that no earlier round decided leaves it undecided, else
//                            it is kept.  The state word of a member is written once, round << 1 | kept, and a word that
//                            holds round k reads as undecided in round k: the synchronous rule on one buffer.  The
//                            still-undecided members are counted into counters[k], one ballot and one atomic per wave
//   reduce_finish_kernel     one thread per slot: keep_out of the kept members, their count; thread 0 writes members,
//                            undecided and rounds
// The key of a candidate is recomputed from its index (three 64-bit products) rather than stored: only the candidates that
// are near need it.  No floating-point atomics.  Compiled with -ffp-contract=off: d2, the cap, the cell index, the voxel
// and the plane's value are the header's fp64 restatement.
//
// mvs_cloud_select: one kernel, one thread per point, three counts by ballots and integer atomics.
#include "mvs_reduce_abi.h"
#include "cloud_knn.h"

#include <atomic>

namespace mvs {

constexpr int kReduceCounters = MVS_REDUCE_ROUNDS_MAX + 2;      // members, one per round, one spare (8-byte slots)

struct ReduceParams {
    KnnGrid G;
    unsigned* state;               // [P], by slot: 0 = undecided, else round << 1 | kept
    long long* counters;           // [kReduceCounters]: [0] members, [k] undecided after round k
    double md2;                    // min_dist * min_dist
    double reach;                  // how far a near member's coordinate can lie from the member's, see reduce_round_kernel
    unsigned long long seed;
    int max_rounds;
    unsigned char* keep_out;
    long long* counts_out;
};

__host__ __device__ __forceinline__ unsigned long long reduce_key(unsigned long long seed, int i) {
    unsigned long long z = seed + ((unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) reduce_classify_kernel(ReduceParams R) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    knn_classify<T>(R.G, i, &R.counters[0]);
    if (i < R.G.P) R.keep_out[i] = 0;
}

// Round k.  The cells a near member j of the member at p can lie in: d2 <= md2 bounds each |p[j][a] - p[a]| by
// min_dist * (1 + 2^-51), or by 2^-511 where the square underflowed; `reach` is min_dist * (1 + 2^-48) + 2^-500 + G.slack,
// so fl(p[a] - reach) <= p[j][a] <= fl(p[a] + reach) as real numbers.  knn_cell is a monotone function of the coordinate
// (a difference, a quotient and a floor, each monotone), so j's cell lies between the cells of those two bounds on every
// axis, whatever the cell size.  The clamps of the spans cannot bite, see knn_take.
// kCapped: the grid is short of the members' lanes (kLaunchRoundWide under its cap) and a block goes on to every
// gridDim.x-th group; else one group per block, the kernel without a loop
template <int kLanes, bool kCapped>
__global__ void __launch_bounds__(kCloudThreads) reduce_round_kernel(ReduceParams R, int k) {
    if (R.counters[k - 1] == 0) return;       // nobody was undecided after the round before: the same in every thread
    const KnnGrid& G = R.G;
    const int M = knn_members(G);
    // group `block` of kCloudThreads / kLanes members, block-stride: with kKnnGroup lanes per member the grid is capped
    // (kLaunchRoundWide).  A round reads only what earlier rounds decided, so the order of its members is free
    long long block = blockIdx.x;
    do {
        const long long t = block * kCloudThreads + threadIdx.x;
        const long long s = t / kLanes;
        const int sub = (int)(t % kLanes);
        bool active = s < M;
        if (active) active = __hip_atomic_load(&R.state[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
        bool removed = false, waiting = false;
        if (active) {
            double p[3], lo[3], hi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                p[a] = G.sxyz[(size_t)s * 3 + a];
                lo[a] = p[a] - R.reach;
                hi[a] = p[a] + R.reach;
            }
            const int i = G.sidx[s];
            const unsigned long long hi_key = reduce_key(R.seed, i);
            int c0[3], c1[3];
            knn_cell(G, lo, c0);
            knn_cell(G, hi, c1);
            for (int z = c0[2]; z <= c1[2] && !(kLanes == 1 && removed); ++z) {
                for (int y = c0[1]; y <= c1[1] && !(kLanes == 1 && removed); ++y) {
                    const int line = knn_linear(G, 0, y, z);
                    int a = knn_begin(G, line + c0[0]), b = G.cells_end[line + c1[0]];
                    a = a < 0 ? 0 : a;
                    b = b > G.P ? G.P : b;
                    for (int j = a + sub; j < b; j += kLanes) {
                        if (j == s) continue;
                        const double* q = G.sxyz + (size_t)j * 3;
                        const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        if (!(d2 <= R.md2)) continue;
                        const int ij = G.sidx[j];
                        const unsigned long long hj = reduce_key(R.seed, ij);
                        if (!(hj < hi_key || (hj == hi_key && ij < i))) continue;
                        const unsigned w = __hip_atomic_load(&R.state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (w == 0u || (int)(w >> 1) >= k) {
                            waiting = true;             // no earlier round decided j
                        } else if (w & 1u) {
                            removed = true;             // an earlier round kept j
                            if (kLanes == 1) break;
                        }
                    }
                }
            }
        }
        if (kLanes > 1) {      // the lanes of a member put their findings together; every lane of the wave is here
            const int shift = (threadIdx.x & 63) / kLanes * kLanes;
            const unsigned long long group = (kLanes >= 64 ? ~0ull : (1ull << kLanes) - 1ull) << shift;
            removed = (__ballot(removed) & group) != 0;
            waiting = (__ballot(waiting) & group) != 0;
        }
        bool still = false;
        if (active && sub == 0) {
            if (removed)
                __hip_atomic_store(&R.state[s], (unsigned)k << 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else if (!waiting)
                __hip_atomic_store(&R.state[s], ((unsigned)k << 1) | 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                still = true;
        }
        const int count = __popcll(__ballot(still));
        if ((threadIdx.x & 63) == 0 && count)
            __hip_atomic_fetch_add(&R.counters[k], (long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } while (kCapped && (block += gridDim.x) * kCloudThreads < (long long)M * kLanes);
}

__global__ void __launch_bounds__(kCloudThreads) reduce_finish_kernel(ReduceParams R) {
    const KnnGrid& G = R.G;
    const int M = knn_members(G);
    const long long s = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    bool kept = false;
    if (s < M) {
        kept = (R.state[s] & 1u) != 0;
        const int i = G.sidx[s];
        if (kept && i >= 0 && i < G.P) R.keep_out[i] = 1;      // the index test cannot bite, see knn_take
    }
    const int count = __popcll(__ballot(kept));
    if ((threadIdx.x & 63) == 0 && count)
        __hip_atomic_fetch_add(&R.counts_out[1], (long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s == 0) {
        int rounds = 0;        // the first k after which nobody is undecided, at most max_rounds; counters[0] = members
        while (rounds < R.max_rounds && R.counters[rounds] != 0) ++rounds;
        R.counts_out[0] = M;
        R.counts_out[2] = R.counters[rounds];
        R.counts_out[3] = rounds;
    }
}

// behind the grid's knn_workspace(P, cells): the state words, then the counters
static size_t reduce_tail(long long P) { return 8 * (size_t)((P + 1) / 2) + 8 * (size_t)kReduceCounters; }
static size_t reduce_workspace(long long P, long long cells) { return knn_workspace(P, cells) + reduce_tail(P); }

// lanes per member of the round kernel: 1 or kKnnGroup.  mvs_test_reduce_lanes (below) sets it for the timing tool and
// the tests; the default is the faster form on the 49-view scan of tools/time_cloud_reduce.py
static std::atomic<int> g_reduce_lanes{1};

struct SelectParams {
    const void* xyz;
    const unsigned char* mask;     // or nullptr
    int P;
    int n[3];
    double origin[3], res;
    double plane[4];
    bool with_plane;
    unsigned char* keep_out;
    long long* counts_out;
};

// MATLAB's round: half away from zero
__device__ __forceinline__ double mround(double x) { return x < 0.0 ? -floor(-x + 0.5) : floor(x + 0.5); }

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) select_kernel(SelectParams S) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    bool finite = false, observed = false, kept = false;
    if (i < S.P) {
        const T* src = static_cast<const T*>(S.xyz) + (size_t)i * 3;
        double p[3];
        finite = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = (double)src[a];
            finite = finite && fabs(p[a]) < INFINITY;       // false for NaN
        }
        if (finite) {
            observed = true;
            if (S.mask) {
                double g[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    g[a] = mround((p[a] - S.origin[a]) / S.res);
                    observed = observed && g[a] >= 0.0 && g[a] < (double)S.n[a];
                }
                if (observed) {        // 0 <= g < n: the conversions are exact and the index is below 2^31
                    const long long lin = ((long long)(int)g[0] * S.n[1] + (int)g[1]) * S.n[2] + (int)g[2];
                    observed = S.mask[lin] != 0;
                }
            }
            kept = observed;
            if (S.with_plane) {
                const double v = ((S.plane[0] * p[0] + S.plane[1] * p[1]) + S.plane[2] * p[2]) + S.plane[3];
                kept = kept && v > 0.0;
            }
        }
        S.keep_out[i] = kept ? 1 : 0;
    }
    const bool first = (threadIdx.x & 63) == 0;
    int c = __popcll(__ballot(finite));
    if (first && c) __hip_atomic_fetch_add(&S.counts_out[0], (long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c = __popcll(__ballot(observed));
    if (first && c) __hip_atomic_fetch_add(&S.counts_out[1], (long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c = __popcll(__ballot(kept));
    if (first && c) __hip_atomic_fetch_add(&S.counts_out[2], (long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

// The hook of tools/time_cloud_reduce.py and the tests, not part of the ABI: the lanes per member (1 or 16) of the round
// kernel in later mvs_cloud_reduce calls of this process.  Returns the value it replaces; any other argument only reads it.
int mvs_test_reduce_lanes(int lanes) {
    if (lanes == 1 || lanes == kKnnGroup) return g_reduce_lanes.exchange(lanes, std::memory_order_relaxed);
    return g_reduce_lanes.load(std::memory_order_relaxed);
}

int mvs_query_reduce_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes) {
    return grid_query("mvs_query_reduce_workspace", kCellGrid, P, box_min, box_max, cell, bytes, reduce_workspace);
}

int mvs_cloud_reduce(const void* xyz, int dtype, long long P, const double box_min[3], const double box_max[3], double cell,
                     double min_dist, unsigned long long seed, int max_rounds, unsigned char* keep_out,
                     long long* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!xyz || !box_min || !box_max || !keep_out || !counts_out || !workspace)
        return fail(MVS_ERR_NULL, "mvs_cloud_reduce: NULL argument");
    int n[3];
    long long cells;
    if (int rc = grid_check("mvs_cloud_reduce", kCellGrid, P, box_min, box_max, cell, n, &cells)) return rc;
    if (!(min_dist >= 0.0) || !std::isfinite(min_dist))         // also NaN
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_reduce: min_dist = %g (need a finite min_dist >= 0)", min_dist);
    if (max_rounds < 1 || max_rounds > MVS_REDUCE_ROUNDS_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_reduce: max_rounds = %d (need 1 <= max_rounds <= %d)", max_rounds,
                    MVS_REDUCE_ROUNDS_MAX);
    if (int rc = check_xyz_dtype("mvs_cloud_reduce", dtype)) return rc;
    if (int rc = check_workspace8("mvs_cloud_reduce", workspace, workspace_bytes, reduce_workspace(P, cells))) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(hipMemsetAsync(counts_out, 0, 4 * sizeof(long long), s), "zeroing the counts")) return rc;
    if (P == 0) return MVS_OK;
    ReduceParams R{};
    knn_bind(R.G, xyz, P, box_min, box_max, cell, 1, n, cells, workspace);
    char* tail = static_cast<char*>(workspace) + knn_workspace(P, cells);
    R.state = reinterpret_cast<unsigned*>(tail);
    R.counters = reinterpret_cast<long long*>(tail + 8 * (size_t)((P + 1) / 2));
    R.md2 = min_dist * min_dist;
    R.reach = ((min_dist + min_dist * 0x1p-48) + 0x1p-500) + R.G.slack;
    R.seed = seed;
    R.max_rounds = max_rounds;
    R.keep_out = keep_out;
    R.counts_out = counts_out;
    if (int rc = check_hip(hipMemsetAsync(tail, 0, reduce_tail(P), s), "zeroing the states and the counters")) return rc;
    if (int rc = knn_build_begin(R.G, s)) return rc;
    const bool f64 = dtype == MVS_CLOUD_F64;
    if (f64) reduce_classify_kernel<double><<<knn_point_blocks(R.G), kCloudThreads, 0, s>>>(R);
    else reduce_classify_kernel<float><<<knn_point_blocks(R.G), kCloudThreads, 0, s>>>(R);
    if (int rc = check_hip(hipGetLastError(), "reduce_classify_kernel")) return rc;
    if (int rc = knn_build_finish(R.G, f64, s)) return rc;
    const int lanes = g_reduce_lanes.load(std::memory_order_relaxed);
    // one lane per member is a per-point launch; kKnnGroup lanes would need up to 2^27 blocks, eight times what HIP
    // launches, so that grid is capped and the kernel loops
    const int round_blocks = cloud_blocks(lanes == 1 ? kLaunchRow : kLaunchRoundWide, P);
    const bool capped = lanes != 1 && cloud_capped(kLaunchRoundWide, P);
    for (int k = 1; k <= max_rounds; ++k) {
        if (lanes == 1) reduce_round_kernel<1, false><<<round_blocks, kCloudThreads, 0, s>>>(R, k);
        else if (capped) reduce_round_kernel<kKnnGroup, true><<<round_blocks, kCloudThreads, 0, s>>>(R, k);
        else reduce_round_kernel<kKnnGroup, false><<<round_blocks, kCloudThreads, 0, s>>>(R, k);
        if (int rc = check_hip(hipGetLastError(), "reduce_round_kernel")) return rc;
    }
    reduce_finish_kernel<<<knn_point_blocks(R.G), kCloudThreads, 0, s>>>(R);
    return check_hip(hipGetLastError(), "reduce_finish_kernel");
}

int mvs_cloud_select(const void* xyz, int dtype, long long P, const unsigned char* obs_mask, const int n[3],
                     const double origin[3], double res, const double* plane, unsigned char* keep_out,
                     long long* counts_out, void* stream) {
    if (!xyz || !keep_out || !counts_out) return fail(MVS_ERR_NULL, "mvs_cloud_select: NULL argument");
    if (obs_mask && (!n || !origin)) return fail(MVS_ERR_NULL, "mvs_cloud_select: a mask with a NULL n or origin");
    if (P < 0 || P >= (1LL << 31)) return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_select: P = %lld (need 0 <= P < 2^31)", P);
    if (!std::isfinite(res) || res <= 0.0)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_select: res = %g (need a finite size > 0)", res);
    SelectParams S{};
    if (obs_mask) {
        long long voxels = 1;
        for (int a = 0; a < 3; ++a) {
            if (n[a] < 1) return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_select: n[%d] = %d (need n >= 1)", a, n[a]);
            voxels *= n[a];                      // < 2^31 before this factor, so < 2^62 after it
            if (voxels >= (1LL << 31))
                return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_select: a mask of %d x %d x %d has 2^31 voxels or more", n[0], n[1],
                            n[2]);
        }
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(origin[a]))
                return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_select: origin[%d] = %g (need a finite origin)", a, origin[a]);
            S.n[a] = n[a];
            S.origin[a] = origin[a];
        }
    }
    if (plane)
        for (int a = 0; a < 4; ++a) {
            if (!std::isfinite(plane[a]))
                return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_select: plane[%d] = %g (need finite numbers)", a, plane[a]);
            S.plane[a] = plane[a];
        }
    if (int rc = check_xyz_dtype("mvs_cloud_select", dtype)) return rc;
    S.xyz = xyz;
    S.mask = obs_mask;
    S.P = (int)P;
    S.res = res;
    S.with_plane = plane != nullptr;
    S.keep_out = keep_out;
    S.counts_out = counts_out;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(hipMemsetAsync(counts_out, 0, 3 * sizeof(long long), s), "zeroing the counts")) return rc;
    if (P == 0) return MVS_OK;
    const int blocks = cloud_blocks(kLaunchRow, P);
    if (dtype == MVS_CLOUD_F64) select_kernel<double><<<blocks, kCloudThreads, 0, s>>>(S);
    else select_kernel<float><<<blocks, kCloudThreads, 0, s>>>(S);
    return check_hip(hipGetLastError(), "select_kernel");
}

}  // extern "C"
