// cloud_distance.hip -- the distance from every point of a query cloud to the nearest point of a reference cloud inside a
// box, with its counts and its mean, as include/mvs_distance_abi.h defines them: one direction of accuracy / completeness.
//
// The cell grid is cloud_knn.h's (shared with cloud_normals.hip and cloud_outliers.hip), built over the reference cloud;
// the search is its knn_nearest, the sum cloud_sum.h's tree.  Launches, ordered by the stream alone:
//   hipMemsetAsync            counts_out; the scalar block; the grid's cell counters
//   distance_classify_kernel  one thread per reference point: a member is counted into its cell
//   the grid's three scans and its scatter (knn_build_finish)
//   distance_search_kernel    one WAVE per query, kKnnPerWave queries in turn: knn_nearest, one square root, dist_out and
//                             idx_out.  With P == 0 there is no grid and every counted query gets +inf
//   distance_count_kernel     one thread per query: n_counted, n_within and the below counts, each by one ballot and one
//                             integer atomic per wave
//   cloud_sum_tree            S(x) over dist_out, x formed on load (kSumFinite: -1.0 and +inf contribute +0.0)
//   distance_stats_kernel     one thread: S(x) and the mean into stats_out
// No floating-point atomics.  Compiled with -ffp-contract=off: d2, the cell index, the cap and the sum are the header's
// fp64 restatement.
#include "mvs_distance_abi.h"
#include "cloud_knn.h"
#include "cloud_sum.h"

namespace mvs {

static_assert(MVS_DISTANCE_SCALARS >= 4 * sizeof(double), "the sum tree's three doubles, then M");
constexpr int kScalarMembers = 3;       // the scalar block's fourth slot, a long long: what knn_classify counts

struct DistanceParams {
    KnnGrid G;                          // over the reference cloud; not built when P == 0
    const void* query;
    int N, T;
    double max_d2;
    double thresholds[MVS_DISTANCE_THRESHOLDS_MAX];
    double* dist_out;
    int* idx_out;
    long long* counts_out;
};

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) distance_classify_kernel(KnnGrid G, long long* members) {
    knn_classify<T>(G, (long long)blockIdx.x * kCloudThreads + threadIdx.x, members);
}

// kCapped: the grid is short of the queries (kLaunchQuerySearch) and a block takes every gridDim.x-th group of
// kCloudWaves * kKnnPerWave of them; else one group per block, the kernel without a loop
template <typename T, bool kCapped>
__global__ void __launch_bounds__(kCloudThreads) distance_search_kernel(DistanceParams O) {
    const KnnGrid& G = O.G;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int M = G.P > 0 ? knn_members(G) : 0;
    long long block = blockIdx.x;
    do
    for (int t = 0; t < kKnnPerWave; ++t) {
        const long long i = (block * kCloudWaves + wave) * kKnnPerWave + t;
        if (i >= O.N) break;
        const T* src = static_cast<const T*>(O.query) + (size_t)i * 3;
        double q[3];
        bool counted = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            q[a] = (double)src[a];
            counted = counted && fabs(q[a]) < INFINITY;       // false for NaN
        }
        double dist = -1.0;
        int idx = -1;
        if (counted) {
            double d2 = INFINITY;
            int j = INT_MAX;
            if (M > 0) knn_nearest(G, q, O.max_d2, d2, j);
            const bool within = j != INT_MAX;
            dist = within ? sqrt(d2) : INFINITY;
            idx = within ? j : -1;
        }
        if (lane == 0) {
            O.dist_out[i] = dist;
            if (O.idx_out) O.idx_out[i] = idx;
        }
    }
    while (kCapped && (block += gridDim.x) * (kCloudWaves * kKnnPerWave) < O.N);
}

__global__ void __launch_bounds__(kCloudThreads) distance_count_kernel(DistanceParams O) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const double d = i < O.N ? O.dist_out[i] : -1.0;
    const bool counted = d >= 0.0, within = counted && d < INFINITY;
    const bool first = (threadIdx.x & 63) == 0;
    int n = __popcll(__ballot(counted));
    if (first && n) __hip_atomic_fetch_add(&O.counts_out[0], (long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    n = __popcll(__ballot(within));
    if (first && n) __hip_atomic_fetch_add(&O.counts_out[1], (long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int t = 0; t < O.T; ++t) {
        n = __popcll(__ballot(within && d < O.thresholds[t]));
        if (first && n)
            __hip_atomic_fetch_add(&O.counts_out[2 + t], (long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void distance_stats_kernel(const double* total, const long long* counts, double* stats_out) {
    const long long n_within = counts[1];
    stats_out[0] = *total;
    stats_out[1] = n_within > 0 ? *total / (double)n_within : 0.0;
}

// behind the grid's knn_workspace(P, cells): the sum tree's partials and the scalar block
static size_t distance_tail(long long N) { return 8 * (size_t)cloud_sum_partials(N) + MVS_DISTANCE_SCALARS; }

static int distance_check_n(const char* who, long long N) {
    if (N < 0 || N >= (1LL << 31)) return fail(MVS_ERR_BAD_SHAPE, "%s: N = %lld (need 0 <= N < 2^31)", who, N);
    return MVS_OK;
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_distance_workspace(long long P, long long N, const double box_min[3], const double box_max[3], double cell,
                                 size_t* bytes) {
    size_t grid = 0;       // *bytes is written only once N has passed too
    if (int rc = grid_query("mvs_query_distance_workspace", kCellGrid, P, box_min, box_max, cell, bytes ? &grid : nullptr,
                            knn_workspace))
        return rc;
    if (int rc = distance_check_n("mvs_query_distance_workspace", N)) return rc;
    *bytes = grid + distance_tail(N);
    return MVS_OK;
}

int mvs_cloud_distance(const void* ref_xyz, int ref_dtype, long long P, const void* query_xyz, int query_dtype, long long N,
                       const double box_min[3], const double box_max[3], double cell, double max_dist,
                       const double* thresholds, int T, double* dist_out, int* idx_out, long long* counts_out,
                       double* stats_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ref_xyz || !query_xyz || !box_min || !box_max || !dist_out || !counts_out || !stats_out || !workspace)
        return fail(MVS_ERR_NULL, "mvs_cloud_distance: NULL argument");
    int n[3];
    long long cells;
    if (int rc = grid_check("mvs_cloud_distance", kCellGrid, P, box_min, box_max, cell, n, &cells)) return rc;
    if (int rc = distance_check_n("mvs_cloud_distance", N)) return rc;
    if (T < 0 || T > MVS_DISTANCE_THRESHOLDS_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_distance: T = %d (need 0 <= T <= %d)", T, MVS_DISTANCE_THRESHOLDS_MAX);
    if (T > 0 && !thresholds) return fail(MVS_ERR_NULL, "mvs_cloud_distance: NULL thresholds with T = %d", T);
    if (!(max_dist >= 0.0))         // also NaN
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_distance: max_dist = %g (need max_dist >= 0; +inf is allowed)", max_dist);
    for (int t = 0; t < T; ++t)
        if (!(thresholds[t] >= 0.0) || !std::isfinite(thresholds[t]))
            return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_distance: thresholds[%d] = %g (need a finite threshold >= 0)", t,
                        thresholds[t]);
    for (int dtype : {ref_dtype, query_dtype})
        if (int rc = check_xyz_dtype("mvs_cloud_distance", dtype)) return rc;
    const size_t need = knn_workspace(P, cells) + distance_tail(N);
    if (int rc = check_workspace8("mvs_cloud_distance", workspace, workspace_bytes, need)) return rc;
    DistanceParams O{};
    knn_bind(O.G, ref_xyz, P, box_min, box_max, cell, 1, n, cells, workspace);
    O.query = query_xyz;
    O.N = (int)N;
    O.T = T;
    O.max_d2 = max_dist * max_dist;
    for (int t = 0; t < T; ++t) O.thresholds[t] = thresholds[t];
    O.dist_out = dist_out;
    O.idx_out = idx_out;
    O.counts_out = counts_out;
    double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + knn_workspace(P, cells));
    double* scalars = partials + cloud_sum_partials(N);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(hipMemsetAsync(counts_out, 0, (2 + T) * sizeof(long long), s), "zeroing the counts")) return rc;
    if (N == 0) return check_hip(hipMemsetAsync(stats_out, 0, 2 * sizeof(double), s), "zeroing the statistics");
    if (P > 0) {
        const bool f64 = ref_dtype == MVS_CLOUD_F64;
        long long* members = reinterpret_cast<long long*>(scalars) + kScalarMembers;
        if (int rc = check_hip(hipMemsetAsync(members, 0, sizeof(long long), s), "zeroing the member count")) return rc;
        if (int rc = knn_build_begin(O.G, s)) return rc;
        if (f64) distance_classify_kernel<double><<<knn_point_blocks(O.G), kCloudThreads, 0, s>>>(O.G, members);
        else distance_classify_kernel<float><<<knn_point_blocks(O.G), kCloudThreads, 0, s>>>(O.G, members);
        if (int rc = check_hip(hipGetLastError(), "distance_classify_kernel")) return rc;
        if (int rc = knn_build_finish(O.G, f64, s)) return rc;
    }
    const int search_blocks = cloud_blocks(kLaunchQuerySearch, N);       // capped: the kernel loops
    if (cloud_capped(kLaunchQuerySearch, N)) {
        if (query_dtype == MVS_CLOUD_F64) distance_search_kernel<double, true><<<search_blocks, kCloudThreads, 0, s>>>(O);
        else distance_search_kernel<float, true><<<search_blocks, kCloudThreads, 0, s>>>(O);
    } else {
        if (query_dtype == MVS_CLOUD_F64) distance_search_kernel<double, false><<<search_blocks, kCloudThreads, 0, s>>>(O);
        else distance_search_kernel<float, false><<<search_blocks, kCloudThreads, 0, s>>>(O);
    }
    if (int rc = check_hip(hipGetLastError(), "distance_search_kernel")) return rc;
    distance_count_kernel<<<cloud_blocks(kLaunchRow, N), kCloudThreads, 0, s>>>(O);
    if (int rc = check_hip(hipGetLastError(), "distance_count_kernel")) return rc;
    const double* total = nullptr;
    if (int rc = cloud_sum_tree(kSumFinite, dist_out, N, partials, scalars, s, &total)) return rc;
    distance_stats_kernel<<<1, 1, 0, s>>>(total, counts_out, stats_out);
    return check_hip(hipGetLastError(), "distance_stats_kernel");
}

}  // extern "C"
