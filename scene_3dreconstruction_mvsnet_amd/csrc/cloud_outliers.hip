// cloud_outliers.hip -- statistical outlier removal among the points of a cloud inside a box (reference eval.py:495,
// pcd.remove_statistical_outlier()), as include/mvs_outliers_abi.h defines it.
//
// The cell grid and the ring search are cloud_knn.h's (shared with cloud_normals.hip).  Launches, ordered by the stream alone:
//   hipMemsetAsync            counts_out; the grid's cell counters
//   outliers_classify_kernel  one thread per point: a non-member gets -1.0, 0 and the NaNs, a member is counted
//   the grid's three scans and its scatter (knn_build_finish)
//   outliers_search_kernel    one WAVE per member: the ring search, then the sum of the m square roots in neighbour order
//                             over readlane, one division, and the count of valid points
//   cloud_sum_tree            S(x), cloud_sum.h's pairwise tree (shared with cloud_distance.hip): blocks of
//                             MVS_OUTLIERS_BLOCK consecutive elements, relaunched on the partial sums until one is left
//   outliers_mean_kernel      one thread: the mean, into the scalar block
//   cloud_sum_tree            S(y), the deviations formed on load
//   outliers_stats_kernel     one thread: std and threshold; writes stats_out and the threshold into the scalar block
//   outliers_mark_kernel      one thread per point: keep_out, xyz_masked_out; `kept` by a ballot and one atomic per wave
// No floating-point atomics: a block's sum has one owner, and the tree's shape depends on P alone.
// Compiled with -ffp-contract=off: every sum, the deviations and the threshold are the header's fp64 restatement.
#include "mvs_outliers_abi.h"
#include "cloud_knn.h"
#include "cloud_sum.h"

namespace mvs {

struct OutliersParams {
    KnnGrid G;
    double* dist_out;
    unsigned char* keep_out;
    void* masked_out;
    long long* counts_out;
};

template <typename T> struct OutliersBits;
template <> struct OutliersBits<float> {
    using type = unsigned int;
    static constexpr type nan = 0x7FC00000u;
};
template <> struct OutliersBits<double> {
    using type = unsigned long long;
    static constexpr type nan = 0x7FF8000000000000ull;
};

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) outliers_classify_kernel(OutliersParams O) {
    using U = typename OutliersBits<T>::type;
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const bool member = knn_classify<T>(O.G, i, &O.counts_out[0]);
    if (!member && i < O.G.P) {
        O.dist_out[i] = -1.0;
        O.keep_out[i] = 0;
        if (O.masked_out) {
#pragma unroll
            for (int a = 0; a < 3; ++a) static_cast<U*>(O.masked_out)[(size_t)i * 3 + a] = OutliersBits<T>::nan;
        }
    }
}

// kCapped: as in normals_search_kernel
template <bool kCapped>
__global__ void __launch_bounds__(kCloudThreads) outliers_search_kernel(OutliersParams O) {
    const KnnGrid& G = O.G;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int M = knn_members(G);
    const int m = M < G.knn ? M : G.knn;        // neighbours of every member
    long long valid = 0;
    long long block = blockIdx.x;
    do
    for (int t = 0; t < kKnnPerWave; ++t) {
        const long long s = (block * kCloudWaves + wave) * kKnnPerWave + t;
        if (s >= M) break;
        const int i = G.sidx[s];
        if (i < 0 || i >= G.P) continue;        // cannot happen: the scatter filled every slot below M
        double p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = G.sxyz[(size_t)s * 3 + a];
        KnnList L;
        knn_search(G, p, L);
        // ---- lanes 0 .. m-1 hold the neighbours in order
        const double root = lane < m ? sqrt(L.d2) : 0.0;
        double sum = 0.0;
        for (int j = 0; j < m; ++j) sum = sum + lane_double(root, j);
        const double dist = sum / (double)m;    // m >= 1: this member itself
        if (lane == 0) O.dist_out[i] = dist;
        if (dist > 0.0) ++valid;
    }
    while (kCapped && (block += gridDim.x) * (kCloudWaves * kKnnPerWave) < M);
    if (lane == 0 && valid)
        __hip_atomic_fetch_add(&O.counts_out[1], valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void outliers_mean_kernel(const double* total, const long long* counts, double* scalars) {
    const long long n_valid = counts[1];
    scalars[kScalarMean] = n_valid > 0 ? *total / (double)n_valid : 0.0;
}

__global__ void outliers_stats_kernel(const double* total, const long long* counts, double std_ratio, double* scalars,
                                      double* stats_out) {
    const long long n_valid = counts[1];
    const double mean = scalars[kScalarMean];
    const double std = n_valid > 1 ? sqrt(*total / (double)(n_valid - 1)) : 0.0;
    const double scaled = std_ratio * std;
    const double threshold = n_valid > 0 ? mean + scaled : 0.0;
    scalars[kScalarThreshold] = threshold;
    stats_out[0] = mean;
    stats_out[1] = std;
    stats_out[2] = threshold;
}

// members only: the classify pass wrote the non-members
template <typename T>
__global__ void __launch_bounds__(kCloudThreads) outliers_mark_kernel(OutliersParams O, const double* scalars) {
    using U = typename OutliersBits<T>::type;
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const double d = i < O.G.P ? O.dist_out[i] : -1.0;
    const bool member = d >= 0.0;
    const bool keep = d > 0.0 && d < scalars[kScalarThreshold];
    if (member) {
        O.keep_out[i] = keep ? 1 : 0;
        if (O.masked_out) {
            const U* src = static_cast<const U*>(O.G.xyz) + (size_t)i * 3;
            U* dst = static_cast<U*>(O.masked_out) + (size_t)i * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) dst[a] = keep ? src[a] : OutliersBits<T>::nan;
        }
    }
    const int kept = __popcll(__ballot(keep));
    if ((threadIdx.x & 63) == 0 && kept)
        __hip_atomic_fetch_add(&O.counts_out[2], (long long)kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static size_t outliers_workspace(long long P, long long cells) {
    return knn_workspace(P, cells) + 8 * (size_t)cloud_sum_partials(P) + MVS_OUTLIERS_SCALARS;
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_outliers_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes) {
    return grid_query("mvs_query_outliers_workspace", kCellGrid, P, box_min, box_max, cell, bytes, outliers_workspace);
}

int mvs_cloud_outliers(const void* xyz, int xyz_dtype, long long P, const double box_min[3], const double box_max[3],
                       double cell, int nb_neighbors, double std_ratio, double* dist_out, unsigned char* keep_out,
                       void* xyz_masked_out, long long* counts_out, double* stats_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!xyz || !box_min || !box_max || !dist_out || !keep_out || !counts_out || !stats_out || !workspace)
        return fail(MVS_ERR_NULL, "mvs_cloud_outliers: NULL argument");
    int n[3];
    long long cells;
    if (int rc = grid_check("mvs_cloud_outliers", kCellGrid, P, box_min, box_max, cell, n, &cells)) return rc;
    if (nb_neighbors < 2 || nb_neighbors > MVS_NORMALS_KNN_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_outliers: nb_neighbors = %d (need 2 <= nb_neighbors <= %d)", nb_neighbors,
                    MVS_NORMALS_KNN_MAX);
    if (!std::isfinite(std_ratio) || std_ratio <= 0.0)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_outliers: std_ratio = %g (need a finite ratio > 0)", std_ratio);
    if (int rc = check_xyz_dtype("mvs_cloud_outliers", xyz_dtype)) return rc;
    if (int rc = check_workspace8("mvs_cloud_outliers", workspace, workspace_bytes, outliers_workspace(P, cells))) return rc;
    OutliersParams O{};
    knn_bind(O.G, xyz, P, box_min, box_max, cell, nb_neighbors, n, cells, workspace);
    O.dist_out = dist_out;
    O.keep_out = keep_out;
    O.masked_out = xyz_masked_out;
    O.counts_out = counts_out;
    double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + knn_workspace(P, cells));
    double* scalars = partials + cloud_sum_partials(P);
    const bool f64 = xyz_dtype == MVS_CLOUD_F64;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(hipMemsetAsync(counts_out, 0, 3 * sizeof(long long), s), "zeroing the counts")) return rc;
    if (P == 0) return check_hip(hipMemsetAsync(stats_out, 0, 3 * sizeof(double), s), "zeroing the statistics");
    if (int rc = knn_build_begin(O.G, s)) return rc;
    const int blocks = knn_point_blocks(O.G);
    if (f64) outliers_classify_kernel<double><<<blocks, kCloudThreads, 0, s>>>(O);
    else outliers_classify_kernel<float><<<blocks, kCloudThreads, 0, s>>>(O);
    if (int rc = check_hip(hipGetLastError(), "outliers_classify_kernel")) return rc;
    if (int rc = knn_build_finish(O.G, f64, s)) return rc;
    if (cloud_capped(kLaunchSearch, P)) outliers_search_kernel<true><<<knn_search_blocks(O.G), kCloudThreads, 0, s>>>(O);
    else outliers_search_kernel<false><<<knn_search_blocks(O.G), kCloudThreads, 0, s>>>(O);
    if (int rc = check_hip(hipGetLastError(), "outliers_search_kernel")) return rc;
    const double* total = nullptr;
    if (int rc = cloud_sum_tree(kSumPositive, dist_out, P, partials, scalars, s, &total)) return rc;
    outliers_mean_kernel<<<1, 1, 0, s>>>(total, counts_out, scalars);
    if (int rc = check_hip(hipGetLastError(), "outliers_mean_kernel")) return rc;
    if (int rc = cloud_sum_tree(kSumDeviation, dist_out, P, partials, scalars, s, &total)) return rc;
    outliers_stats_kernel<<<1, 1, 0, s>>>(total, counts_out, std_ratio, scalars, stats_out);
    if (int rc = check_hip(hipGetLastError(), "outliers_stats_kernel")) return rc;
    if (f64) outliers_mark_kernel<double><<<blocks, kCloudThreads, 0, s>>>(O, scalars);
    else outliers_mark_kernel<float><<<blocks, kCloudThreads, 0, s>>>(O, scalars);
    return check_hip(hipGetLastError(), "outliers_mark_kernel");
}

}  // extern "C"
