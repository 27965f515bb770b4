// cloud_normals.hip -- a normal for every point of a cloud inside a box from its k nearest neighbours (reference
// eval.py:817, pcd.estimate_normals()), as include/mvs_normals_abi.h defines it.
//
// The cell grid and the ring search are cloud_knn.h's (shared with cloud_outliers.hip); this file adds what a non-member
// gets (normals_classify_kernel) and what is done with a member's neighbours (normals_search_kernel: mean, covariance,
// eigenvector, sign and counts, the sums in neighbour order).
// Compiled with -ffp-contract=off: d2, the cell index and the sums are the header's fp64 restatement.
#include "cloud_knn.h"

namespace mvs {

constexpr int kNormalsSweeps = 8;

struct NormalsParams {
    KnnGrid G;
    const long long* view_starts;
    const double* centres;
    float* normals_out;
    int* nbr_out;
    long long* counts_out;
    int R;
};

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) normals_classify_kernel(NormalsParams N) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    const bool member = knn_classify<T>(N.G, i, &N.counts_out[0]);
    if (!member && i < N.G.P) {
#pragma unroll
        for (int a = 0; a < 3; ++a) N.normals_out[(size_t)i * 3 + a] = 0.0f;
        if (N.nbr_out)
            for (int j = 0; j < N.G.knn; ++j) N.nbr_out[(size_t)i * N.G.knn + j] = -1;
    }
}

// one Jacobi rotation that zeroes A[P][Q] of the symmetric A (its third index is R), accumulated into the columns of V
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rotate(double A[3][3], double V[3][3]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = A[P][R] = c * arp - s * arq;
    A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// kCapped: the grid is short of the members (kLaunchSearch) and a block takes every gridDim.x-th group of
// kCloudWaves * kKnnPerWave of them; else one group per block, the kernel without a loop
template <typename T, bool kCapped>
__global__ void __launch_bounds__(kCloudThreads) normals_search_kernel(NormalsParams N) {
    const KnnGrid& G = N.G;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int M = knn_members(G);
    const int m = M < G.knn ? M : G.knn;        // neighbours of every member
    long long estimated = 0, uncertified = 0;
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
        if (N.nbr_out && lane < G.knn) N.nbr_out[(size_t)i * G.knn + lane] = lane < m ? L.idx : -1;
        double q[3] = {0.0, 0.0, 0.0};
        if (lane < m && L.idx != INT_MAX) {
            double tmp[3];
            box_load<T>(G.xyz, G.bmin, G.bmax, L.idx, tmp);
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = tmp[a];
        }
        double nrm[3] = {0.0, 0.0, 1.0};
        if (m >= 3) {
            ++estimated;
            double mean[3] = {0.0, 0.0, 0.0};
            for (int j = 0; j < m; ++j)
#pragma unroll
                for (int a = 0; a < 3; ++a) mean[a] = mean[a] + lane_double(q[a], j);
#pragma unroll
            for (int a = 0; a < 3; ++a) mean[a] = mean[a] / (double)m;
            double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
            for (int j = 0; j < m; ++j) {
                double d[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) d[a] = lane_double(q[a], j) - mean[a];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = a; b < 3; ++b) A[a][b] = A[a][b] + d[a] * d[b];
            }
            bool any = false;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = a; b < 3; ++b) {
                    A[a][b] = A[a][b] / (double)m;
                    A[b][a] = A[a][b];
                    any = any || A[a][b] != 0.0;
                }
            if (any) {
                double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
                for (int sweep = 0; sweep < kNormalsSweeps; ++sweep) {
                    jacobi_rotate<0, 1, 2>(A, V);
                    jacobi_rotate<0, 2, 1>(A, V);
                    jacobi_rotate<1, 2, 0>(A, V);
                }
                const bool use1 = A[1][1] < A[0][0];
                const double l01 = use1 ? A[1][1] : A[0][0];
                const bool use2 = A[2][2] < l01;
                double v[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) v[k] = use2 ? V[k][2] : use1 ? V[k][1] : V[k][0];
                const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
                if (len > 0.0 && len < INFINITY) {       // false for NaN
#pragma unroll
                    for (int k = 0; k < 3; ++k) nrm[k] = v[k] / len;
                }
            }
        }
        // ---- sign
        bool flip;
        int lo = 0, hi = N.R;                   // the last r in [0, R] with view_starts[r] <= i, by bisection
        bool viewed = false;
        if (N.R > 0 && N.view_starts[0] <= i) {
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (N.view_starts[mid] <= i) lo = mid;
                else hi = mid;
            }
            viewed = i < N.view_starts[lo + 1];
        }
        if (viewed) {
            const double* ctr = N.centres + (size_t)lo * 3;
            const double cx = ctr[0] - p[0], cy = ctr[1] - p[1], cz = ctr[2] - p[2];
            flip = (nrm[0] * cx + nrm[1] * cy) + nrm[2] * cz < 0.0;
        } else {
            const double a0 = fabs(nrm[0]), a1 = fabs(nrm[1]), a2 = fabs(nrm[2]);
            const double big = a0 >= a1 && a0 >= a2 ? nrm[0] : a1 >= a2 ? nrm[1] : nrm[2];
            flip = big < 0.0;
        }
        if (lane < 3) {
            const double v = lane == 0 ? nrm[0] : lane == 1 ? nrm[1] : nrm[2];
            N.normals_out[(size_t)i * 3 + lane] = (float)(flip ? -v : v);
        }
        // ---- could a point outside the box have served better?
        double f = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double dl = p[a] - G.bmin[a], dh = G.bmax[a] - p[a];
            f = dl < f ? dl : f;
            f = dh < f ? dh : f;
        }
        const double last = lane_double(L.d2, m - 1);     // m >= 1: this member itself
        if (m < G.knn || last > f * f) ++uncertified;
    }
    while (kCapped && (block += gridDim.x) * (kCloudWaves * kKnnPerWave) < M);
    if (lane == 0) {
        if (estimated)
            __hip_atomic_fetch_add(&N.counts_out[1], estimated, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (uncertified)
            __hip_atomic_fetch_add(&N.counts_out[2], uncertified, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_normals_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes) {
    return grid_query("mvs_query_normals_workspace", kCellGrid, P, box_min, box_max, cell, bytes, knn_workspace);
}

int mvs_cloud_normals(const void* xyz, int xyz_dtype, long long P, const double box_min[3], const double box_max[3],
                      double cell, int knn, const long long* view_starts, const double* centres, int R, float* normals_out,
                      int* nbr_out, long long* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!xyz || !box_min || !box_max || !normals_out || !counts_out || !workspace)
        return fail(MVS_ERR_NULL, "mvs_cloud_normals: NULL argument");
    if (R < 0) return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_normals: R = %d (need R >= 0)", R);
    if ((R == 0) != (view_starts == nullptr) || (R == 0) != (centres == nullptr))
        return fail(MVS_ERR_NULL, "mvs_cloud_normals: view_starts and centres must be NULL when R == 0 and only then (R = %d)",
                    R);
    int n[3];
    long long cells;
    if (int rc = grid_check("mvs_cloud_normals", kCellGrid, P, box_min, box_max, cell, n, &cells)) return rc;
    if (knn < 3 || knn > MVS_NORMALS_KNN_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_normals: knn = %d (need 3 <= knn <= %d)", knn, MVS_NORMALS_KNN_MAX);
    if (int rc = check_xyz_dtype("mvs_cloud_normals", xyz_dtype)) return rc;
    if (int rc = check_workspace8("mvs_cloud_normals", workspace, workspace_bytes, knn_workspace(P, cells))) return rc;
    NormalsParams N{};
    knn_bind(N.G, xyz, P, box_min, box_max, cell, knn, n, cells, workspace);
    N.view_starts = view_starts;
    N.centres = centres;
    N.normals_out = normals_out;
    N.nbr_out = nbr_out;
    N.counts_out = counts_out;
    N.R = R;
    const bool f64 = xyz_dtype == MVS_CLOUD_F64;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(hipMemsetAsync(counts_out, 0, 3 * sizeof(long long), s), "zeroing the counts")) return rc;
    if (P == 0) return MVS_OK;
    if (int rc = knn_build_begin(N.G, s)) return rc;
    if (f64) normals_classify_kernel<double><<<knn_point_blocks(N.G), kCloudThreads, 0, s>>>(N);
    else normals_classify_kernel<float><<<knn_point_blocks(N.G), kCloudThreads, 0, s>>>(N);
    if (int rc = check_hip(hipGetLastError(), "normals_classify_kernel")) return rc;
    if (int rc = knn_build_finish(N.G, f64, s)) return rc;
    const int search_blocks = knn_search_blocks(N.G);
    if (cloud_capped(kLaunchSearch, P)) {
        if (f64) normals_search_kernel<double, true><<<search_blocks, kCloudThreads, 0, s>>>(N);
        else normals_search_kernel<float, true><<<search_blocks, kCloudThreads, 0, s>>>(N);
    } else {
        if (f64) normals_search_kernel<double, false><<<search_blocks, kCloudThreads, 0, s>>>(N);
        else normals_search_kernel<float, false><<<search_blocks, kCloudThreads, 0, s>>>(N);
    }
    return check_hip(hipGetLastError(), "normals_search_kernel");
}

}  // extern "C"
