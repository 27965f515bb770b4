// cloud_register.hip -- the rigid registration of a source cloud onto a target cloud (ICP), as
// include/ext/mvs_register_abi.h defines it: Open3D's registration_icp, point-to-point or point-to-plane, with no host in
// the loop.
//
// The cell grid is cloud_knn.h's, built once over the target; the search is its knn_nearest; the solve is
// cloud_register_solve.h's.  Launches, ordered by the stream alone:
//   hipMemsetAsync            the scalar block (the stop word, the zero sums of N == 0); history_out and system_out to 0xFF
//   register_begin_kernel     one thread: T_0 = init into the scalar block
//   the grid's classify, three scans and scatter (P > 0, N > 0)
//   then max_iterations + 1 times (once when N == 0):
//     register_step_kernel    one WAVE per source, kKnnPerWave sources in turn: s = T p, knn_nearest; lane t keeps the
//                             result of source t, so that after the searches eight lanes fetch their target points (and
//                             normals) in one round trip and form their term vectors side by side; an xor butterfly over
//                             those lanes, the four waves through LDS, one partial vector per group of 32 sources in its
//                             own slot (term-major, so every level of the tree reads and writes consecutive doubles)
//     register_sum_kernel     one launch per further level: blockIdx.y = the term, 256 partial sums per block
//     register_solve_kernel   one thread: fitness, rmse, the history row, the stop test, the step, T_{k+1}
//   Every kernel after register_begin_kernel returns at entry once the stop word is set.
// No floating-point atomics and none of integers either: the counts travel as sums of ones, which are exact.
// Compiled with -ffp-contract=off: every term, sum and solve is the header's fp64 restatement.
#include "ext/mvs_register_abi.h"
#include "cloud_knn.h"
#include "cloud_register_solve.h"

namespace mvs {

constexpr int kTerms = MVS_REGISTER_TERMS;
constexpr int kTermsPoint = 18;         // the terms a point-to-point step uses: 0..17; the others stay +0.0
constexpr int kRegisterGroup = MVS_REGISTER_GROUP;
constexpr int kRegisterFanin = MVS_REGISTER_FANIN;
constexpr int kTermChunk = 8;          // terms the step kernel forms and sums side by side
// terms 3..23 of a point-to-plane step: J[kPairA[k - 3]] * J[kPairB[k - 3]], the upper triangle row by row
__device__ constexpr int kPairA[21] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5};
__device__ constexpr int kPairB[21] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 2, 3, 4, 5, 3, 4, 5, 4, 5, 5};
static_assert(kRegisterGroup == kCloudWaves * kKnnPerWave, "one level-0 partial sum per block and trip of the step kernel");
static_assert(kKnnPerWave == 8, "the butterfly over the lanes that keep a source runs over bits 1, 2, 4");
static_assert(kRegisterFanin == kCloudThreads, "one partial sum per thread of register_sum_kernel");
static_assert(kRegisterJacobiSweeps == MVS_REGISTER_JACOBI_SWEEPS, "the header states the sweep count");
static_assert(MVS_REGISTER_HISTORY == 19, "T (16), fitness, rmse, n_inliers");

// the scalar block, at the end of the workspace
struct RegisterState {
    double zero_sums[kTerms];      // what the solve kernel reads when N == 0
    double T[16];                  // T_k
    double fitness, rmse;          // of Evaluate(T_{k-1})
    int stop;                      // 0, or the reason: every later kernel returns at entry
};
static_assert(sizeof(RegisterState) <= MVS_REGISTER_SCALARS - 8, "the scalar block holds the state and, last, the member count");

struct RegisterParams {
    KnnGrid G;                     // over the target cloud; not built when P == 0 or N == 0
    const void* source;
    const void* normals;           // the target's, or NULL: point-to-point
    int N;
    long long groups;              // L_0
    double max_d2;
    double origin[3];              // the box's centre: the point-to-point sums are taken about it
    const RegisterState* state;
    double* partials;              // level 0: [kTerms][groups]
    int* idx_out;
};

struct RegisterSolveParams {
    RegisterState* state;
    const double* sums;            // [kTerms]: the last level of the tree
    double origin[3];
    double rel_fitness, rel_rmse;
    int max_iterations;
    bool plane;
    double* transform_out;
    long long* counts_out;
    double* stats_out;
    double* history_out;
    double* system_out;
};

struct RegisterInit {
    double T[16];
};

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) register_classify_kernel(KnnGrid G, long long* members) {
    knn_classify<T>(G, (long long)blockIdx.x * kCloudThreads + threadIdx.x, members);
}

__global__ void register_begin_kernel(RegisterState* state, RegisterInit init) {
#pragma unroll
    for (int i = 0; i < 16; ++i) state->T[i] = init.T[i];
}

// TS: the source's type, TT: the target's (and its normals')
template <typename TS, typename TT, bool kPlane>
__global__ void __launch_bounds__(kCloudThreads) register_step_kernel(RegisterParams O) {
    if (O.state->stop) return;
    constexpr int kUsed = kPlane ? kTerms : kTermsPoint;
    __shared__ double wave_terms[kCloudWaves][kTerms];
    const KnnGrid& G = O.G;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int M = G.P > 0 ? knn_members(G) : 0;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = O.state->T[i];
    // s = the image of source i under T -> 0: the source is not counted, 1: counted, 2: counted and s is finite
    auto image = [&](long long i, double s[3]) -> int {
        const TS* src = static_cast<const TS*>(O.source) + (size_t)i * 3;
        double p[3];
        bool counted = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = (double)src[a];
            counted = counted && fabs(p[a]) < INFINITY;       // false for NaN
        }
        bool finite = counted;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[a] = ((T[4 * a] * p[0] + T[4 * a + 1] * p[1]) + T[4 * a + 2] * p[2]) + T[4 * a + 3];
            finite = finite && fabs(s[a]) < INFINITY;
        }
        return counted ? (finite ? 2 : 1) : 0;
    };
    long long block = blockIdx.x;
    do {
        // lane t keeps what the search of this wave's t-th source gave
        double md2 = 0.0;
        int midx = -1;
        const long long first = (block * kCloudWaves + wave) * kKnnPerWave;
        for (int t = 0; t < kKnnPerWave; ++t) {
            if (first + t >= O.N) break;
            double s[3];
            double d2 = INFINITY;
            int j = INT_MAX;
            if (image(first + t, s) == 2 && M > 0) knn_nearest(G, s, O.max_d2, d2, j);
            if (lane == t) {
                midx = j != INT_MAX ? j : -1;
                md2 = d2;
            }
        }
        // and forms its image again (the same operations, the same bits) rather than carry it through the searches
        const bool holder = lane < kKnnPerWave && first + lane < O.N;
        double ms[3] = {0.0, 0.0, 0.0};
        const bool mcounted = holder && image(first + lane, ms) > 0;
        const bool inlier = holder && midx >= 0;
        // the factors of this lane's terms: all +0.0 unless the lane keeps an inlier (with a finite normal)
        if (holder && O.idx_out) O.idx_out[first + lane] = midx;
        double head[3] = {mcounted ? 1.0 : 0.0, inlier ? 1.0 : 0.0, inlier ? md2 : 0.0};
        double f[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // plane: J and r; point: s' and q'
        if (inlier) {
            const TT* tq = static_cast<const TT*>(G.xyz) + (size_t)midx * 3;
            double q[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = (double)tq[a];
            if constexpr (kPlane) {
                const TT* tn = static_cast<const TT*>(O.normals) + (size_t)midx * 3;
                double n[3];
                bool ok = true;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    n[a] = (double)tn[a];
                    ok = ok && fabs(n[a]) < INFINITY;
                }
                if (ok) {
                    const double e0 = ms[0] - q[0], e1 = ms[1] - q[1], e2 = ms[2] - q[2];
                    f[0] = ms[1] * n[2] - ms[2] * n[1];
                    f[1] = ms[2] * n[0] - ms[0] * n[2];
                    f[2] = ms[0] * n[1] - ms[1] * n[0];
                    f[3] = n[0];
                    f[4] = n[1];
                    f[5] = n[2];
                    f[6] = (e0 * n[0] + e1 * n[1]) + e2 * n[2];
                }
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    f[a] = ms[a] - O.origin[a];
                    f[3 + a] = q[a] - O.origin[a];
                }
            }
        }
        // term k of this lane; k is a constant wherever this is called
        auto term = [&](int k) -> double {
            if (k < 3) return head[k];
            if constexpr (kPlane) {
                if (k < 24) return f[kPairA[k - 3]] * f[kPairB[k - 3]];
                return k < 30 ? f[k - 24] * f[6] : f[6] * f[6];
            } else {
                return k < 9 ? f[k - 3] : f[(k - 9) / 3] * f[3 + (k - 9) % 3];
            }
        };
        __syncthreads();       // the trip before has read wave_terms
        // the group's sum in index order, bit 0 first: the lanes of a wave here, then the waves.  A few terms at a time, so
        // that the term vector is never in registers as a whole
#pragma unroll
        for (int k0 = 0; k0 < kUsed; k0 += kTermChunk) {
#pragma unroll
            for (int k = k0; k < (k0 + kTermChunk < kUsed ? k0 + kTermChunk : kUsed); ++k) {
                double v = term(k);
#pragma unroll
                for (int bit = 1; bit < kKnnPerWave; bit <<= 1) v = v + __shfl_xor(v, bit);
                if (lane == 0) wave_terms[wave][k] = v;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        if (threadIdx.x < kTerms) {
            const int k = threadIdx.x;
            const double sum = k < kUsed ? (wave_terms[0][k] + wave_terms[1][k]) + (wave_terms[2][k] + wave_terms[3][k]) : 0.0;
            O.partials[(size_t)k * O.groups + block] = sum;
        }
    } while ((block += gridDim.x) < O.groups);
}

// out[term][block] = the sum of in[term][block * 256 ..], +0.0 past n, in the header's pairing
__global__ void __launch_bounds__(kRegisterFanin) register_sum_kernel(const RegisterState* state, const double* in,
                                                                      long long n, double* out, long long n_out) {
    if (state->stop) return;
    __shared__ double wave_sum[kRegisterFanin / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * kRegisterFanin + threadIdx.x;
    double v = i < n ? in[(size_t)blockIdx.y * n + i] : 0.0;
#pragma unroll
    for (int bit = 1; bit < 64; bit <<= 1) v = v + __shfl_xor(v, bit);
    if (lane == 0) wave_sum[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        out[(size_t)blockIdx.y * n_out + blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// evaluation k: the history row, the stop test, the step
__global__ void register_solve_kernel(RegisterSolveParams S, int k) {
    RegisterState* st = S.state;
    if (st->stop) return;
    __shared__ double sums[kTerms], work[kRegisterSolveWork], dT[16], Tn[16];
    const int used = S.plane ? kTerms : kTermsPoint;      // the tree sums no other term
    for (int i = 0; i < kTerms; ++i) sums[i] = i < used ? S.sums[i] : 0.0;
    const double n_counted = sums[0], n_inliers = sums[1];
    const double fitness = n_counted > 0.0 ? n_inliers / n_counted : 0.0;
    const double rmse = n_inliers > 0.0 ? sqrt(sums[2] / n_inliers) : 0.0;
    if (S.history_out) {
        double* row = S.history_out + (size_t)k * MVS_REGISTER_HISTORY;
        for (int i = 0; i < 16; ++i) row[i] = st->T[i];
        row[16] = fitness;
        row[17] = rmse;
        row[18] = n_inliers;
    }
    int stop = 0;
    if (k > 0 && fabs(fitness - st->fitness) < S.rel_fitness && fabs(rmse - st->rmse) < S.rel_rmse) {
        stop = MVS_REGISTER_STOP_CONVERGED;
    } else if (k == S.max_iterations) {
        stop = MVS_REGISTER_STOP_MAX_ITERATIONS;
    } else {
        bool ok = n_inliers >= (S.plane ? 6.0 : 3.0);
        for (int i = 0; i < used; ++i) ok = ok && solve_finite(sums[i]);
        ok = ok && (S.plane ? register_plane_step(sums, work, dT) : register_point_step(sums, n_inliers, S.origin, work, dT));
        if (ok) {
            register_compose(dT, st->T, Tn);
            for (int i = 0; i < 12; ++i) ok = ok && solve_finite(Tn[i]);
        }
        if (ok) {
            if (S.system_out)
                for (int i = 0; i < kTerms; ++i) S.system_out[(size_t)k * kTerms + i] = sums[i];
            for (int i = 0; i < 16; ++i) st->T[i] = Tn[i];
            st->fitness = fitness;
            st->rmse = rmse;
        } else {
            stop = MVS_REGISTER_STOP_DEGENERATE;
        }
    }
    if (stop) {
        for (int i = 0; i < 16; ++i) S.transform_out[i] = st->T[i];
        S.counts_out[0] = (long long)n_counted;
        S.counts_out[1] = (long long)n_inliers;
        S.counts_out[2] = k;
        S.counts_out[3] = stop;
        S.stats_out[0] = fitness;
        S.stats_out[1] = rmse;
        st->stop = stop;
    }
}

// L_0, L_1, ... down to and including the first 1: how many partial vectors the tree keeps
static long long register_partials(long long N) {
    if (N <= 0) return 0;
    long long L = (N + kRegisterGroup - 1) / kRegisterGroup, total = L;
    while (L > 1) {
        L = (L + kRegisterFanin - 1) / kRegisterFanin;
        total += L;
    }
    return total;
}

static size_t register_tail(long long N) { return 8 * (size_t)kTerms * (size_t)register_partials(N) + MVS_REGISTER_SCALARS; }

static int register_check_counts(const char* who, long long N, int max_iterations) {
    if (N < 0 || N >= (1LL << 31)) return fail(MVS_ERR_BAD_SHAPE, "%s: N = %lld (need 0 <= N < 2^31)", who, N);
    if (max_iterations < 0 || max_iterations > MVS_REGISTER_ITERATIONS_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "%s: max_iterations = %d (need 0 <= max_iterations <= %d)", who, max_iterations,
                    MVS_REGISTER_ITERATIONS_MAX);
    return MVS_OK;
}

template <typename TS, typename TT>
static void register_launch_step(bool plane, int blocks, hipStream_t s, const RegisterParams& O) {
    if (plane) register_step_kernel<TS, TT, true><<<blocks, kCloudThreads, 0, s>>>(O);
    else register_step_kernel<TS, TT, false><<<blocks, kCloudThreads, 0, s>>>(O);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_register_workspace(long long P, long long N, const double box_min[3], const double box_max[3], double cell,
                                 int max_iterations, size_t* bytes) {
    size_t grid = 0;       // *bytes is written only once N and max_iterations have passed too
    if (int rc = grid_query("mvs_query_register_workspace", kCellGrid, P, box_min, box_max, cell, bytes ? &grid : nullptr,
                            knn_workspace))
        return rc;
    if (int rc = register_check_counts("mvs_query_register_workspace", N, max_iterations)) return rc;
    *bytes = grid + register_tail(N);
    return MVS_OK;
}

int mvs_cloud_register(const void* target_xyz, int target_dtype, long long P, const void* target_normals,
                       const void* source_xyz, int source_dtype, long long N, const double box_min[3],
                       const double box_max[3], double cell, double max_dist, const double* init, int max_iterations,
                       double rel_fitness, double rel_rmse, double* transform_out, long long* counts_out, double* stats_out,
                       double* history_out, double* system_out, int* idx_out, void* workspace, size_t workspace_bytes,
                       void* stream) {
    const char* who = "mvs_cloud_register";
    if (!target_xyz || !source_xyz || !box_min || !box_max || !transform_out || !counts_out || !stats_out || !workspace)
        return fail(MVS_ERR_NULL, "%s: NULL argument", who);
    int n[3];
    long long cells;
    if (int rc = grid_check(who, kCellGrid, P, box_min, box_max, cell, n, &cells)) return rc;
    if (int rc = register_check_counts(who, N, max_iterations)) return rc;
    if (!(max_dist >= 0.0))         // also NaN
        return fail(MVS_ERR_BAD_SHAPE, "%s: max_dist = %g (need max_dist >= 0; +inf is allowed)", who, max_dist);
    if (!(rel_fitness >= 0.0)) return fail(MVS_ERR_BAD_SHAPE, "%s: rel_fitness = %g (need rel_fitness >= 0)", who, rel_fitness);
    if (!(rel_rmse >= 0.0)) return fail(MVS_ERR_BAD_SHAPE, "%s: rel_rmse = %g (need rel_rmse >= 0)", who, rel_rmse);
    RegisterInit T0{};
    for (int i = 0; i < 16; ++i) T0.T[i] = init ? init[i] : (i % 5 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(T0.T[i])) return fail(MVS_ERR_BAD_SHAPE, "%s: init[%d] = %g (need finite entries)", who, i, T0.T[i]);
    if (T0.T[12] != 0.0 || T0.T[13] != 0.0 || T0.T[14] != 0.0 || T0.T[15] != 1.0)
        return fail(MVS_ERR_BAD_SHAPE, "%s: the last row of init is %g %g %g %g (need 0 0 0 1)", who, T0.T[12], T0.T[13],
                    T0.T[14], T0.T[15]);
    for (int dtype : {target_dtype, source_dtype})
        if (int rc = check_xyz_dtype(who, dtype)) return rc;
    const size_t need = knn_workspace(P, cells) + register_tail(N);
    if (int rc = check_workspace8(who, workspace, workspace_bytes, need)) return rc;

    RegisterParams O{};
    knn_bind(O.G, target_xyz, P, box_min, box_max, cell, 1, n, cells, workspace);
    double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + knn_workspace(P, cells));
    RegisterState* state = reinterpret_cast<RegisterState*>(partials + (size_t)kTerms * register_partials(N));
    O.source = source_xyz;
    O.normals = target_normals;
    O.N = (int)N;
    O.groups = (N + kRegisterGroup - 1) / kRegisterGroup;
    O.max_d2 = max_dist * max_dist;
    for (int a = 0; a < 3; ++a) O.origin[a] = 0.5 * (box_min[a] + box_max[a]);
    O.state = state;
    O.partials = partials;
    O.idx_out = idx_out;
    const bool plane = target_normals != nullptr;
    const hipStream_t s = static_cast<hipStream_t>(stream);

    if (int rc = check_hip(hipMemsetAsync(state, 0, MVS_REGISTER_SCALARS, s), "zeroing the scalar block")) return rc;
    if (history_out)
        if (int rc = check_hip(hipMemsetAsync(history_out, 0xFF, sizeof(double) * MVS_REGISTER_HISTORY * ((size_t)max_iterations + 1), s),
                               "filling the history"))
            return rc;
    if (system_out && max_iterations > 0)
        if (int rc = check_hip(hipMemsetAsync(system_out, 0xFF, sizeof(double) * kTerms * (size_t)max_iterations, s),
                               "filling the systems"))
            return rc;
    register_begin_kernel<<<1, 1, 0, s>>>(state, T0);
    if (int rc = check_hip(hipGetLastError(), "register_begin_kernel")) return rc;
    if (P > 0 && N > 0) {
        const bool f64 = target_dtype == MVS_CLOUD_F64;
        // the member count of knn_classify: a slot of the scalar block nothing else reads
        long long* members = reinterpret_cast<long long*>(reinterpret_cast<char*>(state) + MVS_REGISTER_SCALARS - 8);
        if (int rc = knn_build_begin(O.G, s)) return rc;
        if (f64) register_classify_kernel<double><<<knn_point_blocks(O.G), kCloudThreads, 0, s>>>(O.G, members);
        else register_classify_kernel<float><<<knn_point_blocks(O.G), kCloudThreads, 0, s>>>(O.G, members);
        if (int rc = check_hip(hipGetLastError(), "register_classify_kernel")) return rc;
        if (int rc = knn_build_finish(O.G, f64, s)) return rc;
    }

    RegisterSolveParams S{};
    S.state = state;
    for (int a = 0; a < 3; ++a) S.origin[a] = O.origin[a];
    S.rel_fitness = rel_fitness;
    S.rel_rmse = rel_rmse;
    S.max_iterations = max_iterations;
    S.plane = plane;
    S.transform_out = transform_out;
    S.counts_out = counts_out;
    S.stats_out = stats_out;
    S.history_out = history_out;
    S.system_out = system_out;
    const int step_blocks = cloud_blocks(kLaunchQuerySearch, N);       // capped: the kernel loops
    const int terms = plane ? kTerms : kTermsPoint;
    // without a source every evaluation is the first: it stops at k = 0
    for (int k = 0; k <= (N > 0 ? max_iterations : 0); ++k) {
        const double* sums = state->zero_sums;
        if (N > 0) {
            const bool s64 = source_dtype == MVS_CLOUD_F64, t64 = target_dtype == MVS_CLOUD_F64;
            if (s64 && t64) register_launch_step<double, double>(plane, step_blocks, s, O);
            else if (s64) register_launch_step<double, float>(plane, step_blocks, s, O);
            else if (t64) register_launch_step<float, double>(plane, step_blocks, s, O);
            else register_launch_step<float, float>(plane, step_blocks, s, O);
            if (int rc = check_hip(hipGetLastError(), "register_step_kernel")) return rc;
            const double* in = partials;
            for (long long L = O.groups; L > 1;) {
                const long long next = (L + kRegisterFanin - 1) / kRegisterFanin;      // <= 2^18 blocks: never capped
                double* out = const_cast<double*>(in) + (size_t)kTerms * L;
                register_sum_kernel<<<dim3((unsigned)cloud_blocks(L, kRegisterFanin), (unsigned)terms), kRegisterFanin, 0, s>>>(
                    state, in, L, out, next);
                if (int rc = check_hip(hipGetLastError(), "register_sum_kernel")) return rc;
                in = out;
                L = next;
            }
            sums = in;
        }
        S.sums = sums;
        register_solve_kernel<<<1, 1, 0, s>>>(S, k);
        if (int rc = check_hip(hipGetLastError(), "register_solve_kernel")) return rc;
    }
    return MVS_OK;
}

}  // extern "C"
