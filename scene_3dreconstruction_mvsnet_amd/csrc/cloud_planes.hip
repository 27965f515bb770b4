// cloud_planes.hip -- the dominant planes of a cloud (RANSAC, round after round), as include/ext/mvs_planes_abi.h defines
// them, with no host in the loop.
//
// labels_out is the state of the loop: -2 no member, -1 active, r on plane r.  Launches, ordered by the stream alone:
//   hipMemsetAsync              the scalar block; planes_out, rounds_out, cand_counts_out and sums_out to 0xFF
//   planes_classify_kernel      one thread per point: the members (round 0's ranking counts them)
//   then max_planes times:
//     planes_tile_count_kernel  one block per tile of 1024 points: its active members (tile_count)
//     planes_scan_kernel        one block: the tile counts to offsets (tile_scan_exclusive), M_r, the EXHAUSTED stop
//     planes_emit_kernel        one block per tile: q = p - o of its active members in rank order (tile_ranks)
//     planes_candidates_kernel  one thread per candidate: three ranks, n, d0, thr; a void one gets thr = -1
//     planes_count_kernel       THE HOT ONE: lanes over points, four points of a tile per lane in registers, the
//                               candidates by loads that are uniform across the wave; a candidate's count of a wave is a
//                               ballot's population count, 64 candidates' counts are kept one per lane and added into the
//                               block's LDS counters at once; every block adds its counters once, at its end;
//                               gridDim.x blocks loop over the tiles, gridDim.y over the chunks of 64 candidates
//     planes_winner_kernel      one block: the smallest c of the largest count, the NO_PLANE stop
//     planes_sum0_kernel        one thread per point: the nine terms of the winner's inliers, one partial per 256 points
//     planes_sum_kernel         one launch per further level: blockIdx.y = the term, 256 partial sums per block
//     planes_fit_kernel         one thread: cloud_planes_fit.h
//     planes_label_kernel       one block per tile of 1024 points: the final inliers, and their number
//   planes_finish_kernel        one thread: counts_out
//   Every kernel of a round returns at entry once the stop word is set.
// Integer atomics add counts; no floating-point value is added atomically.
// Compiled with -ffp-contract=off: every test, term, sum and the fit are the header's fp64 restatement.
#include "ext/mvs_planes_abi.h"
#include "cloud_common.h"
#include "cloud_planes_fit.h"

#include <algorithm>
#include <climits>

namespace mvs {

constexpr int kPlanesGroup = MVS_PLANES_GROUP;
constexpr int kPlanesFanin = MVS_PLANES_FANIN;
constexpr int kPlanesChunk = 64;              // candidates whose counts a wave keeps one per lane
constexpr int kPlanesCountBlocks = 1024;      // the count kernel's grid over tiles: four blocks per compute unit, each looping
constexpr int kPlanesCountSplit = 16;         // and over chunks of candidates (gridDim.y), at most
static_assert(MVS_PLANES_TILE == kCloudTile, "the ranking's tile is the cloud path's");
static_assert(kPlanesGroup == kCloudThreads && kPlanesFanin == kCloudThreads, "one point, one partial sum per thread");
static_assert(kPlanesJacobiSweeps == MVS_PLANES_JACOBI_SWEEPS && kPlanesSums == MVS_PLANES_SUMS, "the header states both");
static_assert(MVS_PLANES_CANDIDATES_MAX % kPlanesChunk == 0, "K64 <= MVS_PLANES_CANDIDATES_MAX");

// the scalar block, at the end of the workspace
struct PlanesState {
    long long members;
    long long active;                  // M_r
    double winner[kPlanesCand];        // the winning candidate of this round
    int winner_count;
    int found;                         // planes so far
    int stop;                          // 0, or the reason: every later kernel of a round returns at entry
};
static_assert(sizeof(PlanesState) <= MVS_PLANES_SCALARS, "the scalar block holds the state");

struct PlanesParams {
    const void* xyz;
    int P, K, K64, max_planes;
    double bmin[3], bmax[3], origin[3], toward[3];
    bool has_toward;
    double t;
    unsigned long long seed;
    long long min_inliers;
    long long n_tiles, groups;         // ceil(P / 1024), L_0
    PlanesState* state;
    double* aq;                        // [M_r][3]: q of the active members in rank order
    int* tiles;                        // [n_tiles + 1]
    double* cand;                      // [K64][kPlanesCand]
    int* counts;                       // [K64]
    double* partials;                  // level 0: [kPlanesSums][groups]
    double* planes_out;
    long long* rounds_out;
    long long* counts_out;
    int* labels_out;
    int* cand_counts_out;
    double* sums_out;
};

__device__ __forceinline__ unsigned long long planes_key(unsigned long long seed, unsigned long long i) {
    unsigned long long z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ void planes_add(long long* where, int n) {
    atomicAdd(reinterpret_cast<unsigned long long*>(where), (unsigned long long)n);
}

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) planes_classify_kernel(PlanesParams O) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    double p[3];
    const bool in = i < O.P && box_load<T>(O.xyz, O.bmin, O.bmax, (int)i, p);
    if (i < O.P) O.labels_out[i] = in ? -1 : -2;      // the members are counted by round 0's ranking: M_0
}

__global__ void __launch_bounds__(kCloudThreads) planes_tile_count_kernel(PlanesParams O) {
    if (O.state->stop) return;
    const long long first = (long long)blockIdx.x * kCloudTile + threadIdx.x;
    const int n = tile_count<kCloudPasses, kCloudThreads>([&](int pass) {
        const long long i = first + pass * kCloudThreads;
        return i < O.P && O.labels_out[i] == -1;
    });
    if (threadIdx.x == 0) O.tiles[blockIdx.x] = n;
}

__global__ void __launch_bounds__(kCloudScanWidth) planes_scan_kernel(PlanesParams O, int r) {
    const int stop = O.state->stop;
    __syncthreads();       // everyone has read the word this kernel may set
    if (stop) return;
    const int total = tile_scan_exclusive<kCloudScanWidth>(O.tiles, O.n_tiles);
    if (threadIdx.x == 0) {
        O.state->active = total;
        if (r == 0) O.state->members = total;
        O.rounds_out[(size_t)r * 4] = total;
        if (total < 3) O.state->stop = MVS_PLANES_STOP_EXHAUSTED;
    }
}

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) planes_emit_kernel(PlanesParams O) {
    if (O.state->stop) return;
    const long long first = (long long)blockIdx.x * kCloudTile + threadIdx.x;
    const long long base = O.tiles[blockIdx.x];
    tile_ranks<kCloudPasses, kCloudThreads>(
        [&](int pass) {
            const long long i = first + pass * kCloudThreads;
            return i < O.P && O.labels_out[i] == -1;
        },
        [&](int pass, int rank, bool set) {
            if (!set) return;
            double p[3];
            box_load<T>(O.xyz, O.bmin, O.bmax, (int)(first + pass * kCloudThreads), p);
#pragma unroll
            for (int a = 0; a < 3; ++a) O.aq[(size_t)(base + rank) * 3 + a] = p[a] - O.origin[a];
        });
}

__global__ void __launch_bounds__(kCloudThreads) planes_candidates_kernel(PlanesParams O, int r) {
    if (O.state->stop) return;
    const int c = blockIdx.x * kCloudThreads + threadIdx.x;
    if (c >= O.K64) return;
    O.counts[c] = 0;
    double out[kPlanesCand] = {0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0};      // void: s * s <= -1 never holds
    if (c < O.K) {
        const unsigned long long M = (unsigned long long)O.state->active;
        unsigned long long k[3];
        double q[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            k[j] = planes_key(O.seed, 3ull * ((unsigned long long)r * (unsigned long long)O.K + (unsigned long long)c) + j) % M;
#pragma unroll
            for (int a = 0; a < 3; ++a) q[j][a] = O.aq[(size_t)k[j] * 3 + a];
        }
        const double a0 = q[1][0] - q[0][0], a1 = q[1][1] - q[0][1], a2 = q[1][2] - q[0][2];
        const double b0 = q[2][0] - q[0][0], b1 = q[2][1] - q[0][1], b2 = q[2][2] - q[0][2];
        const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
        const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
        const double d0 = (n0 * q[0][0] + n1 * q[0][1]) + n2 * q[0][2];
        const double thr = (O.t * O.t) * nn;
        const bool valid = k[0] != k[1] && k[0] != k[2] && k[1] != k[2] && nn > 0.0 && fit_finite(nn) && fit_finite(thr);
        if (valid) {
            out[0] = n0;
            out[1] = n1;
            out[2] = n2;
            out[3] = d0;
            out[4] = thr;
#pragma unroll
            for (int a = 0; a < 3; ++a) out[5 + a] = q[0][a];
        }
    }
#pragma unroll
    for (int a = 0; a < kPlanesCand; ++a) O.cand[(size_t)c * kPlanesCand + a] = out[a];
}

// count[c] += the active members of this block's tiles with s * s <= thr
__global__ void __launch_bounds__(kCloudThreads) planes_count_kernel(PlanesParams O) {
    if (O.state->stop) return;
    __shared__ int block_counts[MVS_PLANES_CANDIDATES_MAX];
    const long long M = O.state->active;
    const long long tiles = (M + kCloudTile - 1) / kCloudTile;
    if (blockIdx.x >= tiles) return;
    for (int c = threadIdx.x; c < O.K64; c += kCloudThreads) block_counts[c] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const double* __restrict__ cand = O.cand;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        double q[kCloudPasses][3];
#pragma unroll
        for (int u = 0; u < kCloudPasses; ++u) {
            const long long i = tile * kCloudTile + u * kCloudThreads + threadIdx.x;
#pragma unroll
            for (int a = 0; a < 3; ++a) q[u][a] = i < M ? O.aq[(size_t)i * 3 + a] : NAN;      // NaN: in no candidate's count
        }
        // blockIdx.y takes every gridDim.y-th chunk of candidates: a round with few points left still fills the machine
        for (int c0 = blockIdx.y * kPlanesChunk; c0 < O.K64; c0 += kPlanesChunk * gridDim.y) {
            int mine = 0;      // lane j: this wave's count of candidate c0 + j
#pragma unroll 8
            for (int j = 0; j < kPlanesChunk; ++j) {
                const double* cd = cand + (size_t)(c0 + j) * kPlanesCand;
                const double n0 = cd[0], n1 = cd[1], n2 = cd[2], d0 = cd[3], thr = cd[4];
                int n = 0;
#pragma unroll
                for (int u = 0; u < kCloudPasses; ++u) {
                    const double s = ((n0 * q[u][0] + n1 * q[u][1]) + n2 * q[u][2]) - d0;
                    n += __popcll(__ballot(s * s <= thr));
                }
                mine = lane == j ? n : mine;
            }
            if (mine) atomicAdd(&block_counts[c0 + lane], mine);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < O.K64; c += kCloudThreads) {
        const int n = block_counts[c];
        if (n) atomicAdd(&O.counts[c], n);
    }
}

#ifdef MVS_PLANES_MEASURE
// Only in a build with -DMVS_PLANES_MEASURE (make PLANES_MEASURE=-DMVS_PLANES_MEASURE), for tools/time_cloud_planes.py:
// what the count kernel's arithmetic costs by itself: the same eight double-precision
// operations per test on four points a thread makes up in registers, against a table of 64 candidates read by loads that
// are uniform across the wave, `iters` times over; no point is loaded, nothing goes through LDS, one word per wave is
// stored at the end so that the loop is kept
__global__ void __launch_bounds__(kCloudThreads) planes_rate_kernel(const double* __restrict__ cand, int iters, int* out) {
    double q[kCloudPasses][3];
#pragma unroll
    for (int u = 0; u < kCloudPasses; ++u)
#pragma unroll
        for (int a = 0; a < 3; ++a) q[u][a] = 0.001 * (double)((threadIdx.x + 1) * (u + 1) + a * 7 + blockIdx.x % 13);
    int total = 0;
    for (int it = 0; it < iters; ++it) {
#pragma unroll 8
        for (int j = 0; j < kPlanesChunk; ++j) {
            const double* cd = cand + (size_t)j * kPlanesCand;
            const double n0 = cd[0], n1 = cd[1], n2 = cd[2], d0 = cd[3], thr = cd[4];
#pragma unroll
            for (int u = 0; u < kCloudPasses; ++u) {
                const double s = ((n0 * q[u][0] + n1 * q[u][1]) + n2 * q[u][2]) - d0;
                total += __popcll(__ballot(s * s <= thr));
            }
        }
#pragma unroll
        for (int u = 0; u < kCloudPasses; ++u) q[u][0] = q[u][0] + 1e-9;      // the next pass is not this one again
    }
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * kCloudWaves + (threadIdx.x >> 6)] = total;
}
#endif  // MVS_PLANES_MEASURE

__global__ void __launch_bounds__(kCloudScanWidth) planes_winner_kernel(PlanesParams O, int r) {
    const int stop = O.state->stop;
    __syncthreads();
    if (stop) return;
    __shared__ int best_n[kCloudScanWidth], best_c[kCloudScanWidth];
    int bn = -1, bc = INT_MAX;
    for (int c = threadIdx.x; c < O.K; c += kCloudScanWidth) {
        const int n = O.counts[c];
        if (O.cand_counts_out) O.cand_counts_out[(size_t)r * O.K + c] = n;
        if (n > bn) {      // c ascends: the first of equal counts stays
            bn = n;
            bc = c;
        }
    }
    best_n[threadIdx.x] = bn;
    best_c[threadIdx.x] = bc;
    __syncthreads();
    for (int half = kCloudScanWidth / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            const int on = best_n[threadIdx.x + half], oc = best_c[threadIdx.x + half];
            if (on > best_n[threadIdx.x] || (on == best_n[threadIdx.x] && oc < best_c[threadIdx.x])) {
                best_n[threadIdx.x] = on;
                best_c[threadIdx.x] = oc;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int c = best_c[0], n = best_n[0];
        O.rounds_out[(size_t)r * 4 + 1] = c;
        O.rounds_out[(size_t)r * 4 + 2] = n;
        if (n < O.min_inliers) {
            O.state->stop = MVS_PLANES_STOP_NO_PLANE;
        } else {
            for (int a = 0; a < kPlanesCand; ++a) O.state->winner[a] = O.cand[(size_t)c * kPlanesCand + a];
            O.state->winner_count = n;
        }
    }
}

// partials[term][block] = the sum of the term over this block's 256 points, +0.0 for a point that is no inlier of the winner
template <typename T>
__global__ void __launch_bounds__(kCloudThreads) planes_sum0_kernel(PlanesParams O) {
    if (O.state->stop) return;
    __shared__ double wave_terms[kCloudWaves][kPlanesSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    double q[3] = {0.0, 0.0, 0.0};
    bool in = false;
    if (i < O.P && O.labels_out[i] == -1) {
        const double* w = O.state->winner;
        double p[3];
        box_load<T>(O.xyz, O.bmin, O.bmax, (int)i, p);
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = p[a] - O.origin[a];
        const double s = ((w[0] * q[0] + w[1] * q[1]) + w[2] * q[2]) - w[3];
        in = s * s <= w[4];
    }
    double term[kPlanesSums];
#pragma unroll
    for (int a = 0; a < 3; ++a) term[a] = in ? q[a] : 0.0;
    int k = 3;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) term[k++] = in ? q[a] * q[b] : 0.0;
#pragma unroll
    for (int t = 0; t < kPlanesSums; ++t) {
        double v = term[t];
#pragma unroll
        for (int bit = 1; bit < 64; bit <<= 1) v = v + __shfl_xor(v, bit);
        if (lane == 0) wave_terms[wave][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < kPlanesSums) {
        const int t = threadIdx.x;
        O.partials[(size_t)t * O.groups + blockIdx.x] = (wave_terms[0][t] + wave_terms[1][t]) + (wave_terms[2][t] + wave_terms[3][t]);
    }
}

// out[term][block] = the sum of in[term][block * 256 ..], +0.0 past n, in the header's pairing
__global__ void __launch_bounds__(kPlanesFanin) planes_sum_kernel(const PlanesState* state, const double* in, long long n,
                                                                  double* out, long long n_out) {
    if (state->stop) return;
    __shared__ double wave_sum[kPlanesFanin / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * kPlanesFanin + threadIdx.x;
    double v = i < n ? in[(size_t)blockIdx.y * n + i] : 0.0;
#pragma unroll
    for (int bit = 1; bit < 64; bit <<= 1) v = v + __shfl_xor(v, bit);
    if (lane == 0) wave_sum[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        out[(size_t)blockIdx.y * n_out + blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

__global__ void planes_fit_kernel(PlanesParams O, const double* sums, int r) {
    PlanesState* st = O.state;
    if (st->stop) return;
    double s[kPlanesSums], plane[4];
    for (int a = 0; a < kPlanesSums; ++a) s[a] = sums[a];
    planes_fit(s, (double)st->winner_count, O.origin, O.has_toward ? O.toward : nullptr, st->winner, plane);
    for (int a = 0; a < 4; ++a) O.planes_out[(size_t)r * 4 + a] = plane[a];
    if (O.sums_out)
        for (int a = 0; a < kPlanesSums; ++a) O.sums_out[(size_t)r * kPlanesSums + a] = s[a];
    O.rounds_out[(size_t)r * 4 + 3] = 0;      // the label kernel adds the final inliers
    st->found = r + 1;
}

// one block per tile of 1024 points, four per thread: a hot counter takes one addition per block, not one per wave
template <typename T>
__global__ void __launch_bounds__(kCloudThreads) planes_label_kernel(PlanesParams O, int r) {
    if (O.state->stop) return;
    const long long first = (long long)blockIdx.x * kCloudTile + threadIdx.x;
    const double* pl = O.planes_out + (size_t)r * 4;
    const double n0 = pl[0], n1 = pl[1], n2 = pl[2], d = pl[3];
    const int n = tile_count<kCloudPasses, kCloudThreads>([&](int pass) {
        const long long i = first + pass * kCloudThreads;
        if (i >= O.P || O.labels_out[i] != -1) return false;
        double p[3];
        box_load<T>(O.xyz, O.bmin, O.bmax, (int)i, p);
        const bool on = fabs(((n0 * p[0] + n1 * p[1]) + n2 * p[2]) + d) <= O.t;
        if (on) O.labels_out[i] = r;
        return on;
    });
    if (threadIdx.x == 0 && n) planes_add(&O.rounds_out[(size_t)r * 4 + 3], n);
}

__global__ void planes_finish_kernel(PlanesParams O, int forced) {
    const PlanesState* st = O.state;
    if (forced) O.rounds_out[0] = 0;          // P == 0: M_0 = 0, and no round was enqueued to say so
    O.counts_out[0] = st->members;
    O.counts_out[1] = st->found;
    long long on_planes = 0;
    for (int r = 0; r < st->found; ++r) on_planes += O.rounds_out[(size_t)r * 4 + 3];
    O.counts_out[2] = on_planes;
    O.counts_out[3] = st->stop ? st->stop : forced ? forced : MVS_PLANES_STOP_MAX_PLANES;
}

// L_0, L_1, ... down to and including the first 1: how many partial vectors the tree keeps
static long long planes_partials(long long P) {
    if (P <= 0) return 0;
    long long L = (P + kPlanesGroup - 1) / kPlanesGroup, total = L;
    while (L > 1) {
        L = (L + kPlanesFanin - 1) / kPlanesFanin;
        total += L;
    }
    return total;
}

static int planes_k64(int K) { return (K + kPlanesChunk - 1) / kPlanesChunk * kPlanesChunk; }
static size_t planes_tiles_bytes(long long P) { return 8 * (size_t)(((P + kCloudTile - 1) / kCloudTile + 1 + 1) / 2); }

static size_t planes_workspace(long long P, int K) {
    return 24 * (size_t)P + planes_tiles_bytes(P) + (8 * kPlanesCand + 4) * (size_t)planes_k64(K)
           + 8 * (size_t)kPlanesSums * (size_t)planes_partials(P) + MVS_PLANES_SCALARS;
}

static int planes_check_counts(const char* who, long long P, int K, int max_planes) {
    if (P < 0 || P >= (1LL << 31)) return fail(MVS_ERR_BAD_SHAPE, "%s: P = %lld (need 0 <= P < 2^31)", who, P);
    if (K < 1 || K > MVS_PLANES_CANDIDATES_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "%s: num_candidates = %d (need 1 <= num_candidates <= %d)", who, K,
                    MVS_PLANES_CANDIDATES_MAX);
    if (max_planes < 1 || max_planes > MVS_PLANES_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "%s: max_planes = %d (need 1 <= max_planes <= %d)", who, max_planes, MVS_PLANES_MAX);
    return MVS_OK;
}

}  // namespace mvs

using namespace mvs;

#define PLANES_LAUNCH(call, what)                                       \
    do {                                                                \
        call;                                                           \
        if (int rc_ = check_hip(hipGetLastError(), what)) return rc_;   \
    } while (0)

extern "C" {

#ifdef MVS_PLANES_MEASURE
// For the timing tool, not part of the ABI and not in the library as it ships: planes_rate_kernel on `blocks` blocks, `iters` passes over the 64
// candidates of cand (DEVICE, double [64][8]); out is DEVICE int [blocks * 4].  blocks * 256 * 4 * 64 * iters tests
int mvs_test_planes_rate(const double* cand, int blocks, int iters, int* out, void* stream) {
    if (!cand || !out) return fail(MVS_ERR_NULL, "mvs_test_planes_rate: NULL argument");
    if (blocks < 1 || blocks > 65536 || iters < 1) return fail(MVS_ERR_BAD_SHAPE, "mvs_test_planes_rate: blocks = %d, iters = %d", blocks, iters);
    planes_rate_kernel<<<blocks, kCloudThreads, 0, static_cast<hipStream_t>(stream)>>>(cand, iters, out);
    return check_hip(hipGetLastError(), "planes_rate_kernel");
}
#endif  // MVS_PLANES_MEASURE

int mvs_query_planes_workspace(long long P, int num_candidates, int max_planes, size_t* bytes) {
    const char* who = "mvs_query_planes_workspace";
    if (!bytes) return fail(MVS_ERR_NULL, "%s: NULL argument", who);
    if (int rc = planes_check_counts(who, P, num_candidates, max_planes)) return rc;
    *bytes = planes_workspace(P, num_candidates);
    return MVS_OK;
}

int mvs_cloud_planes(const void* xyz, int dtype, long long P, const double box_min[3], const double box_max[3], double dist,
                     int num_candidates, int max_planes, long long min_inliers, unsigned long long seed,
                     const double* toward, double* planes_out, long long* rounds_out, long long* counts_out, int* labels_out,
                     int* cand_counts_out, double* sums_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "mvs_cloud_planes";
    if (!xyz || !box_min || !box_max || !planes_out || !rounds_out || !counts_out || !labels_out || !workspace)
        return fail(MVS_ERR_NULL, "%s: NULL argument", who);
    if (int rc = planes_check_counts(who, P, num_candidates, max_planes)) return rc;
    if (min_inliers < 3) return fail(MVS_ERR_BAD_SHAPE, "%s: min_inliers = %lld (need min_inliers >= 3)", who, min_inliers);
    if (!std::isfinite(dist) || dist < 0.0) return fail(MVS_ERR_BAD_SHAPE, "%s: dist = %g (need a finite dist >= 0)", who, dist);
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(box_min[a]) || !std::isfinite(box_max[a]) || box_min[a] > box_max[a])
            return fail(MVS_ERR_BAD_SHAPE, "%s: box axis %d is [%g, %g] (need finite bounds, min <= max)", who, a, box_min[a],
                        box_max[a]);
        if (toward && !std::isfinite(toward[a]))
            return fail(MVS_ERR_BAD_SHAPE, "%s: toward[%d] = %g (need finite numbers)", who, a, toward[a]);
    }
    if (int rc = check_xyz_dtype(who, dtype)) return rc;
    const int K = num_candidates;
    if (int rc = check_workspace8(who, workspace, workspace_bytes, planes_workspace(P, K))) return rc;

    PlanesParams O{};
    O.xyz = xyz;
    O.P = (int)P;
    O.K = K;
    O.K64 = planes_k64(K);
    O.max_planes = max_planes;
    for (int a = 0; a < 3; ++a) {
        O.bmin[a] = box_min[a];
        O.bmax[a] = box_max[a];
        O.origin[a] = 0.5 * (box_min[a] + box_max[a]);
        O.toward[a] = toward ? toward[a] : 0.0;
    }
    O.has_toward = toward != nullptr;
    O.t = dist;
    O.seed = seed;
    O.min_inliers = min_inliers;
    O.n_tiles = (P + kCloudTile - 1) / kCloudTile;
    O.groups = (P + kPlanesGroup - 1) / kPlanesGroup;
    char* w = static_cast<char*>(workspace);
    O.aq = reinterpret_cast<double*>(w);
    w += 24 * (size_t)P;
    O.tiles = reinterpret_cast<int*>(w);
    w += planes_tiles_bytes(P);
    O.cand = reinterpret_cast<double*>(w);
    w += 8 * kPlanesCand * (size_t)O.K64;
    O.counts = reinterpret_cast<int*>(w);
    w += 4 * (size_t)O.K64;
    O.partials = reinterpret_cast<double*>(w);
    w += 8 * (size_t)kPlanesSums * (size_t)planes_partials(P);
    O.state = reinterpret_cast<PlanesState*>(w);
    O.planes_out = planes_out;
    O.rounds_out = rounds_out;
    O.counts_out = counts_out;
    O.labels_out = labels_out;
    O.cand_counts_out = cand_counts_out;
    O.sums_out = sums_out;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t rounds = (size_t)max_planes;

    if (int rc = check_hip(hipMemsetAsync(O.state, 0, MVS_PLANES_SCALARS, s), "zeroing the scalar block")) return rc;
    if (int rc = check_hip(hipMemsetAsync(planes_out, 0xFF, sizeof(double) * 4 * rounds, s), "filling the planes")) return rc;
    if (int rc = check_hip(hipMemsetAsync(rounds_out, 0xFF, sizeof(long long) * 4 * rounds, s), "filling the rounds")) return rc;
    if (cand_counts_out)
        if (int rc = check_hip(hipMemsetAsync(cand_counts_out, 0xFF, sizeof(int) * (size_t)K * rounds, s), "filling the counts"))
            return rc;
    if (sums_out)
        if (int rc = check_hip(hipMemsetAsync(sums_out, 0xFF, sizeof(double) * kPlanesSums * rounds, s), "filling the sums"))
            return rc;
    if (P > 0) {
        const bool f64 = dtype == MVS_CLOUD_F64;
        const int row_blocks = cloud_blocks(kLaunchRow, P), tile_blocks = cloud_blocks(kLaunchRowTile, P);
        // the count kernel loops over the tiles: its grid is capped at four blocks per compute unit, and by the tests' hook
        const long long cap = std::min<long long>(kPlanesCountBlocks, g_cloud_loop_cap.load(std::memory_order_relaxed));
        const int count_blocks = (int)std::min<long long>(tile_blocks, cap);
        const int cand_blocks = cloud_blocks(O.K64, kCloudThreads);
        const dim3 count_grid((unsigned)count_blocks, (unsigned)std::min(O.K64 / kPlanesChunk, kPlanesCountSplit));
        if (f64) PLANES_LAUNCH((planes_classify_kernel<double><<<row_blocks, kCloudThreads, 0, s>>>(O)), "planes_classify_kernel");
        else PLANES_LAUNCH((planes_classify_kernel<float><<<row_blocks, kCloudThreads, 0, s>>>(O)), "planes_classify_kernel");
        for (int r = 0; r < max_planes; ++r) {
            PLANES_LAUNCH((planes_tile_count_kernel<<<tile_blocks, kCloudThreads, 0, s>>>(O)), "planes_tile_count_kernel");
            PLANES_LAUNCH((planes_scan_kernel<<<1, kCloudScanWidth, 0, s>>>(O, r)), "planes_scan_kernel");
            if (f64) PLANES_LAUNCH((planes_emit_kernel<double><<<tile_blocks, kCloudThreads, 0, s>>>(O)), "planes_emit_kernel");
            else PLANES_LAUNCH((planes_emit_kernel<float><<<tile_blocks, kCloudThreads, 0, s>>>(O)), "planes_emit_kernel");
            PLANES_LAUNCH((planes_candidates_kernel<<<cand_blocks, kCloudThreads, 0, s>>>(O, r)), "planes_candidates_kernel");
            PLANES_LAUNCH((planes_count_kernel<<<count_grid, kCloudThreads, 0, s>>>(O)), "planes_count_kernel");
            PLANES_LAUNCH((planes_winner_kernel<<<1, kCloudScanWidth, 0, s>>>(O, r)), "planes_winner_kernel");
            if (f64) PLANES_LAUNCH((planes_sum0_kernel<double><<<row_blocks, kCloudThreads, 0, s>>>(O)), "planes_sum0_kernel");
            else PLANES_LAUNCH((planes_sum0_kernel<float><<<row_blocks, kCloudThreads, 0, s>>>(O)), "planes_sum0_kernel");
            const double* in = O.partials;
            for (long long L = O.groups; L > 1;) {
                const long long next = (L + kPlanesFanin - 1) / kPlanesFanin;      // <= 2^15 blocks: never capped
                double* out = const_cast<double*>(in) + (size_t)kPlanesSums * L;
                PLANES_LAUNCH((planes_sum_kernel<<<dim3((unsigned)cloud_blocks(L, kPlanesFanin), (unsigned)kPlanesSums),
                                                   kPlanesFanin, 0, s>>>(O.state, in, L, out, next)),
                              "planes_sum_kernel");
                in = out;
                L = next;
            }
            PLANES_LAUNCH((planes_fit_kernel<<<1, 1, 0, s>>>(O, in, r)), "planes_fit_kernel");
            if (f64) PLANES_LAUNCH((planes_label_kernel<double><<<tile_blocks, kCloudThreads, 0, s>>>(O, r)), "planes_label_kernel");
            else PLANES_LAUNCH((planes_label_kernel<float><<<tile_blocks, kCloudThreads, 0, s>>>(O, r)), "planes_label_kernel");
        }
    }
    PLANES_LAUNCH((planes_finish_kernel<<<1, 1, 0, s>>>(O, P > 0 ? 0 : MVS_PLANES_STOP_EXHAUSTED)), "planes_finish_kernel");
    return MVS_OK;
}

}  // extern "C"
