// cloud_normals.hip -- a normal for every point of a cloud inside a box from its k nearest neighbours (reference
// eval.py:817, pcd.estimate_normals()), as include/mvs_normals_abi.h defines it.
//
// The box bounds a dense grid of `cell`-sized cells.  Launches, ordered by the stream alone:
//   hipMemsetAsync          counts_out and the cell counters
//   normals_classify_kernel one thread per point: a non-member gets its zeros (and -1s), a member adds 1 to its cell
//   normals_tile_sum_kernel, normals_tile_scan_kernel <<<1>>>, normals_cell_scan_kernel
//                           the cell counts become exclusive offsets, in place
//   normals_scatter_kernel  one thread per member: claims the next slot of its cell (which turns the cell's offset into its
//                           END) and writes its index and its point, as doubles, there
//   normals_search_kernel   one WAVE per member, kNormalsPerWave members in turn: see below
// The order of the points inside a cell is whatever the atomics gave.  It cannot reach the output: the neighbours are the
// first min(knn, M) of a TOTAL order, (d2, index), every candidate that could be among them is examined, and the sums run
// over them in that order.
//
// The search keeps the 64 best candidates so far sorted over the 64 lanes of the wave, lane j holding the j-th: no array a
// thread would index dynamically, no LDS, no scratch.  A batch of 64 candidates is loaded one per lane; the lanes whose
// candidate beats the current knn-th are found with a ballot, and each of those is inserted in turn: its rank is the
// population count of a ballot, the lanes behind it shift up by one.  Rings of cells are taken in Chebyshev order around
// the member's cell; the (z, y) rows of a ring are looked up 64 at a time, one per lane, so the latency of the offset
// loads is paid once per 64 rows and empty rows cost nothing more.  After ring r the examined cells form a block; whatever
// lies outside it is at least as far as the block's nearest face that is not also the grid's, less a slack of
// kNormalsSlack cells + 2^-48 of the box's largest coordinate: the index of a point is the floor of a quotient that is off
// by at most 2^-52 of itself, i.e. by less than 2^-21 cells on a grid of fewer than 2^31, and a face bmin + k * cell is
// computed to 2^-52 of the box's largest coordinate, so the slack is conservative many times over.  The search ends when
// the knn-th candidate is strictly nearer than that, or when no face is left.
// Compiled with -ffp-contract=off: d2, the cell index and the sums are the header's fp64 restatement.
#include "mvs_normals_abi.h"
#include "mvs_internal.h"

#include <climits>
#include <cmath>

namespace mvs {

constexpr int kNormalsThreads = 256;
constexpr int kNormalsWaves = kNormalsThreads / 64;
constexpr int kNormalsPerWave = 8;                    // members one wave of the search kernel serves
constexpr int kNormalsTile = MVS_NORMALS_TILE;        // cells per block of the two tile kernels: 4 per thread
constexpr int kNormalsScanWidth = 1024;
constexpr int kNormalsSweeps = 8;
constexpr double kNormalsSlack = 1e-3;                // of a cell, see above
static_assert(MVS_NORMALS_KNN_MAX == 64, "one candidate per lane");
static_assert(kNormalsTile == 4 * kNormalsThreads, "four cells per thread");

struct NormalsParams {
    const void* xyz;
    const long long* view_starts;
    const double* centres;
    float* normals_out;
    int* nbr_out;
    long long* counts_out;
    double* sxyz;                  // [P][3]: the members' points, cell by cell
    int* sidx;                     // [P]: their indices
    int* cells_end;                // [cells]: counts, then exclusive offsets, then (after the scatter) each cell's end
    int* tiles;                    // [n_tiles + 1]
    double bmin[3], bmax[3];
    double cell;
    double slack;                  // what a face of the examined block is pulled in by: kNormalsSlack cells + 2^-48 of the box
    int P, R, knn;
    int n[3];
    int cells, n_tiles;
};

template <typename T>
__device__ __forceinline__ bool normals_load(const NormalsParams& N, int i, double p[3]) {
    const T* src = static_cast<const T*>(N.xyz) + (size_t)i * 3;
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = (double)src[a];
        in = in && N.bmin[a] <= p[a] && p[a] <= N.bmax[a];      // false for NaN
    }
    return in;
}

// the header's cell of a member; at most n - 1 by the header's argument, the clamp only keeps an access inside the grid
__device__ __forceinline__ void normals_cell(const NormalsParams& N, const double p[3], int c[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double k = floor((p[a] - N.bmin[a]) / N.cell);
        c[a] = k >= (double)(N.n[a] - 1) ? N.n[a] - 1 : k > 0.0 ? (int)k : 0;
    }
}
__device__ __forceinline__ int normals_linear(const NormalsParams& N, int x, int y, int z) {
    return (z * N.n[1] + y) * N.n[0] + x;      // < cells < 2^31
}

template <typename T>
__global__ void __launch_bounds__(kNormalsThreads) normals_classify_kernel(NormalsParams N) {
    const long long i = (long long)blockIdx.x * kNormalsThreads + threadIdx.x;
    double p[3];
    const bool valid = i < N.P;
    const bool member = valid && normals_load<T>(N, (int)i, p);
    if (member) {
        int c[3];
        normals_cell(N, p, c);
        __hip_atomic_fetch_add(&N.cells_end[normals_linear(N, c[0], c[1], c[2])], 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    } else if (valid) {
#pragma unroll
        for (int a = 0; a < 3; ++a) N.normals_out[(size_t)i * 3 + a] = 0.0f;
        if (N.nbr_out)
            for (int j = 0; j < N.knn; ++j) N.nbr_out[(size_t)i * N.knn + j] = -1;
    }
    const int members = __popcll(__ballot(member));
    if ((threadIdx.x & 63) == 0 && members)
        __hip_atomic_fetch_add(&N.counts_out[0], (long long)members, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int normals_count(const NormalsParams& N, long long cell) {
    return cell < N.cells ? N.cells_end[cell] : 0;
}

__global__ void __launch_bounds__(kNormalsThreads) normals_tile_sum_kernel(NormalsParams N) {
    __shared__ int wave_sum[kNormalsWaves];
    const long long base = (long long)blockIdx.x * kNormalsTile + 4 * threadIdx.x;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += normals_count(N, base + k);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int wv = 0; wv < kNormalsWaves; ++wv) t += wave_sum[wv];
        N.tiles[blockIdx.x] = t;
    }
}

// exclusive scan of the tile sums with a running carry (the pattern of cloud_scan_kernel); tiles[n_tiles] = M
__global__ void __launch_bounds__(kNormalsScanWidth) normals_tile_scan_kernel(NormalsParams N) {
    __shared__ int wave_total[kNormalsScanWidth / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (long long base = 0; base < N.n_tiles; base += kNormalsScanWidth) {
        const long long i = base + tid;
        const int v = i < N.n_tiles ? N.tiles[i] : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int wv = 0; wv < kNormalsScanWidth / 64; ++wv) {
            const int c = wave_total[wv];
            before += wv < wave ? c : 0;
            total += c;
        }
        if (i < N.n_tiles) N.tiles[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) N.tiles[N.n_tiles] = carry;
}

__global__ void __launch_bounds__(kNormalsThreads) normals_cell_scan_kernel(NormalsParams N) {
    __shared__ int wave_total[kNormalsWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kNormalsTile + 4 * threadIdx.x;
    int v[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = normals_count(N, base + k);
        mine += v[k];
    }
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int run = N.tiles[blockIdx.x] + incl - mine;
#pragma unroll
    for (int wv = 0; wv < kNormalsWaves; ++wv) run += wv < wave ? wave_total[wv] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < N.cells) N.cells_end[base + k] = run;
        run += v[k];
    }
}

template <typename T>
__global__ void __launch_bounds__(kNormalsThreads) normals_scatter_kernel(NormalsParams N) {
    const long long i = (long long)blockIdx.x * kNormalsThreads + threadIdx.x;
    double p[3];
    if (i >= N.P || !normals_load<T>(N, (int)i, p)) return;
    int c[3];
    normals_cell(N, p, c);
    const int slot = __hip_atomic_fetch_add(&N.cells_end[normals_linear(N, c[0], c[1], c[2])], 1, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
    if (slot < 0 || slot >= N.P) return;       // cannot happen: the classify pass counted this very point into this very cell
    N.sidx[slot] = (int)i;
#pragma unroll
    for (int a = 0; a < 3; ++a) N.sxyz[(size_t)slot * 3 + a] = p[a];
}

// ---- wave-level helpers: values that are the same in every lane are read with readlane, `lane` wave-uniform
__device__ __forceinline__ int lane_int(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double lane_double(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ bool key_less(double d2a, int ia, double d2b, int ib) {
    return d2a < d2b || (d2a == d2b && ia < ib);
}

// the sorted list of the 64 best: lane j holds the j-th smallest (d2, idx); (inf, INT_MAX) where nothing is yet
struct NormalsList {
    double d2;
    int idx;
    double kth_d2;     // the knn-th entry, the same in every lane
    int kth_idx;
};

// the candidates [a, b) of the sorted arrays against the list.  The clamps and the index test cannot bite (the offsets
// are a scan of the very counts the scatter fills); they keep every access inside the buffers whatever the offsets hold.
__device__ __forceinline__ void normals_take(const NormalsParams& N, NormalsList& L, const double p[3], int a, int b) {
    const int lane = threadIdx.x & 63;
    a = a < 0 ? 0 : a;
    b = b > N.P ? N.P : b;
    for (int base = a; base < b; base += 64) {
        const int j = base + lane;
        double d2 = INFINITY;
        int idx = INT_MAX;
        if (j < b) {
            const double* q = N.sxyz + (size_t)j * 3;
            const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
            d2 = (dx * dx + dy * dy) + dz * dz;
            idx = N.sidx[j];
        }
        const bool real = j < b && idx >= 0 && idx < N.P;
        unsigned long long better = __ballot(real && key_less(d2, idx, L.kth_d2, L.kth_idx));
        while (better) {
            const int src = __builtin_ctzll(better);
            better &= better - 1;
            const double cd = lane_double(d2, src);
            const int ci = lane_int(idx, src);
            if (!key_less(cd, ci, L.kth_d2, L.kth_idx)) continue;      // the list has moved on since the ballot
            const int pos = __popcll(__ballot(key_less(L.d2, L.idx, cd, ci)));
            const double up_d2 = __shfl_up(L.d2, 1);
            const int up_idx = __shfl_up(L.idx, 1);
            if (lane > pos) {
                L.d2 = up_d2;
                L.idx = up_idx;
            } else if (lane == pos) {
                L.d2 = cd;
                L.idx = ci;
            }
            L.kth_d2 = lane_double(L.d2, N.knn - 1);
            L.kth_idx = lane_int(L.idx, N.knn - 1);
        }
    }
}

// first slot of cell `lin` after the scatter: the end of the cell before it
__device__ __forceinline__ int normals_begin(const NormalsParams& N, int lin) { return lin > 0 ? N.cells_end[lin - 1] : 0; }

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

template <typename T>
__global__ void __launch_bounds__(kNormalsThreads) normals_search_kernel(NormalsParams N) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int M = N.tiles[N.n_tiles] < N.P ? N.tiles[N.n_tiles] : N.P;
    const int m = M < N.knn ? M : N.knn;        // neighbours of every member
    long long estimated = 0, uncertified = 0;
    for (int t = 0; t < kNormalsPerWave; ++t) {
        const long long s = ((long long)blockIdx.x * kNormalsWaves + wave) * kNormalsPerWave + t;
        if (s >= M) break;
        const int i = N.sidx[s];
        if (i < 0 || i >= N.P) continue;        // cannot happen: the scatter filled every slot below M
        double p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = N.sxyz[(size_t)s * 3 + a];
        int c[3];
        normals_cell(N, p, c);
        NormalsList L{INFINITY, INT_MAX, INFINITY, INT_MAX};
        for (int r = 0;; ++r) {
            // the ring's block of cells, clipped to the grid.  r stays below the longest axis (the loop ends once the block
            // covers the grid) and every test is written so that no sum of two of c, r and n is formed unless it fits
            const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = r < N.n[0] - 1 - c[0] ? c[0] + r : N.n[0] - 1;
            const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = r < N.n[1] - 1 - c[1] ? c[1] + r : N.n[1] - 1;
            const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = r < N.n[2] - 1 - c[2] ? c[2] + r : N.n[2] - 1;
            const int hy = y1 - y0 + 1, rows = (z1 - z0 + 1) * hy;       // <= cells
            for (int row = 0; row < rows; row = rows - row > 64 ? row + 64 : rows) {
                // lane -> one (z, y) row of the block: the whole x span on the ring's z and y faces, its two end cells else
                const int q = lane < rows - row ? row + lane : row;       // never past rows: it may be close to 2^31
                const int z = z0 + q / hy, y = y0 + q % hy;
                const int dz = z - c[2], dy = y - c[1];
                int a0 = 0, b0 = 0, a1 = 0, b1 = 0;
                if (lane < rows - row) {
                    const int line = normals_linear(N, 0, y, z);
                    if (dz == -r || dz == r || dy == -r || dy == r) {
                        a0 = normals_begin(N, line + x0);
                        b0 = N.cells_end[line + x1];
                    } else {
                        if (c[0] - r >= 0) {
                            a0 = normals_begin(N, line + c[0] - r);
                            b0 = N.cells_end[line + c[0] - r];
                        }
                        if (r < N.n[0] - c[0]) {
                            a1 = normals_begin(N, line + c[0] + r);
                            b1 = N.cells_end[line + c[0] + r];
                        }
                    }
                }
                unsigned long long busy = __ballot(b0 > a0);
                while (busy) {
                    const int src = __builtin_ctzll(busy);
                    busy &= busy - 1;
                    normals_take(N, L, p, lane_int(a0, src), lane_int(b0, src));
                }
                busy = __ballot(b1 > a1);
                while (busy) {
                    const int src = __builtin_ctzll(busy);
                    busy &= busy - 1;
                    normals_take(N, L, p, lane_int(a1, src), lane_int(b1, src));
                }
            }
            // the nearest face of the examined block that has cells behind it
            double face = INFINITY;
            bool open = false;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (c[a] - r > 0) {
                    const double d = p[a] - (N.bmin[a] + (double)(c[a] - r) * N.cell);
                    face = d < face ? d : face;
                    open = true;
                }
                if (r < N.n[a] - 1 - c[a]) {
                    const double d = (N.bmin[a] + (double)(c[a] + r + 1) * N.cell) - p[a];      // c + r + 1 <= n - 1
                    face = d < face ? d : face;
                    open = true;
                }
            }
            if (!open) break;
            const double safe = face - N.slack;
            if (safe > 0.0 && L.kth_d2 < safe * safe) break;
        }
        // ---- lanes 0 .. m-1 hold the neighbours in order
        if (N.nbr_out && lane < N.knn) N.nbr_out[(size_t)i * N.knn + lane] = lane < m ? L.idx : -1;
        double q[3] = {0.0, 0.0, 0.0};
        if (lane < m && L.idx != INT_MAX) {
            double tmp[3];
            normals_load<T>(N, L.idx, tmp);
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
            const double dl = p[a] - N.bmin[a], dh = N.bmax[a] - p[a];
            f = dl < f ? dl : f;
            f = dh < f ? dh : f;
        }
        const double last = lane_double(L.d2, m - 1);     // m >= 1: this member itself
        if (m < N.knn || last > f * f) ++uncertified;
    }
    if (lane == 0) {
        if (estimated)
            __hip_atomic_fetch_add(&N.counts_out[1], estimated, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (uncertified)
            __hip_atomic_fetch_add(&N.counts_out[2], uncertified, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// n[a] and their product; BAD_SHAPE for anything the header refuses about P, the box and the cell
static int normals_check(const char* who, long long P, const double* bmin, const double* bmax, double cell, int n[3],
                         long long* cells) {
    if (P < 0 || P >= (1LL << 31)) return fail(MVS_ERR_BAD_SHAPE, "%s: P = %lld (need 0 <= P < 2^31)", who, P);
    if (!std::isfinite(cell) || cell <= 0.0)
        return fail(MVS_ERR_BAD_SHAPE, "%s: cell = %g (need a finite size > 0)", who, cell);
    long long c = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(bmin[a]) || !std::isfinite(bmax[a]) || bmin[a] > bmax[a])
            return fail(MVS_ERR_BAD_SHAPE, "%s: box axis %d is [%g, %g] (need finite bounds, min <= max)", who, a, bmin[a],
                        bmax[a]);
        const double na = std::floor((bmax[a] - bmin[a]) / cell) + 1.0;
        if (!(na < 2147483648.0))          // also an infinite quotient
            return fail(MVS_ERR_BAD_SHAPE, "%s: axis %d needs %g cells (the grid must have fewer than 2^31 cells)", who, a, na);
        n[a] = (int)na;
        c *= n[a];                         // < 2^31 before this factor, so < 2^62 after it
        if (c >= (1LL << 31))
            return fail(MVS_ERR_BAD_SHAPE, "%s: the grid of the box at cell %g has 2^31 cells or more", who, cell);
    }
    *cells = c;
    return MVS_OK;
}

static long long normals_tiles(long long cells) { return (cells + kNormalsTile - 1) / kNormalsTile; }
static size_t normals_workspace(long long P, long long cells) {
    return 24 * (size_t)P + 8 * (size_t)((P + 1) / 2) + 8 * (size_t)((cells + 1) / 2) +
           8 * (size_t)((normals_tiles(cells) + 2) / 2);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_normals_workspace(long long P, const double box_min[3], const double box_max[3], double cell, size_t* bytes) {
    if (!bytes || !box_min || !box_max) return fail(MVS_ERR_NULL, "mvs_query_normals_workspace: NULL argument");
    int n[3];
    long long cells;
    if (int rc = normals_check("mvs_query_normals_workspace", P, box_min, box_max, cell, n, &cells)) return rc;
    *bytes = normals_workspace(P, cells);
    return MVS_OK;
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
    if (int rc = normals_check("mvs_cloud_normals", P, box_min, box_max, cell, n, &cells)) return rc;
    if (knn < 3 || knn > MVS_NORMALS_KNN_MAX)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_cloud_normals: knn = %d (need 3 <= knn <= %d)", knn, MVS_NORMALS_KNN_MAX);
    if (xyz_dtype != MVS_CLOUD_F32 && xyz_dtype != MVS_CLOUD_F64)
        return fail(MVS_ERR_BAD_DTYPE, "mvs_cloud_normals: xyz dtype %d (MVS_CLOUD_F32 or MVS_CLOUD_F64)", xyz_dtype);
    const size_t need = normals_workspace(P, cells);
    if (workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 8)
        return fail(MVS_ERR_WORKSPACE, "mvs_cloud_normals: workspace of %zu bytes at %p, need %zu (8-byte aligned)",
                    workspace_bytes, workspace, need);
    NormalsParams N{};
    N.xyz = xyz;
    N.view_starts = view_starts;
    N.centres = centres;
    N.normals_out = normals_out;
    N.nbr_out = nbr_out;
    N.counts_out = counts_out;
    char* ws = static_cast<char*>(workspace);
    N.sxyz = reinterpret_cast<double*>(ws);
    N.sidx = reinterpret_cast<int*>(ws + 24 * (size_t)P);
    N.cells_end = reinterpret_cast<int*>(ws + 24 * (size_t)P + 8 * (size_t)((P + 1) / 2));
    N.tiles = reinterpret_cast<int*>(reinterpret_cast<char*>(N.cells_end) + 8 * (size_t)((cells + 1) / 2));
    for (int a = 0; a < 3; ++a) {
        N.bmin[a] = box_min[a];
        N.bmax[a] = box_max[a];
        N.n[a] = n[a];
    }
    N.cell = cell;
    double far = 0.0;
    for (int a = 0; a < 3; ++a) far = std::fmax(far, std::fmax(std::fabs(box_min[a]), std::fabs(box_max[a])));
    N.slack = kNormalsSlack * cell + far * 0x1p-48;
    N.P = (int)P;
    N.R = R;
    N.knn = knn;
    N.cells = (int)cells;
    N.n_tiles = (int)normals_tiles(cells);
    const bool f64 = xyz_dtype == MVS_CLOUD_F64;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = check_hip(hipMemsetAsync(counts_out, 0, 3 * sizeof(long long), s), "zeroing the counts")) return rc;
    if (P == 0) return MVS_OK;
    if (int rc = check_hip(hipMemsetAsync(N.cells_end, 0, sizeof(int) * (size_t)cells, s), "zeroing the cell counts"))
        return rc;
    const int blocks = (int)((P + kNormalsThreads - 1) / kNormalsThreads);
    if (f64) normals_classify_kernel<double><<<blocks, kNormalsThreads, 0, s>>>(N);
    else normals_classify_kernel<float><<<blocks, kNormalsThreads, 0, s>>>(N);
    if (int rc = check_hip(hipGetLastError(), "normals_classify_kernel")) return rc;
    normals_tile_sum_kernel<<<N.n_tiles, kNormalsThreads, 0, s>>>(N);
    if (int rc = check_hip(hipGetLastError(), "normals_tile_sum_kernel")) return rc;
    normals_tile_scan_kernel<<<1, kNormalsScanWidth, 0, s>>>(N);
    if (int rc = check_hip(hipGetLastError(), "normals_tile_scan_kernel")) return rc;
    normals_cell_scan_kernel<<<N.n_tiles, kNormalsThreads, 0, s>>>(N);
    if (int rc = check_hip(hipGetLastError(), "normals_cell_scan_kernel")) return rc;
    if (f64) normals_scatter_kernel<double><<<blocks, kNormalsThreads, 0, s>>>(N);
    else normals_scatter_kernel<float><<<blocks, kNormalsThreads, 0, s>>>(N);
    if (int rc = check_hip(hipGetLastError(), "normals_scatter_kernel")) return rc;
    const int per_block = kNormalsWaves * kNormalsPerWave;
    const int search_blocks = (int)((P + per_block - 1) / per_block);
    if (f64) normals_search_kernel<double><<<search_blocks, kNormalsThreads, 0, s>>>(N);
    else normals_search_kernel<float><<<search_blocks, kNormalsThreads, 0, s>>>(N);
    return check_hip(hipGetLastError(), "normals_search_kernel");
}

}  // extern "C"
