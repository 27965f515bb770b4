// cloud_knn.h -- the exact k-nearest-neighbour search among the points of a cloud inside a box, shared by
// cloud_normals.hip (mvs_cloud_normals), cloud_outliers.hip (mvs_cloud_outliers) and cloud_distance.hip
// (mvs_cloud_distance): the cell grid and the ring search, as include/mvs_normals_abi.h describes them.  cloud_reduce.hip
// (mvs_cloud_reduce) uses the grid alone and walks the cells within a fixed reach itself.  Each user adds its
// own classify kernel (what a non-member gets) around knn_classify and its own search kernel (what is done with the
// neighbours) around knn_search -- the knn nearest members of a member -- or knn_nearest -- the one nearest member of a
// point anywhere in space, which is no member of the grid (include/mvs_distance_abi.h).
//
// The box bounds a dense grid of `cell`-sized cells.  Launches, ordered by the stream alone:
//   hipMemsetAsync          the cell counters (knn_build_begin)
//   the user's classify     one thread per point: knn_classify adds a member to its cell and to the count of members
//   knn_tile_sum_kernel, knn_tile_scan_kernel <<<1>>>, knn_cell_scan_kernel
//                           the cell counts become exclusive offsets, in place
//   knn_scatter_kernel      one thread per member: claims the next slot of its cell (which turns the cell's offset into its
//                           END) and writes its index and its point, as doubles, there (all four: knn_build_finish)
//   the user's search       one WAVE per member, kKnnPerWave members in turn: knn_search, see below.  Its grid is capped
//                           (cloud_common.h's kLaunchSearch): a block takes group blockIdx.x of kCloudWaves * kKnnPerWave
//                           members, then every gridDim.x-th, which is one trip below 32 * (2^24 - 1) points
// The order of the points inside a cell is whatever the atomics gave.  It cannot reach the output: the neighbours are the
// first min(knn, M) of a TOTAL order, (d2, index), every candidate that could be among them is examined, and the users' sums
// run over them in that order.
//
// The search keeps the 64 best candidates so far sorted over the 64 lanes of the wave, lane j holding the j-th: no array a
// thread would index dynamically, no LDS, no scratch.  A batch of 64 candidates is loaded one per lane; the lanes whose
// candidate beats the current knn-th are found with a ballot, and each of those is inserted in turn: its rank is the
// population count of a ballot, the lanes behind it shift up by one.  Rings of cells are taken in Chebyshev order around
// the member's cell; the (z, y) rows of a ring are looked up 64 at a time, one per lane, so the latency of the offset
// loads is paid once per 64 rows and empty rows cost nothing more.  After ring r the examined cells form a block; whatever
// lies outside it is at least as far as the block's nearest face that is not also the grid's, less a slack of
// kKnnSlack cells + 2^-48 of the box's largest coordinate: the index of a point is the floor of a quotient that is off
// by at most 2^-52 of itself, i.e. by less than 2^-21 cells on a grid of fewer than 2^31, and a face bmin + k * cell is
// computed to 2^-52 of the box's largest coordinate, so the slack is conservative many times over.  The search ends when
// the knn-th candidate is strictly nearer than that, or when no face is left.
// All users are compiled with -ffp-contract=off: d2 and the cell index are the header's fp64 restatement.
// knn_nearest keeps no list: each lane holds the best (d2, index) of the candidates it loaded; a ballot closes every ring
// and one minimum over the wave the search.  Both searches walk the same rings (knn_walk).
// The kernels here are static: each translation unit that includes this header carries its own copy of them.  The tile
// scan's loop, the in-box load, the grid check and the refusals are cloud_common.h's, shared with the fuse and the downsample.
#pragma once

#include "cloud_common.h"

#include <climits>

namespace mvs {

constexpr double kKnnSlack = 1e-3;                // of a cell, see above (kKnnPerWave, kKnnGroup: cloud_common.h)
static_assert(MVS_NORMALS_KNN_MAX == 64, "one candidate per lane");
static_assert(kCloudTile == 4 * kCloudThreads, "four cells per thread");

struct KnnGrid {
    const void* xyz;
    double* sxyz;                  // [P][3]: the members' points, cell by cell
    int* sidx;                     // [P]: their indices
    int* cells_end;                // [cells]: counts, then exclusive offsets, then (after the scatter) each cell's end
    int* tiles;                    // [n_tiles + 1]
    double bmin[3], bmax[3];
    double cell;
    double slack;                  // what a face of the examined block is pulled in by: kKnnSlack cells + 2^-48 of the box
    int P, knn;
    int n[3];
    int cells, n_tiles;
};

// the header's cell of a member; at most n - 1 by the header's argument, the clamp only keeps an access inside the grid
__device__ __forceinline__ void knn_cell(const KnnGrid& G, const double p[3], int c[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double k = floor((p[a] - G.bmin[a]) / G.cell);
        c[a] = k >= (double)(G.n[a] - 1) ? G.n[a] - 1 : k > 0.0 ? (int)k : 0;
    }
}
__device__ __forceinline__ int knn_linear(const KnnGrid& G, int x, int y, int z) {
    return (z * G.n[1] + y) * G.n[0] + x;      // < cells < 2^31
}

// the body of a classify kernel of kCloudThreads threads, one per point, called by every thread of the block: is point i a
// member?  A member is counted into its cell, and the members of each wave into *members, with integer atomics.
template <typename T>
__device__ __forceinline__ bool knn_classify(const KnnGrid& G, long long i, long long* members) {
    double p[3];
    const bool member = i < G.P && box_load<T>(G.xyz, G.bmin, G.bmax, (int)i, p);
    if (member) {
        int c[3];
        knn_cell(G, p, c);
        __hip_atomic_fetch_add(&G.cells_end[knn_linear(G, c[0], c[1], c[2])], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int count = __popcll(__ballot(member));
    if ((threadIdx.x & 63) == 0 && count)
        __hip_atomic_fetch_add(members, (long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return member;
}

__device__ __forceinline__ int knn_count(const KnnGrid& G, long long cell) {
    return cell < G.cells ? G.cells_end[cell] : 0;
}

static __global__ void __launch_bounds__(kCloudThreads) knn_tile_sum_kernel(KnnGrid G) {
    __shared__ int wave_sum[kCloudWaves];
    const long long base = (long long)blockIdx.x * kCloudTile + 4 * threadIdx.x;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += knn_count(G, base + k);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int wv = 0; wv < kCloudWaves; ++wv) t += wave_sum[wv];
        G.tiles[blockIdx.x] = t;
    }
}

// exclusive scan of the tile sums; tiles[n_tiles] = M
static __global__ void __launch_bounds__(kCloudScanWidth) knn_tile_scan_kernel(KnnGrid G) {
    const int carry = tile_scan_exclusive<kCloudScanWidth>(G.tiles, G.n_tiles);
    if (threadIdx.x == 0) G.tiles[G.n_tiles] = carry;
}

static __global__ void __launch_bounds__(kCloudThreads) knn_cell_scan_kernel(KnnGrid G) {
    __shared__ int wave_total[kCloudWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kCloudTile + 4 * threadIdx.x;
    int v[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = knn_count(G, base + k);
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
    int run = G.tiles[blockIdx.x] + incl - mine;
#pragma unroll
    for (int wv = 0; wv < kCloudWaves; ++wv) run += wv < wave ? wave_total[wv] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < G.cells) G.cells_end[base + k] = run;
        run += v[k];
    }
}

template <typename T>
static __global__ void __launch_bounds__(kCloudThreads) knn_scatter_kernel(KnnGrid G) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    double p[3];
    if (i >= G.P || !box_load<T>(G.xyz, G.bmin, G.bmax, (int)i, p)) return;
    int c[3];
    knn_cell(G, p, c);
    const int slot = __hip_atomic_fetch_add(&G.cells_end[knn_linear(G, c[0], c[1], c[2])], 1, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
    if (slot < 0 || slot >= G.P) return;       // cannot happen: the classify pass counted this very point into this very cell
    G.sidx[slot] = (int)i;
#pragma unroll
    for (int a = 0; a < 3; ++a) G.sxyz[(size_t)slot * 3 + a] = p[a];
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
struct KnnList {
    double d2;
    int idx;
    double kth_d2;     // the knn-th entry, the same in every lane
    int kth_idx;
};

// the candidates [a, b) of the sorted arrays against the list.  The clamps and the index test cannot bite (the offsets
// are a scan of the very counts the scatter fills); they keep every access inside the buffers whatever the offsets hold.
__device__ __forceinline__ void knn_take(const KnnGrid& G, KnnList& L, const double p[3], int a, int b) {
    const int lane = threadIdx.x & 63;
    a = a < 0 ? 0 : a;
    b = b > G.P ? G.P : b;
    for (int base = a; base < b; base += 64) {
        const int j = base + lane;
        double d2 = INFINITY;
        int idx = INT_MAX;
        if (j < b) {
            const double* q = G.sxyz + (size_t)j * 3;
            const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
            d2 = (dx * dx + dy * dy) + dz * dz;
            idx = G.sidx[j];
        }
        const bool real = j < b && idx >= 0 && idx < G.P;
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
            L.kth_d2 = lane_double(L.d2, G.knn - 1);
            L.kth_idx = lane_int(L.idx, G.knn - 1);
        }
    }
}

// first slot of cell `lin` after the scatter: the end of the cell before it
__device__ __forceinline__ int knn_begin(const KnnGrid& G, int lin) { return lin > 0 ? G.cells_end[lin - 1] : 0; }

// M as the tile scan left it, never more than P
__device__ __forceinline__ int knn_members(const KnnGrid& G) { return G.tiles[G.n_tiles] < G.P ? G.tiles[G.n_tiles] : G.P; }

// The rings of cells around the cell of p, in Chebyshev order, called by a whole wave with p wave-uniform.  p may lie
// anywhere: knn_cell clamps, so a point outside the box starts at the cell nearest to it.  take(a, b) is called by the
// whole wave with one span [a, b) of the sorted arrays PER LANE (empty where b <= a): the spans that up to 64 rows of ring
// r add; how the lanes share the work is the user's.  done(safe) closes ring r: every member not yet handed to take() is
// at least `safe` away from p on one axis (+inf once the block covers the grid), and a true return ends the walk.  `slack` is what a face is pulled in by: G.slack for a point of the box, see knn_nearest
// for any other.
//
// Why `safe` is a lower bound wherever p lies.  After ring r the examined block is [c - r, c + r] per axis, clipped to
// the grid.  A side of an axis is OPEN when cells lie beyond it.  Low side, open iff c - r > 0: a member beyond it has
// a cell index below c - r, so its coordinate is below F = bmin + (c - r) * cell (give or take the slack), and p[a] - F
// bounds its offset from below provided p[a] >= F.  That holds for p inside the box (c is p's own cell) and for p above
// the box (c = n - 1 and p[a] > bmax >= F); for p below the box c = 0, so the side is never open.  High side, open iff
// c + r < n - 1, F = bmin + (c + r + 1) * cell: the mirror image, p above the box has c = n - 1 and the side closed, p
// below the box has p[a] < bmin <= F.  So a clamped axis has its near side closed and its far side farther than the
// true offset of every member behind it, and the smallest open face remains a lower bound of the distance.
template <typename Take, typename Done>
__device__ __forceinline__ void knn_walk(const KnnGrid& G, const double p[3], double slack, Take take, Done done) {
    const int lane = threadIdx.x & 63;
    int c[3];
    knn_cell(G, p, c);
    for (int r = 0;; ++r) {
        // the ring's block of cells, clipped to the grid.  r stays below the longest axis (the loop ends once the block
        // covers the grid) and every test is written so that no sum of two of c, r and n is formed unless it fits
        const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = r < G.n[0] - 1 - c[0] ? c[0] + r : G.n[0] - 1;
        const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = r < G.n[1] - 1 - c[1] ? c[1] + r : G.n[1] - 1;
        const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = r < G.n[2] - 1 - c[2] ? c[2] + r : G.n[2] - 1;
        const int hy = y1 - y0 + 1, rows = (z1 - z0 + 1) * hy;       // <= cells
        for (int row = 0; row < rows; row = rows - row > 64 ? row + 64 : rows) {
            // lane -> one (z, y) row of the block: the whole x span on the ring's z and y faces, its two end cells else
            const int q = lane < rows - row ? row + lane : row;       // never past rows: it may be close to 2^31
            const int z = z0 + q / hy, y = y0 + q % hy;
            const int dz = z - c[2], dy = y - c[1];
            int a0 = 0, b0 = 0, a1 = 0, b1 = 0;
            if (lane < rows - row) {
                const int line = knn_linear(G, 0, y, z);
                if (dz == -r || dz == r || dy == -r || dy == r) {
                    a0 = knn_begin(G, line + x0);
                    b0 = G.cells_end[line + x1];
                } else {
                    if (c[0] - r >= 0) {
                        a0 = knn_begin(G, line + c[0] - r);
                        b0 = G.cells_end[line + c[0] - r];
                    }
                    if (r < G.n[0] - c[0]) {
                        a1 = knn_begin(G, line + c[0] + r);
                        b1 = G.cells_end[line + c[0] + r];
                    }
                }
            }
            take(a0, b0);
            take(a1, b1);
        }
        // the nearest face of the examined block that has cells behind it
        double face = INFINITY;
        bool open = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) {
                const double d = p[a] - (G.bmin[a] + (double)(c[a] - r) * G.cell);
                face = d < face ? d : face;
                open = true;
            }
            if (r < G.n[a] - 1 - c[a]) {
                const double d = (G.bmin[a] + (double)(c[a] + r + 1) * G.cell) - p[a];      // c + r + 1 <= n - 1
                face = d < face ? d : face;
                open = true;
            }
        }
        if (done(face - slack) || !open) break;
    }
}

// The ring search for the member at p, called by a whole wave with p wave-uniform.  On return lane j of L holds the j-th
// smallest (d2, idx) over ALL members for j < min(knn, M); the lanes behind hold whatever else was seen, or (inf, INT_MAX).
__device__ __forceinline__ void knn_search(const KnnGrid& G, const double p[3], KnnList& L) {
    L = KnnList{INFINITY, INT_MAX, INFINITY, INT_MAX};
    knn_walk(G, p, G.slack,
             [&](int a, int b) {       // one span at a time, the whole wave on it: the list is the wave's
                 unsigned long long busy = __ballot(b > a);
                 while (busy) {
                     const int src = __builtin_ctzll(busy);
                     busy &= busy - 1;
                     knn_take(G, L, p, lane_int(a, src), lane_int(b, src));
                 }
             },
             [&](double safe) { return safe > 0.0 && L.kth_d2 < safe * safe; });
}

// d2 of the box's nearest point to q, in the operation order of a member's d2.  No member is nearer, not even in the
// rounded arithmetic: for q[a] < bmin[a] <= r[a] the exact r[a] - q[a] is at least bmin[a] - q[a], rounding is monotone, so
// is the square of a non-negative value, so is each of the two sums; likewise above the box.
__device__ __forceinline__ double knn_box_d2(const KnnGrid& G, const double q[3]) {
    double e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) e[a] = q[a] < G.bmin[a] ? G.bmin[a] - q[a] : q[a] > G.bmax[a] ? q[a] - G.bmax[a] : 0.0;
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// the smallest (d2, idx) of every lane's pair, in every lane: an xor butterfly over the wave
__device__ __forceinline__ void knn_wave_min(double& d2, int& idx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(d2, off);
        const int oi = __shfl_xor(idx, off);
        if (key_less(od, oi, d2, idx)) {
            d2 = od;
            idx = oi;
        }
    }
}

// The nearest member to a point q anywhere in space (finite coordinates), called by a whole wave with q wave-uniform:
// the smallest (d2, idx) over ALL members whose d2 is finite, if that d2 <= max_d2; else (inf, INT_MAX).  The k = 1 form
// of the search: no sorted list, each lane keeps the best of the candidates it loaded.  The walk ends after ring r when
// the best d2 is strictly below safe^2, or max_d2 is, or no face is left; safe^2 is the larger of the face bound
// (knn_walk) and knn_box_d2.  "The best d2 of the wave is below safe^2" is "some lane's best is": one ballot closes a
// ring, and the one minimum over the wave on (d2, idx) closes the search.  A q farther than max_d2 from the box is
// answered before the first cell is read.
// The slack: q is not bounded by the box, so the rounding of a face distance p[a] - F, 2^-53 of |p[a]| + |F|, is covered by
// 2^-48 of q's largest coordinate on top of G.slack (which covers F and the cell index, see the head of this file).
__device__ __forceinline__ void knn_nearest(const KnnGrid& G, const double q[3], double max_d2, double& best_d2,
                                            int& best_idx) {
    const int lane = threadIdx.x & 63;
    best_d2 = INFINITY;
    best_idx = INT_MAX;
    const double box_d2 = knn_box_d2(G, q);
    if (max_d2 < box_d2) return;
    const double reach = fmax(fabs(q[0]), fmax(fabs(q[1]), fabs(q[2])));
    knn_walk(G, q, G.slack + reach * 0x1p-48,
             [&](int a, int b) {
                 // a lane's candidate j against its own best.  The index test cannot bite, see knn_take
                 auto candidate = [&](int j) {
                     const double* r = G.sxyz + (size_t)j * 3;
                     const double dx = r[0] - q[0], dy = r[1] - q[1], dz = r[2] - q[2];
                     const double d2 = (dx * dx + dy * dy) + dz * dz;
                     const int idx = G.sidx[j];
                     if (idx >= 0 && idx < G.P && d2 < INFINITY && key_less(d2, idx, best_d2, best_idx)) {
                         best_d2 = d2;
                         best_idx = idx;
                     }
                 };
                 unsigned long long busy = __ballot(b > a);
                 if (__popcll(busy) == 1) {          // one span (ring 0, or a grid of few cells): the whole wave on it
                     const int src = __builtin_ctzll(busy);
                     const int ga = lane_int(a, src), gb = lane_int(b, src);
                     for (int j = (ga > 0 ? ga : 0) + lane; j < (gb < G.P ? gb : G.P); j += 64) candidate(j);
                     return;
                 }
                 // the spans of a ring are short where the cloud is a surface, and each costs a round trip to memory: four
                 // at a time, one per group of kKnnGroup lanes.  No lane talks to another in here
                 while (busy) {
                     int sa = 0, sb = 0;
#pragma unroll
                     for (int g = 0; g < 64 / kKnnGroup; ++g) {
                         if (busy) {
                             const int src = __builtin_ctzll(busy);
                             busy &= busy - 1;
                             const int ga = lane_int(a, src), gb = lane_int(b, src);
                             if (lane / kKnnGroup == g) {
                                 sa = ga > 0 ? ga : 0;
                                 sb = gb < G.P ? gb : G.P;
                             }
                         }
                     }
                     for (int j = sa + lane % kKnnGroup; j < sb; j += kKnnGroup) candidate(j);
                 }
             },
             [&](double safe) {
                 const double face2 = safe > 0.0 ? safe * safe : 0.0;
                 const double safe2 = face2 > box_d2 ? face2 : box_d2;
                 return __ballot(best_d2 < safe2) != 0 || max_d2 < safe2;
             });
    knn_wave_min(best_d2, best_idx);
    if (best_d2 > max_d2) {
        best_d2 = INFINITY;
        best_idx = INT_MAX;
    }
}

// ---- host side
static long long knn_tiles(long long cells) { return cloud_blocks(kLaunchCellTile, cells); }      // cells / 1024 <= 2^21: never capped
// mvs_query_normals_workspace: the sorted points and indices, the cells, the tiles
static size_t knn_workspace(long long P, long long cells) {
    return 24 * (size_t)P + 8 * (size_t)((P + 1) / 2) + 8 * (size_t)((cells + 1) / 2) + 8 * (size_t)((knn_tiles(cells) + 2) / 2);
}

// G over a workspace of knn_workspace(P, cells) bytes, for a box and a cell that passed grid_check
static void knn_bind(KnnGrid& G, const void* xyz, long long P, const double* box_min, const double* box_max, double cell,
                     int knn, const int n[3], long long cells, void* workspace) {
    G.xyz = xyz;
    char* ws = static_cast<char*>(workspace);
    G.sxyz = reinterpret_cast<double*>(ws);
    G.sidx = reinterpret_cast<int*>(ws + 24 * (size_t)P);
    G.cells_end = reinterpret_cast<int*>(ws + 24 * (size_t)P + 8 * (size_t)((P + 1) / 2));
    G.tiles = reinterpret_cast<int*>(reinterpret_cast<char*>(G.cells_end) + 8 * (size_t)((cells + 1) / 2));
    for (int a = 0; a < 3; ++a) {
        G.bmin[a] = box_min[a];
        G.bmax[a] = box_max[a];
        G.n[a] = n[a];
    }
    G.cell = cell;
    double far = 0.0;
    for (int a = 0; a < 3; ++a) far = std::fmax(far, std::fmax(std::fabs(box_min[a]), std::fabs(box_max[a])));
    G.slack = kKnnSlack * cell + far * 0x1p-48;
    G.P = (int)P;
    G.knn = knn;
    G.cells = (int)cells;
    G.n_tiles = (int)knn_tiles(cells);
}

static int knn_point_blocks(const KnnGrid& G) { return cloud_blocks(kLaunchRow, G.P); }
static int knn_tile_blocks(const KnnGrid& G) { return cloud_blocks(kLaunchCellTile, G.cells); }      // = G.n_tiles
static int knn_search_blocks(const KnnGrid& G) { return cloud_blocks(kLaunchSearch, G.P); }          // capped: the kernel loops

// before the user's classify kernel (P > 0)
static int knn_build_begin(const KnnGrid& G, hipStream_t s) {
    return check_hip(hipMemsetAsync(G.cells_end, 0, sizeof(int) * (size_t)G.cells, s), "zeroing the cell counts");
}

// after it: offsets, then the scatter
static int knn_build_finish(const KnnGrid& G, bool f64, hipStream_t s) {
    knn_tile_sum_kernel<<<knn_tile_blocks(G), kCloudThreads, 0, s>>>(G);
    if (int rc = check_hip(hipGetLastError(), "knn_tile_sum_kernel")) return rc;
    knn_tile_scan_kernel<<<1, kCloudScanWidth, 0, s>>>(G);
    if (int rc = check_hip(hipGetLastError(), "knn_tile_scan_kernel")) return rc;
    knn_cell_scan_kernel<<<knn_tile_blocks(G), kCloudThreads, 0, s>>>(G);
    if (int rc = check_hip(hipGetLastError(), "knn_cell_scan_kernel")) return rc;
    if (f64) knn_scatter_kernel<double><<<knn_point_blocks(G), kCloudThreads, 0, s>>>(G);
    else knn_scatter_kernel<float><<<knn_point_blocks(G), kCloudThreads, 0, s>>>(G);
    return check_hip(hipGetLastError(), "knn_scatter_kernel");
}

}  // namespace mvs
