// cloud_common.h -- what the cloud path's translation units share: fuse_points.hip, cloud_downsample.hip and, through
// cloud_knn.h, cloud_normals.hip, cloud_outliers.hip, cloud_distance.hip and cloud_reduce.hip.
//
// Device side, all inlined into the kernels that call them (the kernels keep their names and their launch order):
//   tile_scan_exclusive   the single-block exclusive scan with a running carry over tiles[0 .. n_tiles)
//   tile_count            the count half of the ballot compaction: how many flags of a block's tile are set
//   tile_ranks            the emit half: the output rank of every set flag, in (pass, wave, lane) order
//   box_load              a point as doubles, and whether it lies inside a box
// Host side: the block count of every launch (cloud_blocks, capped at HIP's limit; the capped kernels loop), the one check
// of P, the box and the grid's edge (grid_check), the xyz dtype and workspace refusals, and the body of a workspace query
// over such a grid.
// Everything is integer bookkeeping except box_load, which converts and compares: nothing here rounds.
#pragma once

#include "mvs_cloud_abi.h"
#include "mvs_fuse_abi.h"
#include "mvs_normals_abi.h"
#include "mvs_outliers_abi.h"

#include <atomic>

// ---- the launch geometry: plain C++, no HIP.  tests/cloud_launch_sweep.cpp defines MVS_CLOUD_GEOMETRY_ONLY and includes
// this part alone, with the host compiler, and asks it about every launch below at the ends of the ABI's domain.
namespace mvs {

// one block of a tile kernel: kCloudThreads threads cover a tile of kCloudTile elements in kCloudPasses passes, element
// (pass, wave, lane) in that order; the scan kernels are one block of kCloudScanWidth threads
constexpr int kCloudThreads = 256;
constexpr int kCloudWaves = kCloudThreads / 64;
constexpr int kCloudTile = 1024;
constexpr int kCloudPasses = kCloudTile / kCloudThreads;
constexpr int kCloudScanWidth = 1024;
constexpr int kCloudChunk = MVS_CLOUD_CHUNK;      // points one block of the downsample's crop pass covers
constexpr int kSumBlock = MVS_OUTLIERS_BLOCK;     // elements, and threads, of one block of cloud_sum.h's tree
constexpr int kKnnPerWave = 8;                    // members one wave of a search kernel serves in turn
constexpr int kKnnGroup = 16;                     // lanes that share one span in knn_nearest and in the wide reduce round
static_assert(MVS_FUSE_TILE == kCloudTile && MVS_CLOUD_TILE == kCloudTile && MVS_NORMALS_TILE == kCloudTile,
              "one tile size for fuse, downsample and the k-NN grid");
static_assert(MVS_FUSE_SCAN_WIDTH == kCloudScanWidth && MVS_CLOUD_SCAN_WIDTH == kCloudScanWidth, "one scan width");
static_assert(kCloudThreads % 64 == 0 && kCloudTile % kCloudThreads == 0 && kCloudScanWidth % 64 == 0, "whole waves");

// HIP launches no grid of 2^32 threads or more (gridDim.x * blockDim.x, the note at hipModuleLaunchKernel in
// hip_runtime_api.h), so a launch of kCloudThreads-thread blocks has at most this many of them
constexpr long long kCloudMaxBlocks = (1LL << 32) / kCloudThreads - 1;
static_assert(kCloudMaxBlocks == (1 << 24) - 1 && (kCloudMaxBlocks + 1) * kCloudThreads == (1LL << 32),
              "the cap is the last block count below 2^32 threads of kCloudThreads per block");

// THE block count of a cloud-path launch: `work` items, `per_block` of them per block and trip
inline int cloud_blocks(long long work, int per_block) {
    const long long needed = (work + per_block - 1) / per_block;
    return (int)(needed < kCloudMaxBlocks ? needed : kCloudMaxBlocks);
}

// Every launch of the cloud path whose grid grows with the problem (the single-block scans and scalar kernels are <<<1>>>).
// A launch with loops = true can be capped inside the ABI's domain (P, N, cells, R*h*w < 2^31): its kernel takes group
// blockIdx.x of its work, then every gridDim.x-th, which below the cap is one trip.  One with loops = false stays below
// the cap for every legal size, by the bound written next to it, and its kernel is one trip by construction.
enum CloudWork { kWorkRows, kWorkCells, kWorkFuseTiles };      // rows: the P points of a cloud or the N queries
struct CloudLaunch {
    const char* kernels;
    CloudWork work;
    int per_block;     // items one block takes per trip
    int threads;       // of a block
    bool loops;
};
// one thread per row: P / 256 <= 2^23.  The classify, scatter, mark, count, finish, select, accumulate, core, union and
// label kernels, and the reduce round with one lane per member
constexpr CloudLaunch kLaunchRow{"one thread per point or query", kWorkRows, kCloudThreads, kCloudThreads, false};
// one block per tile of cells or voxels: cells / 1024 <= 2^21.  knn_tile_sum, knn_cell_scan, cloud_count, cloud_emit
constexpr CloudLaunch kLaunchCellTile{"one block per tile of cells", kWorkCells, kCloudTile, kCloudThreads, false};
// one block per tile of point indices: P / 1024 <= 2^21.  cluster_flatten, cluster_number
constexpr CloudLaunch kLaunchRowTile{"one block per tile of points", kWorkRows, kCloudTile, kCloudThreads, false};
// cloud_crop_min: P / 1024 <= 2^21
constexpr CloudLaunch kLaunchChunk{"cloud_crop_min_kernel", kWorkRows, kCloudChunk, kCloudThreads, false};
// cloud_sum_kernel, every level of cloud_sum_tree: blocks of kSumBlock = 1024 threads, n / 1024 <= 2^21 < 2^22 - 1
constexpr CloudLaunch kLaunchSum{"cloud_sum_kernel", kWorkRows, kSumBlock, kSumBlock, false};
// one wave per member, kKnnPerWave in turn (cloud_knn.h's knn_search_blocks): capped above 32 * (2^24 - 1) points
constexpr CloudLaunch kLaunchSearch{"normals_search_kernel, outliers_search_kernel", kWorkRows, kCloudWaves * kKnnPerWave,
                                    kCloudThreads, true};
// the same shape over the N queries of mvs_cloud_distance
constexpr CloudLaunch kLaunchQuerySearch{"distance_search_kernel", kWorkRows, kCloudWaves * kKnnPerWave, kCloudThreads,
                                         true};
// reduce_round_kernel with kKnnGroup lanes per member (the test hook's form): capped from P = 2^28 - 15 on
constexpr CloudLaunch kLaunchRoundWide{"reduce_round_kernel, 16 lanes per member", kWorkRows, kCloudThreads / kKnnGroup,
                                       kCloudThreads, true};
// one block per tile of one view: R * ceil(h*w / 1024) tiles, capped from 2^24 tiles on (h = w = 1, R = 2^24)
constexpr CloudLaunch kLaunchFuseTile{"fuse_count_kernel, fuse_scatter_kernel", kWorkFuseTiles, 1, kCloudThreads, true};
constexpr CloudLaunch kCloudLaunches[] = {kLaunchRow, kLaunchCellTile, kLaunchRowTile,     kLaunchChunk,     kLaunchSum,
                                          kLaunchSearch, kLaunchQuerySearch, kLaunchRoundWide, kLaunchFuseTile};

// The hook of the tests, not part of the ABI (mvs_test_cloud_max_blocks, fuse_points.hip): a lower cap for the launches
// that loop, so that clouds of ordinary size go round those loops several times.  One variable for the whole library
inline std::atomic<long long> g_cloud_loop_cap{kCloudMaxBlocks};

inline long long cloud_groups(const CloudLaunch& L, long long work) { return (work + L.per_block - 1) / L.per_block; }
inline int cloud_blocks(const CloudLaunch& L, long long work) {
    const int blocks = cloud_blocks(work, L.per_block);
    const long long cap = L.loops ? g_cloud_loop_cap.load(std::memory_order_relaxed) : kCloudMaxBlocks;
    return blocks < cap ? blocks : (int)cap;
}
// Is the grid of launch L short of its work?  Then the launch takes the kernel's looping form; else the one-trip form,
// which is the kernel as it was before there was a cap
inline bool cloud_capped(const CloudLaunch& L, long long work) { return cloud_blocks(L, work) < cloud_groups(L, work); }
// how often the kernel of launch L goes round its block-stride loop at most
inline long long cloud_trips(const CloudLaunch& L, long long work) {
    if (!L.loops) return 1;
    const long long groups = cloud_groups(L, work), blocks = cloud_blocks(L, work);
    return blocks ? (groups + blocks - 1) / blocks : 0;
}

// the fuse's tiles: those of one view, and of the scan (R*h*w < 2^31, so neither wraps)
inline int cloud_fuse_tiles_per_view(int h, int w) { return (int)(((long long)h * w + kCloudTile - 1) / kCloudTile); }
inline long long cloud_fuse_tiles(int R, int h, int w) { return (long long)R * cloud_fuse_tiles_per_view(h, w); }

}  // namespace mvs

#ifndef MVS_CLOUD_GEOMETRY_ONLY

#include "mvs_internal.h"

#include <cmath>

namespace mvs {

// In-place exclusive scan of tiles[0 .. n_tiles), kWidth of them per pass with a running carry.  Called by all kWidth
// threads of a single block; returns the total in every thread.  tiles[n_tiles] is the caller's to write.  The last
// __syncthreads() of the loop orders a pass's wave_total against the next pass, not the stores to tiles[]: a caller that
// reads the offsets back synchronises again.
template <int kWidth>
__device__ __forceinline__ int tile_scan_exclusive(int* tiles, long long n_tiles) {
    __shared__ int wave_total[kWidth / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;           // elements before this pass; every thread holds the same value
    for (long long base = 0; base < n_tiles; base += kWidth) {
        const long long i = base + tid;
        const int v = i < n_tiles ? tiles[i] : 0;
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
        for (int wv = 0; wv < kWidth / 64; ++wv) {
            const int c = wave_total[wv];
            before += wv < wave ? c : 0;
            total += c;
        }
        if (i < n_tiles) tiles[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();     // wave_total is rewritten by the next pass
    }
    return carry;
}

// How many of a tile's flags are set: flag(pass) is this thread's element of that pass.  Called by all kThreads threads of
// the block; the sum is returned in thread 0 (0 elsewhere).
template <int kPasses, int kThreads, typename Flag>
__device__ __forceinline__ int tile_count(Flag flag) {
    __shared__ int wave_count[kThreads / 64];
    int n = 0;
#pragma unroll
    for (int i = 0; i < kPasses; ++i) n += __popcll(__ballot(flag(i)));
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = n;
    __syncthreads();
    int s = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int wv = 0; wv < kThreads / 64; ++wv) s += wave_count[wv];
    }
    return s;
}

// The same flags again, ranked: emit(pass, rank, set) is called once per pass with the number of set flags of this tile
// before this thread's element in (pass, wave, lane) order, and whether its own flag is set.
template <int kPasses, int kThreads, typename Flag, typename Emit>
__device__ __forceinline__ void tile_ranks(Flag flag, Emit emit) {
    constexpr int kWaves = kThreads / 64, kSlots = kPasses * kWaves;      // (pass, wave) groups of 64 elements in a tile
    __shared__ int slot_count[kSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long ballots[kPasses];
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        ballots[i] = __ballot(flag(i));
        if (lane == 0) slot_count[i * kWaves + wave] = __popcll(ballots[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPasses; ++i) {
        int before = 0;      // set flags of this tile in the (pass, wave) slots before this one
#pragma unroll
        for (int j = 0; j < kSlots; ++j) before += j < i * kWaves + wave ? slot_count[j] : 0;
        const unsigned long long b = ballots[i];
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        emit(i, before + rank, ((b >> lane) & 1ull) != 0);
    }
}

// point i of xyz ([P][3] of T) as doubles; is it inside the closed box?  The bounds are references to arrays, not pointers:
// known to be readable, so the three comparisons stay straight-line code
template <typename T>
__device__ __forceinline__ bool box_load(const void* xyz, const double (&bmin)[3], const double (&bmax)[3], int i,
                                         double p[3]) {
    const T* src = static_cast<const T*>(xyz) + (size_t)i * 3;
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = (double)src[a];
        in = in && bmin[a] <= p[a] && p[a] <= bmax[a];      // false for NaN
    }
    return in;
}

// ---- host side
// The two dense grids a box bounds: the downsample's voxels, floor(extent / edge + 0.5) + 2 per axis (the grid starts half
// a voxel below the smallest kept point), and the search's cells, floor(extent / edge) + 1.
struct GridKind {
    const char* edge;      // what the messages call the edge
    const char* cells;     // and the cells of one axis
    double round, extra;   // cells of an axis = floor(extent / edge + round) + extra
};
constexpr GridKind kVoxelGrid{"voxel_size", "voxels", 0.5, 2.0};
constexpr GridKind kCellGrid{"cell", "cells", 0.0, 1.0};

// n[a] and their product; BAD_SHAPE for anything the headers refuse about P, the box and the edge
static int grid_check(const char* who, const GridKind& kind, long long P, const double* bmin, const double* bmax,
                      double edge, int n[3], long long* cells) {
    if (P < 0 || P >= (1LL << 31)) return fail(MVS_ERR_BAD_SHAPE, "%s: P = %lld (need 0 <= P < 2^31)", who, P);
    if (!std::isfinite(edge) || edge <= 0.0)
        return fail(MVS_ERR_BAD_SHAPE, "%s: %s = %g (need a finite size > 0)", who, kind.edge, edge);
    long long c = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(bmin[a]) || !std::isfinite(bmax[a]) || bmin[a] > bmax[a])
            return fail(MVS_ERR_BAD_SHAPE, "%s: box axis %d is [%g, %g] (need finite bounds, min <= max)", who, a, bmin[a],
                        bmax[a]);
        const double na = std::floor((bmax[a] - bmin[a]) / edge + kind.round) + kind.extra;
        if (!(na < 2147483648.0))          // also an infinite quotient
            return fail(MVS_ERR_BAD_SHAPE, "%s: axis %d needs %g %s (the grid must have fewer than 2^31 cells)", who, a, na,
                        kind.cells);
        n[a] = (int)na;
        c *= n[a];                         // < 2^31 before this factor, so < 2^62 after it
        if (c >= (1LL << 31))
            return fail(MVS_ERR_BAD_SHAPE, "%s: the grid of the box at %s %g has 2^31 cells or more", who, kind.edge, edge);
    }
    *cells = c;
    return MVS_OK;
}

static int check_xyz_dtype(const char* who, int dtype) {
    if (dtype != MVS_CLOUD_F32 && dtype != MVS_CLOUD_F64)
        return fail(MVS_ERR_BAD_DTYPE, "%s: xyz dtype %d (MVS_CLOUD_F32 or MVS_CLOUD_F64)", who, dtype);
    return MVS_OK;
}

static int check_workspace8(const char* who, const void* workspace, size_t bytes, size_t need) {
    if (bytes < need || reinterpret_cast<uintptr_t>(workspace) % 8)
        return fail(MVS_ERR_WORKSPACE, "%s: workspace of %zu bytes at %p, need %zu (8-byte aligned)", who, bytes, workspace,
                    need);
    return MVS_OK;
}

// the body of an mvs_query_*_workspace over such a grid: NULL check, grid check, *bytes = formula(P, cells)
static int grid_query(const char* who, const GridKind& kind, long long P, const double* box_min, const double* box_max,
                      double edge, size_t* bytes, size_t (*formula)(long long P, long long cells)) {
    if (!bytes || !box_min || !box_max) return fail(MVS_ERR_NULL, "%s: NULL argument", who);
    int n[3];
    long long cells;
    if (int rc = grid_check(who, kind, P, box_min, box_max, edge, n, &cells)) return rc;
    *bytes = formula(P, cells);
    return MVS_OK;
}

}  // namespace mvs

#endif  // MVS_CLOUD_GEOMETRY_ONLY
