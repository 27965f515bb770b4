// cloud_downsample.hip -- crop a coloured point cloud to a box and keep one mean point per occupied voxel
// (reference eval.py:831-840: pcd.crop(bbox2), pcd.voxel_down_sample(voxel_size), pcd.scale(0.01)), as
// include/mvs_cloud_abi.h defines it.
//
// The box bounds the grid, so the grid is dense: one kCloudRecord-byte record per voxel in the workspace.  Launches,
// ordered by the stream alone:
//   cloud_crop_min_kernel    one block per kCloudChunk points: in-box test, per-axis minimum and count of the kept
//                            points (wave shuffles, waves merged through LDS) -> partial[block]
//   cloud_merge_kernel       one block: minimum and sum of the partials -> vmin = m - v/2, counts_out[0]
//   hipMemsetAsync           the records
//   cloud_accumulate_kernel  one thread per point: voxel index in fp64, then seven integer atomics into the record
//   cloud_count_kernel       one block per tile of kCloudTile voxels: ballot + popcount of count != 0 -> tiles[T]
//   cloud_scan_kernel        one block: exclusive scan of the tile counts with a running carry; counts_out[1]
//   cloud_emit_kernel        one block per tile: lanes ranked by mbcnt, one thread per occupied voxel writes its mean
// The last three are cloud_common.h's tile_count, tile_scan_exclusive and tile_ranks around this file's flag (count != 0)
// and its write per voxel; the in-box load and the host's checks of the box, the dtype and the workspace are there too.
// A floating-point minimum and integer sums do not depend on the order of their operands, no block waits for another,
// and linear voxel order is (iz, iy, ix) order: the same inputs give the same bytes on every run and stream.
// mvs_cloud_downsample_normals (include/mvs_normals_abi.h) is the same launches with the accumulate and emit kernels'
// kNormals = true forms, which also keep three 64-bit fixed-point sums of the points' normals per voxel, in an array of
// their own behind the workspace of the plain call: the record and the plain call's kernels are what they were.
// This file is compiled with -ffp-contract=off: voxel_index and voxel_corner are the header's fp64 restatement,
// operation for operation, and the emit pass must recompute the very corner the accumulate pass subtracted.
#include "cloud_common.h"

namespace mvs {

constexpr int kCloudRecord = MVS_CLOUD_RECORD;
static_assert(kCloudChunk % kCloudThreads == 0, "whole waves");

// one voxel: 64 bytes, zeroed before the accumulate pass
struct CloudRecord {
    unsigned int count;
    unsigned int pad;
    unsigned long long rgb[3];     // byte sums
    long long fix[3];              // sums of round(offset / voxel_size * 2^32), offset = p - corner
    unsigned long long pad2;
};
static_assert(sizeof(CloudRecord) == kCloudRecord, "record size is part of the workspace formula");

struct CloudPartial {              // what one block of the crop pass found
    double m[3];
    long long kept;
};
struct CloudHead {                 // written by the merge pass
    double vmin[3];
    long long kept;
    char pad[32];
};
static_assert(sizeof(CloudPartial) == 32 && sizeof(CloudHead) == 64, "workspace formula");

struct CloudParams {
    const void* xyz;
    const unsigned char* rgb;
    float* xyz_out;
    unsigned char* rgb_out;
    long long* counts_out;
    CloudHead* head;
    CloudRecord* grid;
    CloudPartial* partial;
    int* tiles;                    // [n_tiles + 1]
    const float* normals;          // the three below: mvs_cloud_downsample_normals only
    float* normals_out;
    long long* nsum;               // [cells][3]: sums of rint(clamp(n, -1, 1) * 2^30), zeroed with the records
    double bmin[3], bmax[3];
    double v, scale;
    long long capacity;
    int P, n_chunks;
    int n[3];
    int cells, n_tiles;
};

// the header's restatement: idx = floor((p - vmin) / v), corner = vmin + idx * v
__device__ __forceinline__ double voxel_index(double p, double vmin, double v) { return floor((p - vmin) / v); }
__device__ __forceinline__ double voxel_corner(double idx, double vmin, double v) { return vmin + idx * v; }

template <typename T>
__global__ void __launch_bounds__(kCloudThreads) cloud_crop_min_kernel(CloudParams C) {
    __shared__ double wave_min[kCloudWaves][3];
    __shared__ int wave_kept[kCloudWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double m[3] = {INFINITY, INFINITY, INFINITY};
    int kept = 0;
#pragma unroll
    for (int k = 0; k < kCloudChunk / kCloudThreads; ++k) {
        const long long i = (long long)blockIdx.x * kCloudChunk + k * kCloudThreads + threadIdx.x;
        double p[3];
        if (i < C.P && box_load<T>(C.xyz, C.bmin, C.bmax, (int)i, p)) {
            ++kept;
#pragma unroll
            for (int a = 0; a < 3; ++a) m[a] = p[a] < m[a] ? p[a] : m[a];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kept += __shfl_down(kept, off);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double o = __shfl_down(m[a], off);
            m[a] = o < m[a] ? o : m[a];
        }
    }
    if (lane == 0) {
        wave_kept[wave] = kept;
#pragma unroll
        for (int a = 0; a < 3; ++a) wave_min[wave][a] = m[a];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        CloudPartial r;
        r.kept = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) r.m[a] = INFINITY;
#pragma unroll
        for (int wv = 0; wv < kCloudWaves; ++wv) {
            r.kept += wave_kept[wv];
#pragma unroll
            for (int a = 0; a < 3; ++a) r.m[a] = wave_min[wv][a] < r.m[a] ? wave_min[wv][a] : r.m[a];
        }
        C.partial[blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(kCloudScanWidth) cloud_merge_kernel(CloudParams C) {
    __shared__ double wave_min[kCloudScanWidth / 64][3];
    __shared__ long long wave_kept[kCloudScanWidth / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m[3] = {INFINITY, INFINITY, INFINITY};
    long long kept = 0;
    for (int i = tid; i < C.n_chunks; i += kCloudScanWidth) {
        const CloudPartial r = C.partial[i];
        kept += r.kept;
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = r.m[a] < m[a] ? r.m[a] : m[a];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kept += __shfl_down(kept, off);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double o = __shfl_down(m[a], off);
            m[a] = o < m[a] ? o : m[a];
        }
    }
    if (lane == 0) {
        wave_kept[wave] = kept;
#pragma unroll
        for (int a = 0; a < 3; ++a) wave_min[wave][a] = m[a];
    }
    __syncthreads();
    if (tid == 0) {
        kept = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = INFINITY;
        for (int wv = 0; wv < kCloudScanWidth / 64; ++wv) {
            kept += wave_kept[wv];
#pragma unroll
            for (int a = 0; a < 3; ++a) m[a] = wave_min[wv][a] < m[a] ? wave_min[wv][a] : m[a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) C.head->vmin[a] = m[a] - 0.5 * C.v;
        C.head->kept = kept;
        C.counts_out[0] = kept;
    }
}

template <typename T, bool kNormals>
__global__ void __launch_bounds__(kCloudThreads) cloud_accumulate_kernel(CloudParams C) {
    const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
    double p[3];
    if (i >= C.P || !box_load<T>(C.xyz, C.bmin, C.bmax, (int)i, p)) return;
    long long fix[3];
    int idx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double vmin = C.head->vmin[a];
        const double k = voxel_index(p[a], vmin, C.v);
        // 0 <= k <= n - 1 by the header's argument; the test only keeps a store inside the grid should that ever fail
        if (!(k >= 0.0 && k < (double)C.n[a])) return;
        idx[a] = (int)k;
        // the offset lies in [0, 1) up to a rounding of the corner: signed, so that a tiny negative one adds as such
        fix[a] = __double2ll_rn(((p[a] - voxel_corner(k, vmin, C.v)) / C.v) * 4294967296.0);
    }
    const size_t cell = ((size_t)idx[2] * C.n[1] + idx[1]) * C.n[0] + idx[0];
    CloudRecord* r = C.grid + cell;
    const unsigned char* c = C.rgb + (size_t)i * 3;
    __hip_atomic_fetch_add(&r->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        __hip_atomic_fetch_add(&r->rgb[a], (unsigned long long)c[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&r->fix[a], fix[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (kNormals) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double n = (double)C.normals[(size_t)i * 3 + a];
            n = n != n ? 0.0 : n < -1.0 ? -1.0 : n > 1.0 ? 1.0 : n;
            __hip_atomic_fetch_add(&C.nsum[cell * 3 + a], __double2ll_rn(n * 1073741824.0), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__device__ __forceinline__ bool cloud_flag(const CloudParams& C, unsigned cell) {
    return cell < (unsigned)C.cells && C.grid[cell].count != 0;
}
__device__ __forceinline__ unsigned cloud_cell(int pass) {
    return (unsigned)blockIdx.x * kCloudTile + pass * kCloudThreads + threadIdx.x;
}

__global__ void __launch_bounds__(kCloudThreads) cloud_count_kernel(CloudParams C) {
    const int s = tile_count<kCloudPasses, kCloudThreads>([&](int i) { return cloud_flag(C, cloud_cell(i)); });
    if (threadIdx.x == 0) C.tiles[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kCloudScanWidth) cloud_scan_kernel(CloudParams C) {
    const int carry = tile_scan_exclusive<kCloudScanWidth>(C.tiles, C.n_tiles);       // the occupied voxels
    if (threadIdx.x == 0) {
        C.tiles[C.n_tiles] = carry;
        C.counts_out[1] = carry;
    }
}

template <bool kNormals>
__global__ void __launch_bounds__(kCloudThreads) cloud_emit_kernel(CloudParams C) {
    const long long tile_base = C.tiles[blockIdx.x];
    tile_ranks<kCloudPasses, kCloudThreads>(
        [&](int i) { return cloud_flag(C, cloud_cell(i)); },
        [&](int i, int rank, bool set) {
            const long long o = tile_base + rank;
            if (!set || o >= C.capacity) return;
            const int cell = (int)cloud_cell(i);           // occupied, so below cells
            const CloudRecord r = C.grid[cell];
            const int plane = C.n[0] * C.n[1];
            const int iz = cell / plane, rest = cell - iz * plane;
            const int iy = rest / C.n[0], ix = rest - iy * C.n[0];
            const int idx[3] = {ix, iy, iz};
            const double count = (double)r.count;
            float* dst = C.xyz_out + (size_t)o * 3;
            unsigned char* col = C.rgb_out + (size_t)o * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double corner = voxel_corner((double)idx[a], C.head->vmin[a], C.v);
                const double mean = corner + ((double)r.fix[a] / count) * C.v * (1.0 / 4294967296.0);
                dst[a] = (float)(mean * C.scale);          // v_cvt_f32_f64, round-to-nearest-even
                col[a] = (unsigned char)((2ull * r.rgb[a] + r.count) / (2ull * r.count));
            }
            if constexpr (kNormals) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    C.normals_out[(size_t)o * 3 + a] =
                        (float)(((double)C.nsum[(size_t)cell * 3 + a] / count) * (1.0 / 1073741824.0));
            }
        });
}

// neither is ever capped: P / 1024 and cells / 1024 are at most 2^21 (cloud_common.h)
static long long cloud_chunks(long long P) { return cloud_blocks(kLaunchChunk, P); }
static long long cloud_tiles(long long cells) { return cloud_blocks(kLaunchCellTile, cells); }

static size_t cloud_workspace(long long P, long long cells) {
    return sizeof(CloudHead) + sizeof(CloudRecord) * (size_t)cells + sizeof(CloudPartial) * (size_t)cloud_chunks(P) +
           8 * (size_t)((cloud_tiles(cells) + 2) / 2);
}

constexpr size_t kCloudNormalSums = 3 * sizeof(long long);     // per voxel, mvs_cloud_downsample_normals only
static size_t cloud_normals_workspace(long long P, long long cells) {
    return cloud_workspace(P, cells) + kCloudNormalSums * (size_t)cells;
}

// both entry points, after their NULL checks
static int cloud_downsample(const char* who, bool with_normals, const void* xyz, int xyz_dtype, const unsigned char* rgb,
                            const float* normals, long long P, const double* box_min, const double* box_max,
                            double voxel_size, double scale, long long capacity, float* xyz_out, unsigned char* rgb_out,
                            float* normals_out, long long* counts_out, void* workspace, size_t workspace_bytes,
                            void* stream) {
    int n[3];
    long long cells;
    if (int rc = grid_check(who, kVoxelGrid, P, box_min, box_max, voxel_size, n, &cells)) return rc;
    if (capacity < 0 || !std::isfinite(scale))
        return fail(MVS_ERR_BAD_SHAPE, "%s: capacity = %lld, scale = %g (need capacity >= 0 and a finite scale)", who, capacity,
                    scale);
    if (int rc = check_xyz_dtype(who, xyz_dtype)) return rc;
    const size_t need = with_normals ? cloud_normals_workspace(P, cells) : cloud_workspace(P, cells);
    if (int rc = check_workspace8(who, workspace, workspace_bytes, need)) return rc;
    CloudParams C{};
    C.xyz = xyz;
    C.rgb = rgb;
    C.xyz_out = xyz_out;
    C.rgb_out = rgb_out;
    C.counts_out = counts_out;
    C.normals = normals;
    C.normals_out = normals_out;
    char* ws = static_cast<char*>(workspace);
    C.head = reinterpret_cast<CloudHead*>(ws);
    C.grid = reinterpret_cast<CloudRecord*>(ws + sizeof(CloudHead));
    C.partial = reinterpret_cast<CloudPartial*>(ws + sizeof(CloudHead) + sizeof(CloudRecord) * (size_t)cells);
    C.n_chunks = (int)cloud_chunks(P);
    C.tiles = reinterpret_cast<int*>(reinterpret_cast<char*>(C.partial) + sizeof(CloudPartial) * (size_t)C.n_chunks);
    // behind everything the plain call lays out (the tile offsets end on an 8-byte boundary)
    C.nsum = with_normals ? reinterpret_cast<long long*>(ws + cloud_workspace(P, cells)) : nullptr;
    for (int a = 0; a < 3; ++a) {
        C.bmin[a] = box_min[a];
        C.bmax[a] = box_max[a];
        C.n[a] = n[a];
    }
    C.v = voxel_size;
    C.scale = scale;
    C.capacity = capacity;
    C.P = (int)P;
    C.cells = (int)cells;
    C.n_tiles = (int)cloud_tiles(cells);
    const bool f64 = xyz_dtype == MVS_CLOUD_F64;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C.n_chunks > 0) {
        if (f64) cloud_crop_min_kernel<double><<<C.n_chunks, kCloudThreads, 0, s>>>(C);
        else cloud_crop_min_kernel<float><<<C.n_chunks, kCloudThreads, 0, s>>>(C);
        if (int rc = check_hip(hipGetLastError(), "cloud_crop_min_kernel")) return rc;
    }
    cloud_merge_kernel<<<1, kCloudScanWidth, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cloud_merge_kernel")) return rc;
    if (int rc = check_hip(hipMemsetAsync(C.grid, 0, sizeof(CloudRecord) * (size_t)cells, s), "zeroing the voxel grid"))
        return rc;
    if (with_normals)
        if (int rc = check_hip(hipMemsetAsync(C.nsum, 0, kCloudNormalSums * (size_t)cells, s), "zeroing the normal sums"))
            return rc;
    if (P > 0) {
        const int blocks = cloud_blocks(kLaunchRow, P);
        if (with_normals) {
            if (f64) cloud_accumulate_kernel<double, true><<<blocks, kCloudThreads, 0, s>>>(C);
            else cloud_accumulate_kernel<float, true><<<blocks, kCloudThreads, 0, s>>>(C);
        } else {
            if (f64) cloud_accumulate_kernel<double, false><<<blocks, kCloudThreads, 0, s>>>(C);
            else cloud_accumulate_kernel<float, false><<<blocks, kCloudThreads, 0, s>>>(C);
        }
        if (int rc = check_hip(hipGetLastError(), "cloud_accumulate_kernel")) return rc;
    }
    cloud_count_kernel<<<C.n_tiles, kCloudThreads, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cloud_count_kernel")) return rc;
    cloud_scan_kernel<<<1, kCloudScanWidth, 0, s>>>(C);
    if (int rc = check_hip(hipGetLastError(), "cloud_scan_kernel")) return rc;
    if (with_normals) cloud_emit_kernel<true><<<C.n_tiles, kCloudThreads, 0, s>>>(C);
    else cloud_emit_kernel<false><<<C.n_tiles, kCloudThreads, 0, s>>>(C);
    return check_hip(hipGetLastError(), "cloud_emit_kernel");
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_cloud_workspace(long long P, const double box_min[3], const double box_max[3], double voxel_size,
                              size_t* bytes) {
    return grid_query("mvs_query_cloud_workspace", kVoxelGrid, P, box_min, box_max, voxel_size, bytes, cloud_workspace);
}

int mvs_cloud_downsample(const void* xyz, int xyz_dtype, const unsigned char* rgb, long long P, const double box_min[3],
                         const double box_max[3], double voxel_size, double scale, long long capacity, float* xyz_out,
                         unsigned char* rgb_out, long long* counts_out, void* workspace, size_t workspace_bytes,
                         void* stream) {
    if (!xyz || !rgb || !box_min || !box_max || !counts_out || !workspace || (capacity != 0 && (!xyz_out || !rgb_out)))
        return fail(MVS_ERR_NULL, "mvs_cloud_downsample: NULL argument");
    return cloud_downsample("mvs_cloud_downsample", false, xyz, xyz_dtype, rgb, nullptr, P, box_min, box_max, voxel_size,
                            scale, capacity, xyz_out, rgb_out, nullptr, counts_out, workspace, workspace_bytes, stream);
}

int mvs_query_cloud_normals_downsample_workspace(long long P, const double box_min[3], const double box_max[3],
                                                 double voxel_size, size_t* bytes) {
    return grid_query("mvs_query_cloud_normals_downsample_workspace", kVoxelGrid, P, box_min, box_max, voxel_size, bytes,
                      cloud_normals_workspace);
}

int mvs_cloud_downsample_normals(const void* xyz, int xyz_dtype, const unsigned char* rgb, const float* normals, long long P,
                                 const double box_min[3], const double box_max[3], double voxel_size, double scale,
                                 long long capacity, float* xyz_out, unsigned char* rgb_out, float* normals_out,
                                 long long* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!xyz || !rgb || !normals || !box_min || !box_max || !counts_out || !workspace ||
        (capacity != 0 && (!xyz_out || !rgb_out || !normals_out)))
        return fail(MVS_ERR_NULL, "mvs_cloud_downsample_normals: NULL argument");
    return cloud_downsample("mvs_cloud_downsample_normals", true, xyz, xyz_dtype, rgb, normals, P, box_min, box_max,
                            voxel_size, scale, capacity, xyz_out, rgb_out, normals_out, counts_out, workspace,
                            workspace_bytes, stream);
}

}  // extern "C"
