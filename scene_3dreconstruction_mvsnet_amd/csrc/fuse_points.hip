// fuse_points.hip -- ordered compaction of a scan's filtered depth maps into one coloured point cloud
// (reference eval.py:745-758: xyz_world[final], img[1::4, 1::4][final], np.concatenate over the views).
//
// A tile is kCloudTile consecutive pixels of ONE view; tile T = r * tiles_per_view + t, so tile order is the output
// order.  Three launches, ordered by the stream alone:
//   fuse_count_kernel    one block per tile: ballot + popcount of the final mask per wave, waves added through LDS
//                        -> workspace[T]
//   fuse_scan_kernel     one block: exclusive scan of workspace[0 .. tiles) in place, kCloudScanWidth tiles per pass
//                        with a running carry; workspace[tiles] = total; counts_out from the view boundaries
//   fuse_scatter_kernel  one block per tile: the same ballots again, lanes ranked by mbcnt, points written at
//                        workspace[T] + rank while rank < capacity
// The count, the scan loop and the ranks are cloud_common.h's tile_count, tile_scan_exclusive and tile_ranks (shared with
// cloud_downsample.hip and cloud_knn.h); this file supplies the flag of a pixel and what is written per selected point.
// No block waits for another block and nothing is atomic: the output is the same bytes on every run and stream.
// Within a tile, pass i of a block covers pixels [i * 256, (i + 1) * 256): wave wv its 64 lanes in order, so
// (pass, wave, lane) is the pixel order.  Mask bytes are read twice (1 B per pixel each); only selected pixels read
// their 24 B of xyz_world and 3 colour bytes.
#include "mvs_fuse_abi.h"
#include "cloud_common.h"

namespace mvs {

struct FuseParams {
    const double* xyz;
    const unsigned char* masks;
    const unsigned char* images;
    const int* ref_idx;
    float* xyz_out;
    unsigned char* rgb_out;
    int* counts_out;
    int* tiles;              // workspace: [n_tiles + 1]
    long long capacity;
    int V, R, h, w, hw;
    int tiles_per_view, n_tiles;
    int hwc;                 // 1: [V][4h][4w][3], 0: [V][3][4h][4w]
};

// final-mask flag of pixel (tile, pass, thread); false past the end of the view and for a view without an image
// (p is unsigned: the last tile of a view of nearly 2^31 pixels runs past INT_MAX)
__device__ __forceinline__ bool fuse_flag(const FuseParams& P, bool view_ok, int r, unsigned p) {
    return view_ok && p < (unsigned)P.hw && P.masks[((size_t)r * 3 + 2) * P.hw + p] != 0;
}
__device__ __forceinline__ unsigned fuse_pixel(int t, int pass) {
    return (unsigned)t * kCloudTile + pass * kCloudThreads + threadIdx.x;
}

// Both tile kernels take tile blockIdx.x, then every gridDim.x-th: the grid is capped (cloud_common.h's kLaunchFuseTile),
// and below 2^24 tiles that is one trip.  tile_count and tile_ranks keep their partial counts in LDS, so a block that goes
// round again synchronises first.
// the tile after T of this block, n_tiles when there is none: 32-bit like T itself (n_tiles < 2^31, gridDim.x < 2^24), and
// the sum is formed only where it fits
__device__ __forceinline__ int fuse_next_tile(const FuseParams& P, int T) {
    return P.n_tiles - T > (int)gridDim.x ? T + (int)gridDim.x : P.n_tiles;
}
// kCapped: the grid is short of the tiles; else one tile per block, the kernel without a loop
template <bool kCapped>
__global__ void __launch_bounds__(kCloudThreads) fuse_count_kernel(FuseParams P) {
    int T = blockIdx.x;
    do {
        const int r = T / P.tiles_per_view, t = T - r * P.tiles_per_view;
        const int ref = P.ref_idx[r];
        const bool view_ok = ref >= 0 && ref < P.V;
        const int s = tile_count<kCloudPasses, kCloudThreads>([&P, view_ok, r, t](int i) { return fuse_flag(P, view_ok, r, fuse_pixel(t, i)); });
        if (threadIdx.x == 0) P.tiles[T] = s;
        if (kCapped && fuse_next_tile(P, T) < P.n_tiles) __syncthreads();      // the same in every thread of the block
    } while (kCapped && (T = fuse_next_tile(P, T)) < P.n_tiles);
}

__global__ void __launch_bounds__(kCloudScanWidth) fuse_scan_kernel(FuseParams P) {
    const int tid = threadIdx.x;
    const int carry = tile_scan_exclusive<kCloudScanWidth>(P.tiles, P.n_tiles);       // the points of the scan
    if (tid == 0) P.tiles[P.n_tiles] = carry;
    __syncthreads();         // the offsets this block wrote are read back below
    for (int r = tid; r < P.R; r += kCloudScanWidth)
        P.counts_out[r] = P.tiles[(r + 1) * P.tiles_per_view] - P.tiles[r * P.tiles_per_view];
    if (tid == 0) P.counts_out[P.R] = carry;
}

template <bool kCapped>
__global__ void __launch_bounds__(kCloudThreads) fuse_scatter_kernel(FuseParams P) {
    const size_t H = (size_t)4 * P.h, W = (size_t)4 * P.w;   // image rows and columns
    int T = blockIdx.x;
    do {
        const int r = T / P.tiles_per_view, t = T - r * P.tiles_per_view;
        const int ref = P.ref_idx[r];
        const bool view_ok = ref >= 0 && ref < P.V;
        const long long tile_base = P.tiles[T];
        tile_ranks<kCloudPasses, kCloudThreads>(
            [&P, view_ok, r, t](int i) { return fuse_flag(P, view_ok, r, fuse_pixel(t, i)); },
            [=, &P](int i, int rank, bool set) {
                const long long o = tile_base + rank;
                if (!set || o >= P.capacity) return;
                const int p = (int)fuse_pixel(t, i);       // selected, so below h*w
                const double* src = P.xyz + ((size_t)r * P.hw + p) * 3;
                float* dst = P.xyz_out + (size_t)o * 3;
                dst[0] = (float)src[0];      // v_cvt_f32_f64, round-to-nearest-even
                dst[1] = (float)src[1];
                dst[2] = (float)src[2];
                const int y = p / P.w, x = p - y * P.w;
                const size_t py = (size_t)4 * y + 1, px = (size_t)4 * x + 1;
                unsigned char* c = P.rgb_out + (size_t)o * 3;
                if (P.hwc) {
                    const unsigned char* s = P.images + (((size_t)ref * H + py) * W + px) * 3;
                    c[0] = s[0];
                    c[1] = s[1];
                    c[2] = s[2];
                } else {
                    const size_t plane = H * W;
                    const unsigned char* s = P.images + (size_t)ref * 3 * plane + py * W + px;
                    c[0] = s[0];
                    c[1] = s[plane];
                    c[2] = s[2 * plane];
                }
            });
        if (kCapped && fuse_next_tile(P, T) < P.n_tiles) __syncthreads();      // the same in every thread of the block
    } while (kCapped && (T = fuse_next_tile(P, T)) < P.n_tiles);
}

static int fuse_check(int R, int h, int w) {
    if (R < 1 || h < 1 || w < 1 || (long long)R * h * w >= (1LL << 31))
        return fail(MVS_ERR_BAD_SHAPE, "fuse points: R,h,w = %d,%d,%d (need R,h,w >= 1 and R*h*w < 2^31)", R, h, w);
    return MVS_OK;
}

static size_t fuse_workspace(int R, int h, int w) {
    return sizeof(int) * ((size_t)cloud_fuse_tiles(R, h, w) + 1);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

// The hook of the tests, not part of the ABI: the cap on the blocks of the cloud path's looping launches (1 .. 2^24 - 1)
// in later calls of this process.  Returns the value it replaces; any other argument only reads it.
long long mvs_test_cloud_max_blocks(long long blocks) {
    if (blocks >= 1 && blocks <= kCloudMaxBlocks) return g_cloud_loop_cap.exchange(blocks, std::memory_order_relaxed);
    return g_cloud_loop_cap.load(std::memory_order_relaxed);
}

int mvs_query_fuse_workspace(int R, int h, int w, size_t* bytes) {
    if (!bytes) return fail(MVS_ERR_NULL, "mvs_query_fuse_workspace: NULL bytes");
    if (int rc = fuse_check(R, h, w)) return rc;
    *bytes = fuse_workspace(R, h, w);
    return MVS_OK;
}

int mvs_fuse_points(const double* xyz_world, const unsigned char* masks, const void* images, int image_format,
                    const int* ref_idx, int V, int R, int h, int w, long long capacity, float* xyz_out,
                    unsigned char* rgb_out, int* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!xyz_world || !masks || !images || !ref_idx || !counts_out || !workspace ||
        (capacity != 0 && (!xyz_out || !rgb_out)))
        return fail(MVS_ERR_NULL, "mvs_fuse_points: NULL argument");
    if (int rc = fuse_check(R, h, w)) return rc;
    if (V < 1 || capacity < 0)
        return fail(MVS_ERR_BAD_SHAPE, "mvs_fuse_points: V = %d, capacity = %lld (need V >= 1, capacity >= 0)", V,
                    capacity);
    if (image_format != MVS_IMG_U8_HWC && image_format != MVS_IMG_U8_CHW)
        return fail(MVS_ERR_BAD_DTYPE, "mvs_fuse_points: image format %d (MVS_IMG_U8_CHW or MVS_IMG_U8_HWC: the "
                    "colours are copied bytes)", image_format);
    const size_t need = fuse_workspace(R, h, w);
    if (workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % alignof(int))
        return fail(MVS_ERR_WORKSPACE, "mvs_fuse_points: workspace of %zu bytes at %p, need %zu (4-byte aligned)",
                    workspace_bytes, workspace, need);
    FuseParams P{};
    P.xyz = xyz_world;
    P.masks = masks;
    P.images = static_cast<const unsigned char*>(images);
    P.ref_idx = ref_idx;
    P.xyz_out = xyz_out;
    P.rgb_out = rgb_out;
    P.counts_out = counts_out;
    P.tiles = static_cast<int*>(workspace);
    P.capacity = capacity;
    P.V = V;
    P.R = R;
    P.h = h;
    P.w = w;
    P.hw = h * w;
    P.tiles_per_view = cloud_fuse_tiles_per_view(h, w);
    P.n_tiles = (int)cloud_fuse_tiles(R, h, w);      // <= R*h*w < 2^31
    const int tile_blocks = cloud_blocks(kLaunchFuseTile, P.n_tiles);      // capped: the kernels loop
    P.hwc = image_format == MVS_IMG_U8_HWC;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const bool capped = cloud_capped(kLaunchFuseTile, P.n_tiles);
    if (capped) fuse_count_kernel<true><<<tile_blocks, kCloudThreads, 0, s>>>(P);
    else fuse_count_kernel<false><<<tile_blocks, kCloudThreads, 0, s>>>(P);
    if (int rc = check_hip(hipGetLastError(), "fuse_count_kernel")) return rc;
    fuse_scan_kernel<<<1, kCloudScanWidth, 0, s>>>(P);
    if (int rc = check_hip(hipGetLastError(), "fuse_scan_kernel")) return rc;
    if (capped) fuse_scatter_kernel<true><<<tile_blocks, kCloudThreads, 0, s>>>(P);
    else fuse_scatter_kernel<false><<<tile_blocks, kCloudThreads, 0, s>>>(P);
    return check_hip(hipGetLastError(), "fuse_scatter_kernel");
}

}  // extern "C"
