// train_backward.hip -- adjoints of the cost volume and of the soft-argmin, for training on gfx950 (MI355X).
//
// Replaces the autograd backward of
//   models/module.py:96-139   homo_warping (grid_sample's backward: bilinear taps scattered with float atomics)
//   models/mvsnet.py:145-177  ref-volume repeat, out-of-place sums / squares of the training branch (167-169), variance
//   models/mvsnet.py:192-193  F.softmax over depth
//   models/module.py:144-147  depth_regression
// The projection and the depth values carry no gradient (the reference builds its sampling grid under no_grad,
// module.py:106-133), nor does the photometric confidence (mvsnet.py:213-218, no_grad).
//
// Warp + variance.  var = Q/N - (S/N)^2 with S = sum_i w_i, Q = sum_i w_i^2 over the N sampled values w_i of a
// (channel, depth, pixel), w_0 = the reference feature itself.  So dvar/dw_i = 2/N * (w_i - S/N), and
//   reference view:  gf0[c][p]  = sum_d g[c][d][p] * 2/N * (f0[c][p] - S/N)
//   source view i:   gw          = g * 2/N * (w_i - S/N), scattered to the four bilinear taps of make_samp
// (warp_common.h) with their weights -- the same taps and weights as the forward kernels, so this is the exact adjoint
// of the forward as implemented: v_rcp_f32 projection, zero weight outside the image, NaN weights for a non-finite
// sampling coordinate.  Nothing of the forward is saved: the warped values and S are recomputed.
//
// Scatter budget (cdna_hip_programming.md, guideline 12).  At the training shape (N = 3, D = 192, 128 x 160, C = 32)
// the four taps of every source-view sample are 4 * 32 * 192 * 20480 * 2 views = 1.0 G adds = 4.0 GB of float atomics
// if each goes to global memory: ~3.1 ms at the chip's ~1.3 TB/s of global float atomics.  Here a block owns one
// 8-channel group, a 32 x 8 tile of reference pixels and a slab of 8 depths; each of its waves (2 rows of 32 pixels)
// sums the taps of its 512 samples per source view into a window of the source image in LDS (the footprint moves by a
// fraction of a texel per depth step: ~36 x 4 texels), then flushes the window with one global_atomic_add_f32 per
// touched texel and channel.  The sums into LDS are plain read-add-writes whenever no two lanes of the wave share a
// 2x2 cell (checked per depth step); ds_add_f32, which the first form of this kernel used for every tap, serialises
// its lanes and made that form 4.4 ms at the training shape (3.5 ms of it waiting on LDS).  A wave whose footprint
// does not fit its window (wide baselines, very oblique views) falls back to direct global atomics: correct for any
// geometry, only slower.
#include <climits>

#include "mvs_internal.h"
#include "warp_common.h"

namespace mvs {

namespace {

constexpr int kTX = 32, kTY = 8;       // reference-pixel tile: one thread per pixel
constexpr int kSlab = 8;               // depths per block
constexpr int kWinWave = 512;          // LDS window per wave: 512 texels x 8 channels x 4 B = 16 KB (64 KB a block)
constexpr int kThreads = kTX * kTY;

// texel (x, y) of an offset o = y * w + x into the image; o < h * w < 2^24 (check_dims: D >= 8 and D*h*w*32 < 2^32),
// so (float)o is exact and the quotient estimate is off by at most one
__device__ __forceinline__ void texel_xy(int o, int w, float rw, int& x, int& y) {
    int q = (int)((float)o * rw);
    if (q * w > o) --q;
    else if ((q + 1) * w <= o) ++q;
    y = q;
    x = o - q * w;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v = min(v, __shfl_xor(v, k));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v = max(v, __shfl_xor(v, k));
    return v;
}

__device__ __forceinline__ void global_add(float* p, float v) { unsafeAtomicAdd(p, v); }   // global_atomic_add_f32

// orders this wave's LDS accesses before and after it (each wave owns its window: no block barrier is needed)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// gather 8 channels of one source view at a sample: feats NCHW, channel stride hw
__device__ __forceinline__ void gather8(const float* __restrict__ f, size_t hw, const Samp& t, float out[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float* fc = f + (size_t)c * hw;
        out[c] = fmaf(fc[t.o00], t.w00, fmaf(fc[t.o01], t.w01, fmaf(fc[t.o10], t.w10, fc[t.o11] * t.w11)));
    }
}

// Grid: one block per (tile, depth slab, channel group), flattened into x.
//   feats [N][32][h][w], rt [(N-1)][12], dv [D], g [32][D][h][w] -> gf [N][32][h][w] (zero-filled by the caller)
__global__ __launch_bounds__(kThreads, 2) void warp_variance_bwd_kernel(const float* __restrict__ feats,
                                                                     const float* __restrict__ rt,
                                                                     const float* __restrict__ dv,
                                                                     const float* __restrict__ g,
                                                                     float* __restrict__ gf, int N, int D, int h,
                                                                     int w, int ntx, int ntiles, int nslab) {
    __shared__ float4 win4[kThreads / 64][kWinWave * 2];   // per wave: [texel][8 channels]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* mywin = reinterpret_cast<float*>(win4[wave]);
    int bid = blockIdx.x;
    const int tile = bid % ntiles;
    bid /= ntiles;
    const int slab = bid % nslab;
    const int pl = bid / nslab;                   // channel group: channels 8*pl .. 8*pl+7
    const int x = (tile % ntx) * kTX + (threadIdx.x & (kTX - 1));
    const int y = (tile / ntx) * kTY + (threadIdx.x / kTX);
    const bool active = x < w && y < h;
    const int hw = h * w;
    const int p = active ? y * w + x : 0;
    const int d0 = slab * kSlab;
    const int nd = min(kSlab, D - d0);
    const float sx = (float)w / (float)(w - 1), sy = (float)h / (float)(h - 1);
    const float fx = (float)x, fy = (float)y;
    const float rw = 1.0f / (float)w;
    const float inv_n = 1.0f / (float)N, two_n = 2.0f * inv_n;
    const size_t HW = (size_t)hw;
    const float* fview = feats + (size_t)(pl * 8) * HW;      // view 0, channel 8*pl
    const size_t vstride = (size_t)kC * HW;                  // floats between views

    float f0[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) f0[c] = active ? fview[(size_t)c * HW + p] : 0.0f;

    // pass A: a = g * 2/N and m = S/N for every depth of the slab (kept in registers), and the reference view's share
    float a[kSlab][8], m[kSlab][8], gref[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) gref[c] = 0.0f;
#pragma unroll
    for (int j = 0; j < kSlab; ++j) {
#pragma unroll
        for (int c = 0; c < 8; ++c) { a[j][c] = 0.0f; m[j][c] = 0.0f; }
        if (!active || j >= nd) continue;
        const int d = d0 + j;
        const float depth = dv[d];
        float S[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            S[c] = f0[c];
            a[j][c] = g[((size_t)(pl * 8 + c) * D + d) * HW + p] * two_n;
        }
        for (int v = 1; v < N; ++v) {
            const float* r = rt + (size_t)(v - 1) * 12;
            const float qx = fmaf(r[0], fx, fmaf(r[1], fy, r[2]));
            const float qy = fmaf(r[3], fx, fmaf(r[4], fy, r[5]));
            const float qz = fmaf(r[6], fx, fmaf(r[7], fy, r[8]));
            const Samp t = make_samp(qx, qy, qz, r[9], r[10], r[11], depth, sx, sy, h, w, 0, 0, w, h);
            float wv[8];
            gather8(fview + (size_t)v * vstride, HW, t, wv);
#pragma unroll
            for (int c = 0; c < 8; ++c) S[c] += wv[c];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            m[j][c] = S[c] * inv_n;
            gref[c] = fmaf(a[j][c], f0[c] - m[j][c], gref[c]);
        }
    }
    if (active && nd > 0) {
        float* o = gf + (size_t)(pl * 8) * HW + p;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (gref[c] != 0.0f) global_add(o + (size_t)c * HW, gref[c]);
    }

    // pass B: one source view at a time -- the window's bounding box, the taps into LDS, the flush
    for (int v = 1; v < N; ++v) {
        const float* r = rt + (size_t)(v - 1) * 12;
        const float qx = fmaf(r[0], fx, fmaf(r[1], fy, r[2]));
        const float qy = fmaf(r[3], fx, fmaf(r[4], fy, r[5]));
        const float qz = fmaf(r[6], fx, fmaf(r[7], fy, r[8]));
        const float* fsrc = fview + (size_t)v * vstride;
        float* gsrc = gf + (size_t)v * vstride + (size_t)(pl * 8) * HW;
        // this wave's bounding box of the taps with a non-zero (or NaN) weight
        int x_lo = 0x7fffffff, x_hi = -1, y_lo = 0x7fffffff, y_hi = -1;
        if (active) {
#pragma unroll
            for (int j = 0; j < kSlab; ++j) {
                if (j >= nd) break;
                const Samp t = make_samp(qx, qy, qz, r[9], r[10], r[11], dv[d0 + j], sx, sy, h, w, 0, 0, w, h);
                int xa, ya, xb, yb;
                texel_xy(t.o00, w, rw, xa, ya);
                texel_xy(t.o11, w, rw, xb, yb);
                const bool c0 = t.w00 != 0.0f || t.w10 != 0.0f, c1 = t.w01 != 0.0f || t.w11 != 0.0f;
                const bool r0 = t.w00 != 0.0f || t.w01 != 0.0f, r1 = t.w10 != 0.0f || t.w11 != 0.0f;
                if (c0) { x_lo = min(x_lo, xa); x_hi = max(x_hi, xa); }
                if (c1) { x_lo = min(x_lo, xb); x_hi = max(x_hi, xb); }
                if (r0) { y_lo = min(y_lo, ya); y_hi = max(y_hi, ya); }
                if (r1) { y_lo = min(y_lo, yb); y_hi = max(y_hi, yb); }
            }
        }
        x_lo = wave_min(x_lo); x_hi = wave_max(x_hi);
        y_lo = wave_min(y_lo); y_hi = wave_max(y_hi);
        if (x_hi < x_lo || y_hi < y_lo) continue;             // no tap of this wave lands in the image (wave-uniform)
        const int bw = x_hi - x_lo + 1, bh = y_hi - y_lo + 1;
        const bool in_lds = (long long)bw * bh <= kWinWave;   // wave-uniform
        const int area = in_lds ? bw * bh : 0;
        for (int i = lane; i < area; i += 64) {
            reinterpret_cast<float4*>(mywin + i * 8)[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            reinterpret_cast<float4*>(mywin + i * 8)[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < kSlab; ++j) {
            if (j >= nd) break;
            // every lane evaluates (the shuffles below need the whole wave); inactive lanes write nothing
            const Samp t = make_samp(qx, qy, qz, r[9], r[10], r[11], dv[d0 + j], sx, sy, h, w, 0, 0, w, h);
            float wv[8], gw[8];
            gather8(fsrc, HW, t, wv);
#pragma unroll
            for (int c = 0; c < 8; ++c) gw[c] = a[j][c] * (wv[c] - m[j][c]);
            const int o[4] = {t.o00, t.o01, t.o10, t.o11};
            const float wt[4] = {t.w00, t.w01, t.w10, t.w11};
            const bool writes = active && (t.w00 != 0.0f || t.w01 != 0.0f || t.w10 != 0.0f || t.w11 != 0.0f);
            if (in_lds) {
                // For finite coordinates, lanes with the same tap k hit the same texel only if their 2x2 cells are
                // equal, i.e. if their (clamped) o00 are: a non-zero weight means an unclamped in-image tap.  When
                // o00 strictly increases over the writing lanes -- the common case: a row of reference pixels maps to
                // a row of increasing source texels -- no two lanes of one LDS instruction share an address and a
                // plain read-add-write is exact; otherwise this step uses ds_add_f32, which costs ~25x more (LDS
                // float atomics are serialised per lane).  A non-finite coordinate clamps all four NaN-weighted taps
                // onto border texels that another lane's cell can reach with a different o00, so a wave with such a
                // lane takes the atomic path too.
                const int key = writes ? o[0] : INT_MIN;
                int pm = key;   // inclusive prefix maximum over lanes
#pragma unroll
                for (int sft = 1; sft < 64; sft <<= 1) {
                    const int up = __shfl_up(pm, sft);
                    if (lane >= sft) pm = max(pm, up);
                }
                int before = __shfl_up(pm, 1);
                if (lane == 0) before = INT_MIN;
                const bool nan_lane = writes && __builtin_isnan(t.w00);   // make_samp sets all four weights NaN
                const bool distinct = !__any((writes && before >= key) || nan_lane);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (!writes || wt[k] == 0.0f) continue;
                    int tx, ty;
                    texel_xy(o[k], w, rw, tx, ty);
                    // inside the box by construction (the same make_samp taps); checked so that LDS is never
                    // addressed outside the window whatever the compiler does with the two evaluations
                    if ((unsigned)(tx - x_lo) < (unsigned)bw && (unsigned)(ty - y_lo) < (unsigned)bh) {
                        float* cell = mywin + ((ty - y_lo) * bw + (tx - x_lo)) * 8;
                        if (distinct) {
                            float4 lo = reinterpret_cast<float4*>(cell)[0], hi = reinterpret_cast<float4*>(cell)[1];
                            lo.x = fmaf(gw[0], wt[k], lo.x); lo.y = fmaf(gw[1], wt[k], lo.y);
                            lo.z = fmaf(gw[2], wt[k], lo.z); lo.w = fmaf(gw[3], wt[k], lo.w);
                            hi.x = fmaf(gw[4], wt[k], hi.x); hi.y = fmaf(gw[5], wt[k], hi.y);
                            hi.z = fmaf(gw[6], wt[k], hi.z); hi.w = fmaf(gw[7], wt[k], hi.w);
                            reinterpret_cast<float4*>(cell)[0] = lo;
                            reinterpret_cast<float4*>(cell)[1] = hi;
                        } else {
#pragma unroll
                            for (int c = 0; c < 8; ++c) atomicAdd(cell + c, gw[c] * wt[k]);   // ds_add_f32
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < 8; ++c) global_add(gsrc + (size_t)c * HW + o[k], gw[c] * wt[k]);
                    }
                }
            } else if (writes) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (wt[k] == 0.0f) continue;
#pragma unroll
                    for (int c = 0; c < 8; ++c) global_add(gsrc + (size_t)c * HW + o[k], gw[c] * wt[k]);
                }
            }
        }
        if (!in_lds) continue;                                // wave-uniform: no LDS to flush or reuse
        wave_lds_fence();
        // flush: consecutive lanes take consecutive texels of one channel (coalesced atomics along x)
        for (int c = 0; c < 8; ++c) {
            float* gc = gsrc + (size_t)c * HW;
            for (int i = lane; i < area; i += 64) {
                const float val = mywin[i * 8 + c];
                if (val != 0.0f) {                            // NaN is flushed too
                    const int ty = i / bw, tx = i - ty * bw;
                    global_add(gc + (size_t)(y_lo + ty) * w + (x_lo + tx), val);
                }
            }
        }
        wave_lds_fence();                                     // the window is zeroed again for the next view
    }
}

// grad_cost[d][p] = grad_depth[p] * p_d * (dv_d - depth[p]), with p_d the max-subtracted softmax of
// softargmin_conf_kernel (softargmin.hip) recomputed from the logits.  Thread = pixel; three coalesced passes over D.
__global__ __launch_bounds__(128) void softargmin_bwd_kernel(const float* __restrict__ cost,
                                                            const float* __restrict__ dv,
                                                            const float* __restrict__ gd,
                                                            float* __restrict__ gc, int D, int hw) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hw) return;
    const float* cp = cost + p;
    float M = -INFINITY;
    for (int d = 0; d < D; ++d) M = fmaxf(M, cp[(size_t)d * hw]);
    float S = 0.0f, SD = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float e = expf(cp[(size_t)d * hw] - M);
        S += e;
        SD = fmaf(e, dv[d], SD);
    }
    const float inv = 1.0f / S;
    const float depth = SD * inv;
    const float gi = gd[p] * inv;
    for (int d = 0; d < D; ++d) {
        const float e = expf(cp[(size_t)d * hw] - M);
        gc[(size_t)d * hw + p] = (e * gi) * (dv[d] - depth);
    }
}

}  // namespace

int launch_warp_variance_backward(const float* feats, const float* rt, const float* dv, const float* g, float* gf,
                                  int N, int D, int h, int w, hipStream_t s) {
    const int ntx = (w + kTX - 1) / kTX, nty = (h + kTY - 1) / kTY;
    const int nslab = (D + kSlab - 1) / kSlab;
    const size_t blocks = (size_t)ntx * nty * nslab * (kC / 8);
    if (blocks >= ((size_t)1 << 31))
        return fail(MVS_ERR_BAD_SHAPE, "warp_variance_backward: %zu blocks exceed the grid", blocks);
    if (int st = check_hip(hipMemsetAsync(gf, 0, (size_t)N * kC * h * w * sizeof(float), s),
                           "warp_variance_backward zero-fill"))
        return st;
    warp_variance_bwd_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(feats, rt, dv, g, gf, N, D, h, w, ntx, ntx * nty,
                                                                   nslab);
    return check_hip(hipGetLastError(), "warp_variance_backward launch");
}

int launch_softargmin_backward(const float* cost, const float* dv, const float* grad_depth, float* grad_cost, int D,
                               int h, int w, hipStream_t s) {
    const int hw = h * w;
    softargmin_bwd_kernel<<<(hw + 127) / 128, 128, 0, s>>>(cost, dv, grad_depth, grad_cost, D, hw);
    return check_hip(hipGetLastError(), "softargmin_backward launch");
}

}  // namespace mvs
