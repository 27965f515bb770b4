// train_conv3d.hip -- CostRegNet's 3x3x3 convolutions in their TRAINING form (raw: no folded BN, no ReLU), fp32 in and
// fp32 accumulate on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32:
//
//   conv_kernel<KC, NC, kFwd1|kFwd2>   y[co][o] = sum_{ci,tap} w[co][ci][tap] x[ci][S o + tap - 1] (+ bias), zero padding
//   conv_kernel<KC, NC, kDgrad2>       the adjoint of kFwd2 (= ConvTranspose3d(k=3, s=2, p=1, output_padding=1) forward)
//   wgrad_kernel<XC, GC, S> + wgrad_reduce_kernel
//                                      gw[co][ci][tap] = sum_o gy[co][o] x[ci][S o + tap - 1], gbias[co] = sum_o gy[co][o]
//
// Two identities keep it at three families for the eleven layers: the transposed layers' forward IS the data gradient
// of the stride-2 conv with the same weight tensor (and their data gradient its forward); the data gradient of a
// stride-1 conv is a stride-1 conv with the taps flipped and the channel pair transposed (`flip` below, an index
// change in the weight staging only).
//
// Layout.  Volumes are channels-last, [D][H][W][C] per batch item (torch's channels_last_3d of a [1,C,D,H,W] tensor;
// a 1-channel volume is a plain [D][H][W]): torch's BatchNorm3d / relu take that memory format without a copy and a
// voxel's channels are one contiguous 32..256-byte vector.  Weights are read in the reference layouts straight from
// device memory ([Cout][Cin][27]; the transposed layers' [Cin_T][Cout_T][27] is the same thing for the conv they are
// the adjoint of): they change every step, so there is no packed blob and no host round trip.
//
// conv_kernel: implicit GEMM, M = 16 output voxels along x (one "tile"), N = output channels padded to 16,
// K = 27 taps x reduction channels.  A wave owns MT tiles at consecutive y (so the three ky taps re-read rows from L1)
// and all N tiles; a lane's A operand for a tap is ONE 4/8/16-byte load of its voxel's channels
// [CPL (l>>4) .. + CPL) of a 4 CPL-channel chunk, which feeds CPL matrix instructions (the k order inside a chunk is
// permuted to match; the weight image in LDS is written in that order, lane-linear, so B is a conflict-free
// ds_read_b32).  Weights are staged per block, TPS taps at a time (all 27 when they fit 56 KB).  kDgrad2 runs the same
// loop over the eight output parity classes: a class keeps the 1, 2, 4 or 8 taps whose parity matches, per axis
// even -> k = 1, odd -> k = 0 (input + 1) and k = 2.
//
// wgrad_kernel: GEMM with M = gy channels, N = x channels, K = output voxels, 4 per instruction.  Split-K without
// atomics: a block owns a fixed range of (z, y) output rows and TW taps, its four waves take rows round-robin, add
// their accumulators in wave order through LDS and write one partial [Cout][Cin][27] slab (and gbias row) to the
// caller's workspace; wgrad_reduce_kernel sums the slabs in a fixed order.  The result is bit-identical from run to
// run and from stream to stream (the split depends on the shape only).
//
// Resources of the three conv0 instantiations (gfx950, -Rpass-analysis=kernel-resource-usage; no kernel of this file
// uses scratch): forward conv_kernel<32,8,kFwd1> 108 VGPR, 55,296 B LDS, 2 waves/SIMD (LDS-bound); data gradient
// conv_kernel<8,32,kFwd1> 100 VGPR, 27,648 B, 4 waves/SIMD; weight gradient wgrad_kernel<32,8,1> 120 VGPR, 18,688 B,
// 4 waves/SIMD.  Measured times and what limits them: DESIGN.md section 11.1.
#include "mvs_internal.h"

namespace mvs {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kBlock = 256;   // 4 waves

enum ConvMode { kFwd1 = 0, kFwd2 = 1, kDgrad2 = 2 };

template <int KC, int NC>
struct ConvCfg {
    static constexpr int CPL = KC >= 16 ? 4 : KC >= 8 ? 2 : 1;   // channels per lane per chunk (one load)
    static constexpr int CH = 4 * CPL;                           // channels per chunk = CPL instructions of k = 4
    static constexpr int NCH = (KC + CH - 1) / CH;
    static constexpr int NT = (NC + 15) / 16;
    static constexpr int MT = NT <= 2 ? 8 : 4;                   // <= 16 accumulator tiles (64 registers)
    static constexpr int TAP_FLOATS = NCH * CPL * NT * 64;       // = padded KC x padded NC
    static constexpr int TPS = 27 * TAP_FLOATS * 4 <= 56 * 1024 ? 27
                             : 9 * TAP_FLOATS * 4 <= 56 * 1024 ? 9
                             : 3 * TAP_FLOATS * 4 <= 56 * 1024 ? 3 : 1;
    static constexpr bool PADDED = (NCH * CH != KC) || (NT * 16 != NC);
};

struct ConvDims {
    int Di, Hi, Wi;   // volume the A operand is read from
    int Do, Ho, Wo;   // volume written
    int Zt, Yt, Xt;   // tile space per parity class (= output dims; for kDgrad2 the input dims)
    int ngy, ntx, ngroups;
};

template <int KC, int NC, int MODE>
__global__ __launch_bounds__(kBlock, 2) void conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y,
                                                         ConvDims d, int flip) {
    using C = ConvCfg<KC, NC>;
    constexpr int CPL = C::CPL, CH = C::CH, NCH = C::NCH, NT = C::NT, MT = C::MT, TPS = C::TPS;
    __shared__ float wl[TPS * C::TAP_FLOATS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, kgrp = lane >> 4;

    // this wave's group of MT tiles: (parity class, z, x tile, y group), y group fastest
    int g = blockIdx.x * 4 + wave;
    const bool active = g < d.ngroups;
    const int yg = g % d.ngy;
    g /= d.ngy;
    const int xt = g % d.ntx;
    g /= d.ntx;
    const int z = g % d.Zt;
    const int cls = g / d.Zt;                      // 0 unless kDgrad2
    const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
    const int y0 = yg * MT, xo = xt * 16 + row;    // this lane's A voxel column in tile space

    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (C::PADDED) {
        for (int e = tid; e < TPS * C::TAP_FLOATS; e += kBlock) wl[e] = 0.f;
        __syncthreads();
    }
    const bool swapped = MODE == kDgrad2 || flip;   // weight tensor is [reduction channel][output channel][27]
    const bool cvalid = CPL * kgrp < KC || NCH > 1; // KC < 4: the upper k groups are padding (NCH > 1: KC % CH == 0)

    for (int s = 0; s < 27 / TPS; ++s) {
        if (s) __syncthreads();
        for (int e = tid; e < KC * NC * TPS; e += kBlock) {
            const int pair = e / TPS, tl = e - pair * TPS, tap = s * TPS + tl;
            const int a = pair / (swapped ? NC : KC), b = pair - a * (swapped ? NC : KC);
            const int kc = swapped ? a : b, nc = swapped ? b : a;
            const int gt = (flip && MODE != kDgrad2) ? 26 - tap : tap;
            const int chunk = kc / CH, rem = kc - chunk * CH, kg = rem / CPL, j = rem - kg * CPL;
            wl[(((tl * NCH + chunk) * CPL + j) * NT + (nc >> 4)) * 64 + kg * 16 + (nc & 15)] = w[pair * 27 + gt];
        }
        __syncthreads();
        if (!active) continue;
        for (int tl = 0; tl < TPS; ++tl) {
            const int tap = s * TPS + tl;
            const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
            int iz, ix;
            if (MODE == kDgrad2) {
                if ((pz ? kz == 1 : kz != 1) || (py ? ky == 1 : ky != 1) || (px ? kx == 1 : kx != 1)) continue;
                iz = z + (kz == 0);
                ix = xo + (kx == 0);
            } else {
                constexpr int S = MODE == kFwd2 ? 2 : 1;
                iz = S * z + kz - 1;
                ix = S * xo + kx - 1;
            }
            if (iz < 0 || iz >= d.Di) continue;
            const bool xvalid = ix >= 0 && ix < d.Wi && xo < d.Xt && cvalid;
#pragma unroll
            for (int chunk = 0; chunk < NCH; ++chunk) {
                float a[MT][CPL];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int yo = y0 + m;
                    int iy;
                    if (MODE == kDgrad2) iy = yo + (ky == 0);
                    else iy = (MODE == kFwd2 ? 2 : 1) * yo + ky - 1;
                    const bool ok = xvalid && yo < d.Yt && iy >= 0 && iy < d.Hi;
                    const float* p = x + ((size_t)(iz * d.Hi + (ok ? iy : 0)) * d.Wi + (ok ? ix : 0)) * KC
                                       + chunk * CH + (cvalid ? CPL * kgrp : 0);
                    if constexpr (CPL == 4) {
                        const float4 v = ok ? *reinterpret_cast<const float4*>(p) : float4{0.f, 0.f, 0.f, 0.f};
                        a[m][0] = v.x; a[m][1] = v.y; a[m][2] = v.z; a[m][3] = v.w;
                    } else if constexpr (CPL == 2) {
                        const float2 v = ok ? *reinterpret_cast<const float2*>(p) : float2{0.f, 0.f};
                        a[m][0] = v.x; a[m][1] = v.y;
                    } else {
                        a[m][0] = ok ? *p : 0.f;
                    }
                }
#pragma unroll
                for (int j = 0; j < CPL; ++j)
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const float b = wl[(((tl * NCH + chunk) * CPL + j) * NT + n) * 64 + lane];
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][j], b, acc[m][n], 0, 0, 0);
                    }
            }
        }
    }
    if (!active) return;
    // C/D map of 16x16x4: column = lane & 15 (output channel), row = 4 (lane >> 4) + register (voxel of the tile)
    const int oz = MODE == kDgrad2 ? 2 * z + pz : z;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int co = n * 16 + row;
        if (co >= NC) continue;
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int yo = y0 + m;
            if (yo >= d.Yt) continue;
            const int oy = MODE == kDgrad2 ? 2 * yo + py : yo;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int xv = xt * 16 + kgrp * 4 + r;
                if (xv >= d.Xt) continue;
                const int ox = MODE == kDgrad2 ? 2 * xv + px : xv;
                y[((size_t)(oz * d.Ho + oy) * d.Wo + ox) * NC + co] = acc[m][n][r] + bv;
            }
        }
    }
}

// ---------------------------------------------------------------- weight gradient
template <int XC, int GC>
struct WgradCfg {
    static constexpr int CPLB = XC >= 16 ? XC / 16 : 1;     // x channels per lane: 16 lanes x CPLB cover a voxel
    static constexpr int MTC = (GC + 15) / 16;
    static constexpr int TILES1 = MTC * CPLB;               // accumulator tiles per tap
    static constexpr int TW = 9 * TILES1 <= 24 ? 9 : 3 * TILES1 <= 24 ? 3 : 1;   // taps per block
    static constexpr int TILES = TW * TILES1;
};

struct WgradDims {
    int D, H, W;      // x volume
    int Do, Ho, Wo;   // gy volume
    int rpc;          // output rows (z, y) per block
};

template <int XC, int GC, int S>
__global__ __launch_bounds__(kBlock, 2) void wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                          float* __restrict__ part, float* __restrict__ bpart,
                                                          WgradDims d) {
    using C = WgradCfg<XC, GC>;
    constexpr int CPLB = C::CPLB, MTC = C::MTC, TW = C::TW, TILES = C::TILES;
    __shared__ float red[TILES * 256 + 4 * MTC * 16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kgrp = lane >> 4;
    const int chunk = blockIdx.x, tap0 = blockIdx.y * TW;
    const int rows = d.Do * d.Ho;
    const int r0 = chunk * d.rpc, r1 = min(r0 + d.rpc, rows);

    f32x4 acc[TW][MTC][CPLB];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int m = 0; m < MTC; ++m)
#pragma unroll
            for (int j = 0; j < CPLB; ++j) acc[t][m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum[MTC];
#pragma unroll
    for (int m = 0; m < MTC; ++m) bsum[m] = 0.f;
    const bool bvalid = CPLB * col < XC;

    for (int r = r0 + wave; r < r1; r += 4) {
        const int zo = r / d.Ho, yo = r - zo * d.Ho;
        const float* grow = gy + (size_t)r * d.Wo * GC;
        for (int x4 = 0; x4 < d.Wo; x4 += 4) {
            const int xo = x4 + kgrp;
            const bool vo = xo < d.Wo;
            float a[MTC];
#pragma unroll
            for (int m = 0; m < MTC; ++m) {
                const bool ok = vo && m * 16 + col < GC;
                a[m] = ok ? grow[(size_t)xo * GC + m * 16 + col] : 0.f;
                bsum[m] += a[m];
            }
#pragma unroll
            for (int t = 0; t < TW; ++t) {
                const int tap = tap0 + t;
                const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
                const int iz = S * zo + kz - 1, iy = S * yo + ky - 1, ix = S * xo + kx - 1;
                const bool ok = vo && bvalid && iz >= 0 && iz < d.D && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
                const float* p = x + ((size_t)((ok ? iz : 0) * d.H + (ok ? iy : 0)) * d.W + (ok ? ix : 0)) * XC
                                   + (bvalid ? CPLB * col : 0);
                float b[CPLB];
                if constexpr (CPLB == 4) {
                    const float4 v = ok ? *reinterpret_cast<const float4*>(p) : float4{0.f, 0.f, 0.f, 0.f};
                    b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
                } else if constexpr (CPLB == 2) {
                    const float2 v = ok ? *reinterpret_cast<const float2*>(p) : float2{0.f, 0.f};
                    b[0] = v.x; b[1] = v.y;
                } else {
                    b[0] = ok ? *p : 0.f;
                }
#pragma unroll
                for (int m = 0; m < MTC; ++m)
#pragma unroll
                    for (int j = 0; j < CPLB; ++j)
                        acc[t][m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[j], acc[t][m][j], 0, 0, 0);
            }
        }
    }

    // the four waves add up in wave order (fixed), then the block writes its slab
    float* bred = red + TILES * 256;
#pragma unroll
    for (int m = 0; m < MTC; ++m) {
        float v = bsum[m];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (kgrp == 0) bred[(wave * MTC + m) * 16 + col] = v;
    }
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int t = 0; t < TW; ++t)
#pragma unroll
                for (int m = 0; m < MTC; ++m)
#pragma unroll
                    for (int j = 0; j < CPLB; ++j)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float* pr = red + ((((t * MTC + m) * CPLB + j) * 4 + q) * 64 + lane);
                            *pr = wv ? *pr + acc[t][m][j][q] : acc[t][m][j][q];
                        }
        }
        __syncthreads();
    }
    constexpr int E = GC * XC * 27;
    float* slab = part + (size_t)chunk * E;
    for (int e = tid; e < TILES * 256; e += kBlock) {
        const int ln = e & 63, q = (e >> 6) & 3;
        int f = e >> 8;
        const int j = f % CPLB;
        f /= CPLB;
        const int m = f % MTC, t = f / MTC;
        const int co = m * 16 + (ln >> 4) * 4 + q, ci = CPLB * (ln & 15) + j;   // C/D map: row = 4 (lane>>4) + reg
        if (co < GC && ci < XC) slab[(co * XC + ci) * 27 + tap0 + t] = red[e];
    }
    if (blockIdx.y == 0 && tid < GC) {
        const int m = tid >> 4, c = tid & 15;
        bpart[(size_t)chunk * GC + tid] = ((bred[(0 * MTC + m) * 16 + c] + bred[(1 * MTC + m) * 16 + c])
                                           + bred[(2 * MTC + m) * 16 + c]) + bred[(3 * MTC + m) * 16 + c];
    }
}

// out[e] = sum over the slabs, fixed order: four interleaved chains per element, combined as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(kBlock) void wgrad_reduce_kernel(const float* __restrict__ part, int E, int nchunks,
                                                              float* __restrict__ out) {
    __shared__ float sm[4][64];
    const int el = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + el;
    float s = 0.f;
    if (e < E)
        for (int c = q; c < nchunks; c += 4) s += part[(size_t)c * E + e];
    sm[q][el] = s;
    __syncthreads();
    if (q == 0 && e < E) out[e] = (sm[0][el] + sm[1][el]) + (sm[2][el] + sm[3][el]);
}

// ---------------------------------------------------------------- host side
struct Pair { int cin, cout; };
// conv channel pairs of CostRegNet by stride (models/mvsnet.py:36-62)
constexpr Pair kPairs1[] = {{32, 8}, {16, 16}, {32, 32}, {64, 64}, {8, 1}};
constexpr Pair kPairs2[] = {{8, 16}, {16, 32}, {32, 64}};

bool conv_pair(int cin, int cout, int stride) {
    if (stride == 1) { for (const Pair& p : kPairs1) if (p.cin == cin && p.cout == cout) return true; }
    if (stride == 2) { for (const Pair& p : kPairs2) if (p.cin == cin && p.cout == cout) return true; }
    return false;
}

// D, H, W: conv input dims.  Refuses what the kernels' int indices cannot address.
int check_conv_dims(const char* who, int Cin, int Cout, int D, int H, int W, int stride) {
    if (stride != 1 && stride != 2) return fail(MVS_ERR_BAD_SHAPE, "%s: stride %d (1 or 2)", who, stride);
    if (D < 1 || H < 1 || W < 1) return fail(MVS_ERR_BAD_SHAPE, "%s: D,H,W = %d,%d,%d", who, D, H, W);
    if (stride == 2 && ((D | H | W) & 1))
        return fail(MVS_ERR_BAD_SHAPE, "%s: stride 2 needs even D,H,W (got %d,%d,%d)", who, D, H, W);
    if (Cin < 1 || Cout < 1) return fail(MVS_ERR_BAD_SHAPE, "%s: Cin,Cout = %d,%d", who, Cin, Cout);
    const size_t vox = (size_t)D * H * W, cmax = Cin > Cout ? Cin : Cout;
    if ((size_t)D * H >= ((size_t)1 << 31) || vox >= ((size_t)1 << 31) || vox * cmax >= ((size_t)1 << 31))
        return fail(MVS_ERR_BAD_SHAPE, "%s: %d x %d x %d x %d channels is beyond the kernels' index range (2^31 elements)",
                    who, D, H, W, (int)cmax);
    return MVS_OK;
}

bool aligned(const void* p, int C) {
    const int a = C >= 4 ? 16 : C >= 2 ? 8 : 4;
    return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

template <int KC, int NC, int MODE>
int launch_conv(const float* x, const float* w, const float* bias, float* y, int Di, int Hi, int Wi, int flip,
                hipStream_t s) {
    using C = ConvCfg<KC, NC>;
    ConvDims d{};
    d.Di = Di; d.Hi = Hi; d.Wi = Wi;
    if (MODE == kFwd1) { d.Do = Di; d.Ho = Hi; d.Wo = Wi; }
    if (MODE == kFwd2) { d.Do = Di / 2; d.Ho = Hi / 2; d.Wo = Wi / 2; }
    if (MODE == kDgrad2) { d.Do = 2 * Di; d.Ho = 2 * Hi; d.Wo = 2 * Wi; }
    d.Zt = MODE == kDgrad2 ? Di : d.Do;
    d.Yt = MODE == kDgrad2 ? Hi : d.Ho;
    d.Xt = MODE == kDgrad2 ? Wi : d.Wo;
    d.ngy = (d.Yt + C::MT - 1) / C::MT;
    d.ntx = (d.Xt + 15) / 16;
    const size_t groups = (size_t)(MODE == kDgrad2 ? 8 : 1) * d.Zt * d.ntx * d.ngy;
    if (groups >= ((size_t)1 << 31)) return fail(MVS_ERR_BAD_SHAPE, "conv3d_train: too many tiles");
    d.ngroups = (int)groups;
    hipLaunchKernelGGL((conv_kernel<KC, NC, MODE>), dim3((unsigned)((groups + 3) / 4)), dim3(kBlock), 0, s, x, w, bias,
                       y, d, flip);
    return check_hip(hipGetLastError(), "conv3d_train kernel launch");
}

// y = conv(x): (Cin, Cout) the channels of x and y.  flip: w is [Cin][Cout][27] and the taps run backwards.
int conv_forward(const float* x, const float* w, const float* bias, float* y, int Cin, int Cout, int D, int H, int W,
                 int stride, int flip, hipStream_t s) {
#define MVS_TC_FWD(ci, co, mode)                                                             \
    if (Cin == ci && Cout == co) return launch_conv<ci, co, mode>(x, w, bias, y, D, H, W, flip, s)
    if (stride == 1) {
        MVS_TC_FWD(32, 8, kFwd1); MVS_TC_FWD(16, 16, kFwd1); MVS_TC_FWD(32, 32, kFwd1); MVS_TC_FWD(64, 64, kFwd1);
        MVS_TC_FWD(8, 1, kFwd1); MVS_TC_FWD(8, 32, kFwd1); MVS_TC_FWD(1, 8, kFwd1);
    } else {
        MVS_TC_FWD(8, 16, kFwd2); MVS_TC_FWD(16, 32, kFwd2); MVS_TC_FWD(32, 64, kFwd2);
    }
#undef MVS_TC_FWD
    return fail(MVS_ERR_BAD_SHAPE, "conv3d_train: no kernel for Cin,Cout,stride = %d,%d,%d", Cin, Cout, stride);
}

// gx = adjoint of the stride-2 conv (Cin -> Cout, input dims D,H,W) applied to gy [D/2][H/2][W/2][Cout]
int conv_dgrad2(const float* gy, const float* w, float* gx, int Cin, int Cout, int D, int H, int W, hipStream_t s) {
#define MVS_TC_DG(ci, co)                                                                    \
    if (Cin == ci && Cout == co) return launch_conv<co, ci, kDgrad2>(gy, w, nullptr, gx, D / 2, H / 2, W / 2, 0, s)
    MVS_TC_DG(8, 16); MVS_TC_DG(16, 32); MVS_TC_DG(32, 64);
#undef MVS_TC_DG
    return fail(MVS_ERR_BAD_SHAPE, "conv3d_train: no data-gradient kernel for Cin,Cout = %d,%d, stride 2", Cin, Cout);
}

int wgrad_tw(int Cin, int Cout) {
    const int tiles1 = ((Cout + 15) / 16) * (Cin >= 16 ? Cin / 16 : 1);
    return 9 * tiles1 <= 24 ? 9 : 3 * tiles1 <= 24 ? 3 : 1;
}

struct WgradPlan { int rpc, nchunks; size_t part_bytes, bias_bytes; };
WgradPlan wgrad_plan(int Cin, int Cout, int D, int H, int W, int stride) {
    WgradPlan p{};
    const int rows = (D / stride) * (H / stride);
    const int target = 1024 * wgrad_tw(Cin, Cout) / 27;   // blocks = chunks x (27 / TW) ~ 1024
    p.rpc = (rows + target - 1) / target;
    p.nchunks = (rows + p.rpc - 1) / p.rpc;
    p.part_bytes = ((size_t)p.nchunks * Cout * Cin * 27 * 4 + 255) & ~(size_t)255;
    p.bias_bytes = ((size_t)p.nchunks * Cout * 4 + 255) & ~(size_t)255;
    return p;
}

template <int XC, int GC, int S>
int launch_wgrad(const float* x, const float* gy, float* gw, float* gbias, float* ws, const WgradPlan& p, int D, int H,
                 int W, hipStream_t s) {
    using C = WgradCfg<XC, GC>;
    WgradDims d{D, H, W, D / S, H / S, W / S, p.rpc};
    float* part = ws;
    float* bpart = ws + p.part_bytes / 4;
    hipLaunchKernelGGL((wgrad_kernel<XC, GC, S>), dim3(p.nchunks, 27 / C::TW), dim3(kBlock), 0, s, x, gy, part, bpart,
                       d);
    if (int st = check_hip(hipGetLastError(), "conv3d_train weight-gradient launch")) return st;
    constexpr int E = GC * XC * 27;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((E + 63) / 64), dim3(kBlock), 0, s, part, E, p.nchunks, gw);
    if (gbias)
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((GC + 63) / 64), dim3(kBlock), 0, s, bpart, GC, p.nchunks, gbias);
    return check_hip(hipGetLastError(), "conv3d_train weight-gradient reduction launch");
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_conv3d_train_workspace(int Cin, int Cout, int D, int H, int W, int stride, size_t* bytes) {
    if (!bytes) return fail(MVS_ERR_NULL, "mvs_query_conv3d_train_workspace: NULL argument");
    if (int st = check_conv_dims("mvs_query_conv3d_train_workspace", Cin, Cout, D, H, W, stride)) return st;
    if (!conv_pair(Cin, Cout, stride))
        return fail(MVS_ERR_BAD_SHAPE, "mvs_query_conv3d_train_workspace: no kernel for Cin,Cout,stride = %d,%d,%d", Cin,
                    Cout, stride);
    const WgradPlan p = wgrad_plan(Cin, Cout, D, H, W, stride);
    *bytes = p.part_bytes + p.bias_bytes;
    return MVS_OK;
}

int mvs_conv3d_train_forward(const float* x, const float* w, const float* bias, float* y, int Cin, int Cout, int D,
                             int H, int W, int stride, int flip_transpose, void* stream) {
    if (!x || !w || !y) return fail(MVS_ERR_NULL, "mvs_conv3d_train_forward: NULL argument");
    if (int st = check_conv_dims("mvs_conv3d_train_forward", Cin, Cout, D, H, W, stride)) return st;
    const bool known = flip_transpose ? (stride == 1 && conv_pair(Cout, Cin, 1)) : conv_pair(Cin, Cout, stride);
    if (!known || (flip_transpose != 0 && flip_transpose != 1))
        return fail(MVS_ERR_BAD_SHAPE, "mvs_conv3d_train_forward: no kernel for Cin,Cout,stride,flip_transpose = "
                    "%d,%d,%d,%d", Cin, Cout, stride, flip_transpose);
    if (!aligned(x, Cin) || !aligned(y, Cout))
        return fail(MVS_ERR_BAD_SHAPE, "mvs_conv3d_train_forward: a volume is not aligned to its channel vector");
    return conv_forward(x, w, bias, y, Cin, Cout, D, H, W, stride, flip_transpose, static_cast<hipStream_t>(stream));
}

int mvs_conv3d_train_backward_data(const float* gy, const float* w, float* gx, int Cin, int Cout, int D, int H, int W,
                                   int stride, void* stream) {
    if (!gy || !w || !gx) return fail(MVS_ERR_NULL, "mvs_conv3d_train_backward_data: NULL argument");
    if (int st = check_conv_dims("mvs_conv3d_train_backward_data", Cin, Cout, D, H, W, stride)) return st;
    if (!conv_pair(Cin, Cout, stride))
        return fail(MVS_ERR_BAD_SHAPE, "mvs_conv3d_train_backward_data: no kernel for Cin,Cout,stride = %d,%d,%d", Cin,
                    Cout, stride);
    if (!aligned(gy, Cout) || !aligned(gx, Cin))
        return fail(MVS_ERR_BAD_SHAPE, "mvs_conv3d_train_backward_data: a volume is not aligned to its channel vector");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (stride == 1) return conv_forward(gy, w, nullptr, gx, Cout, Cin, D, H, W, 1, 1, s);
    return conv_dgrad2(gy, w, gx, Cin, Cout, D, H, W, s);
}

int mvs_conv3d_train_backward_weight(const float* x, const float* gy, float* gw, float* gbias, void* workspace,
                                     size_t workspace_bytes, int Cin, int Cout, int D, int H, int W, int stride,
                                     void* stream) {
    if (!x || !gy || !gw || !workspace) return fail(MVS_ERR_NULL, "mvs_conv3d_train_backward_weight: NULL argument");
    if (int st = check_conv_dims("mvs_conv3d_train_backward_weight", Cin, Cout, D, H, W, stride)) return st;
    if (!conv_pair(Cin, Cout, stride))
        return fail(MVS_ERR_BAD_SHAPE, "mvs_conv3d_train_backward_weight: no kernel for Cin,Cout,stride = %d,%d,%d",
                    Cin, Cout, stride);
    if (!aligned(x, Cin) || !aligned(gy, 1))
        return fail(MVS_ERR_BAD_SHAPE, "mvs_conv3d_train_backward_weight: a volume is not aligned to its channel vector");
    const WgradPlan p = wgrad_plan(Cin, Cout, D, H, W, stride);
    if (workspace_bytes < p.part_bytes + p.bias_bytes)
        return fail(MVS_ERR_WORKSPACE, "mvs_conv3d_train_backward_weight: workspace %zu < %zu bytes", workspace_bytes,
                    p.part_bytes + p.bias_bytes);
    if (reinterpret_cast<uintptr_t>(workspace) & 255)
        return fail(MVS_ERR_WORKSPACE, "mvs_conv3d_train_backward_weight: workspace not 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
#define MVS_TC_WG(ci, co, st)                                                                \
    if (Cin == ci && Cout == co && stride == st) return launch_wgrad<ci, co, st>(x, gy, gw, gbias, ws, p, D, H, W, s)
    MVS_TC_WG(32, 8, 1); MVS_TC_WG(16, 16, 1); MVS_TC_WG(32, 32, 1); MVS_TC_WG(64, 64, 1); MVS_TC_WG(8, 1, 1);
    MVS_TC_WG(8, 16, 2); MVS_TC_WG(16, 32, 2); MVS_TC_WG(32, 64, 2);
#undef MVS_TC_WG
    return fail(MVS_ERR_BAD_SHAPE, "mvs_conv3d_train_backward_weight: no kernel");
}

}  // extern "C"
