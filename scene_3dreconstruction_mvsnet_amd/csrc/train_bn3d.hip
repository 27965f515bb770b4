// train_bn3d.hip -- training: BatchNorm3d with batch statistics (+ ReLU, + skip addition) of CostRegNet's blocks, its
// backward, and the relayout of the cost volume at the boundary of the training convolutions.
//
// Replaces, for training, the nn.BatchNorm3d + F.relu of models/module.py:26-33 (ConvBnReLU3D) and of
// models/mvsnet.py:47-60 (the three deconvolution blocks), the skip additions of models/mvsnet.py:66-70, and their
// autograd backward.  Data is channels-last [M][C] fp32, M = B*D*H*W voxels (statistics pooled over the batch), C in
// {8, 16, 32, 64}.  This file is compiled with -ffp-contract=off: bn_pre() below is ONE instruction sequence (sub, mul,
// mul, add) wherever it is inlined, so the backward's ReLU mask agrees bit for bit with the sign of the forward's output.
// Forward and backward close the ReLU on !(pre <= 0): a NaN pre-activation passes, value and gradient, as in torch.
//
// Geometry (all five sweep kernels).  A block of 256 threads owns 8 * R consecutive rows, R = 256 / (C / 4); a thread
// owns one float4 (4 channels, group cg = tid % (C/4)) of the rows k = j * R + q, j < 8, q = tid / (C/4): a wave's
// 16-byte accesses are consecutive, 1 KiB per instruction.  The grid is ceil(M / (8 R)) blocks: 1 for the smallest
// layer (M = 12, C = 64), 3,840 of 32 KB each for conv0 at the training shape (M = 3.9 M, C = 8).
//
// Statistics (one read of y).  thread: mean of its <= 8 values, then M2 = sum (v - mean)^2 from the registers;
// block: a tree over q of Chan merges  mean += (mb - ma) nb/n,  M2 = (M2a + M2b) + (mb - ma)^2 na nb/n  in LDS;
// the per-block (mean, M2) pairs go to the workspace (counts follow from the geometry and are not stored);
// bn_stats_final_kernel (one block) merges them in a fixed order: slot s of 256/C takes blocks s, s + S, ... in
// sequence, then a tree over the slots.  No atomics; no E[y^2] - E[y]^2 anywhere.
// Backward sums (sum g, sum g xhat) take the same route with plain additions.
//
// Sweeps: forward reads y twice (statistics, apply), reads skip once, writes out once; backward reads y and grad_out
// twice each (sums, apply) and writes grad_y once.
#include "mvs_internal.h"

namespace mvs {
namespace {

constexpr int kBlock = 256;
constexpr int kRows = 8;   // rows per thread

__host__ __device__ constexpr int rows_per_block(int C) { return kRows * (kBlock / (C / 4)); }

// number of k in [0, nrows) with k % m == q  (q < m)
__device__ __forceinline__ int cls(int q, int m, int nrows) { return q < nrows ? (nrows - q - 1) / m + 1 : 0; }

// the pre-activation; the only place it is written (see the header comment)
__device__ __forceinline__ float bn_xhat(float y, float mean, float invstd) { return (y - mean) * invstd; }
__device__ __forceinline__ float bn_pre(float y, float mean, float invstd, float gamma, float beta) {
    return bn_xhat(y, mean, invstd) * gamma + beta;
}

struct F4 { float v[4]; };
__device__ __forceinline__ F4 ld4(const float* p, size_t i4) {
    const float4 t = reinterpret_cast<const float4*>(p)[i4];
    return F4{{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ void st4(float* p, size_t i4, const F4& a) {
    reinterpret_cast<float4*>(p)[i4] = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
}
__device__ __forceinline__ float sum8(const float (&t)[kRows]) {
    return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

// (ma, qa) of na values absorbs (mb, qb) of nb values; an empty side is (0, 0) and leaves the other unchanged
__device__ __forceinline__ void chan_merge(float& ma, float& qa, float mb, float qb, int na, int nb) {
    const int n = na + nb;
    const float wb = (float)nb / (float)(n > 0 ? n : 1);
    const float wab = (float)na * wb;
    const float d = mb - ma;
    ma = ma + d * wb;
    qa = (qa + qb) + (d * d) * wab;
}

template <int C>
struct Geo {
    static constexpr int G = C / 4, R = kBlock / G, RPB = kRows * R;
    int cg, q, nrows;
    size_t base4;   // float4 index of (row0 + q, cg)
    __device__ Geo(int M) {
        cg = threadIdx.x % G;
        q = threadIdx.x / G;
        const int row0 = blockIdx.x * RPB;          // < M < 2^29
        nrows = M - row0 < RPB ? M - row0 : RPB;
        base4 = (size_t)(row0 + q) * G + cg;
    }
    __device__ bool valid(int j) const { return j * R + q < nrows; }
    __device__ size_t at(int j) const { return base4 + (size_t)j * R * G; }
};

// ------------------------------------------------------------------------------------------------ forward
template <int C>
__global__ __launch_bounds__(kBlock) void bn_stats_kernel(const float* __restrict__ y, int M, float* __restrict__ part) {
    using GE = Geo<C>;
    __shared__ float s_m[kBlock * 4], s_q[kBlock * 4];
    const GE g(M);
    const int tid = threadIdx.x;
    F4 v[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) v[j] = g.valid(j) ? ld4(y, g.at(j)) : F4{{0.f, 0.f, 0.f, 0.f}};
    const int cnt = cls(g.q, GE::R, g.nrows);
    const float fc = (float)(cnt > 0 ? cnt : 1);
    float mean[4], m2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float t[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) t[j] = v[j].v[c];
        mean[c] = sum8(t) / fc;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const float d = v[j].v[c] - mean[c];
            t[j] = j < cnt ? d * d : 0.f;
        }
        m2[c] = sum8(t);
        s_m[tid * 4 + c] = mean[c];
        s_q[tid * 4 + c] = m2[c];
    }
    __syncthreads();
    for (int s = GE::R / 2; s >= 1; s >>= 1) {
        if (g.q < s) {
            const int na = cls(g.q, 2 * s, g.nrows), nb = cls(g.q + s, 2 * s, g.nrows);
            const int o = (tid + s * GE::G) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                chan_merge(mean[c], m2[c], s_m[o + c], s_q[o + c], na, nb);
                s_m[tid * 4 + c] = mean[c];
                s_q[tid * 4 + c] = m2[c];
            }
        }
        __syncthreads();
    }
    if (g.q == 0) {
        st4(part, ((size_t)blockIdx.x * 2 + 0) * GE::G + g.cg, F4{{mean[0], mean[1], mean[2], mean[3]}});
        st4(part, ((size_t)blockIdx.x * 2 + 1) * GE::G + g.cg, F4{{m2[0], m2[1], m2[2], m2[3]}});
    }
}

template <int C>
__global__ __launch_bounds__(kBlock) void bn_stats_final_kernel(const float* __restrict__ part, int nblocks, int M,
                                                                float* __restrict__ save_mean,
                                                                float* __restrict__ save_invstd,
                                                                float* __restrict__ running_mean,
                                                                float* __restrict__ running_var, float momentum,
                                                                float eps) {
    constexpr int S = kBlock / C, RPB = rows_per_block(C);
    __shared__ float s_m[kBlock], s_q[kBlock];
    __shared__ int s_n[kBlock];
    const int tid = threadIdx.x, c = tid % C, slot = tid / C;
    float m = 0.f, q2 = 0.f;
    int n = 0;
    for (int p = slot; p < nblocks; p += S) {
        const int nb = M - p * RPB < RPB ? M - p * RPB : RPB;
        chan_merge(m, q2, part[((size_t)p * 2 + 0) * C + c], part[((size_t)p * 2 + 1) * C + c], n, nb);
        n += nb;
    }
    s_m[tid] = m; s_q[tid] = q2; s_n[tid] = n;
    __syncthreads();
    for (int s = S / 2; s >= 1; s >>= 1) {
        if (slot < s) {
            const int o = tid + s * C;
            chan_merge(m, q2, s_m[o], s_q[o], n, s_n[o]);
            n += s_n[o];
            s_m[tid] = m; s_q[tid] = q2; s_n[tid] = n;
        }
        __syncthreads();
    }
    if (slot == 0) {
        const float var = q2 / (float)M;
        save_mean[c] = m;
        save_invstd[c] = 1.0f / sqrtf(var + eps);
        if (running_mean) {
            const float keep = 1.0f - momentum;
            running_mean[c] = keep * running_mean[c] + momentum * m;
            running_var[c] = keep * running_var[c] + momentum * (q2 / (float)(M - 1));
        }
    }
}

template <int C, bool RELU, bool SKIP>
__global__ __launch_bounds__(kBlock) void bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ skip,
                                                          float* __restrict__ out, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int M) {
    using GE = Geo<C>;
    const GE g(M);
    const F4 mu = ld4(mean, g.cg), is = ld4(invstd, g.cg), ga = ld4(gamma, g.cg), be = ld4(beta, g.cg);
    F4 v[kRows], k[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const bool ok = g.valid(j);
        v[j] = ok ? ld4(y, g.at(j)) : F4{{0.f, 0.f, 0.f, 0.f}};
        if (SKIP) k[j] = ok ? ld4(skip, g.at(j)) : F4{{0.f, 0.f, 0.f, 0.f}};
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        F4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float t = bn_pre(v[j].v[c], mu.v[c], is.v[c], ga.v[c], be.v[c]);
            if (RELU) t = !(t <= 0.f) ? t : 0.f;   // NaN passes, as torch's relu
            if (SKIP) t = t + k[j].v[c];
            r.v[c] = t;
        }
        if (g.valid(j)) st4(out, g.at(j), r);
    }
}

// ------------------------------------------------------------------------------------------------ backward
template <int C, bool RELU>
__global__ __launch_bounds__(kBlock) void bn_bwd_sums_kernel(const float* __restrict__ y, const float* __restrict__ go,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int M,
                                                             float* __restrict__ part) {
    using GE = Geo<C>;
    __shared__ float s_a[kBlock * 4], s_b[kBlock * 4];
    const GE g(M);
    const int tid = threadIdx.x;
    const F4 mu = ld4(mean, g.cg), is = ld4(invstd, g.cg), ga = ld4(gamma, g.cg), be = ld4(beta, g.cg);
    F4 v[kRows], d[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const bool ok = g.valid(j);
        v[j] = ok ? ld4(y, g.at(j)) : F4{{0.f, 0.f, 0.f, 0.f}};
        d[j] = ok ? ld4(go, g.at(j)) : F4{{0.f, 0.f, 0.f, 0.f}};   // a zero gradient adds nothing to either sum
    }
    float sg[4], sx[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float tg[kRows], tx[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            float gm = d[j].v[c];
            if (RELU) gm = !(bn_pre(v[j].v[c], mu.v[c], is.v[c], ga.v[c], be.v[c]) <= 0.f) ? gm : 0.f;   // NaN passes, as torch's
            tg[j] = gm;
            tx[j] = gm * bn_xhat(v[j].v[c], mu.v[c], is.v[c]);
        }
        sg[c] = sum8(tg);
        sx[c] = sum8(tx);
        s_a[tid * 4 + c] = sg[c];
        s_b[tid * 4 + c] = sx[c];
    }
    __syncthreads();
    for (int s = GE::R / 2; s >= 1; s >>= 1) {
        if (g.q < s) {
            const int o = (tid + s * GE::G) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sg[c] = sg[c] + s_a[o + c];
                sx[c] = sx[c] + s_b[o + c];
                s_a[tid * 4 + c] = sg[c];
                s_b[tid * 4 + c] = sx[c];
            }
        }
        __syncthreads();
    }
    if (g.q == 0) {
        st4(part, ((size_t)blockIdx.x * 2 + 0) * GE::G + g.cg, F4{{sg[0], sg[1], sg[2], sg[3]}});
        st4(part, ((size_t)blockIdx.x * 2 + 1) * GE::G + g.cg, F4{{sx[0], sx[1], sx[2], sx[3]}});
    }
}

template <int C>
__global__ __launch_bounds__(kBlock) void bn_bwd_final_kernel(const float* __restrict__ part, int nblocks,
                                                              float* __restrict__ grad_gamma,
                                                              float* __restrict__ grad_beta) {
    constexpr int S = kBlock / C;
    __shared__ float s_a[kBlock], s_b[kBlock];
    const int tid = threadIdx.x, c = tid % C, slot = tid / C;
    float a = 0.f, b = 0.f;
    for (int p = slot; p < nblocks; p += S) {
        a = a + part[((size_t)p * 2 + 0) * C + c];
        b = b + part[((size_t)p * 2 + 1) * C + c];
    }
    s_a[tid] = a; s_b[tid] = b;
    __syncthreads();
    for (int s = S / 2; s >= 1; s >>= 1) {
        if (slot < s) {
            a = a + s_a[tid + s * C];
            b = b + s_b[tid + s * C];
            s_a[tid] = a; s_b[tid] = b;
        }
        __syncthreads();
    }
    if (slot == 0) {
        grad_beta[c] = a;
        grad_gamma[c] = b;
    }
}

template <int C, bool RELU>
__global__ __launch_bounds__(kBlock) void bn_bwd_apply_kernel(const float* __restrict__ y, const float* __restrict__ go,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ grad_gamma,
                                                              const float* __restrict__ grad_beta, int M,
                                                              float* __restrict__ gy) {
    using GE = Geo<C>;
    const GE g(M);
    const F4 mu = ld4(mean, g.cg), is = ld4(invstd, g.cg), ga = ld4(gamma, g.cg), be = ld4(beta, g.cg);
    const F4 gg = ld4(grad_gamma, g.cg), gb = ld4(grad_beta, g.cg);
    const float fm = (float)M;
    float kk[4], mb[4], mg[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        kk[c] = ga.v[c] * is.v[c];
        mb[c] = gb.v[c] / fm;
        mg[c] = gg.v[c] / fm;
    }
    F4 v[kRows], d[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const bool ok = g.valid(j);
        v[j] = ok ? ld4(y, g.at(j)) : F4{{0.f, 0.f, 0.f, 0.f}};
        d[j] = ok ? ld4(go, g.at(j)) : F4{{0.f, 0.f, 0.f, 0.f}};
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        F4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float gm = d[j].v[c];
            if (RELU) gm = !(bn_pre(v[j].v[c], mu.v[c], is.v[c], ga.v[c], be.v[c]) <= 0.f) ? gm : 0.f;   // NaN passes, as torch's
            const float xh = bn_xhat(v[j].v[c], mu.v[c], is.v[c]);
            r.v[c] = kk[c] * ((gm - mb[c]) - xh * mg[c]);
        }
        if (g.valid(j)) st4(gy, g.at(j), r);
    }
}

// ------------------------------------------------------------------------------------------------ relayout
constexpr int kTV = 128;   // voxels per tile

// C8-planar [C/8][V][8] -> channels-last [V][C].  The tile is staged in LDS in the source's order (plane stride padded
// by 4 float4 so that the 16 lanes of a read group hit 16 different 16-byte columns at C = 32) and read back permuted.
template <int C>
__global__ __launch_bounds__(kBlock) void c8_to_cl_kernel(const float* __restrict__ src, float* __restrict__ dst, int V) {
    constexpr int P = C / 8, PS = 2 * kTV + 4, Q = C / 4;
    __shared__ float4 tile[P * PS];
    const int v0 = blockIdx.x * kTV;
    const int nv = V - v0 < kTV ? V - v0 : kTV;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int e = threadIdx.x; e < P * 2 * kTV; e += kBlock) {
        const int p = e / (2 * kTV), f = e % (2 * kTV);           // f = 2 * voxel + half
        if (f < 2 * nv) tile[p * PS + f] = s4[((size_t)p * V + v0) * 2 + f];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kTV * Q; e += kBlock) {
        const int v = e / Q, cq = e % Q;
        if (v < nv) d4[(size_t)(v0 + v) * Q + cq] = tile[(cq >> 1) * PS + 2 * v + (cq & 1)];
    }
}

// channels-last [V][C] -> planar [C][V] (V % 4 == 0).  LDS holds the tile transposed, [C][kTV + 4] floats.
template <int C>
__global__ __launch_bounds__(kBlock) void cl_to_planar_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                              int V) {
    constexpr int LS = kTV + 4, Q = C / 4;
    __shared__ __attribute__((aligned(16))) float tile[C * LS];
    const int v0 = blockIdx.x * kTV;
    const int nv = V - v0 < kTV ? V - v0 : kTV;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int e = threadIdx.x; e < kTV * Q; e += kBlock) {
        const int v = e / Q, cq = e % Q;
        if (v < nv) {
            const float4 t = s4[(size_t)(v0 + v) * Q + cq];
            tile[(4 * cq + 0) * LS + v] = t.x;
            tile[(4 * cq + 1) * LS + v] = t.y;
            tile[(4 * cq + 2) * LS + v] = t.z;
            tile[(4 * cq + 3) * LS + v] = t.w;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < C * (kTV / 4); e += kBlock) {
        const int c = e / (kTV / 4), v = 4 * (e % (kTV / 4));
        if (v < nv)   // nv % 4 == 0
            *reinterpret_cast<float4*>(dst + (size_t)c * V + v0 + v) = *reinterpret_cast<const float4*>(&tile[c * LS + v]);
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool bn_channels(int C) { return C == 8 || C == 16 || C == 32 || C == 64; }

int check_bn_dims(const char* who, int C, long long M) {
    if (!bn_channels(C)) return fail(MVS_ERR_BAD_SHAPE, "%s: C = %d (8, 16, 32 or 64)", who, C);
    if (M < 2)
        return fail(MVS_ERR_BAD_SHAPE, "%s: M = %lld: batch statistics need more than one value per channel", who, M);
    if (M * C >= (1LL << 31))
        return fail(MVS_ERR_BAD_SHAPE, "%s: %lld x %d channels is beyond the kernels' index range (2^31 elements)", who,
                    M, C);
    return MVS_OK;
}

int bn_blocks(int C, int M) { return (M + rows_per_block(C) - 1) / rows_per_block(C); }
size_t bn_workspace(int C, int M) { return ((size_t)bn_blocks(C, M) * 2 * C * 4 + 255) & ~(size_t)255; }

int check_bn_workspace(const char* who, const void* ws, size_t bytes, int C, int M) {
    if (bytes < bn_workspace(C, M))
        return fail(MVS_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, bytes, bn_workspace(C, M));
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(MVS_ERR_WORKSPACE, "%s: workspace not 256-byte aligned", who);
    return MVS_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int C>
int bn_forward(const float* y, const float* gamma, const float* beta, const float* skip, float* out, float* save_mean,
               float* save_invstd, float* rm, float* rv, float momentum, float eps, int relu, int M, float* part,
               hipStream_t s) {
    const int nb = bn_blocks(C, M);
    hipLaunchKernelGGL(bn_stats_kernel<C>, dim3(nb), dim3(kBlock), 0, s, y, M, part);
    hipLaunchKernelGGL(bn_stats_final_kernel<C>, dim3(1), dim3(kBlock), 0, s, part, nb, M, save_mean, save_invstd, rm, rv,
                       momentum, eps);
    if (int st = check_hip(hipGetLastError(), "bn3d_train statistics launch")) return st;
#define MVS_BN_APPLY(r, k)                                                                                         \
    hipLaunchKernelGGL((bn_apply_kernel<C, r, k>), dim3(nb), dim3(kBlock), 0, s, y, skip, out, save_mean, save_invstd, \
                       gamma, beta, M)
    if (relu) { if (skip) MVS_BN_APPLY(true, true); else MVS_BN_APPLY(true, false); }
    else      { if (skip) MVS_BN_APPLY(false, true); else MVS_BN_APPLY(false, false); }
#undef MVS_BN_APPLY
    return check_hip(hipGetLastError(), "bn3d_train apply launch");
}

template <int C>
int bn_backward(const float* y, const float* go, const float* gamma, const float* beta, const float* mean,
                const float* invstd, float* gy, float* gg, float* gb, int relu, int M, float* part, hipStream_t s) {
    const int nb = bn_blocks(C, M);
    if (relu) {
        hipLaunchKernelGGL((bn_bwd_sums_kernel<C, true>), dim3(nb), dim3(kBlock), 0, s, y, go, mean, invstd, gamma, beta,
                           M, part);
    } else {
        hipLaunchKernelGGL((bn_bwd_sums_kernel<C, false>), dim3(nb), dim3(kBlock), 0, s, y, go, mean, invstd, gamma, beta,
                           M, part);
    }
    hipLaunchKernelGGL(bn_bwd_final_kernel<C>, dim3(1), dim3(kBlock), 0, s, part, nb, gg, gb);
    if (int st = check_hip(hipGetLastError(), "bn3d_train backward sums launch")) return st;
    if (relu) {
        hipLaunchKernelGGL((bn_bwd_apply_kernel<C, true>), dim3(nb), dim3(kBlock), 0, s, y, go, mean, invstd, gamma, beta,
                           gg, gb, M, gy);
    } else {
        hipLaunchKernelGGL((bn_bwd_apply_kernel<C, false>), dim3(nb), dim3(kBlock), 0, s, y, go, mean, invstd, gamma,
                           beta, gg, gb, M, gy);
    }
    return check_hip(hipGetLastError(), "bn3d_train backward apply launch");
}

}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_bn3d_train_workspace(int C, long long M, size_t* bytes) {
    if (!bytes) return fail(MVS_ERR_NULL, "mvs_query_bn3d_train_workspace: NULL argument");
    if (int st = check_bn_dims("mvs_query_bn3d_train_workspace", C, M)) return st;
    *bytes = bn_workspace(C, (int)M);
    return MVS_OK;
}

int mvs_bn3d_train_forward(const float* y, const float* gamma, const float* beta, const float* skip, float* out,
                           float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                           float momentum, float eps, int relu, int C, long long M, void* workspace,
                           size_t workspace_bytes, void* stream) {
    const char* who = "mvs_bn3d_train_forward";
    if (!y || !gamma || !beta || !out || !save_mean || !save_invstd || !workspace)
        return fail(MVS_ERR_NULL, "%s: NULL argument", who);
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(MVS_ERR_NULL, "%s: running_mean and running_var must both be given or both be NULL", who);
    if (int st = check_bn_dims(who, C, M)) return st;
    if (!aligned16(y) || !aligned16(out) || !aligned16(skip) || !aligned16(gamma) || !aligned16(beta) ||
        !aligned16(save_mean) || !aligned16(save_invstd))
        return fail(MVS_ERR_BAD_SHAPE, "%s: a tensor is not aligned to 16 bytes", who);
    if (int st = check_bn_workspace(who, workspace, workspace_bytes, C, (int)M)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
#define MVS_BN_FWD(c)                                                                                               \
    if (C == c) return bn_forward<c>(y, gamma, beta, skip, out, save_mean, save_invstd, running_mean, running_var, \
                                     momentum, eps, relu, (int)M, part, s)
    MVS_BN_FWD(8); MVS_BN_FWD(16); MVS_BN_FWD(32); MVS_BN_FWD(64);
#undef MVS_BN_FWD
    return fail(MVS_ERR_BAD_SHAPE, "%s: no kernel", who);
}

int mvs_bn3d_train_backward(const float* y, const float* grad_out, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, float* grad_y, float* grad_gamma,
                            float* grad_beta, int relu, int C, long long M, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const char* who = "mvs_bn3d_train_backward";
    if (!y || !grad_out || !gamma || !beta || !save_mean || !save_invstd || !grad_y || !grad_gamma || !grad_beta ||
        !workspace)
        return fail(MVS_ERR_NULL, "%s: NULL argument", who);
    if (int st = check_bn_dims(who, C, M)) return st;
    if (!aligned16(y) || !aligned16(grad_out) || !aligned16(grad_y) || !aligned16(gamma) || !aligned16(beta) ||
        !aligned16(save_mean) || !aligned16(save_invstd) || !aligned16(grad_gamma) || !aligned16(grad_beta))
        return fail(MVS_ERR_BAD_SHAPE, "%s: a tensor is not aligned to 16 bytes", who);
    if (int st = check_bn_workspace(who, workspace, workspace_bytes, C, (int)M)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace);
#define MVS_BN_BWD(c)                                                                                          \
    if (C == c) return bn_backward<c>(y, grad_out, gamma, beta, save_mean, save_invstd, grad_y, grad_gamma, \
                                      grad_beta, relu, (int)M, part, s)
    MVS_BN_BWD(8); MVS_BN_BWD(16); MVS_BN_BWD(32); MVS_BN_BWD(64);
#undef MVS_BN_BWD
    return fail(MVS_ERR_BAD_SHAPE, "%s: no kernel", who);
}

int mvs_volume_relayout(const float* src, float* dst, int C, long long V, int direction, void* stream) {
    const char* who = "mvs_volume_relayout";
    if (!src || !dst) return fail(MVS_ERR_NULL, "%s: NULL argument", who);
    if (!bn_channels(C)) return fail(MVS_ERR_BAD_SHAPE, "%s: C = %d (8, 16, 32 or 64)", who, C);
    if (direction != MVS_RELAYOUT_C8_TO_CHANNELS_LAST && direction != MVS_RELAYOUT_CHANNELS_LAST_TO_PLANAR)
        return fail(MVS_ERR_BAD_SHAPE, "%s: direction %d (0 or 1)", who, direction);
    if (V < 1 || (V & 3)) return fail(MVS_ERR_BAD_SHAPE, "%s: V = %lld (a positive multiple of 4)", who, V);
    if (V * C >= (1LL << 31))
        return fail(MVS_ERR_BAD_SHAPE, "%s: %lld x %d channels is beyond the kernels' index range (2^31 elements)", who,
                    V, C);
    if (!aligned16(src) || !aligned16(dst)) return fail(MVS_ERR_BAD_SHAPE, "%s: a volume is not aligned to 16 bytes", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int v = (int)V, nb = (v + kTV - 1) / kTV;
#define MVS_RELAYOUT(c)                                                                              \
    if (C == c) {                                                                                    \
        if (direction == MVS_RELAYOUT_C8_TO_CHANNELS_LAST)                                           \
            hipLaunchKernelGGL(c8_to_cl_kernel<c>, dim3(nb), dim3(kBlock), 0, s, src, dst, v);       \
        else                                                                                         \
            hipLaunchKernelGGL(cl_to_planar_kernel<c>, dim3(nb), dim3(kBlock), 0, s, src, dst, v);   \
    }
    MVS_RELAYOUT(8) MVS_RELAYOUT(16) MVS_RELAYOUT(32) MVS_RELAYOUT(64)
#undef MVS_RELAYOUT
    return check_hip(hipGetLastError(), "volume_relayout launch");
}

}  // extern "C"
