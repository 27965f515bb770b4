// mfma16_ops.h -- device helpers of the 16-bit MFMA kernels (conv3d_mfma16.hip, conv11_prob.hip, conv0_split.hip):
// the 16-byte fragment types, v_mfma_f32_16x16x32_{f16,bf16}, the split of an fp32 value into the sum of three bf16
// numbers (RNE, exact residuals) that the SPLIT-OPERAND kernels run their six cross products on, and the XCD-aware
// block order of the tile and z-marching kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "mvs_internal.h"
#include "storage.h"

namespace mvs {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// one 16x16x32 MFMA on 16-byte fragments (8 elements of DT = MVS_F16 / MVS_BF16 per lane)
template <int DT>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
    if (DT == MVS_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// 8 16-bit elements of DT (one voxel of one C8 plane) -> 8 floats
template <int DT>
__device__ __forceinline__ void unpack8(u32x4 v, float (&o)[8]) {
    if (DT == MVS_F16) {
        const f16x8 h = __builtin_bit_cast(f16x8, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (float)h[i];
    } else {
        const bf16x8 h = __builtin_bit_cast(bf16x8, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (float)h[i];
    }
}

// packed = (bf16(a.x), bf16(a.y)) RNE; returns a - widen(packed) (exact).  (Tried: the residual as one
// v_dot2c_f32_bf16 per value, D += h . (-1, 0) -- 14 instead of 18 instructions per 4 values.  The build was not faster
// (0.283 vs 0.276-0.283 ms) and its results were WRONG (heavy-tailed test 7.5e4 x its bound): the packed-bf16 inline
// constant hipcc emits for (-1, 0) is not what the instruction reads.  Dropped.)
__device__ __forceinline__ f32x2 split_stage(const f32x2 a, unsigned& packed) {
    const bf16x2 h = __builtin_convertvector(a, bf16x2);
    packed = __builtin_bit_cast(unsigned, h);
    const f32x2 w = {__uint_as_float(packed << 16), __uint_as_float(packed & 0xFFFF0000u)};
    return a - w;
}
// 8 fp32 channels of one voxel -> three 16-byte bf16 fragments
__device__ __forceinline__ void gs_split8(const f32x4 lo, const f32x4 hi, u32x4& p1, u32x4& p2, u32x4& p3) {
    const f32x2 v[4] = {{lo.x, lo.y}, {lo.z, lo.w}, {hi.x, hi.y}, {hi.z, hi.w}};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned a, b;
        const f32x2 r1 = split_stage(v[j], a);
        const f32x2 r2 = split_stage(r1, b);
        p1[j] = a;
        p2[j] = b;
        p3[j] = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
    }
}

// The block's place in the grid's tile sequence.  Blocks are dealt round-robin over the 8 XCDs (blockIdx.x % 8 names
// the XCD: speed only, never correctness) and every XCD has its own L2: XCD k runs q blocks (+1 if k < rem) and works
// through the k-th eighth of the sequence, so that tiles sharing halo planes / rows run on one L2 at about the same time.
__device__ __forceinline__ int xcd_block() {
    const int k = blockIdx.x & 7, q = gridDim.x >> 3, rem = gridDim.x & 7;
    return k * q + min(k, rem) + (blockIdx.x >> 3);
}

}  // namespace mvs
