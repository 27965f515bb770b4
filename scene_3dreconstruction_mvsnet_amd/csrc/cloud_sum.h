// cloud_sum.h -- the balanced pairwise sum S(x) of include/mvs_outliers_abi.h over a device array of doubles, shared by
// cloud_outliers.hip (the mean distance and its deviations) and cloud_distance.hip (the cloud-to-cloud distances).
//
// Each block of cloud_sum_kernel sums kSumBlock consecutive elements in the header's pairing -- an xor butterfly inside a
// wave, bit 0 first, then the same pairing over the 16 wave sums through LDS -- and cloud_sum_tree relaunches it on the
// partial sums until one is left (at most four launches below 2^31 elements).  What an element contributes is the MODE
// of the first launch; every later level adds the partial sums as they are.
// No floating-point atomics: a block's sum has one owner, and the tree's shape depends on the element count alone.
// The users are compiled with -ffp-contract=off.  The kernel is static: each translation unit carries its own copy.
#pragma once

#include "mvs_outliers_abi.h"
#include "cloud_common.h"      // kSumBlock, cloud_blocks

#include <cmath>

namespace mvs {

constexpr int kSumWaves = kSumBlock / 64;
static_assert(kSumWaves == 16, "the second butterfly runs over 16 lanes");
static_assert(MVS_OUTLIERS_SCALARS >= 3 * sizeof(double), "mean, threshold, the total of a single element");

// the scalar block: doubles
constexpr int kScalarMean = 0, kScalarThreshold = 1, kScalarTotal = 2;

// what in[i] contributes to the first level
constexpr int kSumPositive = 0;       // in[i] where in[i] > 0, else +0.0
constexpr int kSumDeviation = 1;      // (in[i] - mean)^2 where in[i] > 0, else +0.0; mean = scalars[kScalarMean]
constexpr int kSumPlain = 2;          // in[i]
constexpr int kSumFinite = 3;         // in[i] where 0 < in[i] < +inf, else +0.0

// out[block] = the header's S over in[block * kSumBlock ..], +0.0 past n
template <int MODE>
static __global__ void __launch_bounds__(kSumBlock) cloud_sum_kernel(const double* in, long long n, const double* scalars,
                                                                      double* out) {
    __shared__ double wave_sum[kSumWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * kSumBlock + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        const double d = in[i];
        if (MODE == kSumPlain) {
            v = d;
        } else if (MODE == kSumFinite) {
            if (d > 0.0 && d < INFINITY) v = d;
        } else if (d > 0.0) {
            if (MODE == kSumPositive) {
                v = d;
            } else {
                const double e = d - scalars[kScalarMean];
                v = e * e;
            }
        }
    }
#pragma unroll
    for (int bit = 1; bit < 64; bit <<= 1) v = v + __shfl_xor(v, bit);
    if (lane == 0) wave_sum[wave] = v;
    __syncthreads();
    if (wave == 0) {
        double w = lane < kSumWaves ? wave_sum[lane] : 0.0;
#pragma unroll
        for (int bit = 1; bit < kSumWaves; bit <<= 1) w = w + __shfl_xor(w, bit);
        if (lane == 0) out[blockIdx.x] = w;
    }
}

// the header's L_1 + L_2 + ... over n elements
static long long cloud_sum_partials(long long n) {
    long long total = 0;
    for (long long L = n; L > 1;) {
        L = (L + kSumBlock - 1) / kSumBlock;
        total += L;
    }
    return total;
}

// S over in[0 .. n) (n >= 1; first_mode is not kSumPlain), level by level; *total is where the one value left lies
static int cloud_sum_tree(int first_mode, const double* in, long long n, double* partials, double* scalars, hipStream_t s,
                          const double** total) {
    double* out = n > 1 ? partials : scalars + kScalarTotal;      // a single element has no level of partial sums
    int mode = first_mode;
    for (;;) {
        const long long blocks = cloud_blocks(kLaunchSum, n);      // n / 1024 <= 2^21: never capped
        if (mode == kSumPositive) cloud_sum_kernel<kSumPositive><<<(int)blocks, kSumBlock, 0, s>>>(in, n, scalars, out);
        else if (mode == kSumDeviation) cloud_sum_kernel<kSumDeviation><<<(int)blocks, kSumBlock, 0, s>>>(in, n, scalars, out);
        else if (mode == kSumFinite) cloud_sum_kernel<kSumFinite><<<(int)blocks, kSumBlock, 0, s>>>(in, n, scalars, out);
        else cloud_sum_kernel<kSumPlain><<<(int)blocks, kSumBlock, 0, s>>>(in, n, scalars, out);
        if (int rc = check_hip(hipGetLastError(), "cloud_sum_kernel")) return rc;
        if (blocks == 1) {
            *total = out;
            return MVS_OK;
        }
        in = out;
        out += blocks;
        n = blocks;
        mode = kSumPlain;
    }
}

}  // namespace mvs
