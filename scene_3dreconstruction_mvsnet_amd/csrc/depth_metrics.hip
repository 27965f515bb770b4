// depth_metrics.hip -- masked depth-error sums of a batch of depth maps against ground truth, the
// quantities behind the reference's test-mode scalars (train.py:302-358): mvsnet_loss
// (models/mvsnet.py:242-244), AbsDepthError_metrics and Thres_metrics (utils.py:128-158), plus
// the error map |est - gt| * mask (train.py:315).
//
// Pass 1 (metrics_partial_kernel): each (image, slice) unit is one 256-thread block that reads its
// strided share of the image with 16-byte loads (scalar head / tail where the image does not start
// on a 16-byte boundary or h*w is not a multiple of 4) and writes one row of partial sums to the
// workspace.  Pass 2 (metrics_reduce_kernel): one wave per image adds its rows in a fixed order.
// The slice count depends on h*w only, so the sums are bit-identical across runs and streams.
// HBM-bound: 12 B read per pixel (+ 4 B written with the error map).
#include "mvs_internal.h"

// the reference's arithmetic is fp32 elementwise (torch): no contraction into fma
#pragma clang fp contract(off)

namespace mvs {

constexpr int kMetricsThreads = 256;
constexpr int kMetricsMaxThres = 8;
constexpr int kMetricsMaxSlices = 1024;

struct MetricsParams {
    const float* est;
    const float* gt;
    const float* mask;
    float* errmap;           // NULL = no error map
    double* partial;         // [B][slices][K]
    double* sums;            // [B][K]
    long long hw;
    int B, slices, n_thres, K;
    int vec;                 // 1: every pointer has the same phase mod 16 B -> float4 body
    int phase;               // (est address / 4) mod 4
    float thres[kMetricsMaxThres];
};

struct MetricsAcc {
    unsigned int n;
    unsigned int cnt[kMetricsMaxThres];
    double abs_sum, sl1_sum;
};

__device__ __forceinline__ void metrics_pixel(const MetricsParams& P, MetricsAcc& a, float est, float gt, float m,
                                              float* err_out) {
    const float z = fabsf(est - gt);
    if (err_out) *err_out = z * m;
    if (m > 0.5f) {
        a.n += 1;
        a.abs_sum += (double)z;
        a.sl1_sum += (double)(z < 1.f ? 0.5f * z * z : z - 0.5f);   // smooth_l1, beta = 1
#pragma unroll
        for (int k = 0; k < kMetricsMaxThres; ++k)
            if (k < P.n_thres && z > P.thres[k]) a.cnt[k] += 1;     // NaN compares false
    }
}

__global__ void __launch_bounds__(kMetricsThreads) metrics_partial_kernel(MetricsParams P) {
    __shared__ double red[kMetricsThreads / 64][3 + kMetricsMaxThres];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long units = (long long)P.B * P.slices;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int b = (int)(u / P.slices), slice = (int)(u % P.slices);
        const long long base = (long long)b * P.hw;
        MetricsAcc a;
        a.n = 0;
        a.abs_sum = 0.0;
        a.sl1_sum = 0.0;
#pragma unroll
        for (int k = 0; k < kMetricsMaxThres; ++k) a.cnt[k] = 0;
        const long long stride = (long long)P.slices * kMetricsThreads;
        const long long first = (long long)slice * kMetricsThreads + tid;
        if (P.vec) {
            const long long head = min((long long)((4 - ((P.phase + base) & 3)) & 3), P.hw);
            const long long n4 = (P.hw - head) >> 2;
            const long long body_end = head + 4 * n4;
            const float4* e4 = reinterpret_cast<const float4*>(P.est + base + head);
            const float4* g4 = reinterpret_cast<const float4*>(P.gt + base + head);
            const float4* m4 = reinterpret_cast<const float4*>(P.mask + base + head);
            float4* o4 = P.errmap ? reinterpret_cast<float4*>(P.errmap + base + head) : nullptr;
            for (long long j = first; j < n4; j += stride) {
                const float4 e = e4[j], g = g4[j], m = m4[j];
                float4 o;
                float* op = o4 ? &o.x : nullptr;
                metrics_pixel(P, a, e.x, g.x, m.x, op ? op + 0 : nullptr);
                metrics_pixel(P, a, e.y, g.y, m.y, op ? op + 1 : nullptr);
                metrics_pixel(P, a, e.z, g.z, m.z, op ? op + 2 : nullptr);
                metrics_pixel(P, a, e.w, g.w, m.w, op ? op + 3 : nullptr);
                if (o4) o4[j] = o;
            }
            // at most 3 head + 3 tail pixels, taken by the first threads of slice 0
            if (slice == 0 && tid < 6) {
                const long long i = tid < 3 ? tid : body_end + (tid - 3);
                if ((tid < 3 && i < head) || (tid >= 3 && i < P.hw))
                    metrics_pixel(P, a, P.est[base + i], P.gt[base + i], P.mask[base + i],
                                  P.errmap ? P.errmap + base + i : nullptr);
            }
        } else {
            for (long long i = first; i < P.hw; i += stride)
                metrics_pixel(P, a, P.est[base + i], P.gt[base + i], P.mask[base + i],
                              P.errmap ? P.errmap + base + i : nullptr);
        }
        // wave reduction (fixed butterfly), then the waves in order
        double v[3 + kMetricsMaxThres];
        v[0] = (double)a.n;
        v[1] = a.abs_sum;
        v[2] = a.sl1_sum;
#pragma unroll
        for (int k = 0; k < kMetricsMaxThres; ++k) v[3 + k] = (double)a.cnt[k];
#pragma unroll
        for (int k = 0; k < 3 + kMetricsMaxThres; ++k) {
            if (k < P.K) {   // wave-uniform
                double x = v[k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
                if (lane == 0) red[wave][k] = x;
            }
        }
        __syncthreads();
        if (tid < P.K) {
            double s = red[0][tid];
#pragma unroll
            for (int wv = 1; wv < kMetricsThreads / 64; ++wv) s += red[wv][tid];
            P.partial[u * P.K + tid] = s;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) metrics_reduce_kernel(MetricsParams P) {
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < P.B; b += gridDim.x) {
        const double* rows = P.partial + (long long)b * P.slices * P.K;
        for (int k = 0; k < P.K; ++k) {
            double s = 0.0;
            for (int r = lane; r < P.slices; r += 64) s += rows[(long long)r * P.K + k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) P.sums[(long long)b * P.K + k] = s;
        }
    }
}

// slices per image: about one float4 per thread, at most kMetricsMaxSlices; a function of h*w only.  At 128x160 that
// is 20 blocks per map (DESIGN.md section 4 has the measured times of this and of 4 float4 per thread).
static int metrics_slices(long long hw) {
    const long long per = (long long)kMetricsThreads * 4;
    const long long s = (hw + per - 1) / per;
    return (int)(s < 1 ? 1 : (s > kMetricsMaxSlices ? kMetricsMaxSlices : s));
}

static int metrics_check(int B, int h, int w, int n_thres) {
    if (B < 1 || h < 1 || w < 1 || n_thres < 0 || n_thres > kMetricsMaxThres ||
        (long long)B * h * w >= (1LL << 31))
        return fail(MVS_ERR_BAD_SHAPE, "depth metrics: B,h,w,n_thres = %d,%d,%d,%d (need B,h,w >= 1, "
                    "0 <= n_thres <= %d, B*h*w < 2^31)", B, h, w, n_thres, kMetricsMaxThres);
    return MVS_OK;
}

static size_t metrics_workspace(int B, int h, int w) {
    return (size_t)B * metrics_slices((long long)h * w) * (3 + kMetricsMaxThres) * sizeof(double);
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_query_metrics_workspace(int B, int h, int w, size_t* bytes) {
    if (!bytes) return fail(MVS_ERR_NULL, "mvs_query_metrics_workspace: NULL bytes");
    if (int rc = metrics_check(B, h, w, 0)) return rc;
    *bytes = metrics_workspace(B, h, w);
    return MVS_OK;
}

int mvs_depth_metrics(const float* depth_est, const float* depth_gt, const float* mask, int B, int h, int w,
                      const float* thresholds, int n_thres, double* sums_out, float* errmap_out, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!depth_est || !depth_gt || !mask || !sums_out || !workspace || (n_thres > 0 && !thresholds))
        return fail(MVS_ERR_NULL, "mvs_depth_metrics: NULL argument");
    if (int rc = metrics_check(B, h, w, n_thres)) return rc;
    const size_t need = metrics_workspace(B, h, w);
    if (workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % alignof(double))
        return fail(MVS_ERR_WORKSPACE, "mvs_depth_metrics: workspace of %zu bytes at %p, need %zu (8-byte aligned)",
                    workspace_bytes, workspace, need);
    MetricsParams P{};
    P.est = depth_est;
    P.gt = depth_gt;
    P.mask = mask;
    P.errmap = errmap_out;
    P.partial = static_cast<double*>(workspace);
    P.sums = sums_out;
    P.hw = (long long)h * w;
    P.B = B;
    P.slices = metrics_slices(P.hw);
    P.n_thres = n_thres;
    P.K = 3 + n_thres;
    for (int k = 0; k < n_thres; ++k) P.thres[k] = thresholds[k];
    const uintptr_t ph = (reinterpret_cast<uintptr_t>(depth_est) >> 2) & 3;
    bool vec = (reinterpret_cast<uintptr_t>(depth_est) & 3) == 0;
    for (const void* p : {(const void*)depth_gt, (const void*)mask, (const void*)errmap_out})
        if (p && reinterpret_cast<uintptr_t>(p) % 16 != reinterpret_cast<uintptr_t>(depth_est) % 16) vec = false;
    P.vec = vec ? 1 : 0;
    P.phase = (int)ph;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const long long units = (long long)B * P.slices;
    const int grid1 = (int)(units < 65536 ? units : 65536);
    metrics_partial_kernel<<<grid1, kMetricsThreads, 0, s>>>(P);
    if (int rc = check_hip(hipGetLastError(), "metrics_partial_kernel")) return rc;
    metrics_reduce_kernel<<<B < 65536 ? B : 65536, 64, 0, s>>>(P);
    return check_hip(hipGetLastError(), "metrics_reduce_kernel");
}

}  // extern "C"
