// Global-norm gradient clipping and the non-finite-step guard of the optimizer step, all on the device
// (torch.nn.utils.clip_grad_norm_ + "do not step on a NaN/Inf gradient", beside mmgclip/experiments/ClassifierExperiment.py:115-118).
//
//   mmg_grad_sumsq          one streaming read of a gradient buffer -> per-workgroup partial sums of squares (fp64)
//   mmg_grad_clip_finalize  the partials of every buffer of the step -> {total_norm, clip coefficient, "apply" flag}, skipped-step counter
//   mmg_adamw_step_guarded  mmg_adamw_step that takes the coefficient and the flag from the device and returns untouched on a bad step
//
// Nothing here reads anything back to the host, uses an atomic or needs a memset: every partial is written by exactly one
// workgroup whose identity depends on n alone, and every sum has a fixed order, so the same gradients give the same bits on
// every device and in every run (data-parallel ranks that hold the same reduced gradients compute the same coefficient).
#include "common.h"
#include <math.h>

#define GC_THREADS 256
#define GC_ELEMS_PER_WG 8192      // 8 x 16 bytes per lane and trip
#define GC_MAX_WGS 2048           // 8 workgroups per CU on a 256-CU part, but NOT a function of the CU count (see above)

static inline int sumsq_workgroups(long long n) {
    if (n <= 0) return 0;
    const long long b = (n + GC_ELEMS_PER_WG - 1) / GC_ELEMS_PER_WG;
    return (int)(b > GC_MAX_WGS ? GC_MAX_WGS : b);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over the 256 threads of a workgroup, valid in thread 0: butterfly inside each wave, the four waves through LDS in wave order
__device__ __forceinline__ double block_sum_f64(double v) {
    __shared__ double part[GC_THREADS / 64];
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}
__device__ __forceinline__ double sq_acc(double a, float x) {
    const double d = (double)x;      // the square of an fp32 is exact in fp64
    return fma(d, d, a);
}
__device__ __forceinline__ double sq_acc4(double a, const float4 v) { return sq_acc(sq_acc(sq_acc(sq_acc(a, v.x), v.y), v.z), v.w); }

// g needs 4-byte alignment only: up to three scalar elements in front of the first 16-byte boundary and up to three behind the
// last whole float4 are taken by workgroup 0; the body is read 16 bytes per lane, four loads in flight per lane.
__global__ __launch_bounds__(GC_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partials) {
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2;
    if (head > n) head = n;
    const size_t nvec = (n - head) >> 2;
    const size_t tail0 = head + (nvec << 2);
    const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
    const size_t stride = (size_t)gridDim.x * GC_THREADS;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    size_t i = (size_t)blockIdx.x * GC_THREADS + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const float4 v0 = gv[i], v1 = gv[i + stride], v2 = gv[i + 2 * stride], v3 = gv[i + 3 * stride];
        a0 = sq_acc4(a0, v0); a1 = sq_acc4(a1, v1); a2 = sq_acc4(a2, v2); a3 = sq_acc4(a3, v3);
    }
    for (; i < nvec; i += stride) a0 = sq_acc4(a0, gv[i]);
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) a1 = sq_acc(a1, g[threadIdx.x]);
        if (threadIdx.x < n - tail0) a2 = sq_acc(a2, g[tail0 + threadIdx.x]);
    }
    const double s = block_sum_f64((a0 + a1) + (a2 + a3));
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

MMG_API int mmg_grad_sumsq_partials(long long n) { return sumsq_workgroups(n); }

MMG_API int mmg_grad_sumsq(const float* g, long long n, double* partials, int n_partials, hipStream_t stream) {
    MMG_CHECK_ARG(g && partials && n > 0, "mmg_grad_sumsq: bad argument (null pointer or n <= 0)");
    MMG_CHECK_ARG((reinterpret_cast<uintptr_t>(g) & 3) == 0 && (reinterpret_cast<uintptr_t>(partials) & 7) == 0,
                  "mmg_grad_sumsq: g must be 4-byte and partials 8-byte aligned");
    const int wgs = sumsq_workgroups(n);
    MMG_CHECK_ARG(n_partials == wgs, "mmg_grad_sumsq: n_partials=%d, but n=%lld takes mmg_grad_sumsq_partials(n)=%d", n_partials, n, wgs);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(wgs), dim3(GC_THREADS), 0, stream, g, (size_t)n, partials);
    MMG_LAUNCH_CHECK("mmg_grad_sumsq");
    return 0;
}

// One workgroup: lane t sums partials t, t + 256, ... in that order, then the fixed-order workgroup sum.
__global__ __launch_bounds__(GC_THREADS) void grad_clip_finalize_kernel(const double* __restrict__ partials, int n, float max_norm,
                                                                         float* __restrict__ out, int* __restrict__ skipped) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += GC_THREADS) a += partials[i];
    const double total = block_sum_f64(a);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(total);
    const bool finite = fabsf(norm) <= 3.402823466e+38f;             // false for NaN and +-Inf
    float coef = 1.0f;
    if (max_norm > 0.f && max_norm <= 3.402823466e+38f) {
        const float c = max_norm / (norm + 1e-6f);                   // torch.nn.utils.clip_grad_norm_
        coef = c > 1.0f ? 1.0f : c;                                  // clamp(max=1): NaN stays NaN, as in torch
    }
    out[0] = norm;
    out[1] = coef;
    out[2] = finite ? 1.0f : 0.0f;
    if (!finite && skipped) *skipped = *skipped + 1;
}

MMG_API int mmg_grad_clip_finalize(const double* partials, int n, float max_norm, float* out, int* skipped, hipStream_t stream) {
    MMG_CHECK_ARG(partials && out && n > 0, "mmg_grad_clip_finalize: bad argument (null pointer or n <= 0)");
    MMG_CHECK_ARG(max_norm == max_norm, "mmg_grad_clip_finalize: max_norm is NaN");
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(GC_THREADS), 0, stream, partials, n, max_norm, out, skipped);
    MMG_LAUNCH_CHECK("mmg_grad_clip_finalize");
    return 0;
}

// beta^t for an integer t >= 1 by repeated squaring in fp64: at most 62 roundings of 2^-53, so the fp32 it is rounded to is the
// correctly rounded beta^t (mmg_adamw_step's host powf is within 0.82 ulp of it: DESIGN.md section 4)
__device__ __forceinline__ float pow_int(float beta, int t) {
    double b = (double)beta, r = 1.0;
    for (; t > 0; t >>= 1) {
        if (t & 1) r *= b;
        b *= b;
    }
    return (float)r;
}

// adamw_kernel of norm_elementwise.hip, element for element, with three things taken from the device instead of the host:
// the gradient scale (clip[1]), whether to step at all (clip[2]) and Adam's clock t = step - *skipped.
__global__ __launch_bounds__(256) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, bf16_t* __restrict__ p16, size_t n, float lr,
                                                            float beta1, float beta2, float eps, float wd, int step,
                                                            const float* __restrict__ clip, const int* __restrict__ skipped) {
    if (skipped && clip[2] == 0.f) return;           // non-finite gradient norm: p, m, v, p16 keep their bits
    const float gscale = clip[1];
    int t = step - (skipped ? *skipped : 0);
    if (t < 1) t = 1;
    const float bc1 = 1.0f - pow_int(beta1, t), bc2 = 1.0f - pow_int(beta2, t);
    const float stepsz = lr / bc1;
    const float isbc2 = rsqrtf(bc2);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float gi = g[i] * gscale;
        float pi = p[i] * (1.0f - lr * wd);
        const float mi = beta1 * m[i] + (1.0f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.0f - beta2) * gi * gi;
        pi -= stepsz * mi / (sqrtf(vi) * isbc2 + eps);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (p16) p16[i] = f2bf(pi);
    }
}

MMG_API int mmg_adamw_step_guarded(float* p, const float* g, float* m, float* v, void* p_bf16, long long n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, int step, const float* clip, const int* skipped,
                                   hipStream_t stream) {
    MMG_CHECK_ARG(p && g && m && v && clip && n > 0 && step >= 1, "mmg_adamw_step_guarded: bad argument");
    int blocks = (int)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
    hipLaunchKernelGGL(adamw_guarded_kernel, dim3(blocks), dim3(256), 0, stream, p, g, m, v, (bf16_t*)p_bf16, (size_t)n, lr, beta1,
                       beta2, eps, weight_decay, step, clip, skipped);
    MMG_LAUNCH_CHECK("mmg_adamw_step_guarded");
    return 0;
}
