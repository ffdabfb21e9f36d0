// AdamW over a flat fp32 parameter arena whose parameters belong to several hyper-parameter groups, in ONE launch
// (torch.optim.AdamW with param groups: per-group lr and weight_decay, shared betas / eps; beside
// mmgclip/experiments/ClassifierExperiment.py:74,118, which hands AdamW a single group).
//
//   mmg_adamw_step_groups   adamw_kernel / adamw_guarded_kernel, element for element, with lr and weight_decay looked up per 64-element chunk
//
// The chunk map: params.ParamArena starts every parameter on a 64-element boundary, so chunk_group[i >> 6] (one byte per 64
// elements, 1/64 byte against the 28 bytes of fp32 traffic per element) is exact per parameter and a float4 never straddles two
// chunks: no search, no segment table.  The per-group values travel BY VALUE in the kernel arguments (1 KiB for 128 groups), so a
// scheduler may change them at every step and there is neither a staging buffer a later step could overwrite nor a copy to wait
// for.  Each workgroup derives the two per-group factors once into LDS.  No atomics, no host read-back.
#include "common.h"
#include <math.h>

#define AG_THREADS 256
#define AG_MAX_WGS 2048           // 8 workgroups per CU on a 256-CU part; the rest is grid-strided
#define AG_MAX_GROUPS 128

struct AdamwGroupHyper {
    float lr[AG_MAX_GROUPS];
    float wd[AG_MAX_GROUPS];
};

// beta^t as grad_clip.hip's pow_int forms it: repeated squaring in fp64, rounded to fp32 once
__device__ __forceinline__ float ag_pow_int(float beta, int t) {
    double b = (double)beta, r = 1.0;
    for (; t > 0; t >>= 1) {
        if (t & 1) r *= b;
        b *= b;
    }
    return (float)r;
}

// One AdamW element, spelled as adamw_kernel spells it: decay = 1 - lr * wd, stepsz = lr / bc1, isbc2 = rsqrtf(bc2).
__device__ __forceinline__ void ag_element(float& p, float g, float& m, float& v, float gscale, float decay, float stepsz, float isbc2,
                                           float beta1, float beta2, float eps) {
    const float gi = g * gscale;
    float pi = p * decay;
    const float mi = beta1 * m + (1.0f - beta1) * gi;
    const float vi = beta2 * v + (1.0f - beta2) * gi * gi;
    pi -= stepsz * mi / (sqrtf(vi) * isbc2 + eps);
    p = pi; m = mi; v = vi;
}

// nvec = n / 4 float4s; lane i of the flat index owns elements 4i .. 4i + 3, all of chunk i >> 4.
// clip == NULL: bc1 / bc2 are the host's; else the gradient scale is clip[1], the step is held back on clip[2] == 0 (when skipped
// is given) and Adam's clock is step - *skipped, as in adamw_guarded_kernel.
__global__ __launch_bounds__(AG_THREADS) void adamw_groups_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                                  float4* __restrict__ v, size_t nvec,
                                                                  const unsigned char* __restrict__ chunk_group, int n_groups,
                                                                  const AdamwGroupHyper hyper, float beta1, float beta2, float eps,
                                                                  float bc1, float bc2, int step, const float* __restrict__ clip,
                                                                  const int* __restrict__ skipped) {
    __shared__ float s_decay[AG_MAX_GROUPS];
    __shared__ float s_stepsz[AG_MAX_GROUPS];
    float gscale = 1.0f;
    if (clip) {
        if (skipped && clip[2] == 0.f) return;       // non-finite gradient norm: p, m, v keep their bits (uniform over the grid)
        gscale = clip[1];
        int t = step - (skipped ? *skipped : 0);
        if (t < 1) t = 1;
        bc1 = 1.0f - ag_pow_int(beta1, t);
        bc2 = 1.0f - ag_pow_int(beta2, t);
    }
    const float isbc2 = rsqrtf(bc2);
    if ((int)threadIdx.x < n_groups) {
        const float lr = hyper.lr[threadIdx.x], wd = hyper.wd[threadIdx.x];
        s_decay[threadIdx.x] = 1.0f - lr * wd;
        s_stepsz[threadIdx.x] = lr / bc1;
    }
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * AG_THREADS + threadIdx.x; i < nvec; i += (size_t)gridDim.x * AG_THREADS) {
        const int gi = chunk_group[i >> 4];
        if (gi >= n_groups) continue;                // not a group of this launch: left untouched
        const float decay = s_decay[gi], stepsz = s_stepsz[gi];
        float4 pv = p[i], mv = m[i], vv = v[i];
        const float4 gv = g[i];
        ag_element(pv.x, gv.x, mv.x, vv.x, gscale, decay, stepsz, isbc2, beta1, beta2, eps);
        ag_element(pv.y, gv.y, mv.y, vv.y, gscale, decay, stepsz, isbc2, beta1, beta2, eps);
        ag_element(pv.z, gv.z, mv.z, vv.z, gscale, decay, stepsz, isbc2, beta1, beta2, eps);
        ag_element(pv.w, gv.w, mv.w, vv.w, gscale, decay, stepsz, isbc2, beta1, beta2, eps);
        p[i] = pv; m[i] = mv; v[i] = vv;
    }
}

MMG_API int mmg_adamw_step_groups(float* p, const float* g, float* m, float* v, long long n, const unsigned char* chunk_group,
                                  int n_groups, const float* group_lr, const float* group_wd, float beta1, float beta2, float eps,
                                  int step, const float* clip, const int* skipped, hipStream_t stream) {
    MMG_CHECK_ARG(p && g && m && v && chunk_group && group_lr && group_wd, "mmg_adamw_step_groups: null pointer");
    MMG_CHECK_ARG(n > 0 && n % 64 == 0 && step >= 1, "mmg_adamw_step_groups: n=%lld must be a positive multiple of 64 and step=%d >= 1",
                  n, step);
    MMG_CHECK_ARG(n_groups >= 1 && n_groups <= AG_MAX_GROUPS, "mmg_adamw_step_groups: n_groups=%d, takes 1 ... %d", n_groups, AG_MAX_GROUPS);
    MMG_CHECK_ARG(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                    reinterpret_cast<uintptr_t>(v)) & 15) == 0, "mmg_adamw_step_groups: p, g, m, v must be 16-byte aligned");
    MMG_CHECK_ARG(!skipped || clip, "mmg_adamw_step_groups: skipped given without clip");
    AdamwGroupHyper hyper;
    for (int i = 0; i < AG_MAX_GROUPS; ++i) {
        hyper.lr[i] = i < n_groups ? group_lr[i] : 0.f;
        hyper.wd[i] = i < n_groups ? group_wd[i] : 0.f;
    }
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
    const size_t nvec = (size_t)n / 4;
    const size_t want = (nvec + AG_THREADS - 1) / AG_THREADS;
    const int blocks = (int)(want > AG_MAX_WGS ? AG_MAX_WGS : want);
    hipLaunchKernelGGL(adamw_groups_kernel, dim3(blocks), dim3(AG_THREADS), 0, stream, reinterpret_cast<float4*>(p),
                       reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v), nvec, chunk_group,
                       n_groups, hyper, beta1, beta2, eps, bc1, bc2, step, clip, skipped);
    MMG_LAUNCH_CHECK("mmg_adamw_step_groups");
    return 0;
}
