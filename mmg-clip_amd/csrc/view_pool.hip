// Pooling the views of an exam: feat fp32 [V, C] (one row per view, the views of a study adjacent) -> out [S, C] (one row per study),
// mean or max over each study's rows, and the backward of both.  Replaces, inside the training graph, the offline
// `torch.stack(features).mean(0)` / `.max(0)[0]` of the reference's StudyFeatureExtractor (mmgclip/networks/image_features.py:225-245).
//
// offsets int32 [S + 1] (device): study s owns rows offsets[s] .. offsets[s + 1] - 1; offsets[0] = 0, offsets[S] = V, every study has a row.
// Both directions write every element of their output exactly once: no atomics, no memset, the same bits on every run.  A few hundred KB
// move per call, so the kernels are launch-latency bound; one thread per float4 of the output, plain vector loads and stores.
#include "common.h"

// mode 0: out = (f_0 + f_1 + ...) / k in view order, one IEEE division.
// mode 1: out = max over the views, argmax = its row in feat; the lowest row wins a tie; a NaN takes the maximum and keeps it (torch.max).
template <int MODE>
__global__ __launch_bounds__(256) void view_pool_fwd_kernel(const float* __restrict__ feat, const int* __restrict__ offsets,
                                                            float* __restrict__ out, int* __restrict__ argmax, int C4, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int s = (int)(i / C4), c4 = (int)(i % C4);
    const int lo = offsets[s], hi = offsets[s + 1];
    const float4* src = reinterpret_cast<const float4*>(feat) + c4;
    float4 acc = src[(size_t)lo * C4];
    if (MODE == 0) {
        for (int v = lo + 1; v < hi; ++v) {
            const float4 f = src[(size_t)v * C4];
            acc.x += f.x; acc.y += f.y; acc.z += f.z; acc.w += f.w;
        }
        const float k = (float)(hi - lo);
        acc.x /= k; acc.y /= k; acc.z /= k; acc.w /= k;
    } else {
        int4 idx = make_int4(lo, lo, lo, lo);
        for (int v = lo + 1; v < hi; ++v) {
            const float4 f = src[(size_t)v * C4];
            if (f.x > acc.x || f.x != f.x) { acc.x = f.x; idx.x = v; }
            if (f.y > acc.y || f.y != f.y) { acc.y = f.y; idx.y = v; }
            if (f.z > acc.z || f.z != f.z) { acc.z = f.z; idx.z = v; }
            if (f.w > acc.w || f.w != f.w) { acc.w = f.w; idx.w = v; }
        }
        reinterpret_cast<int4*>(argmax)[i] = idx;
    }
    reinterpret_cast<float4*>(out)[i] = acc;
}

// One thread per float4 of dfeat [V, C]; the study of row v is found by bisection in offsets (the last s with offsets[s] <= v), so every
// row below V is written whatever the offsets hold.
template <int MODE>
__global__ __launch_bounds__(256) void view_pool_bwd_kernel(const float* __restrict__ dout, const int* __restrict__ offsets,
                                                            const int* __restrict__ argmax, float* __restrict__ dfeat, int S, int C4,
                                                            long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int v = (int)(i / C4), c4 = (int)(i % C4);
    int lo = 0, hi = S;                       // invariant: offsets[lo] <= v, and (hi == S or offsets[hi] > v)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= v) lo = mid; else hi = mid;
    }
    const size_t j = (size_t)lo * C4 + c4;
    float4 g = reinterpret_cast<const float4*>(dout)[j];
    if (MODE == 0) {
        const float k = (float)(offsets[lo + 1] - offsets[lo]);
        g.x /= k; g.y /= k; g.z /= k; g.w /= k;
    } else {
        const int4 idx = reinterpret_cast<const int4*>(argmax)[j];
        g.x = idx.x == v ? g.x : 0.f;
        g.y = idx.y == v ? g.y : 0.f;
        g.z = idx.z == v ? g.z : 0.f;
        g.w = idx.w == v ? g.w : 0.f;
    }
    reinterpret_cast<float4*>(dfeat)[i] = g;
}

MMG_API int mmg_view_pool_fwd(const float* feat, const int* offsets, float* out, int* argmax, int S, int C, int mode,
                              hipStream_t stream) {
    MMG_CHECK_ARG(feat && offsets && out && S > 0 && C % 4 == 0 && C >= 8 && C <= 3072 && (mode == 0 || (mode == 1 && argmax)),
                  "mmg_view_pool_fwd: bad argument");
    const int C4 = C / 4;
    const long total = (long)S * C4;
    MMG_CHECK_ARG(total <= 0x7fffff00L, "mmg_view_pool_fwd: too many elements");
    const int blocks = cdiv(total, 256);
    if (mode == 0)
        hipLaunchKernelGGL(view_pool_fwd_kernel<0>, dim3(blocks), dim3(256), 0, stream, feat, offsets, out, argmax, C4, total);
    else
        hipLaunchKernelGGL(view_pool_fwd_kernel<1>, dim3(blocks), dim3(256), 0, stream, feat, offsets, out, argmax, C4, total);
    MMG_LAUNCH_CHECK("mmg_view_pool_fwd");
    return 0;
}

MMG_API int mmg_view_pool_bwd(const float* dout, const int* offsets, const int* argmax, float* dfeat, int S, int V, int C, int mode,
                              hipStream_t stream) {
    MMG_CHECK_ARG(dout && offsets && dfeat && S > 0 && V >= S && C % 4 == 0 && C >= 8 && C <= 3072 &&
                      (mode == 0 || (mode == 1 && argmax)),
                  "mmg_view_pool_bwd: bad argument");
    const int C4 = C / 4;
    const long total = (long)V * C4;
    MMG_CHECK_ARG(total <= 0x7fffff00L, "mmg_view_pool_bwd: too many elements");
    const int blocks = cdiv(total, 256);
    if (mode == 0)
        hipLaunchKernelGGL(view_pool_bwd_kernel<0>, dim3(blocks), dim3(256), 0, stream, dout, offsets, argmax, dfeat, S, C4, total);
    else
        hipLaunchKernelGGL(view_pool_bwd_kernel<1>, dim3(blocks), dim3(256), 0, stream, dout, offsets, argmax, dfeat, S, C4, total);
    MMG_LAUNCH_CHECK("mmg_view_pool_bwd");
    return 0;
}
