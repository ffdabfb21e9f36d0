// Stochastic depth ("row" mode) for the ConvNeXt tower: moving whole images so that the samples a block keeps form a contiguous prefix of the
// micro-batch, and the block's existing kernels run on that prefix only (mmgclip/networks/convnext_sd.py holds the schedule).  Replaces, for
// training, torchvision's CNBlock.stochastic_depth = StochasticDepth(p, "row") behind the reference's frozen ConvNeXt (mmgclip/networks/encoder.py:53),
// which multiplies a dropped sample's branch by zero after computing it.
//
// An activation is bf16 [n, rows, C] (NHWC, rows = h * w).  Both kernels move 16 bytes per lane and access, grid-stride over (image, chunk),
// write every element they touch exactly once, use no atomics, and index with 64-bit offsets (a stage-1 map of 64 images is > 2^31 bytes).
#include "common.h"

#include <vector>

// pairs int32 [k][2] (device): exchange image pairs[p][0] with image pairs[p][1].  The pairs are disjoint, so a thread that loads chunk c of
// both images and stores both is the only one that touches those 32 bytes.
__global__ __launch_bounds__(256) void image_swap_kernel(uint4* __restrict__ x, const int* __restrict__ pairs, long chunks, long total) {
    for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < total; w += (long)gridDim.x * 256) {
        const long p = w / chunks, c = w - p * chunks;
        const long i = (long)pairs[2 * p] * chunks + c, j = (long)pairs[2 * p + 1] * chunks + c;
        const uint4 a = x[i], b = x[j];
        x[i] = b;
        x[j] = a;
    }
}

__global__ __launch_bounds__(256) void image_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long total) {
    for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < total; w += (long)gridDim.x * 256) dst[w] = src[w];
}

__global__ __launch_bounds__(256) void scaled_add_kernel(float* __restrict__ dst, const float* __restrict__ src, float alpha, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = fmaf(alpha, src[i], dst[i]);
}

static inline int sd_blocks(long total) { return total > 2048L * 256 ? 2048 : cdiv(total, 256); }
static inline bool sd_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

MMG_API int mmg_image_swap(void* x, const int* pairs, const int* pairs_host, int k, int n, long long rows, int C, hipStream_t stream) {
    MMG_CHECK_ARG(x && n > 0 && rows > 0 && C > 0 && k >= 0 && 2 * (long)k <= n, "mmg_image_swap: bad argument");
    MMG_CHECK_ARG(C % 8 == 0, "mmg_image_swap: C=%d must be a multiple of 8 (16-byte accesses)", C);
    MMG_CHECK_ARG(sd_aligned(x), "mmg_image_swap: x must be 16-byte aligned");
    if (k == 0) return 0;
    MMG_CHECK_ARG(pairs && pairs_host, "mmg_image_swap: the pair table is needed on the device and on the host");
    std::vector<char> seen((size_t)n, 0);
    for (int p = 0; p < 2 * k; ++p) {
        const int i = pairs_host[p];
        MMG_CHECK_ARG(i >= 0 && i < n, "mmg_image_swap: pair %d names image %d of %d", p / 2, i, n);
        MMG_CHECK_ARG(!seen[i], "mmg_image_swap: image %d is in two pairs (they must be disjoint)", i);
        seen[i] = 1;
    }
    const long chunks = (long)rows * C / 8, total = chunks * k;
    hipLaunchKernelGGL(image_swap_kernel, dim3(sd_blocks(total)), dim3(256), 0, stream, reinterpret_cast<uint4*>(x), pairs, chunks, total);
    MMG_LAUNCH_CHECK("mmg_image_swap");
    return 0;
}

MMG_API int mmg_image_copy(const void* src, void* dst, int first, int count, int n, long long rows, int C, hipStream_t stream) {
    MMG_CHECK_ARG(src && dst && src != dst && n > 0 && rows > 0 && C > 0, "mmg_image_copy: bad argument");
    MMG_CHECK_ARG(first >= 0 && count >= 0 && (long)first + count <= n, "mmg_image_copy: images %d .. %d + %d are not inside 0 .. %d", first, first,
                  count, n);
    MMG_CHECK_ARG(C % 8 == 0, "mmg_image_copy: C=%d must be a multiple of 8 (16-byte accesses)", C);
    MMG_CHECK_ARG(sd_aligned(src) && sd_aligned(dst), "mmg_image_copy: src and dst must be 16-byte aligned");
    if (count == 0) return 0;
    const long chunks = (long)rows * C / 8, total = chunks * count;
    hipLaunchKernelGGL(image_copy_kernel, dim3(sd_blocks(total)), dim3(256), 0, stream, reinterpret_cast<const uint4*>(src) + chunks * first,
                       reinterpret_cast<uint4*>(dst) + chunks * first, total);
    MMG_LAUNCH_CHECK("mmg_image_copy");
    return 0;
}

MMG_API int mmg_scaled_add_f32(float* dst, const float* src, float alpha, long long n, hipStream_t stream) {
    MMG_CHECK_ARG(dst && src && dst != src && n > 0, "mmg_scaled_add_f32: bad argument");
    hipLaunchKernelGGL(scaled_add_kernel, dim3(sd_blocks(n)), dim3(256), 0, stream, dst, src, alpha, (long)n);
    MMG_LAUNCH_CHECK("mmg_scaled_add_f32");
    return 0;
}
