// Stem patchify from raw pixels, with the augmentation folded into its gather (gfx950): mmg_patchify_aug.
//
// mmg_patchify (norm_elementwise.hip) reads fp32 pixels in [0,1]; mammograms are 16-bit PNGs, so this entry also reads uint16 / uint8
// storage directly (half / a quarter of the bytes over PCIe, in HBM and in a checkpointed forward's record), and applies per image
//     flip (over the FULL H, W) -> integer shift (ty, tx) -> fill 0 outside -> tone (gain, offset, clamped to [0,1]) -> 16-bit scaling
// in the one pass that reads every pixel once.  Output layout = mmg_patchify's: rows (n, H/P, W/P) x columns (kh, kw, ci), bf16, zero-padded
// to Kp; H/P, W/P floored on the OUTPUT canvas.  Arithmetic per canvas pixel (y, x), fp32, no contraction (-ffp-contract=off):
//     ys = y - ty, xs = x - tx, inside = 0 <= ys < H && 0 <= xs < W;  flags & 2: ys = H-1-ys;  flags & 1: xs = W-1-xs
//     r = inside ? img[i, c, ys, xs] : 0;   x01 = r | float(r) / 65535 | float(r) / 255
//     tone and (gain, offset) != (1, 0):  x01 = min(max(gain * x01 + offset, 0), 1)
//     v = scale16 ? (x01 * 65535 - 32767.5) / 32767.5 : x01;   out = bf16(v), round to nearest even
// The `inside` test guards the only read, so any ty / tx / flags value is safe; the tables are never copied to the host.
// uint16 without tone under scale16 takes (float(r) - 32767.5) / 32767.5: the same fp32 number for all 65 536 values (tests/test_augment_cpu.py
// on the CPU, tests/test_pixel_input_gpu.py exhaustively on the device) at one division instead of two.
#include "common.h"

template <int KIND>   // 0 = fp32 in [0,1], 1 = uint16, 2 = uint8
__device__ __forceinline__ float px_value(float r, bool tone_on, float gain, float offset, int scale16) {
    if (KIND == 1 && !tone_on && scale16) return (r - 32767.5f) / 32767.5f;
    float x01 = KIND == 0 ? r : (KIND == 1 ? r / 65535.0f : r / 255.0f);
    if (tone_on) x01 = fminf(fmaxf(gain * x01 + offset, 0.0f), 1.0f);
    return scale16 ? (x01 * 65535.0f - 32767.5f) / 32767.5f : x01;
}

// four consecutive, (4 * sizeof(T))-aligned source pixels as floats
__device__ __forceinline__ void px_load4(const float* p, float* r) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
}
__device__ __forceinline__ void px_load4(const unsigned short* p, float* r) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    r[0] = (float)(v.x & 0xffffu); r[1] = (float)(v.x >> 16); r[2] = (float)(v.y & 0xffffu); r[3] = (float)(v.y >> 16);
}
__device__ __forceinline__ void px_load4(const unsigned char* p, float* r) {
    const unsigned v = *reinterpret_cast<const unsigned*>(p);
    r[0] = (float)(v & 0xffu); r[1] = (float)((v >> 8) & 0xffu); r[2] = (float)((v >> 16) & 0xffu); r[3] = (float)(v >> 24);
}

struct PxImage {      // one image's parameters
    int flags; long long ty, tx; float gain, offset; bool tone_on;
};
__device__ __forceinline__ PxImage px_image(const int* geom, const float* tone, size_t n) {
    PxImage im = {0, 0, 0, 1.0f, 0.0f, false};
    if (geom) {
        const int4 g = reinterpret_cast<const int4*>(geom)[n];
        im.flags = g.x; im.ty = g.y; im.tx = g.z;
    }
    if (tone) {
        const float2 t = reinterpret_cast<const float2*>(tone)[n];
        im.gain = t.x; im.offset = t.y;
        im.tone_on = !(t.x == 1.0f && t.y == 0.0f);
    }
    return im;
}

// any Cin / P (the ViT's P = 16, RGB stems): one thread per output element
template <typename T, int KIND>
__global__ __launch_bounds__(256) void patchify_aug_kernel(const T* __restrict__ img, bf16_t* __restrict__ out, int Cin, int H, int W, int P,
                                                           int Kp, int scale16, const int* __restrict__ geom,
                                                           const float* __restrict__ tone, size_t rows) {
    const int Ho = H / P, Wo = W / P;
    const int K = P * P * Cin;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < rows * Kp; idx += (size_t)gridDim.x * 256) {
        const int k = (int)(idx % Kp);
        const size_t row = idx / Kp;
        float v = 0.f;
        if (k < K) {
            const int ci = k % Cin, kw = (k / Cin) % P, kh = k / (Cin * P);
            const int wo = (int)(row % Wo), ho = (int)((row / Wo) % Ho);
            const size_t n = row / ((size_t)Wo * Ho);
            const PxImage im = px_image(geom, tone, n);
            long long ys = (long long)ho * P + kh - im.ty, xs = (long long)wo * P + kw - im.tx;
            const bool inside = ys >= 0 && ys < H && xs >= 0 && xs < W;
            if (im.flags & 2) ys = H - 1 - ys;
            if (im.flags & 1) xs = W - 1 - xs;
            float r = 0.f;
            if (inside) r = (float)img[((n * Cin + ci) * H + (size_t)ys) * W + (size_t)xs];
            v = px_value<KIND>(r, im.tone_on, im.gain, im.offset, scale16);
        }
        out[idx] = f2bf(v);
    }
}

// Cin = 1, P = 4 (the mammography stem): one thread per output row, as patchify_1x4_kernel - per kernel row four consecutive source pixels
// (reversed under a flip) and 16-byte stores.  The four pixels come as ONE load (16 / 8 / 4 bytes) where they all lie inside the image and
// their address is aligned to that width, else as four guarded scalar loads.  With W % 4 == 0 that choice is the image's (tx % 4 == 0
// <=> aligned, flipped or not), so every wave inside an image takes one branch; with another W it alternates by source row, which a
// wave (consecutive patches of one patch row) still shares.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void patchify_aug_1x4_kernel(const T* __restrict__ img, bf16_t* __restrict__ out, int H, int W, int Kp,
                                                               int scale16, const int* __restrict__ geom, const float* __restrict__ tone,
                                                               size_t rows) {
    const int Ho = H / 4, Wo = W / 4;
    for (size_t row = (size_t)blockIdx.x * 256 + threadIdx.x; row < rows; row += (size_t)gridDim.x * 256) {
        const int wo = (int)(row % Wo), ho = (int)((row / Wo) % Ho);
        const size_t n = row / ((size_t)Wo * Ho);
        const PxImage im = px_image(geom, tone, n);
        const T* base = img + n * H * W;
        const bool flipx = im.flags & 1, flipy = im.flags & 2;
        const long long xs0 = (long long)wo * 4 - im.tx;                 // source column of kw = 0, before the flip
        const long long a = flipx ? (long long)W - 4 - xs0 : xs0;       // first of the four consecutive source columns, ascending
        const bool x_all = a >= 0 && a + 3 < W, x_any = a + 3 >= 0 && a < W;
        unsigned pk[8];
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
            long long ys = (long long)ho * 4 + kh - im.ty;
            const bool y_in = ys >= 0 && ys < H;
            if (flipy) ys = H - 1 - ys;
            float r[4] = {0.f, 0.f, 0.f, 0.f};
            if (y_in && x_any) {
                const T* line = base + (size_t)ys * W;
                if (x_all && (reinterpret_cast<uintptr_t>(line + a) & (4 * sizeof(T) - 1)) == 0) {
                    px_load4(line + a, r);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (a + e >= 0 && a + e < W) r[e] = (float)line[a + e];
                }
            }
            if (flipx) { float t = r[0]; r[0] = r[3]; r[3] = t; t = r[1]; r[1] = r[2]; r[2] = t; }
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = px_value<KIND>(r[e], im.tone_on, im.gain, im.offset, scale16);
            pk[2 * kh] = pack2bf(v[0], v[1]); pk[2 * kh + 1] = pack2bf(v[2], v[3]);
        }
        uint4* dst = reinterpret_cast<uint4*>(out + row * Kp);
        dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        for (int z = 2; z < Kp / 8; ++z) dst[z] = make_uint4(0, 0, 0, 0);
    }
}

template <typename T, int KIND>
static int patchify_aug_launch(const void* img, void* out, int n, int Cin, int H, int W, int P, int Kp, int scale16, const int* geom,
                               const float* tone, hipStream_t stream) {
    const size_t rows = (size_t)n * (H / P) * (W / P);
    if (Cin == 1 && P == 4 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        const int blocks = (int)((rows + 255) / 256 > 16384 ? 16384 : (rows + 255) / 256);
        hipLaunchKernelGGL((patchify_aug_1x4_kernel<T, KIND>), dim3(blocks), dim3(256), 0, stream, (const T*)img, (bf16_t*)out, H, W, Kp,
                           scale16, geom, tone, rows);
        MMG_LAUNCH_CHECK("mmg_patchify_aug");
        return 0;
    }
    const size_t total = rows * Kp;
    const int blocks = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
    hipLaunchKernelGGL((patchify_aug_kernel<T, KIND>), dim3(blocks), dim3(256), 0, stream, (const T*)img, (bf16_t*)out, Cin, H, W, P, Kp,
                       scale16, geom, tone, rows);
    MMG_LAUNCH_CHECK("mmg_patchify_aug");
    return 0;
}

MMG_API int mmg_patchify_aug(const void* img, int src_kind, void* out, int n, int Cin, int H, int W, int P, int Kp, int scale16,
                             const int* geom, const float* tone, hipStream_t stream) {
    MMG_CHECK_ARG(img && out, "mmg_patchify_aug: null %s", img ? "out" : "img");
    MMG_CHECK_ARG(src_kind >= 0 && src_kind <= 2, "mmg_patchify_aug: unknown src_kind %d (0 = fp32, 1 = uint16, 2 = uint8)", src_kind);
    MMG_CHECK_ARG(n > 0 && Cin > 0 && P > 0 && H >= P && W >= P && Kp >= P * P * Cin && Kp % 8 == 0,
                  "mmg_patchify_aug: bad argument (H=%d W=%d P=%d Cin=%d Kp=%d)", H, W, P, Cin, Kp);
    MMG_CHECK_ARG((reinterpret_cast<uintptr_t>(geom) & 15) == 0 && (reinterpret_cast<uintptr_t>(tone) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(img) & (src_kind == 0 ? 3 : (src_kind == 1 ? 1 : 0))) == 0,
                  "mmg_patchify_aug: misaligned pointer (geom rows are 16 bytes, tone rows 8, pixels their own width)");
    if (src_kind == 0) return patchify_aug_launch<float, 0>(img, out, n, Cin, H, W, P, Kp, scale16, geom, tone, stream);
    if (src_kind == 1) return patchify_aug_launch<unsigned short, 1>(img, out, n, Cin, H, W, P, Kp, scale16, geom, tone, stream);
    return patchify_aug_launch<unsigned char, 2>(img, out, n, Cin, H, W, P, Kp, scale16, geom, tone, stream);
}
