// Patch dropout (FLIP, Li et al. 2023; open_clip's `patch_dropout`) for the ViT tower: under train() every image keeps K of its P patches
// plus the class token, and the encoder runs on S_eff = 1 + K tokens.  Not in the reference (its image encoders are ConvNeXt-T /
// ResNet-50, mmgclip/networks/encoder.py:15,57); the ViT tower itself is BASELINE config C4.  mmgclip/patch_dropout.py restates the draw
// in numpy, which is what the tests compare against.
//
// The draw, per image b under its sample id (csrc/dropout.h):
//     key0   = mmg_drop_key(seed, 0x50447270)
//     key_b  = mmg_drop_key_bh(key0, (uint32) sample_id[b])          sample_id[b] = b when no table is given
//     bits_p = mmg_drop_bits(p, key_b)                               p = 0 .. P-1
// and the image keeps the K patches with the smallest bits_p, in ascending patch order.  mmg_drop_bits is fmix32 of an odd multiple of p
// plus a constant, a bijection of the 32-bit p: two patches of an image never draw the same bits, so "the K smallest" needs no tie rule.
//
// Under the foreground prior (mmg_patch_keep_indices_prior) a class bit goes in front of that key: a patch is foreground iff
// counts[b, p] >= min_pixels, where counts comes from mmg_patch_foreground (the pixels above a threshold per patch, under patchify's
// geometry), and the image keeps the K smallest (0 if foreground else 1, bits_p): tissue before background, the hash inside each class.
//
// Memory-bound kernels, no global atomics, every output element written by exactly one thread: bit-reproducible.  The row movers read and
// write 16 bytes per lane, as vit_assemble_kernel (csrc/embedding.hip), and index with 64-bit offsets.
#include "common.h"
#include "dropout.h"

#define PD_SITE 0x50447270u
#define PD_THREADS 1024
#define PD_MAX_P 16384          // 16 patches per thread; the keys take P * 4 <= 64 KiB of LDS

__device__ __forceinline__ void unpack8p(const uint4 v, float* f) {
    f[0] = bf2f_lo(v.x); f[1] = bf2f_hi(v.x); f[2] = bf2f_lo(v.y); f[3] = bf2f_hi(v.y);
    f[4] = bf2f_lo(v.z); f[5] = bf2f_hi(v.z); f[6] = bf2f_lo(v.w); f[7] = bf2f_hi(v.w);
}

// One workgroup per image.  Thread t owns the CH consecutive patches t*CH .. t*CH+CH-1 (CH * 1024 >= P).
//   1. every key into LDS (padded to a multiple of 4 with 0xFFFFFFFF, which is never smaller than anything);
//   2. rank by counting: rank_p = #{q : bits_q < bits_p}, the keys read 16 bytes at a time (every lane the same address: a broadcast);
//      patch p is kept iff rank_p < K;
//   3. an exclusive prefix count of the kept flags over the workgroup (wave scan + 16 wave totals) gives slot[b, p];
//   4. keep[b, slot] = p: ascending by construction.
// PRIOR: the key is (class, bits), class 0 = foreground (counts[b, p] >= min_pixels).  The class flags sit in LDS behind the keys, one bit
// per patch (a wave's ballot is two words; the padding is background), and step 2 counts inside the patch's own class only:
//     rank_p = #{q of p's class : bits_q < bits_p} + (p is background ? n_foreground : 0).
// The flag of q is the same for every lane, so the key that q is compared against - mine for the lanes whose patch has q's class, 0 (below
// which nothing is) for the others - is one select per compare.  A row of one class gets the ranks, and so the bits, of the plain draw.
template <int CH, bool PRIOR>
__global__ __launch_bounds__(PD_THREADS) void patch_keep_kernel(unsigned key0, const long long* __restrict__ sample_ids,
                                                                const int* __restrict__ counts, int min_pixels,
                                                                int* __restrict__ keep, int* __restrict__ slot,
                                                                int* __restrict__ n_foreground, int P, int K) {
    extern __shared__ unsigned pd_keys[];
    __shared__ int wave_tot[PD_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const unsigned id = sample_ids ? (unsigned)sample_ids[b] : (unsigned)b;
    const unsigned key = mmg_drop_key_bh(key0, id);
    const int P4 = (P + 3) & ~3;
    for (int p = t; p < P4; p += PD_THREADS) pd_keys[p] = p < P ? mmg_drop_bits((unsigned)p, key) : 0xFFFFFFFFu;
    unsigned* pd_flags = pd_keys + P4;                  // PRIOR: 2 * ceil(P / 64) words, bit (p & 31) of word p >> 5
    if (PRIOR) {
        for (int base = 0; base < P; base += PD_THREADS) {         // (every lane of a wave takes every trip: the ballot needs them all)
            const int p = base + t;
            const bool fg = p < P && counts[(size_t)b * P + p] >= min_pixels;
            const unsigned long long m = __ballot(fg);
            if ((t & 63) == 0 && p < P) {
                pd_flags[p >> 5] = (unsigned)m;
                pd_flags[(p >> 5) + 1] = (unsigned)(m >> 32);
            }
        }
    }
    __syncthreads();
    unsigned mine[CH];
    int rank[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int p = t * CH + c;
        mine[c] = p < P ? pd_keys[p] : 0u;          // (rank 0 for a patch that does not exist; masked below)
        rank[c] = 0;
    }
    if (!PRIOR) {
        if (t * CH < P) {
            for (int q = 0; q < P4; q += 4) {
                const uint4 k4 = *reinterpret_cast<const uint4*>(pd_keys + q);
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    rank[c] += (int)(k4.x < mine[c]) + (int)(k4.y < mine[c]) + (int)(k4.z < mine[c]) + (int)(k4.w < mine[c]);
            }
        }
    } else if (t * CH < P) {
        unsigned as_fg[CH], as_bg[CH];              // what a foreground / a background q is compared against
        bool bg[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int p = t * CH + c;
            const bool fg = p < P && ((pd_flags[p >> 5] >> (p & 31)) & 1u);
            bg[c] = p < P && !fg;
            as_fg[c] = fg ? mine[c] : 0u;
            as_bg[c] = bg[c] ? mine[c] : 0u;
        }
        int nfg = 0;
        for (int q = 0; q < P4; q += 4) {           // (q % 4 == 0: the four flags of a step lie in one word)
            const uint4 k4 = *reinterpret_cast<const uint4*>(pd_keys + q);
            const unsigned f4 = (pd_flags[q >> 5] >> (q & 31)) & 15u;
            nfg += __popc(f4);
#pragma unroll
            for (int c = 0; c < CH; ++c)
                rank[c] += (int)(k4.x < ((f4 & 1u) ? as_fg[c] : as_bg[c])) + (int)(k4.y < ((f4 & 2u) ? as_fg[c] : as_bg[c])) +
                           (int)(k4.z < ((f4 & 4u) ? as_fg[c] : as_bg[c])) + (int)(k4.w < ((f4 & 8u) ? as_fg[c] : as_bg[c]));
        }
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (bg[c]) rank[c] += nfg;
        if (t == 0 && n_foreground) n_foreground[b] = nfg;
    }
    unsigned flags = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (t * CH + c < P && rank[c] < K) flags |= 1u << c;
    const int count = __popc(flags);
    // inclusive scan inside the wave, then the totals of the waves before this one
    const int lane = t & 63, wave = t >> 6;
    int incl = count;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int pos = incl - count;
    for (int w = 0; w < wave; ++w) pos += wave_tot[w];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int p = t * CH + c;
        if (p >= P) break;
        if (flags & (1u << c)) {
            slot[(size_t)b * P + p] = pos;
            if (pos < K) keep[(size_t)b * K + pos] = p;       // (always true: exactly K ranks are below K)
            ++pos;
        } else {
            slot[(size_t)b * P + p] = -1;
        }
    }
}

template <bool PRIOR>
static void patch_keep_launch(unsigned long long seed, const long long* sample_ids, const int* counts, int min_pixels, int B, int P, int K,
                              int* keep, int* slot, int* n_foreground, hipStream_t stream) {
    const unsigned key0 = mmg_drop_key(seed, PD_SITE);
    const size_t lds = ((size_t)((P + 3) & ~3) + (PRIOR ? 2 * (size_t)cdiv(P, 64) : 0)) * sizeof(unsigned);
    if (P <= PD_THREADS)
        hipLaunchKernelGGL((patch_keep_kernel<1, PRIOR>), dim3(B), dim3(PD_THREADS), lds, stream, key0, sample_ids, counts, min_pixels, keep,
                           slot, n_foreground, P, K);
    else if (P <= 4 * PD_THREADS)
        hipLaunchKernelGGL((patch_keep_kernel<4, PRIOR>), dim3(B), dim3(PD_THREADS), lds, stream, key0, sample_ids, counts, min_pixels, keep,
                           slot, n_foreground, P, K);
    else {
        mmg_allow_lds(patch_keep_kernel<16, PRIOR>, lds);      // P = 16384: 64 KiB of keys (and 2 KiB of flags) beside the wave totals
        hipLaunchKernelGGL((patch_keep_kernel<16, PRIOR>), dim3(B), dim3(PD_THREADS), lds, stream, key0, sample_ids, counts, min_pixels,
                           keep, slot, n_foreground, P, K);
    }
}

MMG_API int mmg_patch_keep_indices(unsigned long long seed, const long long* sample_ids, int B, int P, int K, int* keep, int* slot,
                                   hipStream_t stream) {
    MMG_CHECK_ARG(keep && slot && B > 0 && P > 0, "mmg_patch_keep_indices: bad argument");
    MMG_CHECK_ARG(P <= PD_MAX_P, "mmg_patch_keep_indices: P=%d patches per image, the workgroup's LDS layout holds %d", P, PD_MAX_P);
    MMG_CHECK_ARG(K >= 1 && K <= P, "mmg_patch_keep_indices: K=%d must be in 1 .. P=%d", K, P);
    patch_keep_launch<false>(seed, sample_ids, nullptr, 0, B, P, K, keep, slot, nullptr, stream);
    MMG_LAUNCH_CHECK("mmg_patch_keep_indices");
    return 0;
}

MMG_API int mmg_patch_keep_indices_prior(unsigned long long seed, const long long* sample_ids, const int* counts, int min_pixels, int B,
                                         int NP, int K, int* keep, int* slot, int* n_foreground, hipStream_t stream) {
    MMG_CHECK_ARG(counts && keep && slot && B > 0 && NP > 0, "mmg_patch_keep_indices_prior: bad argument");
    MMG_CHECK_ARG(NP <= PD_MAX_P, "mmg_patch_keep_indices_prior: NP=%d patches per image, the workgroup's LDS layout holds %d", NP, PD_MAX_P);
    MMG_CHECK_ARG(K >= 1 && K <= NP, "mmg_patch_keep_indices_prior: K=%d must be in 1 .. NP=%d", K, NP);
    MMG_CHECK_ARG(min_pixels >= 1, "mmg_patch_keep_indices_prior: min_pixels=%d must be at least 1 (0 would call every patch foreground)",
                  min_pixels);
    patch_keep_launch<true>(seed, sample_ids, counts, min_pixels, B, NP, K, keep, slot, n_foreground, stream);
    MMG_LAUNCH_CHECK("mmg_patch_keep_indices_prior");
    return 0;
}

// counts[i, ho * Wo + wo] = the foreground elements among the Cin * P * P canvas elements of patch (ho, wo) of image i, under the geometry of
// mmg_patchify_aug (csrc/pixel_input.hip) to the letter: canvas pixel (y, x) reads ys = y - ty, xs = x - tx, inside = 0 <= ys < H &&
// 0 <= xs < W, then the flips over the full H, W; it is foreground iff inside && x01 > threshold, x01 = r | float(r) / 65535 | float(r) / 255
// before any tone.  A fill pixel and a NaN are background.  For the integer kinds x01 is a non-decreasing function of r, so
// "float(r) / div > threshold" holds exactly for r >= rmin, the smallest such r: the host finds it by bisection WITH that division
// (fg_rmin), and the kernel compares integers - the same predicate for every r at no division per pixel.
//
// One workgroup per (image, row of patches).  It walks the SOURCE rows that land on its Cin * P canvas rows in 16-byte chunks aligned in
// memory (4 / 8 / 16 pixels), consecutive lanes on consecutive chunks, so a row of any W and any alignment is read coalesced: a chunk that
// lies wholly inside its row is one wide load, a chunk across a row's end guarded scalar loads.  Only the source columns [s_lo, s_hi) that
// land on canvas columns 0 .. Wo*P - 1 count.  A lane follows its chunk's canvas column (ascending, or descending under a flip over x) and
// adds its count to the LDS counter of a patch column whenever it leaves one: integer adds in LDS, then one writer per output.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void patch_foreground_kernel(const T* __restrict__ img, int Cin, int H, int W, int P,
                                                               const int* __restrict__ geom, float threshold, unsigned rmin,
                                                               int* __restrict__ counts) {
    extern __shared__ int fg_cnt[];                     // [Wo]
    constexpr int VEC = 16 / (int)sizeof(T);
    const int Ho = H / P, Wo = W / P, Wc = Wo * P, t = threadIdx.x;
    const int ho = (int)(blockIdx.x % (unsigned)Ho);
    const size_t n = blockIdx.x / (unsigned)Ho;
    for (int i = t; i < Wo; i += 256) fg_cnt[i] = 0;
    __syncthreads();
    int flags = 0;
    long long ty = 0, tx = 0;
    if (geom) {
        const int4 g = reinterpret_cast<const int4*>(geom)[n];
        flags = g.x; ty = g.y; tx = g.z;
    }
    const bool flipx = flags & 1, flipy = flags & 2;
    // canvas column of source column s: x = s + tx, or tx + W-1-s under the flip; the source columns with 0 <= x < Wc
    long long s_lo = flipx ? tx + W - Wc : -tx, s_hi = flipx ? tx + W : (long long)Wc - tx;
    if (s_lo < 0) s_lo = 0;
    if (s_hi > W) s_hi = W;
    if (s_lo < s_hi) {
        const int nch = (int)((s_hi - s_lo + VEC - 1) / VEC) + 1;       // chunks a row's [s_lo, s_hi) can touch, whatever its alignment
        const int items = Cin * P * nch;
        for (int item = t; item < items; item += 256) {
            const int r = item / nch, jj = item - r * nch;
            const int ci = r / P, kh = r - ci * P;
            long long ys = (long long)ho * P + kh - ty;
            if (ys < 0 || ys >= H) continue;
            if (flipy) ys = H - 1 - ys;
            const T* line = img + ((n * Cin + ci) * H + (size_t)ys) * W;
            const int mis = (int)((reinterpret_cast<uintptr_t>(line) / sizeof(T)) & (VEC - 1));    // pixels past a 16-byte boundary
            // chunk j holds the source columns j * VEC - mis .. + VEC - 1
            const long long c0 = ((s_lo + mis) / VEC + jj) * VEC - mis;
            if (c0 >= s_hi) continue;
            T v[VEC];
            if (c0 >= 0 && c0 + VEC <= W) {
                const uint4 u = *reinterpret_cast<const uint4*>(line + c0);
                __builtin_memcpy(v, &u, 16);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] = (c0 + e >= 0 && c0 + e < W) ? line[c0 + e] : (T)0;
            }
            // the chunk touches [s_lo, s_hi), so its first canvas column lies within VEC of 0 .. Wc - 1
            const int x0 = (int)(flipx ? tx + W - 1 - c0 : c0 + tx);
            int q = x0 >= 0 ? x0 / P : -((P - 1 - x0) / P);             // floor(x0 / P)
            int rem = x0 - q * P, cnt = 0;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const bool fg = KIND == 0 ? (float)v[e] > threshold : (unsigned)v[e] >= rmin;
                if (c0 + e >= s_lo && c0 + e < s_hi && fg) ++cnt;
                rem += flipx ? -1 : 1;
                if (rem < 0 || rem >= P) {                              // the next pixel belongs to another patch column
                    if (cnt) atomicAdd(&fg_cnt[q], cnt);
                    cnt = 0;
                    q += flipx ? -1 : 1;
                    rem = flipx ? P - 1 : 0;
                }
            }
            if (cnt) atomicAdd(&fg_cnt[q], cnt);
        }
    }
    __syncthreads();
    for (int i = t; i < Wo; i += 256) counts[((size_t)n * Ho + ho) * Wo + i] = fg_cnt[i];
}

// smallest r in 0 .. maxv with float(r) / div > threshold, maxv + 1 if there is none (the quotient does not decrease with r)
static unsigned fg_rmin(float threshold, float div, unsigned maxv) {
    unsigned lo = 0, hi = maxv + 1;
    while (lo < hi) {
        const unsigned mid = (lo + hi) / 2;
        if ((float)mid / div > threshold) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

MMG_API int mmg_patch_foreground(const void* img, int src_kind, int n, int Cin, int H, int W, int patch, const int* geom, float threshold,
                                 int* counts, hipStream_t stream) {
    MMG_CHECK_ARG(img && counts, "mmg_patch_foreground: null %s", img ? "counts" : "img");
    MMG_CHECK_ARG(src_kind >= 0 && src_kind <= 2, "mmg_patch_foreground: unknown src_kind %d (0 = fp32, 1 = uint16, 2 = uint8)", src_kind);
    MMG_CHECK_ARG(n > 0 && Cin > 0 && patch > 0 && H >= patch && W >= patch,
                  "mmg_patch_foreground: bad argument (n=%d Cin=%d H=%d W=%d patch=%d)", n, Cin, H, W, patch);
    MMG_CHECK_ARG(threshold >= 0.0f && threshold < 1.0f, "mmg_patch_foreground: threshold=%g must be in [0, 1)", (double)threshold);
    // (what the kernel indexes with an int: a patch's count, a workgroup's (row, chunk) items, the grid; and its LDS counters)
    MMG_CHECK_ARG((long long)Cin * patch * patch <= 0x7fffffffLL && (long long)Cin * patch * (W / 4 + 2) <= 0x7fffffffLL &&
                  (long long)n * (H / patch) <= 0x7fffffffLL && W / patch <= 16384,
                  "mmg_patch_foreground: Cin * patch * max(patch, W / 4 + 2) and n * (H / patch) must fit 31 bits, W / patch <= 16384");
    MMG_CHECK_ARG((reinterpret_cast<uintptr_t>(geom) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(img) & (src_kind == 0 ? 3 : (src_kind == 1 ? 1 : 0))) == 0,
                  "mmg_patch_foreground: misaligned pointer (geom rows are 16 bytes, pixels their own width)");
    const dim3 grid((unsigned)((long long)n * (H / patch)));
    const size_t lds = (size_t)(W / patch) * sizeof(int);
    if (src_kind == 0)
        hipLaunchKernelGGL((patch_foreground_kernel<float, 0>), grid, dim3(256), lds, stream, (const float*)img, Cin, H, W, patch, geom,
                           threshold, 0u, counts);
    else if (src_kind == 1)
        hipLaunchKernelGGL((patch_foreground_kernel<unsigned short, 1>), grid, dim3(256), lds, stream, (const unsigned short*)img, Cin, H, W,
                           patch, geom, threshold, fg_rmin(threshold, 65535.0f, 65535u), counts);
    else
        hipLaunchKernelGGL((patch_foreground_kernel<unsigned char, 2>), grid, dim3(256), lds, stream, (const unsigned char*)img, Cin, H, W,
                           patch, geom, threshold, fg_rmin(threshold, 255.0f, 255u), counts);
    MMG_LAUNCH_CHECK("mmg_patch_foreground");
    return 0;
}

// out[b*K + j, :] = p0[b*P + keep[b, j], :]   (bf16 rows of Kp elements, source row stride ld); an index outside 0 .. P-1 gives a zero row
__global__ __launch_bounds__(256) void gather_patch_rows_kernel(const bf16_t* __restrict__ p0, long ld, const int* __restrict__ keep,
                                                                uint4* __restrict__ out, int P, int K, int chunks, long total) {
    for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < total; w += (long)gridDim.x * 256) {
        const long row = w / chunks;
        const int c = (int)(w - row * chunks);
        const long b = row / K;
        const int p = keep[row];
        uint4 v = {0u, 0u, 0u, 0u};
        if ((unsigned)p < (unsigned)P) v = *reinterpret_cast<const uint4*>(p0 + (b * P + p) * ld + (long)c * 8);
        out[w] = v;
    }
}

static inline bool pd_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int pd_blocks(long total) { return total > 4096L * 256 ? 4096 : cdiv(total, 256); }

MMG_API int mmg_gather_patch_rows(const void* p0, long long ld, const int* keep, void* out, int B, int P, int K, int Kp,
                                  hipStream_t stream) {
    MMG_CHECK_ARG(p0 && keep && out && p0 != out && B > 0 && P > 0 && Kp > 0, "mmg_gather_patch_rows: bad argument");
    MMG_CHECK_ARG(K >= 1 && K <= P, "mmg_gather_patch_rows: K=%d must be in 1 .. P=%d", K, P);
    MMG_CHECK_ARG(Kp % 8 == 0 && ld % 8 == 0 && ld >= Kp, "mmg_gather_patch_rows: Kp=%d and ld=%lld must be multiples of 8, ld >= Kp", Kp, ld);
    MMG_CHECK_ARG(pd_aligned(p0) && pd_aligned(out), "mmg_gather_patch_rows: p0 and out must be 16-byte aligned");
    const int chunks = Kp / 8;
    const long total = (long)B * K * chunks;
    hipLaunchKernelGGL(gather_patch_rows_kernel, dim3(pd_blocks(total)), dim3(256), 0, stream, (const bf16_t*)p0, (long)ld, keep,
                       reinterpret_cast<uint4*>(out), P, K, chunks, total);
    MMG_LAUNCH_CHECK("mmg_gather_patch_rows");
    return 0;
}

// X[b, 0, :] = cls + pos[0];  X[b, 1+j, :] = tok[b*K + j, :] + pos[1 + keep[b, j], :]   (bf16 in/out, fp32 add: vit_assemble_kernel's
// arithmetic, positions added as if before the drop).  One wave per token row.
__global__ __launch_bounds__(256) void vit_assemble_keep_kernel(const bf16_t* __restrict__ tok, const bf16_t* __restrict__ cls,
                                                                const bf16_t* __restrict__ pos, const int* __restrict__ keep,
                                                                bf16_t* __restrict__ out, int B, int P, int K, int H) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = H / 8, S = K + 1;
    for (long m = (long)blockIdx.x * 4 + wave; m < (long)B * S; m += (long)gridDim.x * 4) {
        const long b = m / S;
        const int s = (int)(m - b * S);
        const bf16_t* src = s == 0 ? cls : tok + (b * K + (s - 1)) * H;
        int prow = 0;
        if (s > 0) {
            const int p = keep[b * K + (s - 1)];
            prow = 1 + ((unsigned)p < (unsigned)P ? p : 0);         // (a bad index cannot leave the table)
        }
        for (int c = lane; c < nch; c += 64) {
            float a[8], p[8];
            unpack8p(*reinterpret_cast<const uint4*>(src + c * 8), a);
            unpack8p(*reinterpret_cast<const uint4*>(pos + (size_t)prow * H + c * 8), p);
            uint4 o;
            o.x = pack2bf(a[0] + p[0], a[1] + p[1]); o.y = pack2bf(a[2] + p[2], a[3] + p[3]);
            o.z = pack2bf(a[4] + p[4], a[5] + p[5]); o.w = pack2bf(a[6] + p[6], a[7] + p[7]);
            *reinterpret_cast<uint4*>(out + m * H + c * 8) = o;
        }
    }
}

MMG_API int mmg_vit_assemble_keep_fwd(const void* tok, const void* cls, const void* pos, const int* keep, void* out, int B, int P,
                                      int K, int H, hipStream_t stream) {
    MMG_CHECK_ARG(tok && cls && pos && keep && out && B > 0 && P > 0 && H > 0, "mmg_vit_assemble_keep_fwd: bad argument");
    MMG_CHECK_ARG(K >= 1 && K <= P, "mmg_vit_assemble_keep_fwd: K=%d must be in 1 .. P=%d", K, P);
    MMG_CHECK_ARG(H % 8 == 0, "mmg_vit_assemble_keep_fwd: H=%d must be a multiple of 8 (16-byte accesses)", H);
    MMG_CHECK_ARG(pd_aligned(tok) && pd_aligned(cls) && pd_aligned(pos) && pd_aligned(out),
                  "mmg_vit_assemble_keep_fwd: tok, cls, pos and out must be 16-byte aligned");
    int blocks = cdiv((long)B * (K + 1), 4);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(vit_assemble_keep_kernel, dim3(blocks), dim3(256), 0, stream, (const bf16_t*)tok, (const bf16_t*)cls,
                       (const bf16_t*)pos, keep, (bf16_t*)out, B, P, K, H);
    MMG_LAUNCH_CHECK("mmg_vit_assemble_keep_fwd");
    return 0;
}

// backward, one wave per position s = 0 .. P of the FULL table, 8 columns per lane:
//   s = 0:      acc = sum_b g[b, 0, :];  dpos[0] += acc;  dcls += acc
//   s = 1 + p:  acc = sum over the images that kept p, in ascending b, of g[b, 1 + slot[b, p], :], each row copied to dtok[b*K + slot] on
//               the way (every kept row has one p, so one writer);  dpos[s] += acc - or nothing at all when no image kept p.
// fp32 sums from 0 in ascending b, then one add into dpos: the order of vit_assemble_bwd_kernel, so both give the same bits.
__global__ __launch_bounds__(256) void vit_assemble_keep_bwd_kernel(const bf16_t* __restrict__ g, const int* __restrict__ slot,
                                                                    bf16_t* __restrict__ dtok, float* __restrict__ dpos,
                                                                    float* __restrict__ dcls, int B, int P, int K, int H) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * 4 + wave;
    if (s > P) return;
    const int nch = H / 8, S = K + 1;
    for (int c = lane; c < nch; c += 64) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool any = false;
        for (int b = 0; b < B; ++b) {
            int j = 0;
            if (s > 0) {
                j = slot[(size_t)b * P + (s - 1)];
                if (j < 0 || j >= K) continue;
                j += 1;
            }
            any = true;
            const uint4 v = *reinterpret_cast<const uint4*>(g + ((size_t)b * S + j) * H + c * 8);
            float f[8];
            unpack8p(v, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += f[e];
            if (s > 0) *reinterpret_cast<uint4*>(dtok + ((size_t)b * K + (j - 1)) * H + c * 8) = v;
        }
        if (!any) continue;
        float4* dp = reinterpret_cast<float4*>(dpos + (size_t)s * H + c * 8);
        float4 lo = dp[0], hi = dp[1];
        lo.x += acc[0]; lo.y += acc[1]; lo.z += acc[2]; lo.w += acc[3];
        hi.x += acc[4]; hi.y += acc[5]; hi.z += acc[6]; hi.w += acc[7];
        dp[0] = lo; dp[1] = hi;
        if (s == 0) {
            float4* dc = reinterpret_cast<float4*>(dcls + c * 8);
            float4 a = dc[0], d = dc[1];
            a.x += acc[0]; a.y += acc[1]; a.z += acc[2]; a.w += acc[3];
            d.x += acc[4]; d.y += acc[5]; d.z += acc[6]; d.w += acc[7];
            dc[0] = a; dc[1] = d;
        }
    }
}

MMG_API int mmg_vit_assemble_keep_bwd(const void* g, const int* slot, void* dtok, float* dpos, float* dcls, int B, int P, int K, int H,
                                      hipStream_t stream) {
    MMG_CHECK_ARG(g && slot && dtok && dpos && dcls && B > 0 && P > 0 && H > 0, "mmg_vit_assemble_keep_bwd: bad argument");
    MMG_CHECK_ARG(K >= 1 && K <= P, "mmg_vit_assemble_keep_bwd: K=%d must be in 1 .. P=%d", K, P);
    MMG_CHECK_ARG(H % 8 == 0, "mmg_vit_assemble_keep_bwd: H=%d must be a multiple of 8 (16-byte accesses)", H);
    MMG_CHECK_ARG(pd_aligned(g) && pd_aligned(dtok) && pd_aligned(dpos) && pd_aligned(dcls),
                  "mmg_vit_assemble_keep_bwd: g, dtok, dpos and dcls must be 16-byte aligned");
    hipLaunchKernelGGL(vit_assemble_keep_bwd_kernel, dim3(cdiv(P + 1, 4)), dim3(256), 0, stream, (const bf16_t*)g, slot, (bf16_t*)dtok,
                       dpos, dcls, B, P, K, H);
    MMG_LAUNCH_CHECK("mmg_vit_assemble_keep_bwd");
    return 0;
}
