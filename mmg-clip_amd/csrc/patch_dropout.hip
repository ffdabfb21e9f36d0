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
// Four memory-bound kernels, no atomics, every output element written by exactly one thread: bit-reproducible.  The row movers read and
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
template <int CH>
__global__ __launch_bounds__(PD_THREADS) void patch_keep_kernel(unsigned key0, const long long* __restrict__ sample_ids,
                                                                int* __restrict__ keep, int* __restrict__ slot, int P, int K) {
    extern __shared__ unsigned pd_keys[];
    __shared__ int wave_tot[PD_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const unsigned id = sample_ids ? (unsigned)sample_ids[b] : (unsigned)b;
    const unsigned key = mmg_drop_key_bh(key0, id);
    const int P4 = (P + 3) & ~3;
    for (int p = t; p < P4; p += PD_THREADS) pd_keys[p] = p < P ? mmg_drop_bits((unsigned)p, key) : 0xFFFFFFFFu;
    __syncthreads();
    unsigned mine[CH];
    int rank[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int p = t * CH + c;
        mine[c] = p < P ? pd_keys[p] : 0u;          // (rank 0 for a patch that does not exist; masked below)
        rank[c] = 0;
    }
    if (t * CH < P) {
        for (int q = 0; q < P4; q += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(pd_keys + q);
#pragma unroll
            for (int c = 0; c < CH; ++c)
                rank[c] += (int)(k4.x < mine[c]) + (int)(k4.y < mine[c]) + (int)(k4.z < mine[c]) + (int)(k4.w < mine[c]);
        }
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

MMG_API int mmg_patch_keep_indices(unsigned long long seed, const long long* sample_ids, int B, int P, int K, int* keep, int* slot,
                                   hipStream_t stream) {
    MMG_CHECK_ARG(keep && slot && B > 0 && P > 0, "mmg_patch_keep_indices: bad argument");
    MMG_CHECK_ARG(P <= PD_MAX_P, "mmg_patch_keep_indices: P=%d patches per image, the workgroup's LDS layout holds %d", P, PD_MAX_P);
    MMG_CHECK_ARG(K >= 1 && K <= P, "mmg_patch_keep_indices: K=%d must be in 1 .. P=%d", K, P);
    const unsigned key0 = mmg_drop_key(seed, PD_SITE);
    const size_t lds = (size_t)((P + 3) & ~3) * sizeof(unsigned);
    if (P <= PD_THREADS)
        hipLaunchKernelGGL(patch_keep_kernel<1>, dim3(B), dim3(PD_THREADS), lds, stream, key0, sample_ids, keep, slot, P, K);
    else if (P <= 4 * PD_THREADS)
        hipLaunchKernelGGL(patch_keep_kernel<4>, dim3(B), dim3(PD_THREADS), lds, stream, key0, sample_ids, keep, slot, P, K);
    else {
        mmg_allow_lds(patch_keep_kernel<16>, lds);      // P = 16384: 64 KiB of keys beside the wave totals
        hipLaunchKernelGGL(patch_keep_kernel<16>, dim3(B), dim3(PD_THREADS), lds, stream, key0, sample_ids, keep, slot, P, K);
    }
    MMG_LAUNCH_CHECK("mmg_patch_keep_indices");
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
