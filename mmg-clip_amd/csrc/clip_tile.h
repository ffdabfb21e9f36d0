// Tile helpers of the contrastive-head kernels (clip_head.hip, averaged_head.hip): 32 local rows of X in LDS, 32-column tiles of Y
// streamed, fp32 on v_mfma_f32_32x32x2_f32 issued "swapped" (A = Y tile, B = X tile) so that a lane holds ONE row i and 16 columns j.
#pragma once
#include "common.h"

#define CLIP_ROWS 32
#define CLIP_THREADS 256
#define NEG_BIG (-1.0e30f)

// row index inside a 32x32 f32 MFMA accumulator: reg r of lane-half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---------------------------------------------------------------------------------------------
// Z^T tile: acc[reg] of lane (i = lane&31, h = lane>>5) = <Y[j0 + acc_row(reg,h)], X[i]>
// Xs: LDS image of the 32 local rows, row pitch xld floats.  yrow: this lane's (clamped) Y row.
// k order inside a step is arbitrary as long as A and B agree: half h takes k = 8c + 4h + e.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x16 zt_tile(const float* __restrict__ yrow, const float* Xs_row, int D, int h) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float4* yp = reinterpret_cast<const float4*>(yrow) + h;
    const float4* xp = reinterpret_cast<const float4*>(Xs_row) + h;
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
        const float4 yv = yp[2 * c];
        const float4 xv = xp[2 * c];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.x, xv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.y, xv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.z, xv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.w, xv.w, acc, 0, 0, 0);
    }
    return acc;
}

// Stage the workgroup's 32 rows of X into LDS (rows beyond n_loc are clamped duplicates).
__device__ __forceinline__ void stage_x(const float* __restrict__ X, float* Xs, int i0, int n_loc, int D, int xld) {
    const int nvec = D / 4;
    for (int idx = threadIdx.x; idx < CLIP_ROWS * nvec; idx += CLIP_THREADS) {
        const int r = idx / nvec, c = idx - r * nvec;
        const int gr = min(i0 + r, n_loc - 1);
        const float4 v = reinterpret_cast<const float4*>(X + (size_t)gr * D)[c];
        *reinterpret_cast<float4*>(Xs + r * xld + 4 * c) = v;
    }
}
