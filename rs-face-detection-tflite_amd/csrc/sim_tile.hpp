// sim_tile.hpp — one 128 x 128 tile of cosine scores on the f32 matrix cores: the body that similarity_kernel (embed_kernels.hip) and
// gallery_topk_kernel (topk_kernels.hip) share, so that both produce the same bits by construction.  Device code only.
//
// A workgroup of four waves owns a 128 x 128 tile; wave w the 64 x 64 quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles of 32 x 32
// (v_mfma_f32_32x32x2_f32: lane l feeds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31], one f32 each).  K goes through LDS in
// chunks of 32, rows of 33 floats: a ds_read_b32 / ds_write_b32 conflicts within a 32-lane half on (address / 4) % 32, and every access
// below has its 32 lanes either on 32 consecutive floats of one row (the stores) or on one column of 32 consecutive rows (the MFMA
// operands, the norms' walk) — distinct banks with the odd row length.  The next chunk's global loads are issued before the chunk in LDS is
// multiplied.  The K tail and the rows beyond n / m are staged as zeros: a zero adds nothing to a dot product or to a sum of squares.
// Norms: thread t < 128 walks row t of the `a` tile, thread t >= 128 row t - 128 of the `b` tile, chunk after chunk, in index order with the
// multiply and the add rounded separately — the reference's sum, bit for bit.  The dot products are the MFMA's k-ordered fma chains.
#pragma once

#include <hip/hip_runtime.h>

#include "embed.hpp"

namespace mi {

constexpr int kSimTile = 128, kSimK = 32, kSimLd = kSimK + 1, kSimThreads = 256, kSimRows = kSimTile / (kSimThreads / kSimK);
constexpr int kSimStageFloats = kSimTile * kSimLd;   // floats of one staged operand tile
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The tile (i0 .., j0 ..) of a [n][D] against b [m][D].  s_a and s_b hold kSimStageFloats each, s_norm 2 * kSimTile.  Every score of the
// tile, padding rows and columns included (those are 0 / 0: NaN), goes to emit(row, col, score) with row, col 0..127 inside the tile and
// score() the epilogue dot / (norm_a * norm_b), evaluated where emit calls it; the thread that holds the accumulator calls emit.  The first statement that touches LDS is a barrier, and a barrier stands between the last
// read of s_a / s_b and the first emit: a caller may keep data of its own in s_a / s_b from the first emit until it calls this again.
template <class Emit>
__device__ __forceinline__ void sim_tile_scores(const float* __restrict__ a, int n, const float* __restrict__ b, int m, int D, long i0, long j0,
                                                float* s_a, float* s_b, float* s_norm, Emit&& emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // staging: thread t carries column t & 31 of rows (t >> 5) + 8 q, q = 0 .. 15, of both tiles
    const int kk = tid & (kSimK - 1), r0 = tid >> 5;
    float ra[kSimRows], rb[kSimRows];
    // Buffer loads: the tile's rows start at a workgroup-uniform address and an element lies less than 128 * 4096 floats behind it, so a
    // load is a descriptor in scalar registers plus a 32-bit byte offset — the same sixteen offsets for both operands, no 64-bit address
    // per row — and the descriptor ends with the tile's last row inside n / m: the rows beyond read as zeros by the range check.
    const int rows_a = n - i0 < kSimTile ? (int)(n - i0) : kSimTile, rows_b = m - j0 < kSimTile ? (int)(m - j0) : kSimTile;
    const auto rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a + i0 * D), 0, rows_a * D * 4, 0x00020000);
    const auto rsrc_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(b + j0 * D), 0, rows_b * D * 4, 0x00020000);
    const int off0 = (r0 * D + kk) * 4, step = 8 * D * 4;
    auto fetch = [&](int k0) {
        const bool in_k = k0 + kk < D;   // (the K tail reads into the next row, or past the end for zero, and is dropped here)
#pragma unroll
        for (int q = 0; q < kSimRows; q++) {
            const float va = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_a, off0 + q * step, 4 * k0, 0));
            const float vb = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_b, off0 + q * step, 4 * k0, 0));
            ra[q] = in_k ? va : 0.f;
            rb[q] = in_k ? vb : 0.f;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < 2; v++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[u][v][e] = 0.f;
    float sq = 0.f;
    const float* s_mine = tid < kSimTile ? s_a + tid * kSimLd : s_b + (tid - kSimTile) * kSimLd;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64, lr = lane & 31, lh = lane >> 5;
    const float* pa = s_a + (wi + lr) * kSimLd + lh;
    const float* pb = s_b + (wj + lr) * kSimLd + lh;
    fetch(0);
    for (int k0 = 0; k0 < D; k0 += kSimK) {
        __syncthreads();   // the readers of the previous chunk are done
#pragma unroll
        for (int q = 0; q < kSimRows; q++) {
            s_a[(r0 + 8 * q) * kSimLd + kk] = ra[q];
            s_b[(r0 + 8 * q) * kSimLd + kk] = rb[q];
        }
        __syncthreads();
        if (k0 + kSimK < D) fetch(k0 + kSimK);
#pragma unroll
        for (int k = 0; k < kSimK; k++) {
            const float v = s_mine[k];
            sq = embed_add(sq, embed_mul(v, v));
        }
#pragma unroll
        for (int ks = 0; ks < kSimK; ks += 2) {
            const float a0 = pa[ks], a1 = pa[32 * kSimLd + ks], b0 = pb[ks], b1 = pb[32 * kSimLd + ks];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    s_norm[tid] = embed_sqrt(sq);
    __syncthreads();
    // C/D of the 32 x 32 form: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < 2; v++) {
            const int col = wj + 32 * v + lr;
            const float nb = s_norm[kSimTile + col];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int row = wi + 32 * u + (e & 3) + 8 * (e >> 2) + 4 * lh;
                emit(row, col, [&] { return embed_div(acc[u][v][e], embed_mul(s_norm[row], nb)); });
            }
        }
}

}  // namespace mi
