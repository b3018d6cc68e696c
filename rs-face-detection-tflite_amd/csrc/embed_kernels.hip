// embed_kernels.hip — l2_norm and the cosine-similarity matrix of face embeddings on the device (reference:
// /root/reference/src/face_detection_lite/utils.rs:30-50; called from face_embeddings.rs:86 and its test, :143).
#include "embed.hpp"

#include <stdexcept>

#include "engine.hpp"

namespace mi {
namespace {

// One lane per row: the reference's sum is sequential, and D values per item are nothing next to the network in front of this launch.
__global__ __launch_bounds__(64) void l2_norm_kernel(const float* __restrict__ raw, const int* __restrict__ valid, int N, int D,
                                                     float* __restrict__ emb, float* __restrict__ raw_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* x = raw + (long)i * D;
    float* e = emb + (long)i * D;
    float* r = raw_out ? raw_out + (long)i * D : nullptr;
    if (valid && !valid[i]) {
        for (int k = 0; k < D; k++) {
            e[k] = 0.f;
            if (r) r[k] = 0.f;
        }
        return;
    }
    float acc = 0.f;
    for (int k = 0; k < D; k++) acc = embed_add(acc, embed_mul(x[k], x[k]));
    const float norm = embed_sqrt(acc);
    for (int k = 0; k < D; k++) {
        const float v = x[k];
        e[k] = embed_div(v, norm);   // a norm of zero gives what `arr / norm` gives: IEEE division
        if (r) r[k] = v;
    }
}

// ---- similarity matrix.  A workgroup of four waves owns a 128 x 128 tile of `out`; wave w the 64 x 64 quarter (w >> 1, w & 1) as 2 x 2 MFMA
// tiles of 32 x 32 (v_mfma_f32_32x32x2_f32: lane l feeds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31], one f32 each).  K goes
// through LDS in chunks of 32, rows of 33 floats: a ds_read_b32 / ds_write_b32 conflicts within a 32-lane half on (address / 4) % 32, and
// every access below has its 32 lanes either on 32 consecutive floats of one row (the stores) or on one column of 32 consecutive rows (the
// MFMA operands, the norms' walk) — distinct banks with the odd row length.  The next chunk's global loads are issued before the chunk in LDS
// is multiplied.  The K tail and the rows beyond n / m are staged as zeros: a zero adds nothing to a dot product or to a sum of squares.
// Norms: thread t < 128 walks row t of the `a` tile, thread t >= 128 row t - 128 of the `b` tile, chunk after chunk, in index order with the
// multiply and the add rounded separately — the reference's sum, bit for bit.  The dot products are the MFMA's k-ordered fma chains.
constexpr int kSimTile = 128, kSimK = 32, kSimLd = kSimK + 1, kSimThreads = 256, kSimRows = kSimTile / (kSimThreads / kSimK);
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(kSimThreads) void similarity_kernel(const float* __restrict__ a, int n, const float* __restrict__ b, int m, int D,
                                                                 float* __restrict__ out, int tiles_m) {
    __shared__ float s_a[kSimTile * kSimLd], s_b[kSimTile * kSimLd];
    __shared__ float s_norm[2 * kSimTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = blockIdx.x / tiles_m, tj = blockIdx.x - ti * tiles_m;
    const long i0 = (long)ti * kSimTile, j0 = (long)tj * kSimTile;
    // staging: thread t carries column t & 31 of rows (t >> 5) + 8 q, q = 0 .. 15, of both tiles
    const int kk = tid & (kSimK - 1), r0 = tid >> 5;
    float ra[kSimRows], rb[kSimRows];
    auto fetch = [&](int k0) {
        const int k = k0 + kk;
#pragma unroll
        for (int q = 0; q < kSimRows; q++) {
            const long gi = i0 + r0 + 8 * q, gj = j0 + r0 + 8 * q;
            ra[q] = (k < D && gi < n) ? a[gi * D + k] : 0.f;
            rb[q] = (k < D && gj < m) ? b[gj * D + k] : 0.f;
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
            const long gj = j0 + col;
            const float nb = s_norm[kSimTile + col];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int row = wi + 32 * u + (e & 3) + 8 * (e >> 2) + 4 * lh;
                const long gi = i0 + row;
                if (gi < n && gj < m) out[gi * m + gj] = embed_div(acc[u][v][e], embed_mul(s_norm[row], nb));
            }
        }
}

}  // namespace

void launch_l2_norm(const float* d_raw, const int* d_valid, int N, int D, float* d_emb, float* d_raw_out, hipStream_t s) {
    if (N <= 0 || D <= 0) return;
    hipLaunchKernelGGL(l2_norm_kernel, dim3((N + 63) / 64), dim3(64), 0, s, d_raw, d_valid, N, D, d_emb, d_raw_out);
    hip_check(hipGetLastError(), "l2_norm kernel launch");
}

void launch_similarity(const float* d_a, int n, const float* d_b, int m, int D, float* d_out, hipStream_t s) {
    const long tiles_n = (static_cast<long>(n) + kSimTile - 1) / kSimTile, tiles_m = (static_cast<long>(m) + kSimTile - 1) / kSimTile;
    if (tiles_n * tiles_m > 0x7fffffffL) throw std::runtime_error("similarity matrix: n x m is too large for one launch");
    hipLaunchKernelGGL(similarity_kernel, dim3(static_cast<unsigned>(tiles_n * tiles_m)), dim3(kSimThreads), 0, s, d_a, n, d_b, m, D, d_out,
                       static_cast<int>(tiles_m));
    hip_check(hipGetLastError(), "similarity kernel launch");
}

}  // namespace mi
