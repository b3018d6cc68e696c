// embed_kernels.hip — l2_norm and the cosine-similarity matrix of face embeddings on the device (reference:
// /root/reference/src/face_detection_lite/utils.rs:30-50; called from face_embeddings.rs:86 and its test, :143).
#include "embed.hpp"

#include <stdexcept>

#include "engine.hpp"
#include "sim_tile.hpp"

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

// ---- similarity matrix.  One workgroup per 128 x 128 tile of `out`; the tile itself is sim_tile_scores (sim_tile.hpp), which the gallery's
// top-k kernel runs too.
__global__ __launch_bounds__(kSimThreads) void similarity_kernel(const float* __restrict__ a, int n, const float* __restrict__ b, int m, int D,
                                                                 float* __restrict__ out, int tiles_m) {
    __shared__ float s_a[kSimStageFloats], s_b[kSimStageFloats];
    __shared__ float s_norm[2 * kSimTile];
    const int ti = blockIdx.x / tiles_m, tj = blockIdx.x - ti * tiles_m;
    const long i0 = (long)ti * kSimTile, j0 = (long)tj * kSimTile;
    sim_tile_scores(a, n, b, m, D, i0, j0, s_a, s_b, s_norm, [&](int row, int col, auto&& score) {
        const long gi = i0 + row, gj = j0 + col;
        if (gi < n && gj < m) out[gi * m + gj] = score();
    });
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
