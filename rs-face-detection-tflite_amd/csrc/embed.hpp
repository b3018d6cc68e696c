// embed.hpp — what follows the network in FaceEmbeddings::infer and its callers: l2_norm and similarity_score
// (/root/reference/src/face_detection_lite/utils.rs:30-50), for rows that live in device memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace mi {

constexpr int kSimMaxFeatures = 4096;   // features of mi_similarity_matrix: 1..4096

// The reference's sums: `iter().map(..).sum::<f32>()` — f32, in index order, the product and the add rounded separately.  One statement for
// the host entries (mi_l2_norm, mi_similarity_score) and the device kernels.
__host__ __device__ inline float embed_mul(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fmul_rn(a, b);
#else
    volatile float p = a * b;   // (no contraction with the add behind it, whatever the flags)
    return p;
#endif
}
__host__ __device__ inline float embed_add(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
__host__ __device__ inline float embed_sqrt(float a) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fsqrt_rn(a);
#else
    return std::sqrt(a);
#endif
}
__host__ __device__ inline float embed_div(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
// sum of a[k] * b[k], k = 0 .. n-1, as above
__host__ __device__ inline float embed_dot(const float* a, const float* b, int n) {
    float acc = 0.f;
    for (int k = 0; k < n; k++) acc = embed_add(acc, embed_mul(a[k], b[k]));
    return acc;
}

// l2_norm (utils.rs:30-33) of N rows of D values: emb[i] = raw[i] / sqrt(sum raw[i]^2), one lane per row.  valid (may be null: every row)
// = 0 writes zeros into the row of emb and of raw_out; raw_out (may be null) receives a copy of the valid rows.
void launch_l2_norm(const float* d_raw, const int* d_valid, int N, int D, float* d_emb, float* d_raw_out, hipStream_t s);

// out[i][j] = similarity_score(a_i, b_j) (utils.rs:44-50) for a [n][D], b [m][D]: an NT GEMM on v_mfma_f32_32x32x2_f32, the row norms taken
// from the staged rows in the reference's order, the epilogue dot / (norm_a * norm_b).  Device pointers; D 1..kSimMaxFeatures.
void launch_similarity(const float* d_a, int n, const float* d_b, int m, int D, float* d_out, hipStream_t s);

}  // namespace mi
