// head_kernels.hip — convolutions whose window is the whole frame (HeadGemmArgs: the face mesh's 3x3 head, the iris network's 2x2 heads, a
// FULLY_CONNECTED; behind `interpreter.invoke()`, face_landmark.rs:265, iris_landmark.rs:203) as a product over the batch:
//   head_gemm_kernel  32 frames x 32 outputs per wave on v_mfma_f32_32x32x2_f32
//   head_dot_kernel   a wave per (output, frame) for the one to four frames of a single-image call
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "mfma32.hpp"

namespace mi {

// ------------------------------------------------------------------------------------------------ frame-batched head GEMM
// out[b][n] = act(bias[n] + sum_k x[b][k] * W[n][k]) on v_mfma_f32_32x32x2_f32: one wave per 32 frames x 32 outputs.  The
// contraction index is split in two halves (lanes 0-31 take k in [0, K/2), lanes 32-63 take [K/2, K)), so every lane reads
// its operands as float4 of four consecutive k: four MFMAs per pair of 16-byte loads, both operands straight from L2.
__global__ __launch_bounds__(256) void head_gemm_kernel(HeadGemmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * 32, b0 = blockIdx.y * 32;
    if (n0 >= a.N) return;  // whole wave
    const int r = lane & 31, h = lane >> 5, K2 = a.K >> 1;
    const float* xp = a.in + (long)min(b0 + r, a.B - 1) * a.in_fs + h * K2;   // rows past the batch / the outputs re-read the
    const float* wp = a.w + (long)min(n0 + r, a.N - 1) * a.K + h * K2;        // last valid one; their results are not stored
    f32x16 D;
#pragma unroll
    for (int e = 0; e < 16; e++) D[e] = 0.f;
    float4 xa = ld4(xp), wa = ld4(wp);
    for (int j = 0; j < K2; j += 4) {
        const int jn = min(j + 4, K2 - 4);
        const float4 xn = ld4(xp + jn), wn = ld4(wp + jn);  // next chunk in flight under this chunk's MFMAs
        mfma32_quad(xa, wa, D);
        xa = xn; wa = wn;
    }
    // D[v]: frame b0 + 4 * h + 8 * (v / 4) + v % 4, output n0 + r
    const int n = n0 + r;
    if (n >= a.N) return;
    const float bias = a.bias ? a.bias[n] : 0.f;
    const float slope = a.act == ACT_PRELU ? a.alpha[n] : (a.act == ACT_NONE ? 1.f : 0.f);
    const float hi = a.act == ACT_RELU6 ? 6.f : INFINITY;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        const int b = b0 + 4 * h + 8 * (v >> 2) + (v & 3);
        if (b >= a.B) continue;
        const float t = D[v] + bias;
        a.out[(long)b * a.out_fs + n] = act1(t, slope, hi);
    }
}

// The same product for the one to four frames of a single-image call (face_landmark.rs:265, iris_landmark.rs:203): a 32-frame MFMA tile with one live
// frame is 256 dependent 64-cycle MFMAs for the iris network's K = 512 (17 us per head, two heads in line behind the band launch).  Here a wave owns
// one (output, frame): its lanes read 16 bytes of x and of W[n] each per round (coalesced), four partial sums per lane, then a butterfly over the
// wave — a fixed order, so run-to-run bit-identical (it is not the MFMA's order: within the raw tolerance of the batched form, like every small-batch form).
__global__ __launch_bounds__(256) void head_dot_kernel(HeadGemmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wave, b = blockIdx.y;
    if (n >= a.N) return;  // whole wave
    const float4* x = reinterpret_cast<const float4*>(a.in + (long)b * a.in_fs);
    const float4* w = reinterpret_cast<const float4*>(a.w + (long)n * a.K);
    const int K4 = a.K >> 2;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int j = lane; j < K4; j += 64) {
        const float4 xv = x[j], wv = w[j];
        s0 = fmaf(xv.x, wv.x, s0); s1 = fmaf(xv.y, wv.y, s1); s2 = fmaf(xv.z, wv.z, s2); s3 = fmaf(xv.w, wv.w, s3);
    }
    float sum = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) {
        const float t = sum + (a.bias ? a.bias[n] : 0.f);
        const float slope = a.act == ACT_PRELU ? a.alpha[n] : (a.act == ACT_NONE ? 1.f : 0.f);
        const float hi = a.act == ACT_RELU6 ? 6.f : INFINITY;
        a.out[(long)b * a.out_fs + n] = act1(t, slope, hi);
    }
}

bool head_gemm_supports(int K, int N) { return K >= 16 && (K % 8) == 0 && N >= 1; }

int launch_head_gemm(const HeadGemmArgs& a, void* stream) {
    if (!head_gemm_supports(a.K, a.N) || a.B < 1 || (a.in_fs & 3) || !aligned16(a.in) || !aligned16(a.w))
        return (int)hipErrorInvalidValue;
    if (a.B <= 4 && !a.one_form) return (int)launch_kernel(head_dot_kernel, dim3((unsigned)((a.N + 3) / 4), (unsigned)a.B), dim3(256), 0, (hipStream_t)stream, a);
    const unsigned tiles_n = (unsigned)((a.N + 31) / 32);
    return (int)launch_kernel(head_gemm_kernel, dim3((tiles_n + 3) / 4, (unsigned)((a.B + 31) / 32)), dim3(256), 0, (hipStream_t)stream, a);
}

}  // namespace mi
