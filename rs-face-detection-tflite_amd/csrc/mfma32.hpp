// mfma32.hpp — the quad-level vocabulary of the frame-resident MFMA kernels (block, dblock, bneck, chain, resident, xc, bandnet and
// head_kernels.hip's head_gemm on v_mfma_f32_32x32x2_f32, tail on 16x16x4) in the "operand layout": lane = pixel x k-half, the depthwise result of four
// channels is the B operand of four MFMAs, and a quad of the result D is four consecutive output channels of the lane's pixel.
// (stem_kernels.hip and head_dot_kernel take the one-value activation act1 from here and nothing else.)
// Nothing here is a schedule or a layout: 16-byte loads and stores, the four-wide FMA / add / max, the four MFMAs of an (A, B) float4
// pair, the plain nine-tap depthwise chunk, the activation with and without the bias + skip in front of it, the ragged store of output
// heads with Co % 4 != 0, the stage programs' tensor reference and magic division, and the s_memtime stamp of the diagnostic builds.
// A run-time choice between an LDS and a global pointer turns a load FLAT, and a flat load waits on vmcnt AND lgkmcnt: the kernels pick
// the address space of what they hand to ld4 at compile time (template switches ALDS, WL, MODE ...).
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mi {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 max4(float4 a, float4 b, float4 c, float4 d) {
    return make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y)),
                       fmaxf(fmaxf(a.z, b.z), fmaxf(c.z, d.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(c.w, d.w)));
}
// acc += d * w, per component
__device__ __forceinline__ void fma4(const float4& d, const float4& w, float4& acc) {
    acc.x = fmaf(d.x, w.x, acc.x);
    acc.y = fmaf(d.y, w.y, acc.y);
    acc.z = fmaf(d.z, w.z, acc.z);
    acc.w = fmaf(d.w, w.w, acc.w);
}
__device__ __forceinline__ float4 add4(const float4& v, const float4& b) { return make_float4(v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w); }
// quad gq of a result tile: this lane's output channels 8 gq + 4 h .. + 3 of the tile
__device__ __forceinline__ float4 quad4(const f32x16& D, int gq) { return make_float4(D[4 * gq], D[4 * gq + 1], D[4 * gq + 2], D[4 * gq + 3]); }

// D += A . B over the four k-steps of an (A, B) float4 pair
__device__ __forceinline__ void mfma32_quad(const float4& av, const float4& bf, f32x16& D) {
    D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bf.x, D, 0, 0, 0);
    D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bf.y, D, 0, 0, 0);
    D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bf.z, D, 0, 0, 0);
    D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bf.w, D, 0, 0, 0);
}

// Depthwise 3x3 of four channels: tap (ky, kx) at taps + (3 ky + kx) tap_stride, its pixel at win + ky row_stride + kx px_stride; the
// taps in order, starting from the bias (BIAS_FIRST) or from zero with the bias added last.  The plain loop only: the copies with a
// load schedule of their own (block_kernel's row-ahead double buffer, dblock's shared 4 x 3 window, chain's DwTaps) use fma4.
template <bool BIAS_FIRST>
__device__ __forceinline__ float4 dw3x3_quad(const float* taps, int tap_stride, const float* win, int row_stride, int px_stride, const float* bias) {
    float4 bf = BIAS_FIRST ? ld4(bias) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int ky = 0; ky < 3; ky++)
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
            const float4 w = ld4(taps + (ky * 3 + kx) * tap_stride);
            const float4 d = ld4(win + ky * row_stride + kx * px_stride);
            fma4(d, w, bf);
        }
    if (!BIAS_FIRST) bf = add4(bf, ld4(bias));
    return bf;
}

// max(v, 0) + slope min(v, 0), capped at hi: ReLU (slope 0), ReLU6 (hi 6), PReLU, none (slope 1)
__device__ __forceinline__ float4 act4(const float4& v, const float4& slope, float hi) {
    return make_float4(fminf(fmaxf(v.x, 0.f) + slope.x * fminf(v.x, 0.f), hi), fminf(fmaxf(v.y, 0.f) + slope.y * fminf(v.y, 0.f), hi),
                       fminf(fmaxf(v.z, 0.f) + slope.z * fminf(v.z, 0.f), hi), fminf(fmaxf(v.w, 0.f) + slope.w * fminf(v.w, 0.f), hi));
}
// the same for one value (the first convolution's and the whole-frame heads' epilogues)
__device__ __forceinline__ float act1(float v, float slope, float hi) { return fminf(fmaxf(v, 0.f) + slope * fminf(v, 0.f), hi); }
// act((D + bias) + skip), in this order
__device__ __forceinline__ float4 bias_skip_act4(const float4& Dq, const float4& bias, const float4& skip, const float4& slope, float hi) {
    return act4(add4(add4(Dq, bias), skip), slope, hi);
}

// channels ch .. ch + 3 of an output with Co % 4 != 0 (the heads with 213, 15, 1 channels) to dst = the pixel's channel ch; ch < Co
__device__ __forceinline__ void store4_ragged(float* dst, int ch, int Co, const float4& v) {
    dst[0] = v.x;
    if (ch + 1 < Co) dst[1] = v.y;
    if (ch + 2 < Co) dst[2] = v.z;
    if (ch + 3 < Co) dst[3] = v.w;
}

// a stage program's tensor reference -> this frame's pointer
__device__ __forceinline__ float* res_resolve(const ResBases& bs, const ResRef& r, int frame) {
    return bs.p[r.base] + r.root_off * bs.scale[r.base] + r.inner + (long)(frame + bs.frame0[r.base]) * r.fs;
}
// n / d for n * d < 2^32 with m = ceil(2^32 / d) (host: tail_magic; m = 0 stands for d = 1)
__device__ __forceinline__ int magic_div(int n, unsigned m) { return m ? (int)__umulhi((unsigned)n, m) : n; }

}  // namespace

}  // namespace mi

// diagnostic builds: slot <- s_memtime, fenced so that the scheduler moves nothing across the stamp
#define MI_STAMP_AT(slot) { __builtin_amdgcn_sched_barrier(0); slot = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
