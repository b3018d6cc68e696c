// embed_ops_kernels.hip — the operators of pooled-head and ONNX-exported embedding graphs (gfx950): AVERAGE_POOL_2D / MEAN, L2_NORMALIZATION, TRANSPOSE.
//
// Every output element is ONE k-ordered f32 chain, each operation rounded once (__fadd_rn, __fmul_rn, __fsqrt_rn, __fdiv_rn: nothing contracts, nothing
// is approximated), so its bits depend neither on the number of frames nor on the launch shape, and tests/embed_ops_synth.py restates them in numpy
// scalar by scalar.  No tree reductions: the order is the contract.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "launch.hpp"

namespace mi {
namespace {

__device__ __forceinline__ float pool_act(float v, int act) {  // the fused activations a pool can carry: NONE, RELU, RELU6
    if (act == ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == ACT_RELU6) return v < 0.f ? 0.f : (v > 6.f ? 6.f : v);
    return v;
}

// AVERAGE_POOL_2D (MEAN over H and W: the window is the frame).  One thread per output element (V = 4: per four channels, float4 accesses), C the
// fastest index so that a wave's loads are consecutive; from 0.0f the window's in-frame taps are added in (ky, kx) order — taps outside the frame are
// skipped, not added as zeros — then one division by the number of taps that were in the frame.  p0 = filter_h, p1 = filter_w, p2 = stride_h, p3 = stride_w.
template <int V>
__global__ __launch_bounds__(256) void avgpool_kernel(EltArgs a, int pt, int pl) {
    const int CV = a.C / V;
    const long per = (long)a.Ho * a.Wo * CV;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    const int b = (int)(idx / per);
    const long e = idx % per;
    const int c = (int)(e % CV) * V;
    const int ox = (int)((e / CV) % a.Wo), oy = (int)(e / ((long)CV * a.Wo));
    const float* x = a.a + (long)b * a.a_fs;
    float s[V];
#pragma unroll
    for (int j = 0; j < V; j++) s[j] = 0.f;
    int taps = 0;
    for (int ky = 0; ky < a.p0; ky++) {
        const int iy = oy * a.p2 - pt + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < a.p1; kx++) {
            const int ix = ox * a.p3 - pl + kx;
            if (ix < 0 || ix >= a.W) continue;
            const float* p = x + ((long)iy * a.W + ix) * a.C + c;
            if constexpr (V == 4) {
                const float4 v = *reinterpret_cast<const float4*>(p);
                s[0] = __fadd_rn(s[0], v.x); s[1] = __fadd_rn(s[1], v.y); s[2] = __fadd_rn(s[2], v.z); s[3] = __fadd_rn(s[3], v.w);
            } else {
                s[0] = __fadd_rn(s[0], *p);
            }
            taps++;
        }
    }
    const float d = (float)taps;
    float* o = a.out + (long)b * a.out_fs + ((long)oy * a.Wo + ox) * a.C + c;
    if constexpr (V == 4) {
        float4 r;
        r.x = pool_act(__fdiv_rn(s[0], d), a.act); r.y = pool_act(__fdiv_rn(s[1], d), a.act);
        r.z = pool_act(__fdiv_rn(s[2], d), a.act); r.w = pool_act(__fdiv_rn(s[3], d), a.act);
        *reinterpret_cast<float4*>(o) = r;
    } else {
        *o = pool_act(__fdiv_rn(s[0], d), a.act);
    }
}

// L2_NORMALIZATION over the last dimension (C) of the H * W rows of every frame: s = 0, s = s + x[c] * x[c] in channel order (multiply and add rounded
// separately), n = max(sqrt(s), 1e-6f), out[c] = x[c] / n.  The sum is one sequential chain in both forms:
//   WAVE  a wave per row: lane 0 sums, every lane divides (few rows: one embedding per item)
//   else  a thread per row (feature maps: many short rows)
template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 256) void l2norm_rows_kernel(EltArgs a) {
    const long R = (long)a.H * a.W, rows = R * a.B;
    const long row = WAVE ? (long)blockIdx.x : (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;   // (WAVE: the whole wave)
    const int b = (int)(row / R);
    const long r = row % R;
    const float* x = a.a + (long)b * a.a_fs + r * a.C;
    float* o = a.out + (long)b * a.out_fs + r * a.C;
    float n = 0.f;
    if (!WAVE || threadIdx.x == 0) {
        float s = 0.f;
        for (int k = 0; k < a.C; k++) s = __fadd_rn(s, __fmul_rn(x[k], x[k]));
        n = fmaxf(__fsqrt_rn(s), 1e-6f);
    }
    if (WAVE) {
        n = __shfl(n, 0, 64);
        for (int k = (int)threadIdx.x; k < a.C; k += 64) o[k] = __fdiv_rn(x[k], n);
    } else {
        for (int k = 0; k < a.C; k++) o[k] = __fdiv_rn(x[k], n);
    }
}

// TRANSPOSE, any perm that keeps the batch axis: one thread per output element; s1..s3 = the input's stride (in floats) of the dimension that output
// dimension 1..3 walks.  64-bit arithmetic throughout.
__global__ __launch_bounds__(256) void transpose_kernel(EltArgs a, long s1, long s2, long s3) {
    const long per = (long)a.Ho * a.Wo * a.Co;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * a.B) return;
    const int b = (int)(idx / per);
    const long e = idx % per;
    const long o3 = e % a.Co, o2 = (e / a.Co) % a.Wo, o1 = e / ((long)a.Co * a.Wo);
    a.out[(long)b * a.out_fs + e] = a.a[(long)b * a.a_fs + o1 * s1 + o2 * s2 + o3 * s3];
}

// NHWC <-> NCHW: per frame the matrix transpose [R][Cn] -> [Cn][R].  A workgroup (32 x 8 threads) moves one 32 x 32 tile through LDS in rows of 33 floats:
// it reads 32 consecutive floats of eight matrix rows at a time (coalesced), and writes 32 consecutive floats of the transposed rows (coalesced);
// ds_write_b32 / ds_read_b32 bank by dword address mod 32, so tile[j][tx] (33 j + tx) and tile[tx][j] (33 tx + j) are both conflict-free over 32 lanes.
// Ragged edges are bound-checked on both sides.  Tiles on blockIdx.x, frames on blockIdx.y; offsets inside a frame are 32-bit (the launch checks R * Cn < 2^31).
__global__ __launch_bounds__(256) void transpose_tiled_kernel(const float* __restrict__ in, float* __restrict__ out, long in_fs, long out_fs, int R, int Cn, int tiles_c) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = (int)(blockIdx.x / (unsigned)tiles_c) * 32, c0 = (int)(blockIdx.x % (unsigned)tiles_c) * 32;
    const float* x = in + (long)blockIdx.y * in_fs;
    float* o = out + (long)blockIdx.y * out_fs;
    for (int j = ty; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + tx;
        if (r < R && c < Cn) tile[j][tx] = x[(unsigned)r * (unsigned)Cn + (unsigned)c];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + tx;
        if (c < Cn && r < R) o[(unsigned)c * (unsigned)R + (unsigned)r] = tile[tx][j];
    }
}

inline unsigned nblocks(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int launch_avgpool(const EltArgs& a, void* s) {
    if (a.p0 < 1 || a.p1 < 1 || a.p2 < 1 || a.p3 < 1 || a.C != a.Co || a.C < 1) return (int)hipErrorInvalidValue;
    if (a.act != ACT_NONE && a.act != ACT_RELU && a.act != ACT_RELU6) return (int)hipErrorInvalidValue;
    const long n = (long)a.B * a.Ho * a.Wo * a.C;
    if (n <= 0) return 0;
    // TF SAME pads as launch_maxpool has them: total = max(0, (out - 1) * stride + filter - in), before = total / 2 (VALID: total <= 0)
    const int tph = (a.Ho - 1) * a.p2 + a.p0 - a.H, tpw = (a.Wo - 1) * a.p3 + a.p1 - a.W;
    const int pt = tph > 0 ? tph / 2 : 0, pl = tpw > 0 ? tpw / 2 : 0;
    if (n >= (1L << 31) * 256) return (int)hipErrorInvalidValue;
    if (a.C % 4 == 0 && a.a_fs % 4 == 0 && a.out_fs % 4 == 0 && aligned16(a.a) && aligned16(a.out))
        return (int)launch_kernel(avgpool_kernel<4>, dim3(nblocks(n / 4)), dim3(256), 0, (hipStream_t)s, a, pt, pl);
    return (int)launch_kernel(avgpool_kernel<1>, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a, pt, pl);
}

int launch_l2norm_rows(const EltArgs& a, void* s) {
    const long rows = (long)a.B * a.H * a.W;
    if (rows < 0 || a.C < 1) return (int)hipErrorInvalidValue;
    if (rows == 0) return 0;
    if (rows < kL2NormLaneRows) return (int)launch_kernel(l2norm_rows_kernel<true>, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)s, a);
    if (rows >= (1L << 31) * 256) return (int)hipErrorInvalidValue;
    return (int)launch_kernel(l2norm_rows_kernel<false>, dim3(nblocks(rows)), dim3(256), 0, (hipStream_t)s, a);
}

int launch_transpose(const EltArgs& a, void* s) {
    const int p[3] = {a.p1, a.p2, a.p3}, in_dim[4] = {0, a.H, a.W, a.C}, out_dim[3] = {a.Ho, a.Wo, a.Co};
    int seen = 0;
    for (int d = 0; d < 3; d++) {
        if (p[d] < 1 || p[d] > 3 || (seen >> p[d] & 1) || out_dim[d] != in_dim[p[d]]) return (int)hipErrorInvalidValue;
        seen |= 1 << p[d];
    }
    const long n = (long)a.B * a.H * a.W * a.C;
    if (n <= 0) return 0;
    if (transpose_takes_tiled(a)) {
        const bool to_nchw = a.p1 == 3;
        const int R = to_nchw ? a.H * a.W : a.H, Cn = to_nchw ? a.C : a.W * a.C;
        const long tiles_c = (Cn + 31) / 32, tiles_r = (R + 31) / 32;
        if (tiles_c * tiles_r < (1L << 31))
            return (int)launch_kernel(transpose_tiled_kernel, dim3((unsigned)(tiles_c * tiles_r), (unsigned)a.B), dim3(256), 0, (hipStream_t)s, a.a, a.out, a.a_fs, a.out_fs, R, Cn,
                                      (int)tiles_c);
    }
    if (n >= (1L << 31) * 256) return (int)hipErrorInvalidValue;
    const long stride[4] = {0, (long)a.W * a.C, (long)a.C, 1};
    return (int)launch_kernel(transpose_kernel, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)s, a, stride[a.p1], stride[a.p2], stride[a.p3]);
}

}  // namespace mi
