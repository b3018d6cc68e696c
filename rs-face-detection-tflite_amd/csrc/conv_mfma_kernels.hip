// conv_mfma_kernels.hip — dense k x k convolution as an implicit GEMM on the f32 matrix cores (v_mfma_f32_32x32x2_f32), for gfx950.
//
// The ResNet-style embedding networks spend their time in 3x3 convolutions with 32 .. 512 input channels; conv_generic_kernel (kernels.hip) runs
// those as scalar fmaf chains, one thread per pixel and four output channels.  Here the launch is ONE matrix product, laid out like sim_tile.hpp:
//   M = the output pixels of the whole launch, the frames concatenated (a 7 x 7 layer fills its tiles across items),
//   N = Co,   K = KH * KW * C ordered (ky, kx, c) — the order of a TFLite filter row, so the filter [Co][KH][KW][C] IS the B operand [N][K].
// A workgroup of four waves owns a 128 x TN tile (TN = 128, or 64 so that Co = 32 / 64 does not waste half of it); wave w the 64 x TN/2 part
// (w >> 1, w & 1) as 2 x TN/64 MFMA tiles.  K goes through LDS in chunks of 32, rows of 33 floats (the bank argument of sim_tile.hpp holds as it
// stands), the next chunk's buffer loads in flight under this chunk's MFMAs.
//   A: a tile row is an output pixel.  With C % 32 == 0 a chunk lies inside one tap: its 32 floats are contiguous at input pixel
//      (oy sh - pt + ky, ox sw - pl + kx), channel c0.  A thread keeps, for each of its 16 rows, the byte offset of the window's corner from the
//      launch's input base and one bit per tap (is it inside the picture); a tap outside, and a row beyond M, is staged as zeros.
//   B: row n0 + r of the filter, 32 floats at k0; rows beyond Co are staged as zeros.
// Both through buffer loads with 32-bit offsets: the launcher (launch_conv_mfma) splits a launch over frame ranges so that input, output and skip
// of a range fit in 2^31 bytes.  Every access also carries its own test (offset 0 and a zero in place of the value): nothing relies on the range check.
// Determinism: an output element is one chain over k = 0 .. K - 1 (two k per MFMA, chunk after chunk; an outside tap adds x = 0 products), the
// same chain whatever the batch size, the element's place in a tile or the tile width: its bits depend on nothing but its own inputs.
// Epilogue as conv_generic_kernel's: + bias, RES_DIRECT skip in front of or behind the activation, the four activations.  In the MFMA result a
// lane's column (lane & 31) is the output channel: a store instruction writes 32 consecutive channels of a pixel, 128 contiguous bytes in NHWC.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "launch.hpp"

namespace mi {
namespace {

constexpr int kCmTM = 128, kCmK = 32, kCmLd = kCmK + 1, kCmThreads = 256, kCmRowsA = kCmTM / (kCmThreads / kCmK);
typedef float cm_f32x16 __attribute__((ext_vector_type(16)));

template <int TN>
__global__ __launch_bounds__(kCmThreads) void conv_mfma_kernel(ConvArgs a) {
    constexpr int VT = TN / 64;                          // 32-column MFMA tiles of a wave
    constexpr int kRowsB = TN / (kCmThreads / kCmK);     // filter rows a thread stages
    __shared__ float s_a[kCmTM * kCmLd];
    __shared__ float s_b[TN * kCmLd];
    __shared__ long s_out[kCmTM], s_res[kCmTM];          // per tile row: float offset of the pixel in out / in the skip tensor (-1: a row beyond M)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = tid & (kCmK - 1), r0 = tid >> 5;      // staging: column kk of rows r0 + 8 q
    const int tiles_n = (a.Co + TN - 1) / TN;
    const int n0 = (int)(blockIdx.x % tiles_n) * TN;
    const long m0 = (long)(blockIdx.x / tiles_n) * kCmTM;
    const int HoWo = a.Ho * a.Wo, K = a.KH * a.KW * a.C, cpt = a.C / kCmK, nchunks = a.KH * a.KW * cpt;

    const auto rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, (int)((((long)a.B - 1) * a.in_fs + (long)a.H * a.W * a.C) * 4), 0x00020000);
    const auto rsrc_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w_rows), 0, (int)((long)a.Co * K * 4), 0x00020000);

    int aoff[kCmRowsA];        // bytes from a.in to channel kk of the window's corner pixel (it may lie outside: only used where the tap's bit is set)
    unsigned amask[kCmRowsA];  // bit ky * KW + kx: that tap of the row's window is inside the picture
    {
        const long m = m0 + r0;
        int b = (int)(m / HoWo);
        const int p = (int)(m - (long)b * HoWo);
        int oy = p / a.Wo, ox = p - oy * a.Wo;
#pragma unroll
        for (int q = 0; q < kCmRowsA; q++) {
            const bool live = b < a.B;
            const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;
            unsigned mask = 0, bit = 1;
            for (int ky = 0; ky < a.KH; ky++)
                for (int kx = 0; kx < a.KW; kx++, bit <<= 1)
                    if (live && iy0 + ky >= 0 && iy0 + ky < a.H && ix0 + kx >= 0 && ix0 + kx < a.W) mask |= bit;
            amask[q] = mask;
            aoff[q] = live ? (int)(((long)b * a.in_fs + ((long)iy0 * a.W + ix0) * a.C + kk) * 4) : 0;
            if (kk == 0) {
                const long pix = (long)oy * a.Wo + ox;
                s_out[r0 + 8 * q] = live ? (long)b * a.out_fs + pix * a.Co : -1;
                s_res[r0 + 8 * q] = live ? (long)b * a.ep.res_fs + pix * a.ep.res_C : 0;
            }
            ox += 8;   // the thread's next row is eight pixels on
            while (ox >= a.Wo) { ox -= a.Wo; oy++; }
            while (oy >= a.Ho) { oy -= a.Ho; b++; }
        }
    }

    float ra[kCmRowsA], rb[kRowsB];
    // chunk: tap `tap`, whose first element lies `delta` bytes behind the window's corner, filter columns from k0
    auto fetch = [&](int tap, int delta, int k0) {
#pragma unroll
        for (int q = 0; q < kCmRowsA; q++) {
            const bool in = (amask[q] >> tap) & 1u;
            const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_a, in ? aoff[q] + delta : 0, 0, 0));
            ra[q] = in ? v : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kRowsB; q++) {
            const int n = n0 + r0 + 8 * q;
            const bool in = n < a.Co;
            const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_b, in ? (n * K + k0 + kk) * 4 : 0, 0, 0));
            rb[q] = in ? v : 0.f;
        }
    };

    cm_f32x16 acc[2][VT];
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < VT; v++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[u][v][e] = 0.f;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * (TN / 2), lr = lane & 31, lh = lane >> 5;
    const float* pa = s_a + (wi + lr) * kCmLd + lh;
    const float* pb = s_b + (wj + lr) * kCmLd + lh;

    int ky = 0, kx = 0, ci = 0;   // the chunk in flight
    fetch(0, 0, 0);
    for (int j = 0; j < nchunks; j++) {
        __syncthreads();   // the readers of the previous chunk are done
#pragma unroll
        for (int q = 0; q < kCmRowsA; q++) s_a[(r0 + 8 * q) * kCmLd + kk] = ra[q];
#pragma unroll
        for (int q = 0; q < kRowsB; q++) s_b[(r0 + 8 * q) * kCmLd + kk] = rb[q];
        __syncthreads();
        if (j + 1 < nchunks) {
            if (++ci == cpt) { ci = 0; if (++kx == a.KW) { kx = 0; ky++; } }
            fetch(ky * a.KW + kx, ((ky * a.W + kx) * a.C + ci * kCmK) * 4, (j + 1) * kCmK);
        }
#pragma unroll
        for (int ks = 0; ks < kCmK; ks += 2) {
            const float a0 = pa[ks], a1 = pa[32 * kCmLd + ks];
#pragma unroll
            for (int v = 0; v < VT; v++) {
                const float bv = pb[32 * v * kCmLd + ks];
                acc[0][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0][v], 0, 0, 0);
                acc[1][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1][v], 0, 0, 0);
            }
        }
    }

    // C/D of the 32 x 32 form: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int v = 0; v < VT; v++) {
        const int n = n0 + wj + 32 * v + lr;
        if (n >= a.Co) continue;
        const float bias = a.ep.bias ? a.ep.bias[n] : 0.f;
        const bool skip = a.ep.res_mode == RES_DIRECT && n < a.ep.res_C;
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int row = wi + 32 * u + (e & 3) + 8 * (e >> 2) + 4 * lh;
                const long o = s_out[row];
                if (o < 0) continue;
                float r = acc[u][v][e] + bias;
                const float sk = skip ? a.ep.res[s_res[row] + n] : 0.f;
                if (!a.ep.res_after) r += sk;
                switch (a.ep.act) {
                    case ACT_RELU: r = r > 0.f ? r : 0.f; break;
                    case ACT_RELU6: r = r < 0.f ? 0.f : (r > 6.f ? 6.f : r); break;
                    case ACT_PRELU: r = r >= 0.f ? r : a.ep.alpha[n] * r; break;
                    default: break;
                }
                if (a.ep.res_after) r += sk;
                a.out[o + n] = r;
            }
    }
}

constexpr long kCmMaxBytes = 0x7fffffffL;   // what a 32-bit byte offset (kept in an int) reaches

}  // namespace

bool conv_mfma_shape_ok(int C, int KH, int KW, int Co) {
    return C >= kCmK && C % kCmK == 0 && KH >= 1 && KW >= 1 && KH * KW > 1 && KH * KW <= 32 && Co >= 1 && (long)Co * KH * KW * C * 4 <= kCmMaxBytes;
}

bool conv_mfma_supports(const ConvArgs& a) {
    if (!a.mfma || !a.w_rows || a.in_u8 || !a.in || !a.out || !conv_mfma_shape_ok(a.C, a.KH, a.KW, a.Co)) return false;
    if (a.B < 1 || a.H < 1 || a.W < 1 || a.Ho < 1 || a.Wo < 1 || a.sh < 1 || a.sw < 1 || a.pt < 0 || a.pl < 0) return false;
    if (a.ep.res_mode != RES_NONE && a.ep.res_mode != RES_DIRECT) return false;
    if (a.ep.act == ACT_PRELU && !a.ep.alpha) return false;
    if (a.H == a.KH && a.W == a.KW && a.Ho == 1 && a.Wo == 1) return false;   // a whole-frame head: the batch GEMM's, or the generic kernel's
    if (a.sh == a.KH && a.sw == a.KW) return false;   // k x k stride-k (windows that do not overlap): the stage programs' gather form; alone, the generic kernel's, as the shipped iris graph's launch lists have them
    // one frame must fit the 32-bit offsets (the launcher splits a launch between frames, not inside one)
    const long in_frame = std::max((long)a.H * a.W * a.C, a.in_fs), out_frame = std::max((long)a.Ho * a.Wo * a.Co, a.out_fs);
    const long res_frame = a.ep.res_mode == RES_DIRECT ? std::max((long)a.Ho * a.Wo * a.ep.res_C, a.ep.res_fs) : 0;
    return in_frame * 4 <= kCmMaxBytes && out_frame * 4 <= kCmMaxBytes && res_frame * 4 <= kCmMaxBytes && (long)a.H * a.W <= 0x3fffffffL;
}

int launch_conv_mfma(const ConvArgs& a, void* stream) {
    if (!conv_mfma_supports(a)) return (int)hipErrorInvalidValue;
    // frames per launch: input, output and skip of the range within 2^31 bytes of their first frame
    const long in_frame = std::max((long)a.H * a.W * a.C, a.in_fs), out_frame = std::max((long)a.Ho * a.Wo * a.Co, a.out_fs);
    const long res_frame = a.ep.res_mode == RES_DIRECT ? std::max((long)a.Ho * a.Wo * a.ep.res_C, a.ep.res_fs) : 1;
    const long most = std::max(in_frame, std::max(out_frame, res_frame));
    const int per = (int)std::max(1L, std::min((long)a.B, kCmMaxBytes / 4 / most));
    const bool narrow = a.Co <= 64;
    for (int b0 = 0; b0 < a.B; b0 += per) {
        ConvArgs r = a;
        r.B = std::min(per, a.B - b0);
        r.in = a.in + (long)b0 * a.in_fs;
        r.out = a.out + (long)b0 * a.out_fs;
        if (a.ep.res) r.ep.res = a.ep.res + (long)b0 * a.ep.res_fs;
        const long tiles_m = ((long)r.B * r.Ho * r.Wo + kCmTM - 1) / kCmTM;
        // 128 x 64 tiles where Co is at most 64, and where 128 x 128 tiles would leave compute units without one
        const bool tn64 = narrow || tiles_m * ((r.Co + 127) / 128) < device_cu_count();
        const long grid = tiles_m * ((r.Co + (tn64 ? 63 : 127)) / (tn64 ? 64 : 128));
        if (grid > 0x7fffffffL) return (int)hipErrorInvalidValue;
        const hipError_t e = tn64 ? launch_kernel(conv_mfma_kernel<64>, dim3((unsigned)grid), dim3(kCmThreads), 0, (hipStream_t)stream, r)
                                  : launch_kernel(conv_mfma_kernel<128>, dim3((unsigned)grid), dim3(kCmThreads), 0, (hipStream_t)stream, r);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace mi
