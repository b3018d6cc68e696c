// conv_bf16_kernels.hip — the dense k x k convolution of conv_mfma_kernels.hip on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16), for gfx950:
// engine option "conv_bf16" = 1 ("bf16": operands rounded to bf16) or 2 ("bf16x3": every operand split into two bf16 values, three products
// for one).  Tensors stay f32 in memory; only the operands of the MFMAs are narrower.
//
// The GEMM is conv_mfma_kernel's: M = the output pixels of the launch (frames concatenated), N = Co, K = KH * KW * C in (ky, kx, c) order,
// 128 x TN tiles (TN = 128 or 64), four waves, wave w the 64 x TN/2 part (w >> 1, w & 1) as 2 x TN/64 MFMA tiles, K in chunks of 32 (C % 32 == 0:
// a chunk lies inside one tap), the next chunk's buffer loads in flight under this chunk's MFMAs, the same per-row window offset and tap mask,
// the same epilogue (bias, RES_DIRECT skip in front of or behind the activation, the four activations; all in f32, on the unrounded skip),
// the same splitting of a launch between frames so that 32-bit byte offsets reach everything (launch_conv_bf16).
//   A: loaded as f32, 16 bytes a buffer load (a thread takes 8 consecutive channels of two tile rows), converted in registers on the way
//      into LDS: hi = (__bf16)x, round to nearest even (v_cvt_pk_bf16_f32); SPLIT: lo = (__bf16)(x - (float)hi).  LDS holds bf16.
//   B: the filter [Co][K] rounded on the host (consts.cpp) into a bf16 `hi` plane, SPLIT: and a `lo` plane = bf16(w - hi); 16 bytes a load,
//      stored to LDS as they are.  Nothing is converted per launch.
//   MFMA: lane l (r = l & 31, h = l >> 5) holds A[r][8h .. 8h+7] and B[8h .. 8h+7][r] of a 16-deep k-step: one 16-byte LDS read per operand.
//      C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), as in the f32 32 x 32 form.
// LDS rows: a chunk row is 32 bf16 = 64 bytes, kept 80 bytes apart (kCbLd = 40 bf16).  80 is a multiple of 16, so every fragment read
// (row * 80 + 32 ks + 16 h bytes) is a 16-byte-aligned ds_read_b128.  Banks: a ds_read_b128 is served in four groups of 16 lanes
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32); the lanes of a group share h and ks, and their rows are 16 different
// residues mod 16.  A read covers the 16-byte slot (row * 5 + 2 ks + h) mod 16 of the 256-byte bank row, and 5 is odd: 16 rows that differ
// mod 16 take the 16 different slots.  No fragment read conflicts.  The staging stores (ds_write_b128, groups of 8 consecutive lanes = two
// rows of four 16-byte pieces, banks mod 32) overlap on four banks of two rows, 2-way: one LDS-array cycle more on an instruction whose
// 13 cycles are set by moving its data, not by the array.
// K chunk: 32, whatever C (a multiple of 32) is.  The plain form stages TWO chunks per pair of barriers (KC = 2: two register sets in flight, two
// LDS images, each with the row stride above): half the barriers and half the load round trips for 40 KiB of LDS at TN = 128, a quarter of the
// CU's.  The split form's four planes take those 40 KiB with one chunk, so it stays at one.  An odd number of chunks ends in a half-filled pair.
// Workgroup ids are remapped so that the ids an XCD gets (id mod 8) are one contiguous run of tiles: neighbours in M share input rows in that L2.
// Determinism: an output element is one chain: chunks in (ky, kx, c) order (staged two at a time or not), two k-steps a chunk; in a k-step of the split form the three
// MFMAs run small terms first: lo * w_hi, hi * w_lo, hi * w_hi.  The chain is the same whatever the batch size, the element's place in a
// tile or the tile width: its bits depend on nothing but its own inputs.
// Edges: an outside tap, a row beyond M and a filter row beyond Co are staged as zeros; every access carries its own test (offset 0 and a
// zero in place of the value), nothing relies on the buffer range check.
// Non-finite values: a non-finite activation gives non-finite outputs.  In the split form an infinity becomes NaN: hi = inf, and
// x - (float)hi = inf - inf = NaN ends up in lo.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "launch.hpp"

namespace mi {
namespace {

constexpr int kCbTM = 128, kCbK = 32, kCbLd = kCbK + 8, kCbThreads = 256;
constexpr int kCbRowsA = kCbTM / (kCbThreads / 4);   // a thread stages 8 consecutive k of rows r0 + 64 q
typedef float cb_f32x16 __attribute__((ext_vector_type(16)));
typedef float cb_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned cb_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 cb_bf16x8 __attribute__((ext_vector_type(8)));

template <int TN, bool SPLIT>
__global__ __launch_bounds__(kCbThreads) __attribute__((amdgpu_waves_per_eu(2))) void conv_bf16_kernel(ConvArgs a) {   // (two waves a SIMD: VGPRs + AGPRs within 256)
    constexpr int VT = TN / 64;                       // 32-column MFMA tiles of a wave
    constexpr int kRowsB = TN / (kCbThreads / 4);     // filter rows a thread stages
    constexpr int NP = SPLIT ? 2 : 1;                 // planes: hi, lo
    constexpr int KC = SPLIT ? 1 : 2;                 // chunks staged per pair of barriers (the plain form has the LDS and the registers for two)
    // [chunk][plane][row][kCbLd] bf16; after the last chunk the first bytes of s_a hold, per tile row, the float offset of the pixel in out (-1: a row beyond M) and in the skip tensor
    __shared__ __attribute__((aligned(16))) __bf16 s_a[KC * NP * kCbTM * kCbLd];
    __shared__ __attribute__((aligned(16))) __bf16 s_b[KC * NP * TN * kCbLd];
    static_assert(sizeof(s_a) >= 2 * kCbTM * sizeof(int), "the epilogue's row offsets live in s_a");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = tid & 3, r0 = tid >> 2;             // staging: k 8 g .. 8 g + 7 of rows r0 + 64 q
    const int tiles_n = (a.Co + TN - 1) / TN;
    // workgroups whose ids are equal mod 8 share an XCD and its L2: each of the eight groups takes one contiguous run of tiles, so that the N tiles
    // of an M tile and the M tiles next to it (which read the same input rows) meet in one L2.  A bijection for any grid; speed only, no bit depends on it
    const unsigned nwg = gridDim.x, xq = nwg / 8, xr = nwg % 8, xcd = blockIdx.x % 8;
    const unsigned tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + blockIdx.x / 8;
    const int n0 = (int)(tile % tiles_n) * TN;
    const long m0 = (long)(tile / tiles_n) * kCbTM;
    const int HoWo = a.Ho * a.Wo, K = a.KH * a.KW * a.C, cpt = a.C / kCbK, nchunks = a.KH * a.KW * cpt;

    const auto rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, (int)((((long)a.B - 1) * a.in_fs + (long)a.H * a.W * a.C) * 4), 0x00020000);
    const auto rsrc_bh = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w_bf16), 0, (int)((long)a.Co * K * 2), 0x00020000);
    const auto rsrc_bl = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(SPLIT ? a.w_bf16_lo : a.w_bf16), 0, (int)((long)a.Co * K * 2), 0x00020000);

    int aoff[kCbRowsA];        // bytes from a.in to channel 8 g of the window's corner pixel (it may lie outside: only used where the tap's bit is set)
    unsigned amask[kCbRowsA];  // bit ky * KW + kx: that tap of the row's window is inside the picture
    int oout[kCbRowsA], ores[kCbRowsA];   // float offset of the row's pixel in out (-1: a row beyond M) / in the skip tensor
#pragma unroll
    for (int q = 0; q < kCbRowsA; q++) {
        const long m = m0 + r0 + 64 * q;
        const int b = (int)(m / HoWo);
        const int p = (int)(m - (long)b * HoWo);
        const int oy = p / a.Wo, ox = p - oy * a.Wo;
        const bool live = b < a.B;
        const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;
        unsigned mask = 0, bit = 1;
        for (int ky = 0; ky < a.KH; ky++)
            for (int kx = 0; kx < a.KW; kx++, bit <<= 1)
                if (live && iy0 + ky >= 0 && iy0 + ky < a.H && ix0 + kx >= 0 && ix0 + kx < a.W) mask |= bit;
        amask[q] = mask;
        aoff[q] = live ? (int)(((long)b * a.in_fs + ((long)iy0 * a.W + ix0) * a.C + 8 * g) * 4) : 0;
        oout[q] = live ? (int)((long)b * a.out_fs + (long)p * a.Co) : -1;
        ores[q] = live ? (int)((long)b * a.ep.res_fs + (long)p * a.ep.res_C) : 0;
    }

    cb_f32x4 ra[KC][kCbRowsA][2] = {};
    cb_u32x4 rb[KC][NP][kRowsB] = {};
    // chunk into register set s: tap `tap`, whose first element lies `delta` bytes behind the window's corner, filter columns from k0
    auto fetch = [&](int s, int tap, int delta, int k0) {
#pragma unroll
        for (int q = 0; q < kCbRowsA; q++) {
            const bool in = (amask[q] >> tap) & 1u;
            const int off = in ? aoff[q] + delta : 0;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const cb_f32x4 v = __builtin_bit_cast(cb_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, off + 16 * e, 0, 0));
                ra[s][q][e] = in ? v : cb_f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int q = 0; q < kRowsB; q++) {
            const int n = n0 + r0 + 64 * q;
            const bool in = n < a.Co;
            const int off = in ? (n * K + k0 + 8 * g) * 2 : 0;
            const cb_u32x4 v = __builtin_bit_cast(cb_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_bh, off, 0, 0));
            rb[s][0][q] = in ? v : cb_u32x4{0u, 0u, 0u, 0u};
            if (SPLIT) {
                const cb_u32x4 l = __builtin_bit_cast(cb_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_bl, off, 0, 0));
                rb[s][NP - 1][q] = in ? l : cb_u32x4{0u, 0u, 0u, 0u};
            }
        }
    };

    cb_f32x16 acc[2][VT];
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int v = 0; v < VT; v++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[u][v][e] = 0.f;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * (TN / 2), lr = lane & 31, lh = lane >> 5;
    const __bf16* pa = s_a + (wi + lr) * kCbLd + 8 * lh;
    const __bf16* pb = s_b + (wj + lr) * kCbLd + 8 * lh;
    auto frag = [](const __bf16* p) { return *reinterpret_cast<const cb_bf16x8*>(p); };

    int ky = 0, kx = 0, ci = 0, jn = 0;   // the next chunk to fetch: its tap, its channel chunk, its index
    // the next KC chunks (as many as are left) into the register sets
    auto fetch_group = [&]() {
#pragma unroll
        for (int s = 0; s < KC; s++) {
            if (jn >= nchunks) break;
            fetch(s, ky * a.KW + kx, ((ky * a.W + kx) * a.C + ci * kCbK) * 4, jn * kCbK);
            jn++;
            if (++ci == cpt) { ci = 0; if (++kx == a.KW) { kx = 0; ky++; } }
        }
    };
    fetch_group();
    for (int j = 0; j < nchunks; j += KC) {
        __syncthreads();   // the readers of the previous chunks are done
#pragma unroll
        for (int s = 0; s < KC; s++) {   // (a set beyond the last chunk holds old values: staged, never multiplied)
            __bf16* sa = s_a + s * NP * kCbTM * kCbLd;
            __bf16* sb = s_b + s * NP * TN * kCbLd;
#pragma unroll
            for (int q = 0; q < kCbRowsA; q++) {
                cb_bf16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const float x = ra[s][q][e >> 2][e & 3];
                    hi[e] = (__bf16)x;
                    lo[e] = (__bf16)(x - (float)hi[e]);
                }
                *reinterpret_cast<cb_bf16x8*>(sa + (r0 + 64 * q) * kCbLd + 8 * g) = hi;
                if (SPLIT) *reinterpret_cast<cb_bf16x8*>(sa + (kCbTM + r0 + 64 * q) * kCbLd + 8 * g) = lo;
            }
#pragma unroll
            for (int q = 0; q < kRowsB; q++) {
                *reinterpret_cast<cb_u32x4*>(sb + (r0 + 64 * q) * kCbLd + 8 * g) = rb[s][0][q];
                if (SPLIT) *reinterpret_cast<cb_u32x4*>(sb + (TN + r0 + 64 * q) * kCbLd + 8 * g) = rb[s][NP - 1][q];
            }
        }
        __syncthreads();
        fetch_group();
#pragma unroll
        for (int s = 0; s < KC; s++) {
            if (j + s >= nchunks) break;
            const __bf16* qa = pa + s * NP * kCbTM * kCbLd;
            const __bf16* qb = pb + s * NP * TN * kCbLd;
#pragma unroll
            for (int ks = 0; ks < kCbK; ks += 16) {
                const cb_bf16x8 a0 = frag(qa + ks), a1 = frag(qa + 32 * kCbLd + ks);
                cb_bf16x8 l0 = a0, l1 = a1;
                if (SPLIT) { l0 = frag(qa + kCbTM * kCbLd + ks); l1 = frag(qa + (kCbTM + 32) * kCbLd + ks); }
#pragma unroll
                for (int v = 0; v < VT; v++) {
                    const cb_bf16x8 bh = frag(qb + 32 * v * kCbLd + ks);
                    if (SPLIT) {   // small terms first
                        const cb_bf16x8 bl = frag(qb + (TN + 32 * v) * kCbLd + ks);
                        acc[0][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l0, bh, acc[0][v], 0, 0, 0);
                        acc[1][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l1, bh, acc[1][v], 0, 0, 0);
                        acc[0][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bl, acc[0][v], 0, 0, 0);
                        acc[1][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bl, acc[1][v], 0, 0, 0);
                    }
                    acc[0][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bh, acc[0][v], 0, 0, 0);
                    acc[1][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bh, acc[1][v], 0, 0, 0);
                }
            }
        }
    }

    // the operands are done with: the rows' output and skip offsets take their place
    int* s_out = reinterpret_cast<int*>(s_a);
    int* s_res = s_out + kCbTM;
    __syncthreads();
    if (g == 0) {
#pragma unroll
        for (int q = 0; q < kCbRowsA; q++) { s_out[r0 + 64 * q] = oout[q]; s_res[r0 + 64 * q] = ores[q]; }
    }
    __syncthreads();

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
                const int o = s_out[row];
                if (o < 0) continue;
                float r = acc[u][v][e] + bias;
                const float sk = skip ? a.ep.res[(long)s_res[row] + n] : 0.f;
                if (!a.ep.res_after) r += sk;
                switch (a.ep.act) {
                    case ACT_RELU: r = r > 0.f ? r : 0.f; break;
                    case ACT_RELU6: r = r < 0.f ? 0.f : (r > 6.f ? 6.f : r); break;
                    case ACT_PRELU: r = r >= 0.f ? r : a.ep.alpha[n] * r; break;
                    default: break;
                }
                if (a.ep.res_after) r += sk;
                a.out[(long)o + n] = r;
            }
    }
}

constexpr long kCbMaxBytes = 0x7fffffffL;   // what a 32-bit byte offset (kept in an int) reaches

template <int TN>
hipError_t launch_tile(const ConvArgs& r, long grid, hipStream_t s) {
    return r.bf16 == 2 ? launch_kernel(conv_bf16_kernel<TN, true>, dim3((unsigned)grid), dim3(kCbThreads), 0, s, r)
                       : launch_kernel(conv_bf16_kernel<TN, false>, dim3((unsigned)grid), dim3(kCbThreads), 0, s, r);
}

}  // namespace

bool conv_bf16_supports(const ConvArgs& a) {
    if (a.bf16 != 1 && a.bf16 != 2) return false;
    if (!a.w_bf16 || (a.bf16 == 2 && !a.w_bf16_lo)) return false;
    ConvArgs shape = a;   // the shape rule is conv_mfma_kernel's, whatever option "conv_mfma" says
    shape.mfma = 1;
    return conv_mfma_supports(shape);
}

int launch_conv_bf16(const ConvArgs& a, void* stream) {
    if (!conv_bf16_supports(a)) return (int)hipErrorInvalidValue;
    // frames per launch: input, output and skip of the range within 2^31 bytes of their first frame
    const long in_frame = std::max((long)a.H * a.W * a.C, a.in_fs), out_frame = std::max((long)a.Ho * a.Wo * a.Co, a.out_fs);
    const long res_frame = a.ep.res_mode == RES_DIRECT ? std::max((long)a.Ho * a.Wo * a.ep.res_C, a.ep.res_fs) : 1;
    const long most = std::max(in_frame, std::max(out_frame, res_frame));
    const int per = (int)std::max(1L, std::min((long)a.B, kCbMaxBytes / 4 / most));
    const bool narrow = a.Co <= 64;
    for (int b0 = 0; b0 < a.B; b0 += per) {
        ConvArgs r = a;
        r.B = std::min(per, a.B - b0);
        r.in = a.in + (long)b0 * a.in_fs;
        r.out = a.out + (long)b0 * a.out_fs;
        if (a.ep.res) r.ep.res = a.ep.res + (long)b0 * a.ep.res_fs;
        const long tiles_m = ((long)r.B * r.Ho * r.Wo + kCbTM - 1) / kCbTM;
        // 128 x 64 tiles where Co is at most 64, and where 128 x 128 tiles would leave compute units without one
        const bool tn64 = narrow || tiles_m * ((r.Co + 127) / 128) < device_cu_count();
        const long grid = tiles_m * ((r.Co + (tn64 ? 63 : 127)) / (tn64 ? 64 : 128));
        if (grid > 0x7fffffffL) return (int)hipErrorInvalidValue;
        const hipError_t e = tn64 ? launch_tile<64>(r, grid, (hipStream_t)stream) : launch_tile<128>(r, grid, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

}  // namespace mi
