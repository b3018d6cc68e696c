// stem_kernels.hip — the first convolution of every graph (the first CONV_2D behind `interpreter.invoke()`, face_detection.rs:235,
// face_landmark.rs:265, iris_landmark.rs:203), K x K stride 2 on the RGB picture, in its three forms:
//   stem_conv_kernel          packed VALU FMAs, the filter as scalar operands (every stem shape; f32 or 8UC3 pictures)
//   stem_mfma_kernel          the detectors' 5 x 5 -> 24 on the matrix cores, the window's picture rows kept in registers down a column of tiles
//   stem_mfma_rowwise_kernel  the same convolution, every tile loading its five rows (a handful of frames, or engine option "stem_mfma" = 2)
// All three give the same bits.  The two MFMA forms differ in their schedule alone: what a wave holds and does per picture row is
// StemWave, once.  launch_conv (kernels.hip) comes here through stem_applicable / stem_mfma_applicable / launch_stem_conv.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <algorithm>
#include <type_traits>
#include <utility>

#include "kernels.hpp"
#include "launch.hpp"
#include "mfma32.hpp"

namespace mi {

// ------------------------------------------------------------------------------------------------ stem convolution
// First layer of every graph: K x K, stride 2, 3 input channels (RGB) -> CO channels, + bias + ReLU/PReLU.
// (back/front 5x5 -> 24, full 3x3 -> 32, landmark 3x3 -> 16, iris 3x3 -> 64; SURVEY.md Appendix A.)
// One thread = one output pixel x all CO channels: the K*K*3 filter taps are wave-uniform, so the weights travel
// through the scalar cache into SGPR operands of v_fmac and every VALU lane does useful work; the input patch comes
// from an LDS tile (zero padded, TF SAME), staged with coalesced row-segment loads.  Output 16 B stores.
// U8: the input is 8UC3 frames (rows of u8_row_bytes bytes); a byte is normalised through a 256-entry table while the tile is filled.
// CS: the output channels are split over CS workgroups per tile (a single-image call, face_detection.rs:205, has 2 - 32 tiles for 256 CUs and
// a thread's K K 3 CO FMAs are one dependent chain of scalar-cache round trips: CO / CS channels per thread shorten it; the per-channel
// arithmetic is the same, so the results are bit-identical).
template <int K, int CO_ALL, bool U8 = false, int CS = 1, int PP = 2>
__global__ __launch_bounds__(256) void stem_conv_kernel(ConvArgs a) {
    constexpr int CO = CO_ALL / CS;
    static_assert(CO * CS == CO_ALL && CO % 4 == 0, "channel split");
    // PP output pixels per thread (rows ly and ly + 8): every scalar-loaded weight pair then feeds PP packed FMAs, which
    // halves the scalar-cache round trips per FMA (they, not the VALU, set the pace at one pixel per thread).  The channel-split form of a
    // single-image call takes PP = 1: twice the workgroups, half the chain.
    constexpr int TW = 32, TH = 8 * PP;                  // output tile
    constexpr int IW = 2 * TW + K - 2, IH = 2 * TH + K - 2;  // input tile (stride 2)
    constexpr int RS = (IW * 3 + 1) & ~1;                // row stride in floats (even: 8-byte aligned float2 reads)
    constexpr int LDSF = (IH * RS > 8 * TW * (CO + 4)) ? IH * RS : 8 * TW * (CO + 4);
    __shared__ __attribute__((aligned(16))) float tile[LDSF];
    const int tid = threadIdx.x;
    const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
    int t = blockIdx.x;
    const int cs0 = (t % CS) * CO; t /= CS;   // first output channel of this workgroup
    const int tx0 = (t % tiles_x) * TW; t /= tiles_x;
    const int ty0 = (t % tiles_y) * TH;
    const int b = t / tiles_y;
    const float* in = a.in + (long)b * a.in_fs;
    const int ix0 = tx0 * 2 - a.pl, iy0 = ty0 * 2 - a.pt;
    // All loads of the tile are issued before the first LDS write (a load -> wait -> write loop pays one HBM round trip per
    // iteration).  Thread e owns float e of every tile row (a row is IW * 3 <= 201 consecutive floats of the image): the column
    // arithmetic is done once per thread, a row costs an add and a select — the flat (index -> row, column) mapping this
    // replaces spent a third of the kernel's VALU instructions on divisions and bounds tests.  Loads are unconditional
    // (clamped address, value zeroed afterwards): a predicated load would put a branch around each of them.
    constexpr int ROWF = IW * 3;
    static_assert(ROWF <= 256, "one thread per float of a tile row");
    const int e_col = min(tid, ROWF - 1);
    const int ix = ix0 + e_col / 3;
    const bool x_ok = tid < ROWF && ix >= 0 && ix < a.W;
    float stage[IH];
    if constexpr (U8) {
        __shared__ float lut[256];
        lut[tid] = a.u8_lut[tid];
        const uint8_t* colb = a.in_u8 + (long)b * a.u8_frame_bytes + (long)min(max(ix, 0), a.W - 1) * 3 + (e_col - (e_col / 3) * 3);
        unsigned char raw[IH];
#pragma unroll
        for (int r = 0; r < IH; r++) raw[r] = colb[(long)min(max(iy0 + r, 0), a.H - 1) * a.u8_row_bytes];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < IH; r++) stage[r] = lut[raw[r]];
    } else {
        const float* colp = in + (long)min(max(ix, 0), a.W - 1) * 3 + (e_col - (e_col / 3) * 3);
#pragma unroll
        for (int r = 0; r < IH; r++) stage[r] = colp[(long)min(max(iy0 + r, 0), a.H - 1) * a.W * 3];   // iy0 + r is wave-uniform
    }
    if (tid < ROWF) {
#pragma unroll
        for (int r = 0; r < IH; r++) {
            const int iy = iy0 + r;
            tile[r * RS + tid] = (x_ok && iy >= 0 && iy < a.H) ? stage[r] : 0.f;
        }
    }
    __syncthreads();
    const int lx = tid & (TW - 1), ly = tid / TW;
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f acc2[PP][CO / 2];  // two output channels per v_pk_fma_f32 (the weight pair is an SGPR-pair operand)
#pragma unroll
    for (int p = 0; p < PP; p++)
#pragma unroll
        for (int o = 0; o < CO / 2; o++) acc2[p][o] = v2f{0.f, 0.f};
    const float* __restrict__ w = a.w + cs0;  // [K][K][3][Cop], uniform -> scalar loads
    const int Cop = (CO_ALL + 3) & ~3;
    // Not unrolled beyond 3 taps: the weights of a tap are 24..64 SGPRs; letting the compiler hoist all K*K*3 taps'
    // scalar loads would spill SGPRs into VGPR lanes.  Occupancy (<= 64 VGPRs) hides the scalar-load latency instead.
#pragma unroll 1
    for (int ky = 0; ky < K; ky++) {
        const float* row = tile + (2 * ly + ky) * RS + 2 * lx * 3;
        const float* wk = w + (long)(ky * K * 3) * Cop;
#pragma unroll 3
        for (int e = 0; e < K * 3; e++) {
            float xv[PP];
#pragma unroll
            for (int p = 0; p < PP; p++) xv[p] = row[p * 16 * RS + e];
            const float* we = wk + (long)e * Cop;
#pragma unroll
            for (int o = 0; o < CO / 2; o++)
#pragma unroll
                for (int p = 0; p < PP; p++) acc2[p][o] = __builtin_elementwise_fma(v2f{xv[p], xv[p]}, v2f{we[2 * o], we[2 * o + 1]}, acc2[p][o]);
        }
    }
    // Epilogue through LDS: a thread owns one pixel (CO floats), but 16-byte stores at a CO*4-byte lane stride reach
    // HBM as partial 32-byte sectors (measured 2.85x WRITE_SIZE).  Re-tile so that each wave-instruction writes
    // 1 KiB of consecutive addresses: the tile's rows are contiguous runs of TW*CO floats in the NHWC output.
    float* otile = tile;  // [8*TW][CO + 4] (pad keeps the float4 writes of consecutive pixels on distinct banks)
    constexpr int OS = CO + 4;
    // branch-free activation: act(v) = min(max(v,0) + slope * min(v,0), hi) with slope 0 (ReLU / ReLU6), alpha (PReLU) or 1
    // (none).  A switch per element costs a scalar load + wait + branches for each of the CO channels of every wave,
    // which took longer than the 900 packed FMAs of the 5x5 stem.
    const bool prelu = a.ep.act == ACT_PRELU;
    const float base_slope = a.ep.act == ACT_NONE ? 1.f : 0.f, hi = a.ep.act == ACT_RELU6 ? 6.f : INFINITY;
    const float* __restrict__ bias = a.ep.bias + cs0;
    const float* __restrict__ al = (prelu ? a.ep.alpha : a.ep.bias) + cs0;  // always a readable array: no branch around the loads
    constexpr int C4 = CO / 4;
    const bool relu = a.ep.act == ACT_RELU;  // wave-uniform: the three detector stems; one packed add + one packed max per channel pair
#pragma unroll
    for (int p = 0; p < PP; p++) {
        __syncthreads();  // all reads of the input tile (p = 0) / of the previous half's output image are done; reuse the LDS
        if (relu) {
#pragma unroll
            for (int o = 0; o < CO; o += 4) {
                const v2f r0 = __builtin_elementwise_max(acc2[p][o >> 1] + v2f{bias[o], bias[o + 1]}, v2f{0.f, 0.f});
                const v2f r1 = __builtin_elementwise_max(acc2[p][(o >> 1) + 1] + v2f{bias[o + 2], bias[o + 3]}, v2f{0.f, 0.f});
                *reinterpret_cast<float4*>(otile + tid * OS + o) = make_float4(r0.x, r0.y, r1.x, r1.y);
            }
        } else {
#pragma unroll
            for (int o = 0; o < CO; o += 4) {
                float r[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float acc = (e & 1) ? acc2[p][(o + e) >> 1].y : acc2[p][(o + e) >> 1].x;
                    const float v = acc + bias[o + e];
                    const float sl = prelu ? al[o + e] : base_slope;
                    r[e] = act1(v, sl, hi);
                }
                *reinterpret_cast<float4*>(otile + tid * OS + o) = make_float4(r[0], r[1], r[2], r[3]);
            }
        }
        __syncthreads();
        for (int i = tid; i < 8 * TW * C4; i += 256) {
            int px = i / C4, c4 = i - px * C4;
            int y = ty0 + 8 * p + px / TW, x = tx0 + (px & (TW - 1));
            if (y < a.Ho && x < a.Wo)
                *reinterpret_cast<float4*>(a.out + (long)b * a.out_fs + ((long)y * a.Wo + x) * CO_ALL + cs0 + 4 * c4) =
                    *reinterpret_cast<const float4*>(otile + px * OS + 4 * c4);
        }
    }
}

// ---- the 5 x 5 stem (BackCamera 256x256 -> 128x128x24, Short / Front 128x128 -> 64x64x24) on the matrix cores, round 6.
// stem_conv_kernel does its 1 800 FMAs per output pixel as packed VALU FMAs with the weights as scalar operands: 83 TFLOP/s at 256 frames, of the 104 - 116 the
// packed FMAs reach on this part (0.18 ms of BASELINE config 2's 1.30).  v_mfma_f32_4x4x1_16b_f32 is 16 independent (4 x 1)(1 x 4) outer products with
// D[i][lane] = A[block, i] * B[lane] + C[i][lane] (strip_kernels.hip uses it the same way): with lane = OUTPUT PIXEL, B = one value of the pixel's 5 x 5 x 3
// window and A = four output-channel weights W[4 t .. 4 t + 3][k], broadcast from one block of a weight register (cbsz = 4, abid = block), D = four output
// channels of 64 pixels.  The whole filter — 75 x 24 weights — is 29 registers of 64 lanes, loaded once per wave; a tile of 64 pixels is 75 x 6 = 450 MFMAs
// and nothing else but its loads: five rows of 15 consecutive floats per lane (the window's row: 3 x dwordx4 + dwordx3 buffer loads, the next row's
// in flight while this row's 90 MFMAs issue).  Rows above / below the picture are whole loads outside the buffer resource (zeros); the pixel left of
// column 0 and the two right of column W - 1 are handled in the two edge lanes, which load a window shifted into the picture and move the values
// over (every load is wholly inside or wholly outside the resource).  Each output is the same k-sequential f32 FMA chain from 0, bias added behind it,
// as in stem_conv_kernel: the results are bit-identical (tests/test_gpu_parity.py::test_mfma_stem_bit_equal_to_the_valu_stem).
// Measured (BackCamera, 256 frames; profiles/r06_stem_mfma.txt): 0.182 -> 0.165 ms (one frame: 8.9 -> 7.0 us).  What bounds it now is memory, not the matrix cores: without its MFMAs the
// kernel takes 0.140 ms (201 MB in + 403 MB out = 4.3 TB/s), without its stores 0.147, its 29.5 M MFMAs alone are 0.105 ms at the 8.2 cycles
// tools/probes/mfma4_probe.hip measures for this stream; the tensor it writes is read once more by the first row pipeline.
// This row-wise form (a wave takes consecutive tiles, every tile loads its five picture rows) is engine option "stem_mfma" = 2, and what = 1 launches where a column run
// would be a single row (a handful of frames); the default is the column-run form below it.
namespace {

typedef float sv4f __attribute__((ext_vector_type(4)));
typedef unsigned su4 __attribute__((ext_vector_type(4)));
typedef unsigned su3 __attribute__((ext_vector_type(3)));
__device__ __forceinline__ sv4f stem_mfma4(float a, float b, sv4f c, int blk) {   // (the builtin wants the block as a literal: the switch folds away once the loops are unrolled)
    switch (blk) {
#define MI_SM4(N) case N: return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, N, 0);
        MI_SM4(0) MI_SM4(1) MI_SM4(2) MI_SM4(3) MI_SM4(4) MI_SM4(5) MI_SM4(6) MI_SM4(7) MI_SM4(8) MI_SM4(9) MI_SM4(10) MI_SM4(11) MI_SM4(12) MI_SM4(13) MI_SM4(14)
#undef MI_SM4
        default: return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, 15, 0);
    }
}

template <int N, class F, int... KS>
__device__ __forceinline__ void dfor_tiles_impl(F&& f, std::integer_sequence<int, KS...>) { (f(std::integral_constant<int, KS>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void dfor_tiles(F&& f) { dfor_tiles_impl<N>(f, std::make_integer_sequence<int, N>{}); }

// ---- what the two MFMA forms share: everything but their schedule (which picture row goes into which buffer, and when).
constexpr int KW3 = 15, NK = 75, CQ = 6, NA = (NK * CQ + 15) / 16;   // floats of a window row, window values, channel quads, weight registers (29)

// Workgroup i runs on XCD i % 8, each with an L2 of its own: the workgroups of one XCD take CONSECUTIVE tiles (the rows of one stretch of a frame: a picture
// row is read by two or three output rows), not every eighth group of four — interleaved, an XCD fetched 7 picture rows per 2 output rows.
// Returns this wave's place in that order (wave-uniform); nwv: the waves of the launch.
__device__ __forceinline__ int stem_wave_index(int& nwv) {
    const int G = (int)gridDim.x, wg = (G & 7) ? (int)blockIdx.x : (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3);
    nwv = G * 4;
    return __builtin_amdgcn_readfirstlane(wg * 4 + (int)(threadIdx.x >> 6));
}

// The edge lanes of a row as loaded -> their windows: lane `left` (pixel 0) holds columns 0 .. 4, its window is (zero), 0 .. 3; lane `right` (pixel Wo - 1)
// holds columns W - 5 .. W - 1, its window is W - 3 .. W - 1, (zero), (zero).  has_left / has_right: the wave has such a lane (wave-uniform).
__device__ __forceinline__ void stem_fix_edges(float (&x)[KW3], bool left, bool right, bool has_left, bool has_right) {
    if (has_left) {
#pragma unroll
        for (int e = KW3 - 1; e >= 0; e--) x[e] = left ? (e >= 3 ? x[e - 3] : 0.f) : x[e];
    }
    if (has_right) {
#pragma unroll
        for (int e = 0; e < KW3; e++) x[e] = right ? (e < 9 ? x[e + 6] : 0.f) : x[e];
    }
}

// What a wave holds for the whole launch, and what it does with one picture row and with one finished tile of 64 pixels.
// Timing ablations (development only: -DMI_ABL_STEM_NOLOAD / _NOMFMA / _NOSTORE through build.sh's MI_EXTRA_FLAGS, for both forms; the ablated kernel
// computes wrong values, only its time counts; profiles/stem_rows.txt): no picture loads (the B operands are weight registers), one VALU add per window value
// instead of its six MFMAs, no global stores (a store the compiler cannot rule out, never taken).
template <bool RELU>
struct StemWave {
    int lane;
    float wa[NA];                           // the filter: register r, lanes 4 (n % 16) + i = W[4 t + i][k] for n = 16 r + ... = k CQ + t  (a.w: [k][24])
    float bs[24], sl[RELU ? 1 : 24], hi;    // bias, negative-side slopes, upper clamp
    float* ot;                              // this wave's 64 x 24 tile of the workgroup's LDS
#ifdef MI_ABL_STEM_NOSTORE
    bool nostore;
#endif
    __device__ __forceinline__ void init(const ConvArgs& a, float* otile) {
        lane = threadIdx.x & 63;
        ot = otile + (threadIdx.x >> 6) * (64 * 24);
#pragma unroll
        for (int r = 0; r < NA; r++) {
            const int n = 16 * r + (lane >> 2), k = n / CQ, t = n - CQ * k;
            wa[r] = n < NK * CQ ? a.w[k * 24 + 4 * t + (lane & 3)] : 0.f;
        }
        hi = a.ep.act == ACT_RELU6 ? 6.f : INFINITY;
        // bias and slopes: wave-uniform, read ONCE into scalar registers (read behind the row loop's stores they become vector loads the compiler orders behind
        // each store: six store round trips per tile)
        const float* __restrict__ bias = a.ep.bias;
#pragma unroll
        for (int i = 0; i < 24; i++) bs[i] = bias[i];
#ifdef MI_ABL_STEM_NOSTORE
        nostore = a.B >= 0;   // (always: a condition the compiler cannot fold)
#endif
    }
    // this lane's 15 floats at byte `vo` of the picture behind `rs`: four loads, each wholly inside or wholly outside the resource (outside: zeros)
    __device__ __forceinline__ void load_row(__amdgpu_buffer_rsrc_t rs, int vo, float (&x)[KW3]) const {
#ifdef MI_ABL_STEM_NOLOAD
#pragma unroll
        for (int e = 0; e < KW3; e++) x[e] = wa[e + (vo & 1)];
        return;
#endif
        const su4 q0 = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 0, 0), q1 = __builtin_amdgcn_raw_buffer_load_b128(rs, vo + 16, 0, 0),
                  q2 = __builtin_amdgcn_raw_buffer_load_b128(rs, vo + 32, 0, 0);
        const su3 q3 = __builtin_amdgcn_raw_buffer_load_b96(rs, vo + 48, 0, 0);
        x[0] = __uint_as_float(q0.x); x[1] = __uint_as_float(q0.y); x[2] = __uint_as_float(q0.z); x[3] = __uint_as_float(q0.w);
        x[4] = __uint_as_float(q1.x); x[5] = __uint_as_float(q1.y); x[6] = __uint_as_float(q1.z); x[7] = __uint_as_float(q1.w);
        x[8] = __uint_as_float(q2.x); x[9] = __uint_as_float(q2.y); x[10] = __uint_as_float(q2.z); x[11] = __uint_as_float(q2.w);
        x[12] = __uint_as_float(q3.x); x[13] = __uint_as_float(q3.y); x[14] = __uint_as_float(q3.z);
    }
    // window row ky: its 15 values into the six channel quads, 90 MFMAs, the k chain in the order (ky, e, q).  (ky is a literal once the caller's loop is unrolled,
    // as stem_mfma4's block is; as a template argument the callers' loops must be written out, and their row offsets then cost three s_mul_i32 more per tile)
    __device__ __forceinline__ void mfma_row(int ky, const float (&x)[KW3], sv4f (&D)[CQ]) const {
#ifdef MI_ABL_STEM_NOMFMA
#pragma unroll
        for (int e = 0; e < KW3; e++) D[e % CQ].x += x[e];
#else
#pragma unroll
        for (int e = 0; e < KW3; e++)
#pragma unroll
            for (int q = 0; q < CQ; q++) {
                const int n = (ky * KW3 + e) * CQ + q;
                D[q] = stem_mfma4(wa[n >> 4], x[e], D[q], n & 15);
            }
#endif
    }
    // The tile's 64 x 24 results, bias and activation behind the chain, to memory in two steps.  They are 6 KB of consecutive addresses, but a lane holds ONE
    // pixel's 96 bytes: stored from the registers, each of the six 16-byte store instructions touches every line of the tile (partial sectors at the memory side:
    // loads + stores alone took 0.22 ms).  Through LDS instead (to_lds, then to_memory): every store instruction writes 1 KB of consecutive addresses.
    __device__ __forceinline__ void to_lds(const sv4f (&D)[CQ]) const {
#pragma unroll
        for (int q = 0; q < CQ; q++) {
            float r[4] = {D[q].x, D[q].y, D[q].z, D[q].w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float v = r[i] + bs[4 * q + i];
                if constexpr (RELU) r[i] = fmaxf(v, 0.f);
                else r[i] = act1(v, sl[4 * q + i], hi);
            }
            *reinterpret_cast<float4*>(ot + lane * 24 + 4 * q) = make_float4(r[0], r[1], r[2], r[3]);
        }
        __builtin_amdgcn_wave_barrier();   // (the tile is this wave's own: LDS operations of a wave execute in order)
    }
    __device__ __forceinline__ void to_memory(float* op) const {   // op: the tile's first pixel
#ifdef MI_ABL_STEM_NOSTORE
        if (nostore) return;
#endif
#pragma unroll
        for (int q = 0; q < CQ; q++)
            *reinterpret_cast<float4*>(op + (q * 64 + lane) * 4) = *reinterpret_cast<const float4*>(ot + (q * 64 + lane) * 4);
        __builtin_amdgcn_wave_barrier();
    }
};

// The slopes of a wave `w` (no ReLU behind the convolution), behind w.init(a, ..).  Text of the kernel, not a function: filled inside one, the 24 conditional
// loads are paired and the row-wise form comes out with 12 registers more and another block order (profiles/stem_split_isa.txt).
#define MI_STEM_SLOPES(w, a)                                                                          \
    if constexpr (!RELU) {                                                                            \
        const float base_slope = a.ep.act == ACT_NONE ? 1.f : 0.f;                                    \
        const bool prelu = a.ep.act == ACT_PRELU;                                                     \
        const float* __restrict__ al = prelu ? a.ep.alpha : a.ep.bias; /* always a readable array */  \
        _Pragma("unroll") for (int i = 0; i < 24; i++) w.sl[i] = prelu ? al[i] : base_slope;          \
    }

}  // namespace

template <bool RELU>
__global__ __launch_bounds__(256) void stem_mfma_rowwise_kernel(ConvArgs a, int tiles, int tpr) {
    int nwv;
    const int wv = stem_wave_index(nwv);
    __shared__ __attribute__((aligned(16))) float otile[4 * 64 * 24];
    StemWave<RELU> w;
    w.init(a, otile);
    MI_STEM_SLOPES(w, a)
    const int rowb = a.W * 12;                                       // bytes of a picture row
    // A wave's row loads form one stream over its tiles — five rows per tile, the next row's loads issued before this row's 90 MFMAs, the NEXT TILE's first row
    // before this tile's last 90: without that every tile began with an exposed memory round trip that the other waves of the SIMD, in step with this
    // one, did not cover (0.220 ms with, 0.147 ms without the MFMAs, 0.105 ms of MFMAs).  NB buffers in turn, a row's loads issued NB - 1 rows ahead; five
    // rows per tile, so the buffers' roles rotate from tile to tile (P).
    struct Tile { int b, y, half, px, lane_off; bool left, right; };
    auto setup = [&](int t) {
        Tile c;
        c.b = t / (a.Ho * tpr);
        const int rem = t - c.b * (a.Ho * tpr);
        c.y = rem / tpr; c.half = rem - c.y * tpr;                   // wave-uniform
        c.px = 64 * c.half + w.lane;
        c.left = c.px == 0; c.right = c.px == a.Wo - 1;
        // the window of pixel px starts at column 2 px - 1: the edge lanes read columns 0 .. 4 / W - 5 .. W - 1 instead
        c.lane_off = (2 * c.px - 1 + (c.left ? 1 : 0) - (c.right ? 2 : 0)) * 12;
        return c;
    };
    auto load_row = [&](const Tile& c, int ky, float (&x)[KW3]) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + (long)c.b * a.in_fs), 0, a.H * rowb, 0x00020000);
        w.load_row(rs, (2 * c.y - 1 + ky) * rowb + c.lane_off, x);   // row -1: negative = far outside; rows >= H: outside
    };
    constexpr int NB = 2;   // (three buffers, loads two rows ahead: the same 0.165 ms)
    float xb[NB][KW3];
    auto tile = [&](auto pc, const Tile& c, const Tile& nx) {
        constexpr int P = decltype(pc)::value;
        sv4f D[CQ];
#pragma unroll
        for (int q = 0; q < CQ; q++) D[q] = sv4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 5; ky++) {
            if (ky + NB - 1 < 5) load_row(c, ky + NB - 1, xb[(ky + NB - 1 + P) % NB]);
            else load_row(nx, ky + NB - 1 - 5, xb[(ky + NB - 1 + P) % NB]);   // (the last tile loads its own first rows again: no branch around a load)
            float (&x)[KW3] = xb[(ky + P) % NB];
            stem_fix_edges(x, c.left, c.right, c.half == 0, c.half == tpr - 1);
            w.mfma_row(ky, x, D);
        }
        w.to_lds(D);
        w.to_memory(a.out + (long)c.b * a.out_fs + ((long)c.y * a.Wo + 64 * c.half) * 24);
    };
    if (wv >= tiles) return;
    Tile tl[2];
    tl[0] = setup(wv);
#pragma unroll
    for (int r = 0; r < NB - 1; r++) load_row(tl[0], r, xb[r]);
    // tile k of this wave starts at row 5 k of the stream: P = 5 k mod NB
    for (int t = wv;;) {
        bool done = false;
        dfor_tiles<NB>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if (done) return;
            const int tn = t + nwv;
            tl[(k + 1) & 1] = setup(min(tn, tiles - 1));
            tile(std::integral_constant<int, (5 * k) % NB>{}, tl[k & 1], tl[(k + 1) & 1]);
            if (tn >= tiles) done = true;
            t = tn;
        });
        if (done) break;
        if constexpr (NB & 1) { const Tile sw = tl[0]; tl[0] = tl[1]; tl[1] = sw; }   // (an odd number of tiles per round: the roles of tl[] swap)
    }
}

// ---- the same convolution with the window's picture rows kept in registers down a column of tiles (the default form; the row-wise one above is engine option
// "stem_mfma" = 2).  Row-wise, a tile loads the five picture rows of its window although the tile below shares three of them (stride 2): every picture value
// went through the vector-memory path 2.5 times vertically (and 2.5 times horizontally: a lane's 15 floats at a 6-float lane stride) — 1.26 GB of loads per
// launch for 201 MB of pictures.  Here a wave takes a RUN: R consecutive output rows y0 .. y0 + R - 1 of one 64-pixel column of one frame.  The window is five
// row buffers of 15 floats per lane; a step down loads only the two new picture rows, into the buffers of the two rows the step has just finished with (window
// row ky of step s lives in buffer (ky + 2 s) mod 5: the step loop is unrolled five times and the roles rotate, nothing is copied).  The two loads are issued
// behind the MFMAs of window rows 0 and 1 and are first used as rows 3 and 4 of the NEXT step: six to seven rows of 90 MFMAs between request and use.  A run
// starts with a full five-row load (3 rows more than it strictly needs: 35 row loads per 16 output rows against 80 row-wise); the step below the run's last
// loads two rows it never uses (inside the frame or, below it, outside the buffer resource: no branch around a load).  The edge lanes' shifted windows are
// repaired once per picture row — when the row is first used — instead of once per use.  Arithmetic, order of the k chain, epilogue and stores are those of the
// row-wise form: bit-identical results (tests/test_stem_rows_gpu.py).  75 + 29 + 24 registers of window, filter and accumulators: two workgroups per CU.
// Runs in the order (frame, run of rows, column) over the workgroups of an XCD, as the tiles above: neighbouring runs share their picture rows in that XCD's L2.
// Measured (profiles/stem_rows.txt; BackCamera, 256 frames): 0.156 -> 0.138 ms by rocprofv3, the step 1.194 -> 1.183 ms with two batches in flight, 1.267 -> 1.253 with one.  Not for the
// bytes it no longer loads (the row-wise form without ANY picture load is 2.6 % shorter): 8 instead of 20 load instructions per tile, requested far ahead.
template <bool RELU>
__global__ __launch_bounds__(256) void stem_mfma_kernel(ConvArgs a, int runs, int R) {
    constexpr int NR = 5;
    int nwv;
    const int wv = stem_wave_index(nwv);
    if (wv >= runs) return;
    __shared__ __attribute__((aligned(16))) float otile[4 * 64 * 24];
    StemWave<RELU> w;
    w.init(a, otile);
    MI_STEM_SLOPES(w, a)
    const int rowb = a.W * 12, tpr = a.Wo >> 6, rpf = ((a.Ho + R - 1) / R) * tpr;   // bytes of a picture row; tiles per row; runs per frame
    float xb[NR][KW3];
    for (int run = wv; run < runs; run += nwv) {
        const int b = run / rpf, rem = run - b * rpf, half = rem % tpr, y0 = (rem / tpr) * R, yend = min(y0 + R, a.Ho);   // wave-uniform
        const int px = 64 * half + w.lane;
        const bool left = px == 0, right = px == a.Wo - 1, has_left = half == 0, has_right = half == tpr - 1;
        // the window of pixel px starts at column 2 px - 1: the edge lanes read columns 0 .. 4 / W - 5 .. W - 1 instead
        const int lane_off = (2 * px - 1 + (left ? 1 : 0) - (right ? 2 : 0)) * 12;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + (long)b * a.in_fs), 0, a.H * rowb, 0x00020000);
        auto load_row = [&](int row, float (&x)[KW3]) {   // picture row `row`: -1 (a negative offset = far outside) and rows >= H read as zeros
            w.load_row(rs, (int)((unsigned)row * (unsigned)rowb + (unsigned)lane_off), x);
        };
#pragma unroll
        for (int ky = 0; ky < NR; ky++) load_row(2 * y0 - 1 + ky, xb[ky]);
#pragma unroll
        for (int ky = 0; ky < 3; ky++) stem_fix_edges(xb[ky], left, right, has_left, has_right);   // (rows 3 and 4 of every step are new: repaired there)
        float* op = a.out + (long)b * a.out_fs + ((long)y0 * a.Wo + 64 * half) * 24;
        for (int y = y0;;) {
            bool done = false;
            dfor_tiles<NR>([&](auto sc) {
                constexpr int S = decltype(sc)::value;
                if (done) return;
                sv4f D[CQ];
#pragma unroll
                for (int q = 0; q < CQ; q++) D[q] = sv4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ky = 0; ky < NR; ky++) {
                    float (&x)[KW3] = xb[(ky + 2 * S) % NR];
                    if (ky >= 3) stem_fix_edges(x, left, right, has_left, has_right);
                    w.mfma_row(ky, x, D);
                    if (ky < 2) load_row(2 * y + 4 + ky, x);   // window rows 3 and 4 of output row y + 1, into the buffer this row leaves
                }
                w.to_lds(D);
                w.to_memory(op);
                op += a.Wo * 24;
                if (++y >= yend) done = true;
            });
            if (done) break;
        }
    }
}
#undef MI_STEM_SLOPES

bool stem_mfma_applicable(const ConvArgs& a) {
    static const bool off = getenv("MI_NO_STEM_MFMA") != nullptr;   // tuning aid
    if (off || a.no_mfma == 1 || a.in_u8 || a.KH != 5 || a.KW != 5 || a.C != 3 || a.Co != 24 || a.Cop != 24 || a.sh != 2 || a.sw != 2 || a.pt != 1 || a.pl != 1) return false;
    if (a.W != 2 * a.Wo || a.H != 2 * a.Ho || a.Wo % 64 || a.W < 8 || !a.ep.bias || a.ep.res_mode != RES_NONE) return false;
    if ((reinterpret_cast<uintptr_t>(a.in) & 15) || (a.in_fs & 3) || (reinterpret_cast<uintptr_t>(a.out) & 15) || (a.out_fs & 3)) return false;
    if ((long)a.H * a.W * 12 > 0x7fffffffL) return false;
    return (long)a.B * a.Ho * (a.Wo / 64) >= 64;   // tiles of 64 pixels.  (One BackCamera frame = 256 tiles on 64 workgroups: 7.0 us against the split packed-FMA form's 8.9, 8.4 against 15.7 at four frames)
}

static int launch_stem_mfma(const ConvArgs& a, hipStream_t s) {
    const int tpr = a.Wo / 64, tiles = a.B * a.Ho * tpr;
    // The column-run form at two workgroups per CU (its waves hold the window: 162 registers with ReLU, 200 without).  Rows per run: what gives every wave of that grid one run,
    // a power of two up to 32 (BackCamera at 256 frames: 2 048 runs of 32 rows, Short / Front: 2 048 of 8) — or option "stem_run".  Below two rows per run the
    // row-wise split already fills the chip and a run would be one tile behind a five-row load: the row-wise form, as with option "stem_mfma" = 2.
    const int run_cu = 2;
    int R = a.stem_run;
    if (R <= 0 && a.no_mfma == 0)
        for (R = 1; R < 32 && (long)tiles >= 2L * R * 4 * run_cu * device_cu_count(); R *= 2) {}
    if (a.no_mfma == 0 && (R >= 2 || a.stem_run > 0)) {
        R = std::min(R, a.Ho);
        const int runs = a.B * ((a.Ho + R - 1) / R) * tpr;
        unsigned grid = (unsigned)std::min<long>((runs + 3) / 4, (long)run_cu * device_cu_count());
        if (grid >= 64) grid &= ~7u;   // (a multiple of the XCD count: the kernel's run order assumes it)
        if (a.ep.act == ACT_RELU) return (int)launch_kernel(stem_mfma_kernel<true>, dim3(grid), dim3(256), 0, s, a, runs, R);
        return (int)launch_kernel(stem_mfma_kernel<false>, dim3(grid), dim3(256), 0, s, a, runs, R);
    }
    const int per_cu = 4;   // workgroups of four waves (2 .. 6 per CU measured alike: 0.165 - 0.168 ms)
    unsigned grid = (unsigned)std::min<long>((tiles + 3) / 4, (long)per_cu * device_cu_count());
    if (grid >= 64) grid &= ~7u;   // (a multiple of the XCD count: the kernel's tile order assumes it)
    if (a.ep.act == ACT_RELU) return (int)launch_kernel(stem_mfma_rowwise_kernel<true>, dim3(grid), dim3(256), 0, s, a, tiles, tpr);
    return (int)launch_kernel(stem_mfma_rowwise_kernel<false>, dim3(grid), dim3(256), 0, s, a, tiles, tpr);
}

template <int K, int CO>
static int launch_stem(const ConvArgs& a, hipStream_t s) {
    constexpr int TH = 16;  // rows of a tile (two output pixels per thread)
    unsigned tiles = (unsigned)(((a.Wo + 31) / 32) * ((a.Ho + TH - 1) / TH));
    if (a.in_u8) return (int)launch_kernel(stem_conv_kernel<K, CO, true>, dim3(tiles * (unsigned)a.B), dim3(256), 0, s, a);
    // a handful of frames: 8 output channels per workgroup (16 of the iris network's 64), CS times the workgroups
    constexpr int CS = CO == 64 ? 4 : CO / 8;
    const unsigned tiles1 = (unsigned)(((a.Wo + 31) / 32) * ((a.Ho + 7) / 8));   // 8-row tiles: one output pixel per thread
    if (tiles1 * (unsigned)a.B * CS <= 256u) return (int)launch_kernel(stem_conv_kernel<K, CO, false, CS, 1>, dim3(tiles1 * (unsigned)a.B * CS), dim3(256), 0, s, a);
    if (tiles * (unsigned)a.B * CS <= 256u) return (int)launch_kernel(stem_conv_kernel<K, CO, false, CS>, dim3(tiles * (unsigned)a.B * CS), dim3(256), 0, s, a);
    return (int)launch_kernel(stem_conv_kernel<K, CO, false>, dim3(tiles * (unsigned)a.B), dim3(256), 0, s, a);
}

// true when (and how) the specialised stem kernel takes this convolution
bool stem_applicable(const ConvArgs& a) {
    if (a.C != 3 || a.sh != 2 || a.sw != 2 || a.KH != a.KW || !a.ep.bias || a.ep.res_mode != RES_NONE) return false;
    if ((reinterpret_cast<uintptr_t>(a.out) & 15) || (a.out_fs & 3)) return false;
    return (a.KH == 5 && a.Co == 24) || (a.KH == 3 && (a.Co == 16 || a.Co == 32 || a.Co == 64));
}

int launch_stem_conv(const ConvArgs& a, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (stem_mfma_applicable(a)) return launch_stem_mfma(a, st);
    if (a.KH == 5) return launch_stem<5, 24>(a, st);
    if (a.Co == 16) return launch_stem<3, 16>(a, st);
    if (a.Co == 32) return launch_stem<3, 32>(a, st);
    return launch_stem<3, 64>(a, st);
}

}  // namespace mi
