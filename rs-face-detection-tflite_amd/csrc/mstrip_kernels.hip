// mstrip_kernels.hip — fused BlazeBlocks for 32-pixel-wide layers with 48 channels (BackCamera's seven 32x32x48 blocks), the
// pointwise conv on the matrix cores, everything else in the matrix operand layout:
//
//   out = act( PW1x1( DW3x3(in) + b_dw ) + b_pw + in )
//
// Same operator chain as strip_kernels.hip / block_kernels.hip (DEPTHWISE_CONV_2D -> CONV_2D 1x1 -> ADD -> RELU behind
// `interpreter.invoke()`, /root/reference/src/face_detection_lite/face_detection.rs:235; graph: SURVEY.md Appendix A.1,
// "7 x Block(48->48, s1)").  Why not the strip kernel's way (lane = pixel, weights as SGPR operands of v_pk_fma_f32): measured in
// round 3 (tools/wide_bench.hip history, tools/valu_bench.hip) —
//   * a stage's weights (18 + 2 x 48 floats) exceed the SGPR file, so the output channels had to be split over two waves that
//     each repeat the depthwise stage; every wave then streams 6.3 KB of constants through the scalar cache per 64-pixel row
//     and parks ~170 cycles at each of its 48 waits per row (8 waves per CU: SQ_WAIT_ANY 59 %): 43 us per block, no faster
//     than the block kernel;
//   * v_pk_fma_f32 issues at 5.0 cycles per wave alone on a SIMD and 3.47 with two waves (104 / 116 TFLOP/s chip-wide), while
//     v_mfma_f32_16x16x4_f32 sustains its 32 cycles (142-145 TFLOP/s), and a second wave's packed FMAs overlap it almost
//     entirely (MFMA + 1 pk_fma per wave: 34.2 cycles per pair at two waves per SIMD, 46.4 at one).
// So here:
//   * one WAVE = one frame's 32-pixel rows, walking down a band of rows; 48 -> 48 on a 32-pixel row is M = 48 (3 tiles) x
//     N = 32 (2 tiles) x K = 48 (12 steps) of v_mfma_f32_16x16x4_f32 with NO padding: 72 MFMAs = 2304 cycles per row.
//   * the lane layout is the MFMA B-operand's from the start: lane (kq = lane / 16, p = lane % 16) owns channel 4 ks + kq of
//     pixels p and 16 + p for every k-step ks.  The depthwise 3x3 runs in that layout (vertical reuse in registers: the two
//     unfinished output rows an input row contributes to), so its result IS the B operand: no transposition anywhere.  Its taps
//     (9 x 12 values per lane) live in VGPRs for the whole kernel; packed FMAs pair the two pixel tiles.
//   * the pointwise weights are the A operands: 36 wave-wide registers' worth, read from LDS (one copy per workgroup, loaded
//     once), never streamed.  No scalar-cache traffic in the row loop at all.
//   * the result tile has 4 consecutive output channels of one pixel per lane: bias + skip (the centre row, read from the row
//     image as float4) + ReLU, then one global_store_dwordx4 per tile.
// Input rows arrive by LDS-DMA in wave-private images ([34 pixels][52 floats]: zero border columns, 13th float4 slot unused).
// Exact f32; results match the block kernel to reassociation of the sums and the folded depthwise bias.
// The row (mstrip_row) and the frame functions around it are mrow.hpp's; mstrip_walk below is the walk of one wave down its rows of
// one frame of one block, the same code for the per-block kernel and the chain kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "kernels.hpp"
#include "launch.hpp"
#include "mrow.hpp"

namespace mi {

namespace {

struct MstripArgs {
    const float* in;
    float* out;
    const float* consts;   // mstrip_pack_consts()
    long in_fs, out_fs;
    int B, H;              // W == 32
    int bands, band_rows;
    int has_res;
    float hi;              // upper clamp of the activation (6 for ReLU6, +inf otherwise)
    unsigned long long* stamps;  // diagnostic builds only (MI_MSTRIP_STAMPS): 8 accumulators per wave
};

// A run of such blocks in ONE launch (round 5): a workgroup of eight waves owns a frame, wave w its rows [4 w, 4 w + 4) (32 rows), and
// walks through the blocks with a workgroup barrier between them; block j + 1 reads what block j wrote to global memory (every
// intermediate tensor keeps its place in the arena; the halo rows come from the neighbouring waves' stores: same CU, same L1).
constexpr int kMstripChain = 8;
struct MstripChainArgs {
    const float* in[kMstripChain];
    float* out[kMstripChain];
    const float* consts[kMstripChain];
    long in_fs[kMstripChain], out_fs[kMstripChain];
    int has_res[kMstripChain];
    float hi[kMstripChain];
    int nblocks, B, H;
};

template <int CK>   // k-steps: C = 4 * CK channels in and out (CK % 4 == 0: whole 16-channel output tiles)
struct MK {
    static constexpr int C = 4 * CK, MT = C / 16;
    static constexpr int QP = CK + 1;          // float4 slots per pixel of the row image
    static constexpr int PS = 4 * QP;          // pixel stride (floats)
    static constexpr int IMG_F = 34 * PS;      // one row image
    static constexpr int DPX = 64 / QP;        // pixels one LDS-DMA instruction brings in
    static constexpr int NLD = 32 / DPX;       // LDS-DMA instructions per row
    static_assert(32 % DPX == 0 && NLD == 8, "eight DMA instructions per row (two source bases, four immediate offsets each)");
    static_assert((16 * PS) % 64 == 0 && 16 * PS / 64 < 256, "ds_read2st64_b32 reaches the second pixel tile");
    // constants blob (floats): A operands [CK][MT][64] | taps [CK][4][12] | bias [C] | slopes [C]
    static constexpr int OFF_A = 0, A_F = CK * MT * 64, OFF_TAP = A_F, TAP_F = CK * 48, OFF_BIAS = OFF_TAP + TAP_F, OFF_SLOPE = OFF_BIAS + C, TOTAL = OFF_SLOPE + C;
    static constexpr int WG_F = A_F + 2 * C + TAP_F;   // LDS floats shared by a workgroup: A operands, bias, slopes, taps (read once)
    static constexpr int NBUF = 2;
};

// in-kernel time stamps of the diagnostic build: seven accumulators per wave
#ifdef MI_MSTRIP_STAMPS
struct MstripStamps { unsigned long long acc[7] = {0, 0, 0, 0, 0, 0, 0}, prev = __builtin_amdgcn_s_memtime(); };
#define MI_MSTAMP(k) { __builtin_amdgcn_sched_barrier(0); unsigned long long t_ = __builtin_amdgcn_s_memtime(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); st.acc[k] += t_ - st.prev; st.prev = t_; __builtin_amdgcn_sched_barrier(0); }
#else
struct MstripStamps {};
#define MI_MSTAMP(k)
#endif

// LDS-DMA of input row r (clamped to the frame; mrow_dma2) of the frame at `in` into image bi of the wave's images at LDS address lds_img
template <int CK>
__device__ __forceinline__ void mstrip_issue_row(const float* in, const int r, const int H, const unsigned lds_img, const int bi, const int goff) {
    using K = MK<CK>;
    mrow_dma2<K::C, K::PS, K::DPX, K::DPX * K::QP>(reinterpret_cast<const char*>(in + (long)min(max(r, 0), H - 1) * 32 * K::C),
                                                   lds_img + (unsigned)((bi * K::IMG_F + K::PS) * 4), goff);
}

// One wave walks rows [y0, y1] of one frame of one block: in / out = the frame, wgc = the block's constants in LDS ([A_F] A operands, [C]
// bias, [C] slopes, taps), img = this wave's two row images (border columns clear).  On entry the DMA of rows y0 - 1 and y0 into
// images 0 and 1 is issued and at most the second is still in flight: the counted waits below assume that nothing else is outstanding.
// has_res (wave-uniform) keeps the type each kernel had it in, bool from the per-block kernel's argument and int from the chain's table:
// with the other type the compiler places one lgkmcnt wait of the row loop elsewhere.
template <int CK, bool RELU, class HR>
__device__ __forceinline__ void mstrip_walk(const float* in, float* out, const float* wgc, float* img, const unsigned lds_img, const int goff, const HR has_res,
                                            const float hi, const int H, const int y0, const int y1, const int lane, MstripStamps& st) {
    using K = MK<CK>;
    constexpr int C = K::C, MT = K::MT, PS = K::PS, QP = K::QP, IMG_F = K::IMG_F, NLD = K::NLD;
    const int kq = lane >> 4, p = lane & 15;
    // depthwise taps of this lane's channels: tap[ks][t] = w_dw[t][4 ks + kq], resident in registers for the whole block
    float tap[CK][9];
    mrow_load_taps9<CK>(reinterpret_cast<const float4*>(wgc + K::A_F + 2 * C) + kq * 3, tap);
    MI_MSTAMP(0)
    // ---- per-lane addresses
    typedef __attribute__((address_space(3))) float lfloat;
    const unsigned x_lds = (unsigned)(uintptr_t)(lfloat*)(img + p * PS + kq);   // B layout: left neighbour (image pixel p = x - 1 + 1) of pixel p, channel kq
    const unsigned a_lds = (unsigned)(uintptr_t)(lfloat*)const_cast<float*>(wgc + lane);   // A operands: [ks][mt][lane]
    const float* sme = img + (1 + p) * PS + 4 * kq;             // D layout: centre pixel p, channels 4 kq .. 4 kq + 3 of a 16-channel tile
    const unsigned ooff = (unsigned)(p * C + 4 * kq) * 4u;      // bytes: pixel p, channels 4 kq.. of tile (mt, nt) at + (16 nt * C + 16 mt) * 4

    float accA[CK][2], accB[CK][2];   // partial depthwise rows [k-step][pixel tile]: roles alternate from row to row
    df32x4 D[MT][2];
#pragma unroll
    for (int ks = 0; ks < CK; ks++) accA[ks][0] = accA[ks][1] = accB[ks][0] = accB[ks][1] = 0.f;

    // A step's vector-memory operations: the stores of its output row (2 MT, from the third step on), then the DMA of the row two steps
    // ahead (NLD, while the band has one): mrow_wait
    constexpr int NST = 2 * MT;
    auto step = [&](auto emit, int r, float (&aPN)[CK][2], float (&aC)[CK][2]) {
        const int t = r - (y0 - 1), bi = t & 1;   // t = step number
        mrow_wait<NST, NLD>(t - 1 >= 2, t == 0 || (t - 1) + 2 <= (y1 - y0 + 1));  // step 0: the prologue's second row is behind it
        if (r < 0 || r >= H) mrow_clear_row<32 * QP>(img + bi * IMG_F + PS, lane);  // wave-uniform
        wave_sync();
        MI_MSTAMP(1)
        // input row r: its ky = 2 / 1 / 0 taps go to the partial output rows r-1 / r / r+1 (aPN on entry / aC / aPN on exit)
        mstrip_row<CK, MT, PS, decltype(emit)::value>(x_lds + (unsigned)(bi * IMG_F * 4), a_lds, tap, aPN, aC, D);
        MI_MSTAMP(2)
        __builtin_amdgcn_sched_barrier(0);  // (fences: the old and the new accumulator tiles are never live together)
        if constexpr (decltype(emit)::value) mrow_store_row<RELU, C, 32>(D, (gchar*)(out + (long)(r - 1) * 32 * C), ooff, wgc + K::A_F + C + 4 * kq, hi, p);
        MI_MSTAMP(3)
        __builtin_amdgcn_sched_barrier(0);
        // output row r starts from bias + its skip, the centre pixels of input row r
        mrow_init_acc<C, PS>(D, wgc + K::A_F + 4 * kq, sme + bi * IMG_F, has_res != 0);
        __builtin_amdgcn_sched_barrier(0);
        wave_sync();   // every read of image bi is issued before the DMA below overwrites it
        __builtin_amdgcn_s_waitcnt(0xC07F);  // ... and has returned (LDS-DMA writes are not ordered behind this wave's earlier reads)
        if (r + 2 <= y1) mstrip_issue_row<CK>(in, r + 2, H, lds_img, bi, goff);
        MI_MSTAMP(4)
    };
    step(std::false_type{}, y0 - 1, accA, accB);
    step(std::false_type{}, y0, accB, accA);
    for (int r = y0 + 1; r <= y1; r += 2) {
        step(std::true_type{}, r, accA, accB);
        if (r + 1 > y1) break;
        step(std::true_type{}, r + 1, accB, accA);
    }
}

template <int CK, bool RELU>
__global__ __launch_bounds__(256, 2) void mstrip_kernel(MstripArgs a) {
    using K = MK<CK>;
    constexpr int C = K::C, PS = K::PS, QP = K::QP, IMG_F = K::IMG_F, NLD = K::NLD, NBUF = K::NBUF;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    MstripStamps st;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* wgc = lds;                                   // [A_F] A operands, [C] bias, [C] slopes
    float* img = lds + K::WG_F + wave * NBUF * IMG_F;   // this wave's row images
    // unit = (band, frame): the four waves of a workgroup take four consecutive frames of one band; bands of a frame are B
    // units = B / 4 workgroup ids apart (the same XCD when B % 32 == 0: their shared halo rows meet in one L2)
    const int unit = blockIdx.x * 4 + wave;
    const int band = unit / a.B, b = unit - band * a.B;
    const bool active = band < a.bands;  // whole wave; an idle wave still helps with the constants and meets the barrier
    const int y0 = band * a.band_rows, y1 = min(y0 + a.band_rows, a.H);
    const float* in = a.in + (long)b * a.in_fs;
    const int goff = mrow_goff<CK>(lane);
    const unsigned lds_img = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)img);
    mrow_clear_border<QP, NBUF, IMG_F, 33 * PS>(img, lane);

    // the first row is on its way while the constants below are fetched
    if (active) mstrip_issue_row<CK>(in, y0 - 1, a.H, lds_img, 0, goff);
    MI_MSTAMP(5)
    // ---- workgroup constants into LDS (the only workgroup-level synchronisation of the kernel)
    for (int i = threadIdx.x; i < K::A_F / 4; i += 256) reinterpret_cast<float4*>(wgc)[i] = reinterpret_cast<const float4*>(a.consts + K::OFF_A)[i];
    for (int i = threadIdx.x; i < 2 * C; i += 256) wgc[K::A_F + i] = a.consts[K::OFF_BIAS + i];
    for (int i = threadIdx.x; i < K::TAP_F / 4; i += 256) reinterpret_cast<float4*>(wgc + K::A_F + 2 * C)[i] = reinterpret_cast<const float4*>(a.consts + K::OFF_TAP)[i];
    // The second row goes out behind the constants, and only it may still be in flight when the row loop starts (vector-memory
    // operations retire in issue order): the compiler counts only its own loads when it places vmcnt waits — always safe, since a
    // counted wait also covers everything older — but the loop's own counted waits assume that nothing else is outstanding.
    if (active) mstrip_issue_row<CK>(in, y0, a.H, lds_img, 1, goff);
    if (active) wait_vm<NLD>(); else wait_vm<0>();
    MI_MSTAMP(6)
    // raw barrier behind an LDS-only wait: __syncthreads() would also drain vmcnt, i.e. wait for the second row
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (!active) return;
    mstrip_walk<CK, RELU>(in, a.out + (long)b * a.out_fs, wgc, img, lds_img, goff, a.has_res != 0, a.hi, a.H, y0, y1, lane, st);
#ifdef MI_MSTRIP_STAMPS
    if (a.stamps && lane == 0)
        for (int k = 0; k < 7; k++) a.stamps[(long)unit * 8 + k] = st.acc[k];
#endif
}

template <int CK, bool RELU>
__global__ __launch_bounds__(512, 2) void mstrip_chain_kernel(MstripChainArgs ca) {
    using K = MK<CK>;
    constexpr int C = K::C, PS = K::PS, QP = K::QP, IMG_F = K::IMG_F, NLD = K::NLD, NBUF = K::NBUF;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    MstripStamps st;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* img = lds + 2 * K::WG_F + wave * NBUF * IMG_F;   // this wave's row images (behind the two constant areas)
    const int b = blockIdx.x;                               // frame
    const int y0 = 4 * wave, y1 = y0 + 4;                   // this wave's rows (H == 32)
    const int goff = mrow_goff<CK>(lane);
    const unsigned lds_img = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)img);
    mrow_clear_border<QP, NBUF, IMG_F, 33 * PS>(img, lane);

    // constants of block 0 into the first area
    for (int i = threadIdx.x; i < K::A_F / 4; i += 512) reinterpret_cast<float4*>(lds)[i] = reinterpret_cast<const float4*>(ca.consts[0] + K::OFF_A)[i];
    for (int i = threadIdx.x; i < 2 * C; i += 512) lds[K::A_F + i] = ca.consts[0][K::OFF_BIAS + i];
    for (int i = threadIdx.x; i < K::TAP_F / 4; i += 512) reinterpret_cast<float4*>(lds + K::A_F + 2 * C)[i] = reinterpret_cast<const float4*>(ca.consts[0] + K::OFF_TAP)[i];
    for (int blk = 0; blk < ca.nblocks; blk++) {
        float* wgc = lds + (blk & 1) * K::WG_F;
        const float* in = ca.in[blk] + (long)b * ca.in_fs[blk];
        const int has_res = ca.has_res[blk];
        const float hi = ca.hi[blk];
        float* const outp = ca.out[blk] + (long)b * ca.out_fs[blk];
        mstrip_issue_row<CK>(in, y0 - 1, ca.H, lds_img, 0, goff);
        // the next block's constants: loads issued now (a few per thread), stored into the other area before this block's closing barrier
        constexpr int NPRE = (K::WG_F / 4 + 511) / 512;
        float4 pre[NPRE];
        const bool more = blk + 1 < ca.nblocks;
        if (more) {
            const float* cn = ca.consts[blk + 1];
#pragma unroll
            for (int k = 0; k < NPRE; k++) {
                const int i = threadIdx.x + 512 * k;   // area layout: [A_F | bias, slopes 2 C | taps]; blob: [A | taps | bias | slopes]
                const int src = i < K::A_F / 4 ? K::OFF_A + 4 * i : (i < (K::A_F + 2 * C) / 4 ? K::OFF_BIAS + 4 * i - K::A_F : K::OFF_TAP + 4 * i - K::A_F - 2 * C);
                pre[k] = i < K::WG_F / 4 ? *reinterpret_cast<const float4*>(cn + src) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        mstrip_issue_row<CK>(in, y0, ca.H, lds_img, 1, goff);
        wait_vm<NLD>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (blk == 0) {   // block 0's constants (plain stores above) are visible to every wave
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        mstrip_walk<CK, RELU>(in, outp, wgc, img, lds_img, goff, has_res, hi, ca.H, y0, y1, lane, st);
        // this wave's rows of the block are stored, the next block's constants go into the other area (free since the previous block's
        // closing barrier): then every wave of the frame moves on (vmcnt(0): the stores have left this wave; the waves of a workgroup
        // share the CU's L1, so the neighbours' loads see them)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (more) {
            float* nx = lds + ((blk + 1) & 1) * K::WG_F;
#pragma unroll
            for (int k = 0; k < NPRE; k++) {
                const int i = threadIdx.x + 512 * k;
                if (i < K::WG_F / 4) reinterpret_cast<float4*>(nx)[i] = pre[k];
            }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
}

}  // namespace

// Shapes the kernel takes: stride-1 depthwise 3x3 (SAME) + pointwise with C = Co = 48 on 32-pixel-wide frames, skip = the block's
// own input (or none), constants packed by mstrip_pack_consts().
bool mstrip_shape_ok(int C, int Co) {
    static const bool off = getenv("MI_NO_MSTRIP") != nullptr;  // tuning aid: fall back to the LDS-ring block kernel
    return !off && C == Co && C == 48;
}

bool mstrip_kernel_supports(const BlockArgs& a) {
    if (!a.w_strip || !a.has_dw || a.sh != 1 || a.sw != 1 || a.pt != 1 || a.pl != 1) return false;
    if (!mstrip_shape_ok(a.C, a.Co) || a.W != 32 || a.H != a.Ho || a.W != a.Wo || a.H < 2) return false;
    if (a.ep.res_mode != RES_NONE) {
        if (a.ep.res_after) return false;
        if (a.ep.res_mode != RES_DIRECT || a.ep.res != a.in || a.ep.res_fs != a.in_fs || a.ep.res_C != a.C) return false;
    }
    // a wave walks its band row by row (six dependent steps at four rows): below about one wave per SIMD over the chip the launch is
    // latency-bound and the block kernel's wider workgroups finish sooner (B = 5: 14.3 against 11 us)
    static const int min_b = getenv("MI_MSTRIP_MIN_B") ? atoi(getenv("MI_MSTRIP_MIN_B")) : 32;
    if (a.B < min_b) return false;
    return aligned16(a.in) && aligned16(a.out) && !(a.in_fs & 3) && !(a.out_fs & 3);
}

int mstrip_consts_floats(int C) { return C == 48 ? MK<12>::TOTAL : 0; }

// w_dw [3][3][C], b_dw [C] or null, w_pw [Co][C] (TFLite OHWI with H = W = 1), bias [Co] or null, alpha [Co] or null.
void mstrip_pack_consts(int C, const float* w_dw, const float* b_dw, const float* w_pw, const float* bias, const float* alpha, int act, float* dst) {
    using K = MK<12>;
    std::fill(dst, dst + mstrip_consts_floats(C), 0.f);
    mrow_pack_a(dst + K::OFF_A, w_pw, C / 4, K::MT, C);
    mrow_pack_taps(dst + K::OFF_TAP, w_dw, C / 4);
    mrow_pack_bias(dst + K::OFF_BIAS, dst + K::OFF_SLOPE, C, C, w_pw, b_dw, bias, alpha, act);
}

const char* mstrip_kernel_label(const BlockArgs& a, char* buf, size_t cap) {
    snprintf(buf, cap, "mstrip_kernel<%d,%d>", a.C / 4, a.ep.act == ACT_RELU ? 1 : 0);
    return buf;
}

// A run of blocks the single-block kernel takes, each reading its predecessor's output, on 32 x 32 frames: one launch (see MstripChainArgs)
bool mstrip_chain_supports(const BlockArgs* blocks, int n) {
    static const bool off = getenv("MI_NO_MSTRIP_CHAIN") != nullptr;  // tuning aid: one launch per block
    if (off || n < 2 || n > kMstripChain) return false;
    for (int k = 0; k < n; k++) {
        const BlockArgs& a = blocks[k];
        if (!mstrip_kernel_supports(a) || a.H != 32 || a.B != blocks[0].B || (a.ep.act == ACT_RELU) != (blocks[0].ep.act == ACT_RELU)) return false;
        if (k && a.in != blocks[k - 1].out) return false;
    }
    return true;
}

int launch_mstrip_chain(const BlockArgs* blocks, int n, void* stream) {
    using K = MK<12>;
    if (!mstrip_chain_supports(blocks, n)) return (int)hipErrorInvalidValue;
    MstripChainArgs ca{};
    ca.nblocks = n; ca.B = blocks[0].B; ca.H = blocks[0].H;
    for (int k = 0; k < n; k++) {
        const BlockArgs& a = blocks[k];
        ca.in[k] = a.in; ca.out[k] = a.out; ca.consts[k] = a.w_strip; ca.in_fs[k] = a.in_fs; ca.out_fs[k] = a.out_fs;
        ca.has_res[k] = a.ep.res_mode == RES_DIRECT;
        ca.hi[k] = a.ep.act == ACT_RELU6 ? 6.f : INFINITY;
    }
    const size_t lds_bytes = (size_t)(2 * K::WG_F + 8 * K::NBUF * K::IMG_F) * 4;
    return mrow_launch(mstrip_chain_kernel<12, true>, mstrip_chain_kernel<12, false>, blocks[0].ep.act == ACT_RELU, dim3((unsigned)ca.B), dim3(512), lds_bytes,
                       (hipStream_t)stream, ca);
}

unsigned long long* g_mstrip_stamps = nullptr;  // set by the development harness (MI_MSTRIP_STAMPS builds)

int launch_mstrip(const BlockArgs& a, void* stream) {
    using K = MK<12>;
    MstripArgs ma;
    ma.stamps = g_mstrip_stamps;
    ma.in = a.in; ma.out = a.out; ma.consts = a.w_strip; ma.in_fs = a.in_fs; ma.out_fs = a.out_fs;
    ma.B = a.B; ma.H = a.H;
    // bands: about eight waves per CU over the chip; a band costs two priming rows of depthwise work and two halo rows of input
    static const int forced = getenv("MI_MSTRIP_BAND") ? atoi(getenv("MI_MSTRIP_BAND")) : 0;  // tuning aid
    long bands = std::max<long>(1, (8L * device_cu_count() + a.B / 2) / std::max(1, a.B));
    int rows = (int)((a.H + bands - 1) / bands);
    rows = std::max(rows, std::min(a.H, 4));
    if (forced > 0) rows = std::min(forced, a.H);
    ma.band_rows = rows;
    ma.bands = (a.H + rows - 1) / rows;
    ma.has_res = a.ep.res_mode == RES_DIRECT;
    ma.hi = a.ep.act == ACT_RELU6 ? 6.f : INFINITY;
    const long units = (long)a.B * ma.bands;
    const size_t lds_bytes = (size_t)(K::WG_F + 4 * K::NBUF * K::IMG_F) * 4;
    return mrow_launch(mstrip_kernel<12, true>, mstrip_kernel<12, false>, a.ep.act == ACT_RELU, dim3((unsigned)((units + 3) / 4)), dim3(256), lds_bytes,
                       (hipStream_t)stream, ma);
}

}  // namespace mi
