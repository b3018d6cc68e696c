// chain_kernels.hip — frame-resident chains of BlazeBlocks for the small-spatial, channel-heavy stages.
//
// At 16x16x96 (BackCamera, 7 consecutive blocks), 12x12x128 / 6x6x128 (face mesh) … a whole frame fits in the 160 KB LDS
// of a CU, while per-block launches are latency-bound (few pixels, 144 dependent MFMAs per 32-pixel group).  Here ONE
// 512-thread workgroup loads a frame into LDS once, runs every block of the chain on it
//     x <- act( PW1x1( DW3x3(x) + b_dw ) + b_pw + x )
// and writes the frame back once: the chain's intermediate activations never touch HBM (6 of 7 round trips removed for
// the 16x16 stage) and 7 launches become 1.  (Replaces the same TFLite op chains as block_kernels.hip; reference call
// site /root/reference/src/face_detection_lite/face_detection.rs:235.)
//
//   * each of the 8 waves owns one 32-pixel group of the frame for the whole chain (H*W <= 256);
//   * per block: depthwise 3x3 on the VALU in the MFMA B-operand layout (lane = pixel x k-half, see block_kernels.hip),
//     v_mfma_f32_32x32x2_f32 over all output-channel tiles, the MFMAs of channel chunk j interleaved with the depthwise
//     math of chunk j+1; pointwise weights stream from L2 in A-fragment order, one chunk ahead;
//     (the fixed-shape instantiations run the same arithmetic in phases instead — reads of chunk j+1 requested, the MFMAs of chunk j as one
//     block, one wait, the depthwise FMAs of chunk j+1 as one block: SCHED, contract_ph below);
//   * epilogue values stay in registers across a workgroup barrier (all reads of x done), then overwrite x in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "launch.hpp"
#include "mfma32.hpp"

namespace mi {

typedef float f32x2c __attribute__((ext_vector_type(2)));
typedef float f32x4c __attribute__((ext_vector_type(4)));

namespace {

struct ChainGeom {
    int Cp, Ch, C4, PS, RS, MT;
    int off_wdw, off_bdw, off_bias, off_alpha;  // LDS offsets (floats)
    int split;     // stride-1 blocks run as (32-pixel group, output tile) units, one per wave
    int pre_P, pre_RP, pre_GP, pre_PS, pre_RS;  // `pre`: passes, output rows per pass, 32-pixel groups per pass, staged pixel / row stride
    int off_t8;    // where `post`'s output is kept for the heads that read it ([pixels][post.Co + 4]); -1: not kept
    int lds_bytes;
    unsigned long long* stamps;  // diagnostic builds only (MI_CHAIN_STAMPS): 24 s_memtime stamps per workgroup
};
#ifdef MI_CHAIN_STAMPS
unsigned long long* g_chain_stamps = nullptr;
#define MI_CHAIN_STAMP(k) if (g.stamps && threadIdx.x == 0) MI_STAMP_AT(g.stamps[(long)blockIdx.x * 24 + (k)])
#else
#define MI_CHAIN_STAMP(k)
#endif

// `pre`'s staging: the fewest passes P whose input rows fit the LDS beside the constants (and `post`'s kept output) and whose 32-pixel
// groups all find a wave of their own; 0: none.  tile = floats of the resident frame's region, which the staging area shares.
constexpr int chain_pre_passes(int C, int H, int W, int Cin, int post_Co, int MT, bool split, long tile) {
    const int pre_RS = (2 * W + 1) * (Cin + 4);
    for (int P = 1; P <= 4; P++) {
        const int RP = (H + P - 1) / P, GP = (RP * W + 31) / 32;
        const long stage = (long)(2 * RP + 1) * pre_RS;
        const long rest = 9 * C + C + 8 * 32 + 64 + (post_Co ? (long)(H >> 1) * (W >> 1) * (post_Co + 4) : 0);
        if ((P - 1) * RP < H && P * GP * (split ? MT : 1) <= 8 && ((stage > tile ? stage : tile) + rest) * 4 <= kLdsBudget) return P;
    }
    return 0;
}

// Geometry policies of chain_kernel.  GeomRun: every size and stride is read from the arguments (any chain make_chain_geom accepts).
struct GeomRun {
    [[maybe_unused]] static constexpr bool fixed = false;
    static constexpr bool all_res = false;  // a stride-1 block's skip connection is looked up per block
    const ChainArgs& a;
    const ChainGeom& g;
    __device__ GeomRun(const ChainArgs& a_, const ChainGeom& g_) : a(a_), g(g_) {}
    __device__ int C() const { return a.C; }
    __device__ int H() const { return a.H; }
    __device__ int W() const { return a.W; }
    __device__ int pre_on() const { return a.pre.on; }
    __device__ int pre_Cin() const { return a.pre.Cin; }
    __device__ int post_on() const { return a.post.on; }
    __device__ int post_Co() const { return a.post.Co; }
#define MI_GEOM_FIELD(f) __device__ int f() const { return g.f; }
    MI_GEOM_FIELD(Cp) MI_GEOM_FIELD(Ch) MI_GEOM_FIELD(C4) MI_GEOM_FIELD(PS) MI_GEOM_FIELD(RS)
    MI_GEOM_FIELD(off_wdw) MI_GEOM_FIELD(off_bdw) MI_GEOM_FIELD(off_bias) MI_GEOM_FIELD(off_alpha)
    MI_GEOM_FIELD(pre_P) MI_GEOM_FIELD(pre_RP) MI_GEOM_FIELD(pre_GP) MI_GEOM_FIELD(pre_PS) MI_GEOM_FIELD(pre_RS)
#undef MI_GEOM_FIELD
};
// GeomFixed: one shape as constants (CIN / CO = 0: no `pre` / `post`), every stride-1 block with its skip connection (the skip of `pre` and of
// `post` stays a run-time flag: BackCamera's `post` has none, Front's has one).  Strides and LDS offsets are
// immediates: a depthwise tap is one base register plus an offset, the staging loops have constant trip counts, pixel coordinates come
// from shifts.  The formulas are make_chain_geom's; launch_chain takes this form only where every field equals what that computed.
template <int C_, int H_, int W_, int CIN, int CO>
struct GeomFixed {
    static constexpr bool fixed = true;
    static constexpr bool all_res = true;
    struct K {
        static constexpr int C = C_, H = H_, W = W_, Cp = C, Ch = C / 2, C4 = C / 4, PS = C + 4, RS = (W + 2) * PS, MT = (C + 31) / 32;
        static constexpr bool split = MT > 1 && ((H * W + 31) / 32) * MT <= 8;
        static constexpr int pre_on = CIN != 0, pre_Cin = CIN, post_on = CO != 0, post_Co = CO;
        static constexpr int tile = (H + 2) * RS;
        static constexpr int pre_PS = CIN + 4, pre_RS = (2 * W + 1) * pre_PS;
        static constexpr int pre_P = CIN ? chain_pre_passes(C, H, W, CIN, CO, MT, split, tile) : 0;
        static constexpr int pre_RP = CIN ? (H + pre_P - 1) / pre_P : 0, pre_GP = (pre_RP * W + 31) / 32;
        static constexpr int stage = CIN ? (2 * pre_RP + 1) * pre_RS : 0;
        static constexpr int off_wdw = stage > tile ? stage : tile, off_bdw = off_wdw + 9 * Cp, off_bias = (off_bdw + Cp + 3) & ~3;
        static constexpr int off_alpha = off_bias + MT * 32;
    };
    static_assert(!CIN || K::pre_P > 0, "no staging plan for `pre`");
    __device__ GeomFixed(const ChainArgs&, const ChainGeom&) {}
#define MI_GEOM_FIELD(f) static constexpr __device__ int f() { return K::f; }
    MI_GEOM_FIELD(C) MI_GEOM_FIELD(H) MI_GEOM_FIELD(W) MI_GEOM_FIELD(pre_on) MI_GEOM_FIELD(pre_Cin) MI_GEOM_FIELD(post_on) MI_GEOM_FIELD(post_Co)
    MI_GEOM_FIELD(Cp) MI_GEOM_FIELD(Ch) MI_GEOM_FIELD(C4) MI_GEOM_FIELD(PS) MI_GEOM_FIELD(RS)
    MI_GEOM_FIELD(off_wdw) MI_GEOM_FIELD(off_bdw) MI_GEOM_FIELD(off_bias) MI_GEOM_FIELD(off_alpha)
    MI_GEOM_FIELD(pre_P) MI_GEOM_FIELD(pre_RP) MI_GEOM_FIELD(pre_GP) MI_GEOM_FIELD(pre_PS) MI_GEOM_FIELD(pre_RS)
#undef MI_GEOM_FIELD
    static bool matches(const ChainArgs& a, const ChainGeom& g) {
        bool ok = a.C == K::C && a.H == K::H && a.W == K::W && g.Cp == K::Cp && g.Ch == K::Ch && g.C4 == K::C4 && g.PS == K::PS && g.RS == K::RS &&
                  g.MT == K::MT && (g.split != 0) == K::split && g.off_wdw == K::off_wdw && g.off_bdw == K::off_bdw && g.off_bias == K::off_bias &&
                  g.off_alpha == K::off_alpha && (a.pre.on != 0) == (CIN != 0) && (a.post.on != 0) == (CO != 0);
        if (ok && CIN) ok = a.pre.Cin == CIN && g.pre_P == K::pre_P && g.pre_RP == K::pre_RP && g.pre_GP == K::pre_GP && g.pre_PS == K::pre_PS && g.pre_RS == K::pre_RS;
        if (ok && CO) ok = a.post.Co == CO;
        for (int k = 0; ok && k < a.nblocks; k++) ok = a.blocks[k].has_res != 0;
        return ok;
    }
};
constexpr int kActRun = -1;  // chain_kernel's ACT: each block's activation is looked up per block

// ---- the phased contraction of the fixed shapes (chain_kernel's SCHED = 1).  One channel chunk's depthwise operands: the nine window quads, their
// nine weight quads and the bias quad.  They are requested by explicit ds_read (left to the compiler, every read is waited for and consumed where
// it lands, between the MFMAs: a wait for every second read), a whole block of MFMAs ahead of their use; then ONE wait, and the values pass
// through an empty asm statement behind it, so that their consumers depend on something ordered behind the wait (to the compiler the ds_read
// "returned" its value at once).  Every wait is lgkmcnt(0): scalar loads share the counter and return out of order.
struct DwTaps { f32x4c w[9], d[9], b; };
// byte strides in LDS: from tap to tap of the weights (the bias lies behind the ninth), from row to row and pixel to pixel of the window;
// BIAS_FIRST: the FMA chain starts from the bias (`pre`, `post`), or from zero with the bias added last (the stride-1 blocks) — the generic kernel's orders
template <int WS_, int RSB_, int PSB_, bool BIAS_FIRST_>
struct DwForm { static constexpr int WS = WS_, RSB = RSB_, PSB = PSB_; static constexpr bool bias_first = BIAS_FIRST_; };
template <int OFF>
__device__ __forceinline__ void lds_request(unsigned addr, f32x4c& v) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF)); }
template <class F, int... K>
__device__ __forceinline__ void dw_request(unsigned wa, unsigned ta, DwTaps& t, std::integer_sequence<int, K...>) {
    static_assert(9 * F::WS + 16 * 16 < 65536 && 2 * F::RSB + 2 * F::PSB + 16 * 16 < 65536, "ds_read offsets are 16 bits");
    ((lds_request<K * F::WS>(wa, t.w[K]), lds_request<(K / 3) * F::RSB + (K % 3) * F::PSB>(ta, t.d[K])), ...);
    lds_request<9 * F::WS>(wa, t.b);
}
template <class F>
__device__ __forceinline__ void dw_request(unsigned wa, unsigned ta, DwTaps& t) { dw_request<F>(wa, ta, t, std::make_integer_sequence<int, 9>{}); }
__device__ __forceinline__ void dw_landed(DwTaps& t) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < 9; k++) asm volatile("" : "+v"(t.w[k]), "+v"(t.d[k]));
    asm volatile("" : "+v"(t.b));
}
// the chunk's 36 FMAs and 4 adds as 18 + 2 packed instructions over channel pairs, every chain in the generic kernel's order
template <bool BIAS_FIRST>
__device__ __forceinline__ void dw_fma(const DwTaps& t, float4& bf) {
    f32x2c lo = {0.f, 0.f}, up = {0.f, 0.f};
    if constexpr (BIAS_FIRST) { lo = f32x2c{t.b.x, t.b.y}; up = f32x2c{t.b.z, t.b.w}; }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        lo = __builtin_elementwise_fma(f32x2c{t.d[k].x, t.d[k].y}, f32x2c{t.w[k].x, t.w[k].y}, lo);
        up = __builtin_elementwise_fma(f32x2c{t.d[k].z, t.d[k].w}, f32x2c{t.w[k].z, t.w[k].w}, up);
    }
    if constexpr (!BIAS_FIRST) { lo += f32x2c{t.b.x, t.b.y}; up += f32x2c{t.b.z, t.b.w}; }
    asm volatile("" : "+v"(lo), "+v"(up));  // the chunk's arithmetic ends here, in front of the fence that opens the MFMA block
    bf = make_float4(lo.x, lo.y, up.x, up.y);
}

// SPLIT: frames of so few 32-pixel groups that every stage runs as (group, output tile) units, one per wave (g.split)
// GP: geometry policy (above).  ACT: kActRun, or the one activation of every block, `pre` and `post` included (ACT_RELU: a lean epilogue).
// SCHED (fixed shapes): 1 = the contractions of `pre`, the blocks and `post` run in phases (contract_ph / contract1_ph), 0 = interleaved (contract / contract1).
template <int MT, bool SPLIT, class GP = GeomRun, int ACT = kActRun, int SCHED = 0>
__global__ __launch_bounds__(512, 2) void chain_kernel(ChainArgs a, ChainGeom g) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const GP geo(a, g);
    float* tile = lds;  // [(H+2)][(W+2)][PS], zero border
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pl = lane & 31, h = lane >> 5;
    const int b = blockIdx.x;
    const float* in = a.in + (long)b * a.in_fs;
    const int rowf4 = geo.W() * geo.C4();
    const int nch = geo.Ch() >> 2;

    // small per-block constants -> LDS (depthwise taps [9][Cs] zero-padded to Cp, depthwise bias, pointwise bias, negative slopes).
    // fetch_consts issues the global loads of a stage's constants into registers BEFORE the previous stage computes; commit_consts
    // writes them to LDS after the barrier that ends that stage: the L2 round trip hides under the stage's MFMAs.
    struct ConstRegs { float w[3], bdw, bias, alpha; };
    auto fetch_consts = [&](const ChainBlock& cb, int Cs, int Cos, ConstRegs& r) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = tid + 512 * k, c = i % geo.Cp();
            r.w[k] = (i < 9 * geo.Cp() && c < Cs) ? cb.w_dw[(i / geo.Cp()) * Cs + c] : 0.f;
        }
        r.bdw = (tid < Cs && cb.b_dw) ? cb.b_dw[tid] : 0.f;
        r.bias = (tid < Cos && cb.bias) ? cb.bias[tid] : 0.f;
        if constexpr (ACT == kActRun) r.alpha = (tid < Cos && cb.act == ACT_PRELU) ? cb.alpha[tid] : (cb.act == ACT_NONE ? 1.f : 0.f);
    };
    auto commit_consts = [&](const ConstRegs& r) {
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (tid + 512 * k < 9 * geo.Cp()) lds[geo.off_wdw() + tid + 512 * k] = r.w[k];
        if (tid < geo.Cp()) lds[geo.off_bdw() + tid] = r.bdw;
        if (tid < MT * 32) {
            lds[geo.off_bias() + tid] = r.bias;
            if constexpr (ACT == kActRun) lds[geo.off_alpha() + tid] = r.alpha;
        }
    };
    // pointwise weights, packed [tile][chunk][lane][4] in global memory (L2)
    unsigned aoff[MT];  // fixed shapes: this lane's offset into chunk 0 of tile m (floats), kept as registers of their own
#pragma unroll
    for (int m = 0; m < MT; m++) {
        aoff[m] = (unsigned)((m * nch * 64 + lane) * 4);
        if constexpr (GP::fixed) asm volatile("" : "+v"(aoff[m]));
    }
    auto a_frag = [&](const ChainBlock& cb, int nchk, int j, float4 (&av)[MT]) {
#ifdef MI_ABL_CHAIN_NOA  // timing ablation (development only): no weight loads inside the contraction
#pragma unroll
        for (int m = 0; m < MT; m++) { av[m] = make_float4(1.f, 2.f, 3.f, 4.f); asm volatile("" : "+v"(av[m].x), "+v"(av[m].y), "+v"(av[m].z), "+v"(av[m].w)); }
#else
        if constexpr (GP::fixed) {  // a wave-uniform address stepped on the scalar unit plus this lane's loop-invariant 32-bit offsets
            if (nchk == nch) {
#pragma unroll
                for (int m = 0; m < MT; m++) av[m] = ld4(cb.w_pw + (long)j * 256 + (size_t)aoff[m]);
                return;
            }
        }
#pragma unroll
        for (int m = 0; m < MT; m++) av[m] = ld4(cb.w_pw + (((long)m * nchk + j) * 64 + lane) * 4);
#endif
    };
    // first: the contraction's first chunk, whose first MFMA takes a zero C operand (the accumulators are never cleared by moves).
    // The MFMA quads of this file (here, contract1, contract1_ph) stay written out for that first MFMA: fixed-shape code, not mfma32_quad.
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto mfma_chunk = [&](const float4 (&av)[MT], const float4& bf, auto& D, auto first) {
#ifdef MI_ABL_CHAIN_NOMFMA  // timing ablation: one VALU op per chunk and tile instead of the four MFMAs
#pragma unroll
        for (int m = 0; m < MT; m++) D[m][0] = (decltype(first)::value ? 0.f : D[m][0]) + (av[m].x * bf.x + av[m].y * bf.y + av[m].z * bf.z + av[m].w * bf.w);
        return;
#endif
#pragma unroll
        for (int m = 0; m < MT; m++) {
            if constexpr (decltype(first)::value) D[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m].x, bf.x, zero16, 0, 0, 0);
            else D[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m].x, bf.x, D[m], 0, 0, 0);
            D[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m].y, bf.y, D[m], 0, 0, 0);
            D[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m].z, bf.z, D[m], 0, 0, 0);
            D[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m].w, bf.w, D[m], 0, 0, 0);
        }
    };
    // One 32-pixel group on this wave: depthwise chunk j (4 channels of this lane's k-half) by `dw`, the MFMAs of chunk j
    // interleaved with the depthwise math of chunk j + 1, pointwise weights streamed from L2 one chunk ahead.
    auto contract = [&](const ChainBlock& cb, int nchk, auto&& dw, auto& D) {
        // the accumulators start from a zero C operand of the first chunk's MFMAs where that chunk is peeled off the loop (the fixed
        // shapes: nchk is a constant > 1); the generic kernel clears them, which costs it no second copy of the loop body
        constexpr bool kPeel = GP::fixed;
        if constexpr (!kPeel) {
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int e = 0; e < 16; e++) D[m][e] = 0.f;
        }
        float4 bf, av[MT];
        dw(0, bf);
        a_frag(cb, nchk, 0, av);
        auto step = [&](int j, auto first) {
            float4 bn, an[MT];
            mfma_chunk(av, bf, D, first);
            a_frag(cb, nchk, j + 1, an);
            dw(j + 1, bn);
            bf = bn;
#pragma unroll
            for (int m = 0; m < MT; m++) av[m] = an[m];
            constexpr int NM = 4 * MT;
#pragma unroll
            for (int k = 0; k < NM; k++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                  // MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, (19 + NM - 1) / NM, 0);  // DS read
                __builtin_amdgcn_sched_group_barrier(0x002, (20 + NM - 1) / NM, 0);  // VALU
            }
        };
        if constexpr (kPeel) step(0, std::true_type{});
        for (int j = kPeel ? 1 : 0; j + 1 < nchk; j++) step(j, std::false_type{});
        mfma_chunk(av, bf, D, std::false_type{});
    };
    // ONE output tile (mt) of a 32-pixel group: the unit of work when a stage has so few pixels that whole groups would leave
    // waves idle (the 8x8 / 6x6 frames, the stride-2 block behind the chain, the output heads).  A unit is only 4 nchk dependent
    // MFMAs, too short to hide an L2 round trip per chunk behind the previous chunk: every weight chunk is in flight up front.
    constexpr int NJ = MT * 4;  // K <= 32 MT  ->  nchk <= 4 MT
    auto contract1 = [&](const float* w_pw, int nchk, int mt, auto&& dw, f32x16& D1) {
        const float* wa = w_pw + ((long)mt * nchk * 64 + lane) * 4;
        float4 aw[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++)
            if (j < nchk) aw[j] = ld4(wa + 256 * j);
        if constexpr (!GP::fixed) {
#pragma unroll
            for (int e = 0; e < 16; e++) D1[e] = 0.f;
        }
        float4 bf;
        dw(0, bf);
#pragma unroll
        for (int j = 0; j < NJ; j++)
            if (j < nchk) {
                float4 bn = bf;
                // the chunk number reaches `dw` through an opaque scalar: with a literal, every tap address of every chunk is
                // loop-invariant and gets hoisted out of the unit loop into a VGPR of its own (spills)
                int jn = j + 1;
                asm volatile("" : "+s"(jn));
                if (j + 1 < nchk) dw(jn, bn);
                if (GP::fixed && j == 0) D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].x, bf.x, zero16, 0, 0, 0);  // (chunk 0 always runs: nchk >= 1)
                else D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].x, bf.x, D1, 0, 0, 0);
                D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].y, bf.y, D1, 0, 0, 0);
                D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].z, bf.z, D1, 0, 0, 0);
                D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].w, bf.w, D1, 0, 0, 0);
                bf = bn;
                __builtin_amdgcn_sched_barrier(0);  // keeps the scheduler from hoisting every chunk's LDS reads to the top (spills)
            }
    };
    // ---- SCHED = 1: the same contractions in phases.  Chunk j: request chunk j + 1's depthwise operands (LDS) and weight fragments (L2) | the 4 MT
    // MFMAs of chunk j as one block, which covers those reads | one wait | chunk j + 1's depthwise FMAs as one block of packed instructions.  The
    // operands of chunk j are dead when those of chunk j + 1 are requested, so one register set serves; the two waves of a SIMD cover each other's
    // phases.  Switching between FMAs and MFMAs costs issue cycles, and packed FMAs the compiler places behind an MFMA are split in two.
    // Every FMA chain and every accumulator's k order are those of contract / contract1: bit-identical.
    [[maybe_unused]] auto lds_addr = [](const float* p) { return (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)const_cast<float*>(p); };
    // wa / ta: LDS byte addresses of chunk 0's first weight quad and first window quad of this lane; a chunk is 16 bytes further in both
    [[maybe_unused]] auto contract_ph = [&](auto form, auto nchk_c, const ChainBlock& cb, unsigned wa, unsigned ta, auto& D) {
        using F = decltype(form);
        constexpr int NCH = decltype(nchk_c)::value;
        static_assert(NCH >= 4 && NCH % 2 == 0, "chunks are taken in pairs: the weight fragments alternate between two register sets");
        DwTaps t;
        float4 bf, av[2][MT];
        a_frag(cb, NCH, 0, av[0]);
        dw_request<F>(wa, ta, t);
        dw_landed(t);
        dw_fma<F::bias_first>(t, bf);
        auto step = [&](int j, const float4 (&ac)[MT], float4 (&an)[MT], auto first, auto last) {
            if constexpr (!decltype(last)::value) {
                a_frag(cb, NCH, j + 1, an);
                dw_request<F>(wa + 16u * (unsigned)(j + 1), ta + 16u * (unsigned)(j + 1), t);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_chunk(ac, bf, D, first);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (!decltype(last)::value) {
                // (the accumulators pass through an empty asm statement: the compiler splits every packed f32 instruction it finds within an
                // MFMA's latency behind that MFMA in two, unless something in between depends on the MFMA's result)
#pragma unroll
                for (int m = 0; m < MT; m++) asm volatile("" : "+v"(D[m]));
                dw_landed(t);
                dw_fma<F::bias_first>(t, bf);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        step(0, av[0], av[1], std::true_type{}, std::false_type{});
        for (int j = 1; j + 2 < NCH; j += 2) {
            step(j, av[1], av[0], std::false_type{}, std::false_type{});
            step(j + 1, av[0], av[1], std::false_type{}, std::false_type{});
        }
        step(NCH - 1, av[1], av[1], std::false_type{}, std::true_type{});
    };
    // one output tile of a group (contract1's unit): every weight fragment in flight up front, the chunks unrolled
    [[maybe_unused]] auto contract1_ph = [&](auto form, auto nchk_c, const float* w_pw, int mt, unsigned wa, unsigned ta, f32x16& D1) {
        using F = decltype(form);
        constexpr int NCH = decltype(nchk_c)::value;
        const float* wag = w_pw + ((long)mt * NCH * 64 + lane) * 4;
        float4 aw[NCH];
#pragma unroll
        for (int j = 0; j < NCH; j++) aw[j] = ld4(wag + 256 * j);
        DwTaps t;
        float4 bf;
        dw_request<F>(wa, ta, t);
        dw_landed(t);
        dw_fma<F::bias_first>(t, bf);
#pragma unroll
        for (int j = 0; j < NCH; j++) {
            if (j + 1 < NCH) {
                unsigned jn = 16u * (unsigned)(j + 1);  // opaque, as in contract1: a literal makes every chunk's address a register of its own
                asm volatile("" : "+s"(jn));
                dw_request<F>(wa + jn, ta + jn, t);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (j == 0) D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].x, bf.x, zero16, 0, 0, 0);
            else D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].x, bf.x, D1, 0, 0, 0);
            D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].y, bf.y, D1, 0, 0, 0);
            D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].z, bf.z, D1, 0, 0, 0);
            D1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[j].w, bf.w, D1, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (j + 1 < NCH) {
                asm volatile("" : "+v"(D1));  // (as in contract_ph: keeps the packed FMAs behind the MFMAs packed)
                dw_landed(t);
                dw_fma<F::bias_first>(t, bf);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // bias (+ skip) + activation of the 4 channels ch .. ch + 3 (register quad gq) of this lane, in place
    auto finish1 = [&](f32x16& D1, int ch, int gq, const float4& skip, float hi) {
        if constexpr (ACT == ACT_RELU) {
            // the same two adds in the same order, packed, then one max: for finite values the bits of the general form with a slope
            // of 0 and no upper bound (where v < 0 that one gives 0 + (-0) = +0)
            const f32x2c* bb = reinterpret_cast<const f32x2c*>(lds + geo.off_bias() + ch);
            const f32x2c v0 = (f32x2c{D1[4 * gq], D1[4 * gq + 1]} + bb[0]) + f32x2c{skip.x, skip.y};
            const f32x2c v1 = (f32x2c{D1[4 * gq + 2], D1[4 * gq + 3]} + bb[1]) + f32x2c{skip.z, skip.w};
            D1[4 * gq] = fmaxf(v0.x, 0.f);
            D1[4 * gq + 1] = fmaxf(v0.y, 0.f);
            D1[4 * gq + 2] = fmaxf(v1.x, 0.f);
            D1[4 * gq + 3] = fmaxf(v1.y, 0.f);
            return;
        }
        const float4 bb = ld4(lds + geo.off_bias() + ch), al = ld4(lds + geo.off_alpha() + ch);
        const float4 v = bias_skip_act4(quad4(D1, gq), bb, skip, al, hi);
        D1[4 * gq] = v.x; D1[4 * gq + 1] = v.y; D1[4 * gq + 2] = v.z; D1[4 * gq + 3] = v.w;
    };
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // this wave's pixel group in the stride-1 blocks; g.split: frames of so few groups that (group, output tile) units fit the 8 waves
    const int ngrp = (geo.H() * geo.W() + 31) >> 5;
    const int grp_w = SPLIT ? wave % ngrp : wave, mt_w = SPLIT ? wave / ngrp : 0;
    const int q = grp_w * 32 + pl;
    const bool valid = q < geo.H() * geo.W();
    const int oy = valid ? q / geo.W() : 0, ox = valid ? q - (q / geo.W()) * geo.W() : 0;
    const bool wave_active = SPLIT ? wave < ngrp * MT : wave * 32 < geo.H() * geo.W();
    const int base0 = oy * geo.RS() + ox * geo.PS() + h * geo.Ch();  // tap (ky, kx) = base0 + ky*RS + kx*PS (input row oy-1+ky at slot oy+ky)
    float* centre = tile + (oy + 1) * geo.RS() + (ox + 1) * geo.PS();

    MI_CHAIN_STAMP(0)
    ConstRegs cr;
    if (geo.pre_on()) {
        // ---- the stride-2 block in front of the chain: its (2H x 2W x Cin) input is staged through the (still empty) tile region in
        // geo.pre_P() passes of geo.pre_RP() output rows — coalesced loads, every byte read once — and its 3x3 stride-2 taps and 2x2 max-pool
        // skip are gathered from LDS.  (Gathering them from global memory, 16 bytes per lane and tap, cost one cache-line lookup per
        // lane: 60 us of a 110 us launch.)  Pass p runs on waves [p GP, (p + 1) GP): a wave computes in at most one pass and keeps its
        // result in registers until the staged input is dead; then the tile is cleared and the results become the resident frame.
        const ChainBlock& cb = a.pre.blk;
        const int Cin = geo.pre_Cin(), Chp = Cin >> 1, Hi = 2 * geo.H(), Wi = 2 * geo.W(), C4i = Cin >> 2;
        const int PSi = geo.pre_PS(), RSi = geo.pre_RS(), rowf4i = Wi * C4i;
        const float* src = a.pre.in + (long)b * a.pre.in_fs;
        fetch_consts(cb, Cin, geo.C(), cr);
        commit_consts(cr);
        fetch_consts(a.blocks[0], geo.C(), geo.C(), cr);  // block 0's constants travel while this stage runs
        const float* wdw = lds + geo.off_wdw();
        const float* bdw = lds + geo.off_bdw();
        f32x16 D[SPLIT ? 1 : MT];
        bool mine = false;
        float* my_centre = tile;
        int my_mt = 0;
        const int UP = SPLIT ? geo.pre_GP() * MT : geo.pre_GP();  // units (SPLIT) or whole groups per pass
        for (int p = 0; p < geo.pre_P(); p++) {
            const int r0 = p * geo.pre_RP(), r1 = min(r0 + geo.pre_RP(), geo.H());
            const int nrows = 2 * (r1 - r0) + 1;  // input rows 2 r0 .. 2 r1 (row Hi and column Wi are the SAME padding: zero)
            if (p) __syncthreads();               // the previous pass has read its rows
            for (int i = tid; i < nrows * rowf4i; i += 512) {
                const int rr = i / rowf4i, e = i - rr * rowf4i, px = e / C4i, c4 = e - px * C4i, iy = 2 * r0 + rr;
                *reinterpret_cast<float4*>(lds + rr * RSi + px * PSi + 4 * c4) = iy < Hi ? ld4(src + ((long)iy * rowf4i + e) * 4) : zero4;
            }
            for (int i = tid; i < nrows * C4i; i += 512) {
                const int rr = i / C4i, c4 = i - rr * C4i;
                *reinterpret_cast<float4*>(lds + rr * RSi + Wi * PSi + 4 * c4) = zero4;
            }
            __syncthreads();
            MI_CHAIN_STAMP(16 + p)
            const int u = wave - p * UP;
            if (u >= 0 && u < UP) {  // wave-uniform
                const int ugrp = SPLIT ? u % geo.pre_GP() : u, umt = SPLIT ? u / geo.pre_GP() : 0;
                const int qp = ugrp * 32 + pl;
                const bool vp = qp < (r1 - r0) * geo.W();
                const int oyl = vp ? qp / geo.W() : 0, oxp = vp ? qp - (qp / geo.W()) * geo.W() : 0;
                const float* t0 = lds + (2 * oyl) * RSi + (2 * oxp) * PSi;  // tap (ky, kx) of this lane's output pixel
                auto dw = [&](int j, float4& bf) {
                    const int c0 = h * Chp + 4 * j;
                    // the loop stays here (fma4 only): as dw3x3_quad the run-time-geometry instantiations trade packed FMAs for plain ones
                    bf = ld4(bdw + c0);
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) {
                            const float4 w = ld4(wdw + (ky * 3 + kx) * geo.Cp() + c0);
                            const float4 d = ld4(t0 + ky * RSi + kx * PSi + c0);
                            fma4(d, w, bf);
                        }
                };
                if constexpr (SCHED == 1 && !SPLIT) {
                    using K = typename GP::K;
                    contract_ph(DwForm<K::Cp * 4, K::pre_RS * 4, K::pre_PS * 4, true>{}, std::integral_constant<int, K::pre_Cin / 8>{}, cb,
                                lds_addr(wdw + h * Chp), lds_addr(t0 + h * Chp), D);
                } else if constexpr (SPLIT) contract1(cb.w_pw, Chp >> 2, umt, dw, D[0]);
                else contract(cb, Chp >> 2, dw, D);
                const float hi = cb.act == ACT_RELU6 ? 6.f : INFINITY;
#pragma unroll
                for (int m = 0; m < (SPLIT ? 1 : MT); m++)
#pragma unroll
                    for (int gq = 0; gq < 4; gq++) {
                        const int ch = (SPLIT ? umt : m) * 32 + 8 * gq + 4 * h;
                        if (ch >= geo.C()) continue;
                        float4 sk = zero4;
                        if (cb.has_res && ch < Cin) {  // 2x2 max-pool of the input, channels above Cin are the zero pad
                            const float4 s0 = ld4(t0 + ch), s1 = ld4(t0 + PSi + ch), s2 = ld4(t0 + RSi + ch), s3 = ld4(t0 + RSi + PSi + ch);
                            sk = make_float4(fmaxf(fmaxf(s0.x, s1.x), fmaxf(s2.x, s3.x)), fmaxf(fmaxf(s0.y, s1.y), fmaxf(s2.y, s3.y)),
                                             fmaxf(fmaxf(s0.z, s1.z), fmaxf(s2.z, s3.z)), fmaxf(fmaxf(s0.w, s1.w), fmaxf(s2.w, s3.w)));
                        }
                        finish1(D[m], ch, gq, sk, hi);
                    }
                mine = vp;
                my_mt = umt;
                my_centre = tile + (r0 + oyl + 1) * geo.RS() + (oxp + 1) * geo.PS();
            }
        }
        __syncthreads();  // the staged input is dead
        for (int i = tid; i < ((geo.H() + 2) * geo.RS()) >> 2; i += 512) reinterpret_cast<float4*>(tile)[i] = zero4;
        commit_consts(cr);
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int m = 0; m < (SPLIT ? 1 : MT); m++)
#pragma unroll
                for (int gq = 0; gq < 4; gq++) {
                    const int ch = (SPLIT ? my_mt : m) * 32 + 8 * gq + 4 * h;
                    if (ch < geo.C()) *reinterpret_cast<float4*>(my_centre + ch) = make_float4(D[m][4 * gq], D[m][4 * gq + 1], D[m][4 * gq + 2], D[m][4 * gq + 3]);
                }
        }
    } else {
        // ---- load the frame (coalesced)
        fetch_consts(a.blocks[0], geo.C(), geo.C(), cr);
        for (int i = tid; i < ((geo.H() + 2) * geo.RS()) >> 2; i += 512) reinterpret_cast<float4*>(tile)[i] = zero4;
        __syncthreads();
        for (int i = tid; i < geo.H() * rowf4; i += 512) {
            int r = i / rowf4, e = i - r * rowf4;
            int px = e / geo.C4(), c4 = e - px * geo.C4();
            *reinterpret_cast<float4*>(tile + (r + 1) * geo.RS() + (px + 1) * geo.PS() + 4 * c4) = ld4(in + 4 * (long)i);
        }
        commit_consts(cr);
    }
    __syncthreads();

    MI_CHAIN_STAMP(1)
    for (int blk = 0; blk < a.nblocks; blk++) {
        const ChainBlock& cb = a.blocks[blk];
        // ---- the next stage's small constants start their trip now (committed to LDS behind this block's barrier)
        const bool more = blk + 1 < a.nblocks;
        if (more) fetch_consts(a.blocks[blk + 1], geo.C(), geo.C(), cr);
        else if (geo.post_on()) fetch_consts(a.post.blk, geo.C(), geo.post_Co(), cr);
        const float* wdw = lds + geo.off_wdw();
        const float* bdw = lds + geo.off_bdw();
        // fixed shapes: this lane's tap-weight offset as ONE register that already holds the (large) constant part, so that the nine tap
        // weights and the bias are that register plus an immediate (left to itself the compiler adds the constant again for every tap)
        int wlane = geo.off_wdw() + h * geo.Ch();
        if constexpr (GP::fixed) asm volatile("" : "+v"(wlane));

        f32x16 D[SPLIT ? 1 : MT];
        if (wave_active) {
            auto dw = [&](int j, float4& bf) {
                if constexpr (GP::fixed) {
                    // the same FMAs in the same order, written as the packed pairs the loop is scheduled for
                    const float* wj = lds + wlane + 4 * j;
                    const float* tj = tile + base0 + 4 * j;
                    f32x2c lo = {0.f, 0.f}, up = {0.f, 0.f};
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) {
                            const float4 w = ld4(wj + (ky * 3 + kx) * geo.Cp());
                            const float4 d = ld4(tj + ky * geo.RS() + kx * geo.PS());
                            lo = __builtin_elementwise_fma(f32x2c{d.x, d.y}, f32x2c{w.x, w.y}, lo);
                            up = __builtin_elementwise_fma(f32x2c{d.z, d.w}, f32x2c{w.z, w.w}, up);
                        }
                    const float4 bb = ld4(wj + 9 * geo.Cp());  // the depthwise bias lies behind the nine taps
                    lo += f32x2c{bb.x, bb.y};
                    up += f32x2c{bb.z, bb.w};
                    bf = make_float4(lo.x, lo.y, up.x, up.y);
                    return;
                }
                const float* wj = wdw + h * geo.Ch() + 4 * j;
                bf = zero4;
#ifdef MI_ABL_CHAIN_NODW  // timing ablation: centre tap only
                bf = ld4(tile + base0 + geo.RS() + geo.PS() + 4 * j);
                return;
#endif
#pragma unroll
                for (int ky = 0; ky < 3; ky++)
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) {
                        const float4 w = ld4(wj + (ky * 3 + kx) * geo.Cp());
                        const float4 d = ld4(tile + base0 + ky * geo.RS() + kx * geo.PS() + 4 * j);
                        fma4(d, w, bf);
                    }
                bf = add4(bf, ld4(bdw + h * geo.Ch() + 4 * j));
            };
            // ---- contraction, then the epilogue into registers (reads x at the centre pixel), written back after the barrier
            const float hi = cb.act == ACT_RELU6 ? 6.f : INFINITY;
            if constexpr (SCHED == 1) {
                using K = typename GP::K;
                using F = DwForm<K::Cp * 4, K::RS * 4, K::PS * 4, false>;
                using N = std::integral_constant<int, K::Ch / 4>;
                if constexpr (SPLIT) contract1_ph(F{}, N{}, cb.w_pw, mt_w, lds_addr(lds + wlane), lds_addr(tile + base0), D[0]);
                else contract_ph(F{}, N{}, cb, lds_addr(lds + wlane), lds_addr(tile + base0), D);
            } else if constexpr (SPLIT) contract1(cb.w_pw, nch, mt_w, dw, D[0]);
            else contract(cb, nch, dw, D);
#pragma unroll
            for (int m = 0; m < (SPLIT ? 1 : MT); m++)
#pragma unroll
                for (int gq = 0; gq < 4; gq++) {
                    const int ch = (SPLIT ? mt_w : m) * 32 + 8 * gq + 4 * h;
                    if (ch < geo.C()) finish1(D[m], ch, gq, (GP::all_res || cb.has_res) ? ld4(centre + ch) : zero4, hi);
                }
        }
        __syncthreads();  // every wave has read x (and the constants) for this block
        if (more || geo.post_on()) commit_consts(cr);
        if (wave_active && valid) {
#pragma unroll
            for (int m = 0; m < (SPLIT ? 1 : MT); m++)
#pragma unroll
                for (int gq = 0; gq < 4; gq++) {
                    const int ch = (SPLIT ? mt_w : m) * 32 + 8 * gq + 4 * h;
                    if (ch < geo.C()) *reinterpret_cast<float4*>(centre + ch) = make_float4(D[m][4 * gq], D[m][4 * gq + 1], D[m][4 * gq + 2], D[m][4 * gq + 3]);
                }
        }
        __syncthreads();
        MI_CHAIN_STAMP(2 + blk)
    }
    // ---- write the frame back (coalesced 16 B per lane, consecutive addresses)
    if (a.write_out) {
        float* out = a.out + (long)b * a.out_fs;
        for (int i = tid; i < geo.H() * rowf4; i += 512) {
            int r = i / rowf4, e = i - r * rowf4;
            int px = e / geo.C4(), c4 = e - px * geo.C4();
            *reinterpret_cast<float4*>(out + 4 * (long)i) = ld4(tile + (r + 1) * geo.RS() + (px + 1) * geo.PS() + 4 * c4);
        }
    }
    MI_CHAIN_STAMP(10)
    int post_units = 0;
    if (geo.post_on()) {
        // ---- the stride-2 block behind the chain: taps from the resident frame, output straight to global memory
        const ChainBlock& cb = a.post.blk;
        const int Ho = geo.H() >> 1, Wo = geo.W() >> 1, Co = geo.post_Co(), npo = Ho * Wo;  // constants: committed behind the last block
        const float* wdw = lds + geo.off_wdw();
        const float* bdw = lds + geo.off_bdw();
        const int ngo = (npo + 31) >> 5, MTo = (Co + 31) >> 5;
        post_units = ngo * MTo;
        for (int u = wave; u < post_units; u += 8) {  // wave-uniform; unit = (32 output pixels, 32 output channels)
            const int grp = u % ngo, mt = u / ngo;
            const int qo = grp * 32 + pl;
            const bool vo = qo < npo;
            const int py = vo ? qo / Wo : 0, px = vo ? qo - (qo / Wo) * Wo : 0;
            // SAME on an even size: taps at image rows 2py .. 2py+2 = tile slots 2py+1 .. 2py+3 (slot H+1 is the zero border)
            const float* t0 = tile + (2 * py + 1) * geo.RS() + (2 * px + 1) * geo.PS();
            f32x16 D1;
            auto dw = [&](int j, float4& bf) {
                const int c0 = h * geo.Ch() + 4 * j;
                bf = dw3x3_quad<true>(wdw + c0, geo.Cp(), t0 + c0, geo.RS(), geo.PS(), bdw + c0);
            };
            if constexpr (SCHED == 1) {
                using K = typename GP::K;
                contract1_ph(DwForm<K::Cp * 4, K::RS * 4, K::PS * 4, true>{}, std::integral_constant<int, K::Ch / 4>{}, cb.w_pw, mt,
                             lds_addr(wdw + h * geo.Ch()), lds_addr(t0 + h * geo.Ch()), D1);
            } else contract1(cb.w_pw, nch, mt, dw, D1);
            const float hi = cb.act == ACT_RELU6 ? 6.f : INFINITY;
            float* dst = a.post.out + (long)b * a.post.out_fs + (long)qo * Co;
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                const int ch = mt * 32 + 8 * gq + 4 * h;
                if (ch >= Co) continue;
                float4 sk = zero4;
                if (cb.has_res && ch < geo.C()) {  // 2x2 max-pool of the resident frame, zero channel pad above C
                    const float4 s0 = ld4(t0 + ch), s1 = ld4(t0 + geo.PS() + ch), s2 = ld4(t0 + geo.RS() + ch), s3 = ld4(t0 + geo.RS() + geo.PS() + ch);
                    sk = make_float4(fmaxf(fmaxf(s0.x, s1.x), fmaxf(s2.x, s3.x)), fmaxf(fmaxf(s0.y, s1.y), fmaxf(s2.y, s3.y)),
                                     fmaxf(fmaxf(s0.z, s1.z), fmaxf(s2.z, s3.z)), fmaxf(fmaxf(s0.w, s1.w), fmaxf(s2.w, s3.w)));
                }
                finish1(D1, ch, gq, sk, hi);
                if (vo) {
                    const float4 v = make_float4(D1[4 * gq], D1[4 * gq + 1], D1[4 * gq + 2], D1[4 * gq + 3]);
                    *reinterpret_cast<float4*>(dst + ch) = v;
                    if (g.off_t8 >= 0) *reinterpret_cast<float4*>(lds + g.off_t8 + qo * (Co + 4) + ch) = v;
                }
            }
        }
    }
    MI_CHAIN_STAMP(11)
    // ---- output heads: stacked 1x1 convolutions on the resident frame / on `post`'s output; unit = (32 pixels, 32 stacked rows)
    for (int hd = 0; hd < kChainHeads; hd++) {
        MI_CHAIN_STAMP(12 + hd)
        const ChainHead& H = a.heads[hd];
        if (!H.on) continue;
        if (H.src == 1) { __syncthreads(); post_units = 0; }  // `post`'s LDS copy is complete; heads on the frame itself need no barrier
        const bool from_post = H.src == 1;
        const int Wh = from_post ? geo.W() >> 1 : geo.W(), np = from_post ? (geo.H() >> 1) * (geo.W() >> 1) : geo.H() * geo.W();
        const int Cs = from_post ? geo.post_Co() : geo.C(), Chs = Cs >> 1, nchs = Chs >> 2;
        const int Cot = H.Co_a + H.Co_b, MTh = (Cot + 31) >> 5, ng = (np + 31) >> 5;
        // heads on the frame start on the waves that `post` left without a unit
        for (int u = (wave - post_units) & 7; u < ng * MTh; u += 8) {  // wave-uniform
            const int grp = u % ng, mt = u / ng;
            const int qh = grp * 32 + pl;
            const bool vh = qh < np;
            const int qc = vh ? qh : 0;
            const float* px = from_post ? lds + g.off_t8 + qc * (Cs + 4) : tile + (qc / Wh + 1) * geo.RS() + (qc % Wh + 1) * geo.PS();
            float4 bq[4];
#pragma unroll
            for (int gq = 0; gq < 4; gq++) bq[gq] = H.bias ? ld4(H.bias + mt * 32 + 8 * gq + 4 * h) : zero4;  // stacked, zero padded to the tile
            f32x16 D1;
            contract1(H.w_pw, nchs, mt, [&](int j, float4& bf) { bf = ld4(px + h * Chs + 4 * j); }, D1);
            if (!vh) continue;
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                const int ch = mt * 32 + 8 * gq + 4 * h;   // stacked row
                if (ch >= Cot) continue;
                const float v[4] = {D1[4 * gq] + bq[gq].x, D1[4 * gq + 1] + bq[gq].y, D1[4 * gq + 2] + bq[gq].z, D1[4 * gq + 3] + bq[gq].w};
                if (ch < H.Co_a) {  // Co_a % 4 == 0: the quad lies in one head
                    *reinterpret_cast<float4*>(H.out_a + (long)b * H.out_a_fs + (long)qh * H.Co_a + ch) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    float* ob = H.out_b + (long)b * H.out_b_fs + (long)qh * H.Co_b + (ch - H.Co_a);
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (ch + e < Cot) ob[e] = v[e];
                }
            }
        }
    }
    MI_CHAIN_STAMP(14)
}

bool make_chain_geom(const ChainArgs& a, ChainGeom* out) {
    ChainGeom g{};
    if (a.C % 8 || a.H * a.W > 256 || a.nblocks < 1 || a.nblocks > kMaxChain) return false;
    g.Cp = a.C; g.Ch = a.C / 2; g.C4 = a.C / 4; g.PS = a.C + 4; g.RS = (a.W + 2) * g.PS;
    g.MT = (a.C + 31) / 32;
    if (g.MT > 4) return false;
    g.split = g.MT > 1 && ((a.H * a.W + 31) / 32) * g.MT <= 8;
    int off = (a.H + 2) * g.RS;
    if (a.pre.on) {
        // staging area of `pre`'s input (shares the tile region, grows it when larger): fewest passes whose rows fit and whose
        // 32-pixel groups all find a wave of their own
        if (a.pre.Cin % 8 || a.pre.Cin < 8 || a.pre.Cin > a.C) return false;
        g.pre_PS = a.pre.Cin + 4;
        g.pre_RS = (2 * a.W + 1) * g.pre_PS;
        g.pre_P = chain_pre_passes(a.C, a.H, a.W, a.pre.Cin, a.post.on ? a.post.Co : 0, g.MT, g.split != 0, off);
        if (!g.pre_P) return false;
        g.pre_RP = (a.H + g.pre_P - 1) / g.pre_P;
        g.pre_GP = (g.pre_RP * a.W + 31) / 32;
        off = (int)std::max<long>((long)(2 * g.pre_RP + 1) * g.pre_RS, off);
    }
    g.off_wdw = off; off += 9 * g.Cp;
    g.off_bdw = off; off += g.Cp;
    off = (off + 3) & ~3;
    g.off_bias = off; off += g.MT * 32;
    g.off_alpha = off; off += g.MT * 32;
    g.off_t8 = -1;
    for (int hd = 0; hd < kChainHeads; hd++) {
        const ChainHead& H = a.heads[hd];
        if (!H.on) continue;
        if (H.Co_a < 4 || H.Co_a % 4 || H.Co_b < 0 || H.Co_a + H.Co_b > 128 || !H.out_a || (H.Co_b && !H.out_b) || !H.w_pw) return false;
        if ((reinterpret_cast<uintptr_t>(H.out_a) & 15) || (H.out_a_fs & 3) || (reinterpret_cast<uintptr_t>(H.w_pw) & 15)) return false;
        if (H.src == 1) {
            if (!a.post.on) return false;
            if (g.off_t8 < 0) { g.off_t8 = off; off += (a.H >> 1) * (a.W >> 1) * (a.post.Co + 4); }
        }
    }
    g.lds_bytes = off * 4;
    if (g.lds_bytes > kLdsBudget) return false;
    if (!aligned16(a.in) || !aligned16(a.out) || (a.in_fs & 3) || (a.out_fs & 3)) return false;
    if (a.pre.on && (a.pre.Cin % 8 || a.pre.Cin < 8 || a.pre.Cin > a.C || !aligned16(a.pre.in) || (a.pre.in_fs & 3))) return false;
    if (a.post.on && ((a.H & 1) || (a.W & 1) || a.post.Co % 4 || a.post.Co < a.C || a.post.Co > g.MT * 32 || !aligned16(a.post.out) || (a.post.out_fs & 3))) return false;
    *out = g;
    return true;
}

using Geom16 = GeomFixed<96, 16, 16, 48, 96>;  // BackCamera, Short / Front: 32x32x48 -> [s2] -> 16x16x96 blocks -> [s2] -> 8x8x96
using Geom8 = GeomFixed<96, 8, 8, 0, 0>;       // Short / Front: the 8x8x96 blocks behind it (SPLIT)

bool all_relu(const ChainArgs& a) {
    bool ok = (!a.pre.on || a.pre.blk.act == ACT_RELU) && (!a.post.on || a.post.blk.act == ACT_RELU);
    for (int k = 0; ok && k < a.nblocks; k++) ok = a.blocks[k].act == ACT_RELU;
    return ok;
}

template <int MT, bool SPLIT, class GP = GeomRun, int ACT = kActRun, int SCHED = 0>
int launch_chain_inst(const ChainArgs& a, const ChainGeom& g, hipStream_t s) {
    return launch_full_lds(chain_kernel<MT, SPLIT, GP, ACT, SCHED>, dim3((unsigned)a.B), dim3(512), (size_t)g.lds_bytes, s, a, g);
}

}  // namespace

bool chain_kernel_supports(const ChainArgs& a) {
    ChainGeom g;
    return make_chain_geom(a, &g);
}

int launch_chain(const ChainArgs& a, void* stream, int fixed, int sched) {
    ChainGeom g;
    if (!make_chain_geom(a, &g)) return (int)hipErrorInvalidValue;
#ifdef MI_CHAIN_STAMPS
    g.stamps = g_chain_stamps;
#endif
    hipStream_t s = (hipStream_t)stream;
    // the detectors' shapes as constants, where the whole launch is of that form: the shape, `pre` / `post`, ReLU in every block and a skip
    // connection in every stride-1 block (the heads stay run-time arguments in both forms).  Same arithmetic in the same order: bit-equal to the generic kernel.
    if (fixed && all_relu(a)) {
        // sched: the contraction in phases, or interleaved (option "chain_sched"; the same FMA chains and MFMA order in both)
        if (Geom16::matches(a, g)) return sched ? launch_chain_inst<3, false, Geom16, ACT_RELU, 1>(a, g, s) : launch_chain_inst<3, false, Geom16, ACT_RELU, 0>(a, g, s);
        if (Geom8::matches(a, g)) return sched ? launch_chain_inst<3, true, Geom8, ACT_RELU, 1>(a, g, s) : launch_chain_inst<3, true, Geom8, ACT_RELU, 0>(a, g, s);
    }
    switch (g.MT) {
        case 1: return launch_chain_inst<1, false>(a, g, s);
        case 2: return g.split ? launch_chain_inst<2, true>(a, g, s) : launch_chain_inst<2, false>(a, g, s);
        case 3: return g.split ? launch_chain_inst<3, true>(a, g, s) : launch_chain_inst<3, false>(a, g, s);
        case 4: return g.split ? launch_chain_inst<4, true>(a, g, s) : launch_chain_inst<4, false>(a, g, s);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace mi

#ifdef MI_CHAIN_STAMPS
// stamps build only (tools/chain_stamps.py)
extern "C" void mi_debug_set_chain_stamps(unsigned long long* p) { mi::g_chain_stamps = p; }
#endif
