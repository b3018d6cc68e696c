// mrow.hpp — building blocks shared by the row-walking MFMA kernels (mstrip_kernels.hip, mwalk_kernels.hip, ms2_kernels.hip and
// mdblock_kernels.hip with its mbneck_kernel): a wave walks down the rows of a frame, one input row per step, with the depthwise 3x3 +
// pointwise stage in the v_mfma_f32_16x16x4_f32 operand layout.  Lane (kq = lane / 16, p = lane % 16) owns channel 4 ks + kq of pixel p of
// a 16-pixel tile for every k-step ks; see mstrip_kernels.hip for the scheme and its measurements.
// First the depthwise row itself (mdb_row, packed FMAs), then the frame around it, written once for all six kernels: the LDS-DMA of a row
// into a row image (mrow_dma2 / mrow_dma1), the clearing of rows and border columns outside the frame, accumulators <- bias + skip,
// activation + store, the counted vmcnt wait, the scalar tap load and mstrip's row (mstrip_row, plain FMAs); last the host side of the
// constants blobs and the launch.  Every function takes the kernel's own scalars and array references; the kernels keep their schedules.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "kernels.hpp"
#include "launch.hpp"
#include "wave_sync.hpp"

namespace mi {

namespace {

typedef float df32x4 __attribute__((ext_vector_type(4)));

// workgroup barrier behind an LDS-only wait (__syncthreads() would also drain vmcnt: the next row's DMA and the output stores).
// Not wave_sync.hpp's lds_barrier: this one is a single asm statement, so the compiler's own wait counting does not see the wait; with
// lds_barrier in its place mdblock_kernel<MD<4,4,1,2,3,true,8,..,PAIR,STEM>> has 183 / 185 s_waitcnt instead of 193 / 196.
__device__ __forceinline__ void dwg_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <class F, int... KS>
__device__ __forceinline__ void dfor_each(F&& f, std::integer_sequence<int, KS...>) { (f(std::integral_constant<int, KS>{}), ...); }

typedef float dv2f __attribute__((ext_vector_type(2)));

// Partial depthwise rows of a wave's WT pixel tiles for one k-step: tiles 0 / 1 (and 2 / 3) as register PAIRS, an odd last tile alone.
// A pair is one v_pk_fma_f32 per tap: the tap is a half of a register pair too, broadcast to both lanes of the packed operation by op_sel
// (a tap duplicated into both halves was what kept mstrip_kernel on scalar FMAs) — half the depthwise instructions of a row.
template <int WT>
struct RowAcc {
    dv2f p[WT / 2 ? WT / 2 : 1];
    float s[1];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < (WT / 2 ? WT / 2 : 1); q++) p[q] = dv2f{0.f, 0.f};
        s[0] = 0.f;
    }
};

// acc += x * w.lo / w.hi on both lanes (S = 0: the low half of the tap pair, 1: the high half).  Inline asm: written as vector code
// (splat folded into op_sel by LLVM) the register allocator scalarises half of the operations again and spills.  The instructions are
// then invisible to the hazard recogniser (a v_mfma reads a register v_pk_fma_f32 wrote 0 or 1 instructions earlier STALE,
// tools/pk_mfma_hazard.hip): mrow_stage computes a pair's finished row first and puts a scheduling fence in front of the MFMAs, so
// that six packed operations lie between; tests/test_isa_checks.py keeps these kernels free of spills, which would break the count.
template <int S>
__device__ __forceinline__ void dpk_fma(dv2f& acc, const dv2f x, const dv2f w) {
    if constexpr (S == 0) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(x), "v"(w));
    else asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(x), "v"(w));
}
template <int S>
__device__ __forceinline__ dv2f dpk_mul(const dv2f x, const dv2f w) {
    dv2f r;
    if constexpr (S == 0) asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(x), "v"(w));
    else asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(x), "v"(w));
    return r;
}

// The nine taps of a k-step as five register pairs: t[i] = (w[2 i], w[2 i + 1]); from three float4s [w0 w1 w2 w3][w4 w5 w6 w7][w8 . . .]
__device__ __forceinline__ void dtaps_from(const float4 t0, const float4 t1, const float4 t2, dv2f (&t)[5]) {
    t[0] = dv2f{t0.x, t0.y}; t[1] = dv2f{t0.z, t0.w}; t[2] = dv2f{t1.x, t1.y}; t[3] = dv2f{t1.z, t1.w}; t[4] = dv2f{t2.x, 0.f};
}
// tap[ks] <- this lane's taps (tp: its [ks][.][12] block in LDS), resident in registers for the whole kernel
template <int CK>
__device__ __forceinline__ void dload_taps(const float4* tp, dv2f (&tap)[CK][5]) {
#pragma unroll
    for (int ks = 0; ks < CK; ks++) dtaps_from(tp[ks * 12], tp[ks * 12 + 1], tp[ks * 12 + 2], tap[ks]);
#pragma unroll
    for (int ks = 0; ks < CK; ks++)
#pragma unroll
        for (int t = 0; t < 5; t++) asm volatile("" : "+v"(tap[ks][t]));
}

// One input row of a stage in the operand layout.  src: LDS byte address of this lane's left neighbour pixel, channel kq, of the row
// image (pixel stride PSV floats; tile nt is 16 pixels on); its ky = 2 / 1 / 0 taps go to the partial depthwise rows r-1 / r / r+1
// (aPN on entry / aC / aPN on exit).  With EMIT the finished depthwise row r-1 is the B operand of this row's MFMAs into D
// (A operands: LDS byte address aop + lane, [ks][mt][64]).
// The LDS reads are inline asm with their own waits: left to the compiler, the reads of a whole row are merged across k-steps and
// hoisted (the taps get spilled).  Every wait is lgkmcnt(0): scalar loads share the counter and return out of order.
// TAPL: the taps are read from LDS per k-step (tapl: this lane's [ks][.][12] block) instead of living in registers (tap unused).
template <int CK, int MT, int WT, int PSV, bool EMIT, bool TAPL = false>
__device__ __forceinline__ void mdb_row(const unsigned src, const unsigned aop, const dv2f (&tap)[TAPL ? 1 : CK][5], RowAcc<WT> (&aPN)[CK], RowAcc<WT> (&aC)[CK],
                                        df32x4 (&D)[MT][WT], const float4* tapl = nullptr) {
    constexpr int NP = WT / 2, ODD = WT & 1;
    float xs[2][3][WT], av[2][MT];
    auto load_ks = [&](auto ksc, float (&x)[3][WT], float (&aw)[MT]) {
        constexpr int ks = decltype(ksc)::value;
        const unsigned xa = src, aa = aop;
#pragma unroll
        for (int dx = 0; dx < 3; dx++)
#pragma unroll
            for (int nt = 0; nt < WT; nt++) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(x[dx][nt]) : "v"(xa), "n"((dx * PSV + 4 * ks) * 4 + nt * 16 * PSV * 4));
        if constexpr (EMIT) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(aw[mt]) : "v"(aa), "n"((ks * MT + mt) * 64 * 4));
        }
    };
    // The loaded registers pass through an (empty) asm statement behind the wait: their consumers then depend on something that is ordered
    // behind the s_waitcnt, whatever a later compiler would like to hoist (to the compiler the ds_read asm "returned" its value at once).
    auto landed = [&](float (&x)[3][WT], float (&aw)[MT]) {
#pragma unroll
        for (int dx = 0; dx < 3; dx++)
#pragma unroll
            for (int nt = 0; nt < WT; nt++) asm volatile("" : "+v"(x[dx][nt]));
        if constexpr (EMIT) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) asm volatile("" : "+v"(aw[mt]));
        }
    };
    auto kstep = [&](auto ksc) {
        constexpr int ks = decltype(ksc)::value;
        if constexpr (ks + 1 < CK) load_ks(std::integral_constant<int, ks + 1>{}, xs[(ks + 1) & 1], av[(ks + 1) & 1]);
        float (&x)[3][WT] = xs[ks & 1];
        float (&aw)[MT] = av[ks & 1];
        dv2f w[5];
        if constexpr (TAPL) {
            dtaps_from(tapl[ks * 12], tapl[ks * 12 + 1], tapl[ks * 12 + 2], w);
        } else {
#pragma unroll
            for (int t = 0; t < 5; t++) w[t] = tap[ks][t];
        }
        float pch[WT];
        // tile pairs: tap t = half (t & 1) of w[t >> 1]; per accumulator the same order of operations as the single-tile form below
#pragma unroll
        for (int q = 0; q < NP; q++) {
            const dv2f x0 = dv2f{x[0][2 * q], x[0][2 * q + 1]}, x1 = dv2f{x[1][2 * q], x[1][2 * q + 1]}, x2 = dv2f{x[2][2 * q], x[2][2 * q + 1]};
            dv2f c = aC[ks].p[q], pc = aPN[ks].p[q];
            if (EMIT) { dpk_fma<0>(pc, x0, w[3]); dpk_fma<1>(pc, x1, w[3]); dpk_fma<0>(pc, x2, w[4]); }
            dv2f n = dpk_mul<0>(x0, w[0]);
            dpk_fma<1>(n, x1, w[0]);
            dpk_fma<0>(n, x2, w[1]);
            dpk_fma<1>(c, x0, w[1]); dpk_fma<0>(c, x1, w[2]); dpk_fma<1>(c, x2, w[2]);
            aC[ks].p[q] = c;
            aPN[ks].p[q] = n;
            asm volatile("" : "+v"(aC[ks].p[q]), "+v"(aPN[ks].p[q]));  // pinned: LLVM would sink these updates into the next row
            pch[2 * q] = pc.x;
            pch[2 * q + 1] = pc.y;
        }
        if constexpr (ODD) {
            constexpr int nt = WT - 1;
            float n = x[0][nt] * w[0].x, c = aC[ks].s[0], pc = aPN[ks].s[0];
            if (EMIT) { pc = __builtin_fmaf(x[0][nt], w[3].x, pc); pc = __builtin_fmaf(x[1][nt], w[3].y, pc); pc = __builtin_fmaf(x[2][nt], w[4].x, pc); }
            n = __builtin_fmaf(x[1][nt], w[0].y, n);
            n = __builtin_fmaf(x[2][nt], w[1].x, n);
            c = __builtin_fmaf(x[0][nt], w[1].y, c);
            c = __builtin_fmaf(x[1][nt], w[2].x, c);
            c = __builtin_fmaf(x[2][nt], w[2].y, c);
            aC[ks].s[0] = c;
            aPN[ks].s[0] = n;
            asm volatile("" : "+v"(aC[ks].s[0]), "+v"(aPN[ks].s[0]));
            pch[nt] = pc;
        }
        if constexpr (EMIT) {
            // The packed FMAs are inline asm, invisible to the compiler's hazard recogniser, and v_mfma reads a register a v_pk_fma_f32 wrote
            // fewer than two instructions earlier STALE (tools/pk_mfma_hazard.hip: B = old value at 0 / 1 instructions in between, new from 2
            // on).  The asm statements are volatile (program order: a pair's finished row first, then its six other operations) and
            // nothing crosses this fence, so at least six instructions lie between the last write of a B operand and the first MFMA.
            if constexpr (NP > 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int nt = 0; nt < WT; nt++) D[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[mt], pch[nt], D[mt][nt], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next k-step's operands (a whole k-step of cover)
        if constexpr (ks + 1 < CK) landed(xs[(ks + 1) & 1], av[(ks + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
    };
    load_ks(std::integral_constant<int, 0>{}, xs[0], av[0]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    landed(xs[0], av[0]);
    __builtin_amdgcn_sched_barrier(0);
    dfor_each(kstep, std::make_integer_sequence<int, CK>{});
}

// mstrip's row: mdb_row's contract for two pixel tiles (pixel stride PS) with the nine taps of a k-step as scalars in registers and the
// depthwise arithmetic on plain v_fma_f32 (the tap is one register for both tiles; a packed FMA would need it duplicated into a register
// pair): 18 per k-step, which the partner wave's MFMAs cover.  xr / ar: LDS byte addresses as src / aop of mdb_row.
// Left to the compiler, the LDS reads of a whole row are merged across k-steps and hoisted to the top of the row (72 + 36 values live:
// the depthwise taps get spilled).  Every wait is lgkmcnt(0): scalar loads (kernel arguments the compiler re-reads) share the counter
// and return out of order.
template <int CK, int MT, int PS, bool EMIT>
__device__ __forceinline__ void mstrip_row(const unsigned xr, const unsigned ar, const float (&tap)[CK][9], float (&aPN)[CK][2], float (&aC)[CK][2], df32x4 (&D)[MT][2]) {
    float xs[2][3][2], av[2][MT];
    auto load_ks = [&](auto ksc, float (&x)[3][2], float (&aw)[MT]) {  // k-step ks: the three tap columns of both pixel tiles; the A operands
        constexpr int ks = decltype(ksc)::value;
        const unsigned xa = xr, aa = ar;  // (named unconditionally: a capture used only inside `if constexpr` is lost by clang)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(x[dx][0]) : "v"(xa), "n"((dx * PS + 4 * ks) * 4));
            asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(x[dx][1]) : "v"(xa), "n"((dx * PS + 4 * ks + 16 * PS) * 4));
        }
        if constexpr (EMIT) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(aw[mt]) : "v"(aa), "n"((ks * MT + mt) * 64 * 4));
        }
    };
    // the loaded registers pass through an (empty) asm statement behind the wait: their consumers then depend on something that is
    // ordered behind the s_waitcnt (to the compiler the ds_read asm "returned" its value at once)
    auto landed = [&](float (&x)[3][2], float (&aw)[MT]) {
#pragma unroll
        for (int dx = 0; dx < 3; dx++) asm volatile("" : "+v"(x[dx][0]), "+v"(x[dx][1]));
        if constexpr (EMIT) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) asm volatile("" : "+v"(aw[mt]));
        }
    };
    auto kstep = [&](auto ksc) {
        constexpr int ks = decltype(ksc)::value;
        if constexpr (ks + 1 < CK) load_ks(std::integral_constant<int, ks + 1>{}, xs[(ks + 1) & 1], av[(ks + 1) & 1]);
        float (&x)[3][2] = xs[ks & 1];
        float (&aw)[MT] = av[ks & 1];
        const float (&w)[9] = tap[ks];
        float pch[2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            float n = x[0][nt] * w[0], c = aC[ks][nt], pc = aPN[ks][nt];
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                if (EMIT) pc = __builtin_fmaf(x[dx][nt], w[6 + dx], pc);
                if (dx) n = __builtin_fmaf(x[dx][nt], w[dx], n);
                c = __builtin_fmaf(x[dx][nt], w[3 + dx], c);
            }
            aC[ks][nt] = c;
            aPN[ks][nt] = n;
            // pinned here: left alone, LLVM sinks these updates into the next row's block (their only use), which keeps every
            // k-step's pixels alive to the end of the row
            asm volatile("" : "+v"(aC[ks][nt]), "+v"(aPN[ks][nt]));
            pch[nt] = pc;
        }
        if constexpr (EMIT) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                D[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[mt], pch[0], D[mt][0], 0, 0, 0);
                D[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[mt], pch[1], D[mt][1], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next k-step's operands (a whole k-step of cover)
        if constexpr (ks + 1 < CK) landed(xs[(ks + 1) & 1], av[(ks + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
    };
    load_ks(std::integral_constant<int, 0>{}, xs[0], av[0]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    landed(xs[0], av[0]);
    __builtin_amdgcn_sched_barrier(0);
    dfor_each(kstep, std::make_integer_sequence<int, CK>{});
}

// ---- the frame around a row

typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(1))) df32x4 gf32x4;

// LDS-DMA source offset of a lane: instruction k of a row brings in pixels [DPX k, DPX k + DPX): lane -> (pixel lane / QP, quad
// min(lane % QP, CK - 1)) with QP = CK + 1 float4 slots per pixel of the image, lanes >= DPX * QP idle
template <int CK>
__device__ __forceinline__ int mrow_goff(int lane) { return ((lane / (CK + 1)) * 4 * CK + 4 * min(lane % (CK + 1), CK - 1)) * 4; }

constexpr unsigned mrow_exec_hi(int active) { return active == 64 ? 0xffffffffu : (1u << (active - 32)) - 1; }

// One row by LDS-DMA, two-base form: eight instructions, four immediate offsets on each of two source bases (src, and src + half a row).
// The immediate offset moves source and destination alike, M0 makes up the difference between the image's pixel stride PS and the
// tensor's C.  dstb: LDS byte address of the row's first pixel in the image.
template <int C, int PS, int DPX, int ACTIVE>
__device__ __forceinline__ void mrow_dma2(const char* src, const unsigned dstb, const int goff) {
    static_assert(ACTIVE > 32 && ACTIVE < 64, "exec mask written as two 32-bit halves");
    const char* src1 = src + 4 * DPX * C * 4;
    unsigned long long saved;
#define MI_MROW_DMA2(base, k) "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, " base " offset:" #k "*%8\n\t"
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 exec_lo, -1\n\ts_mov_b32 exec_hi, %6\n\t"
                 "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %1\n\t"
                 MI_MROW_DMA2("%1", 1) MI_MROW_DMA2("%1", 2) MI_MROW_DMA2("%1", 3)
                 "s_add_u32 m0, m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %2\n\t"
                 MI_MROW_DMA2("%2", 1) MI_MROW_DMA2("%2", 2) MI_MROW_DMA2("%2", 3)
                 "s_mov_b64 exec, %0"
                 : "=&s"(saved)
                 : "s"(src), "s"(src1), "v"(goff), "s"(dstb), "n"(4 * DPX * PS * 4 - 3 * DPX * (PS - C) * 4),
                   "n"(mrow_exec_hi(ACTIVE)), "n"(DPX * (PS - C) * 4), "n"(DPX * C * 4)
                 : "memory", "scc", "m0");
#undef MI_MROW_DMA2
}
// ... one-base form: N = 4 or 8 instructions on consecutive immediate offsets
template <int N, int C, int PS, int DPX, int ACTIVE>
__device__ __forceinline__ void mrow_dma1(const char* src, const unsigned dstb, const int goff) {
    static_assert((N == 4 || N == 8) && ACTIVE > 32 && ACTIVE <= 64 && (N - 1) * DPX * C * 4 < 4096, "DMA shape");
    unsigned long long saved;
#define MI_MROW_DMA1(k) "s_add_u32 m0, m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1 offset:" #k "*%6\n\t"
#define MI_MROW_DMA1_ROW(more)                                                                                                             \
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 exec_lo, -1\n\ts_mov_b32 exec_hi, %4\n\t"                                                \
                 "s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1\n\t"                                                       \
                 MI_MROW_DMA1(1) MI_MROW_DMA1(2) MI_MROW_DMA1(3) more                                                                      \
                 "s_mov_b64 exec, %0"                                                                                                      \
                 : "=&s"(saved)                                                                                                            \
                 : "s"(src), "v"(goff), "s"(dstb), "n"(mrow_exec_hi(ACTIVE)), "n"(DPX * (PS - C) * 4), "n"(DPX * C * 4)                     \
                 : "memory", "scc", "m0")
    if constexpr (N == 8) MI_MROW_DMA1_ROW(MI_MROW_DMA1(4) MI_MROW_DMA1(5) MI_MROW_DMA1(6) MI_MROW_DMA1(7));
    else MI_MROW_DMA1_ROW("");
#undef MI_MROW_DMA1_ROW
#undef MI_MROW_DMA1
}

// Rows outside the frame are zero padding: the landed (clamped) row — N4 float4s from `part` on — is cleared before it is read
__device__ __forceinline__ float4 mrow_zero4() {
    float zz = 0.f;
    asm volatile("" : "+v"(zz));
    return make_float4(zz, zz, zz, zz);
}
template <int N4>
__device__ __forceinline__ void mrow_clear_row(float* part, const int lane) {
    const float4 z = mrow_zero4();
#pragma unroll
    for (int k = 0; k < (N4 + 63) / 64; k++)
        if (64 * (k + 1) <= N4 || lane < N4 - 64 * k) *reinterpret_cast<float4*>(part + 4 * (lane + 64 * k)) = z;
}
__device__ __forceinline__ void mrow_clear_row(float* part, const int lane, const int n4) {
    const float4 z = mrow_zero4();
    for (int k = lane; k < n4; k += 64) *reinterpret_cast<float4*>(part + 4 * k) = z;
}
// The two border pixel columns (COL_F floats apart) of NIMG row images are never written by the DMA: cleared once
template <int QP, int NIMG, int IMG_F, int COL_F>
__device__ __forceinline__ void mrow_clear_border(float* img, const int lane) {
    if (lane < 2 * QP) {
        const int col = lane / QP, qd = lane - col * QP;
#pragma unroll
        for (int s = 0; s < NIMG; s++) *reinterpret_cast<float4*>(img + s * IMG_F + col * COL_F + 4 * qd) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// D <- bias (+ skip: the centre pixels of a row image, D layout, pixel stride PSV; channels >= C are the skip's zero channel-pad).
// bias / skip: this lane's (+ 4 kq).  has_res is wave-uniform: one branch around all the reads (per tile, each read would be waited for on its own)
template <int C, int PSV, int MT, int WT>
__device__ __forceinline__ void mrow_init_acc(df32x4 (&D)[MT][WT], const float* bias, const float* skip, const bool has_res) {
    float4 bs[MT], x[MT][WT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) bs[mt] = *reinterpret_cast<const float4*>(bias + 16 * mt);
    if (has_res) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < WT; nt++) {
                x[mt][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (16 * mt < C) x[mt][nt] = *reinterpret_cast<const float4*>(skip + 16 * nt * PSV + 16 * mt);
            }
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < WT; nt++) D[mt][nt] = df32x4{x[mt][nt].x + bs[mt].x, x[mt][nt].y + bs[mt].y, x[mt][nt].z + bs[mt].z, x[mt][nt].w + bs[mt].w};
    } else {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < WT; nt++) D[mt][nt] = df32x4{bs[mt].x, bs[mt].y, bs[mt].z, bs[mt].w};
    }
}

// act(v) = min(max(v,0) + slope*min(v,0), hi): ReLU (slope 0), PReLU (alpha), none (1), ReLU6 (hi = 6); RELU: plain ReLU at compile time
template <bool RELU>
__device__ __forceinline__ df32x4 mrow_act(const df32x4 v, const float4& sl, const float hi) {
    if (RELU) return df32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
    return df32x4{fminf(fmaxf(v.x, 0.f) + sl.x * fminf(v.x, 0.f), hi), fminf(fmaxf(v.y, 0.f) + sl.y * fminf(v.y, 0.f), hi),
                  fminf(fmaxf(v.z, 0.f) + sl.z * fminf(v.z, 0.f), hi), fminf(fmaxf(v.w, 0.f) + sl.w * fminf(v.w, 0.f), hi)};
}
template <bool RELU>
__device__ __forceinline__ float4 mrow_slope(const float* slope) {
    return RELU ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(slope);
}
// One output row: activation, then one 16-byte store per lane and tile.  dst: the row (wave-uniform); ooff: bytes to this lane's pixel
// and channels of tile (0, 0), CO channels per pixel; slope: this lane's (+ 4 kq).  Of a W-pixel row's last tile only pixels < W are stored.
template <bool RELU, int CO, int W, int MT, int WT>
__device__ __forceinline__ void mrow_store_row(const df32x4 (&D)[MT][WT], gchar* dst, const unsigned ooff, const float* slope, const float hi, const int p) {
    asm volatile("" : "+s"(dst));
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const float4 sl = mrow_slope<RELU>(slope + 16 * mt);
#pragma unroll
        for (int nt = 0; nt < WT; nt++) {
            const df32x4 v = mrow_act<RELU>(D[mt][nt], sl, hi);
            if (16 * (nt + 1) <= W || 16 * nt + p < W) *(gf32x4*)(dst + ooff + (unsigned)((16 * nt * CO + 16 * mt) * 4)) = v;
        }
    }
}
// The row of the intermediate tensor `a` (CM channels, zeros outside the frame: the next depthwise conv's padding) -> its row image
// (awr: this lane's centre pixel, D layout, pixel stride PSA)
template <bool RELU, int CM, int PSA, int MT, int WT>
__device__ __forceinline__ void mrow_store_a(const df32x4 (&D)[MT][WT], float* awr, const float* slope, const float hi, const bool inside, const int kq) {
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const float4 sl = mrow_slope<RELU>(slope + 16 * mt);
        if (16 * mt + 4 * kq < CM) {
#pragma unroll
            for (int nt = 0; nt < WT; nt++) {
                df32x4 v = mrow_act<RELU>(D[mt][nt], sl, hi);
                if (!inside) v = df32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<float4*>(awr + 16 * nt * PSA + 16 * mt) = make_float4(v.x, v.y, v.z, v.w);
            }
        }
    }
}

// vmcnt bookkeeping: vector-memory operations retire in issue order.  A step's operations: the stores of its output row (NST), then the
// DMA of the row two steps ahead (NLD).  "Row r has landed" = at most what was issued behind its DMA is outstanding: the previous step's
// stores (st: it had some) and DMA (dm: it had one).
template <int NST, int NLD>
__device__ __forceinline__ void mrow_wait(const bool st, const bool dm) {
    if (st && dm) wait_vm<NST + NLD>();
    else if (dm) wait_vm<NLD>();
    else if (st) wait_vm<NST>();
    else wait_vm<0>();
}

// The nine taps of a k-step as scalars (from three float4s, see dtaps_from); tap[ks] <- this lane's taps, resident in registers
__device__ __forceinline__ void mrow_taps9(const float4* tp, float (&w)[9]) {
    const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
    w[0] = t0.x; w[1] = t0.y; w[2] = t0.z; w[3] = t0.w; w[4] = t1.x; w[5] = t1.y; w[6] = t1.z; w[7] = t1.w; w[8] = t2.x;
}
template <int CK>
__device__ __forceinline__ void mrow_load_taps9(const float4* tp, float (&tap)[CK][9]) {
#pragma unroll
    for (int ks = 0; ks < CK; ks++) mrow_taps9(tp + ks * 12, tap[ks]);
#pragma unroll
    for (int ks = 0; ks < CK; ks++)
#pragma unroll
        for (int t = 0; t < 9; t++) asm volatile("" : "+v"(tap[ks][t]));
}

// ---- host side: the pieces of a constants blob, and the launch

// A operands [CK][MT][64] of v_mfma_f32_16x16x4_f32 for (k-step ks, output tile mt): lane l holds W[16 mt + l % 16][4 ks + l / 16]
// (w_pw [Co][4 CK]; rows >= Co are left as they are: zero)
inline void mrow_pack_a(float* dst, const float* w_pw, int CK, int MT, int Co) {
    for (int ks = 0; ks < CK; ks++)
        for (int mt = 0; mt < MT; mt++)
            for (int l = 0; l < 64; l++) {
                const int o = 16 * mt + (l & 15);
                if (o < Co) dst[(ks * MT + mt) * 64 + l] = w_pw[(size_t)o * 4 * CK + 4 * ks + (l >> 4)];
            }
}
// taps [ks][kq][12]: the nine taps of channel 4 ks + kq (three float4 loads per k-step); w_dw [3][3][4 CK]
inline void mrow_pack_taps(float* dst, const float* w_dw, int CK) {
    for (int ks = 0; ks < CK; ks++)
        for (int kq = 0; kq < 4; kq++)
            for (int t = 0; t < 9; t++) dst[(ks * 4 + kq) * 12 + t] = w_dw[t * 4 * CK + 4 * ks + kq];
}
// PW(dw + b_dw) + b_pw = PW(dw) + (W b_dw + b_pw): the depthwise bias (or null) is folded into the pointwise bias; slopes of the activation
inline void mrow_pack_bias(float* dst_bias, float* dst_slope, int Co, int C, const float* w_pw, const float* b_dw, const float* bias, const float* alpha, int act) {
    for (int c = 0; c < Co; c++) {
        double acc = bias ? bias[c] : 0.0;
        if (b_dw)
            for (int k = 0; k < C; k++) acc += (double)w_pw[(size_t)c * C + k] * b_dw[k];
        dst_bias[c] = (float)acc;
        dst_slope[c] = act == ACT_PRELU ? alpha[c] : (act == ACT_NONE ? 1.f : 0.f);
    }
}
// the RELU instantiation or the general one, with the whole LDS
template <class A>
inline int mrow_launch(void (*k_relu)(A), void (*k_any)(A), bool relu, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const A& args) {
    void (*kern)(A) = relu ? k_relu : k_any;
    return launch_full_lds(kern, grid, block, lds_bytes, s, args);
}

}  // namespace

}  // namespace mi
