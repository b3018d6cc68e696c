// wave_sync.hpp — the ordering primitives of the kernels that keep loads and stores in flight across their synchronisation points: the
// wave-level hand-over and the counted vmcnt wait of the kernels that stage rows by LDS-DMA (strip, mstrip, mdblock, mwalk, ms2,
// resident) and the LDS-only workgroup barrier (those, dblock and bneck).
#pragma once

#include <hip/hip_runtime.h>

namespace mi {

namespace {

// LDS traffic between the lanes of ONE wave: the hardware executes a wave's LDS instructions in order; this only has to
// stop the compiler from moving accesses across the hand-over.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Workgroup barrier that orders LDS traffic only: a raw s_barrier behind s_waitcnt lgkmcnt(0), between compiler fences.  __syncthreads()
// would also drain vmcnt, i.e. wait for the loads (the next band's rows, a row's DMA) and the output stores that are meant to stay in flight.
// (MI_ABL_NOBAR, a timing ablation of the strip kernels' two-row forms, drops the barrier itself.)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);
#ifndef MI_ABL_NOBAR
    __builtin_amdgcn_s_barrier();
#endif
    asm volatile("" ::: "memory");
}
// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt = imm[15:14]:imm[3:0], expcnt and lgkmcnt left at their maxima)
template <int N>
__device__ __forceinline__ void wait_vm() { __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0F70); }

}  // namespace

}  // namespace mi
