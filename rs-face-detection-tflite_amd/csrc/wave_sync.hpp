// wave_sync.hpp — the two ordering primitives of the kernels that stage rows by LDS-DMA (strip, mstrip, mdblock, mwalk, ms2, resident).
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
// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt = imm[15:14]:imm[3:0], expcnt and lgkmcnt left at their maxima)
template <int N>
__device__ __forceinline__ void wait_vm() { __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0F70); }

}  // namespace

}  // namespace mi
