// conv_w1.h -- what the one-wave-per-SIMD kernels share (conv_raw3.hip: fp32 raw-window F / T; conv_h3.hip: bf16-resident forward):
// 256 threads = 4 waves, one workgroup per CU, each wave a 256 x 64 sub-tile of a 256 x 256 tile, its 256 accumulator registers in
// AGPRs.  Their loops place every LDS read and gather in an MFMA gap behind scheduling fences (conv_h3.hip has the reasoning), which
// takes reads hipcc cannot move and waits the loop counts itself: those pieces, the written-out epilogue and the launch live here.
#pragma once
#include "conv_common.h"

namespace {

constexpr int W1_NT = 256;                // threads per workgroup

template <int N> __device__ __forceinline__ void w1_wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit count");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}
// The fragment reads are `asm volatile`: hipcc orders plain LDS loads freely against the scheduling fences of the loops (it sank all
// eight A reads of a k-step behind its 11th MFMA).  What that costs: the compiler does not count them -- the loops wait for them
// themselves (w1_lgkm0) before the first use of a fragment set.
__device__ __forceinline__ void w1_lgkm0() { __builtin_amdgcn_s_waitcnt(0xc07f); }      // lgkmcnt(0), the other counters untouched
__device__ __forceinline__ unsigned w1_lds_addr(const float* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) float*)p;
}

// The epilogue of a whole tile: W1_EPILOGUE(CALL) runs CALL(I, J) -- the kernel's epilogue_f / _t / _t_pm call on the 32 x 32 block
// `blk` -- for the 16 blocks of `acc`, one block at a time behind scheduling fences: with all 256 accumulator registers of the wave
// tile in one epilogue hipcc moved them to VGPRs wholesale and spilled ~200 of them, through the MAIN loop as well.  Written out: a
// `#pragma unroll` nest over the 16 blocks exceeds hipcc's unroll budget, stays rolled, and indexes the accumulators dynamically,
// i.e. keeps them in scratch.  The accumulator reads are `asm` (acc_agpr, conv_common.h), which hipcc's hazard recogniser does not see: the kernel
// spells out the wait states an MFMA result needs before a VALU may read it (s_nop) once per tile segment, in front of this.
#define W1_EPI_BLOCK(I, J, CALL)                                                                         \
    {   AccT<1, 1> blk;                                                                                  \
        _Pragma("unroll") for (int q = 0; q < 16; ++q) blk.c[0][0][q] = acc_agpr(acc.c[I][J][q]);        \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        CALL(I, J);                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                               \
    }
#define W1_EPI_ROWS(I, CALL) W1_EPI_BLOCK(I, 0, CALL) W1_EPI_BLOCK(I, 1, CALL) W1_EPI_BLOCK(I + 1, 0, CALL) W1_EPI_BLOCK(I + 1, 1, CALL)
#define W1_EPILOGUE(CALL) W1_EPI_ROWS(0, CALL) W1_EPI_ROWS(2, CALL) W1_EPI_ROWS(4, CALL) W1_EPI_ROWS(6, CALL)

// launch with dynamic LDS above 64 KB (the attribute belongs to (function, current device): set on every call, nothing cached)
template <typename Kernel>
hipError_t w1_launch(Kernel kernel, int lds_bytes, const IgemmParams& p, int grid, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(W1_NT), lds_bytes, st, p);
    return hipGetLastError();
}

}  // namespace
