// conv_fixup.h -- the fixup kernel of the stream-K split (conv_common.h: work decomposition), for every kernel family: add the partial
// segments of every split tile in a fixed order, then the epilogue.  Instantiated by conv_igemm.hip only (launch_fixup).
#pragma once
#include "conv_common.h"

namespace {

// One workgroup per (tile, 32 x 32 block of the wave tile): with few tiles and many segments (small-batch inference: 8 tiles split
// over 512 workgroups) one workgroup per tile would read 8 MB on its own; per block the reduction is MB * NB times wider.
//   KIND     epilogue: F, T, G, or T over phase-major rows (the stride-2 raw-window T kernels: block row bi of a wave tile is phase
//            bi & 1 of its channel block bi >> 1)
//   MB x NB  wave tile of the GEMM kernel in blocks: 4 x 2 (im2col), 2 x 4 (raw-window), 8 x 2 (one wave per SIMD); a partial tile
//            is MB * NB * 16 planes of 256 floats (store_partial)
//   WN       waves of the GEMM kernel along N: 2 -> 2 x 2 waves, 1 -> 4 x 1 (tall raw tile), 4 -> 1 x 4 (one wave per SIMD)
//   WIDE     (small-batch inference: tens of segments per tile) four workgroups per block, one per wave of the GEMM kernel; the four
//            waves of a fixup workgroup each sum every fourth segment (two segments' loads in flight per wave) and wave 0 adds the
//            four sums in order -- a fixed order, chosen by the host from (grid, tiles) alone.  8 tiles x 64 segments: 36 us ->
//            see DESIGN 4.3.
enum FixupKind { FIX_F, FIX_T, FIX_G, FIX_T_PM };
template <int KIND, int MB, int NB, int WN, bool WIDE>
__global__ __launch_bounds__(NT) void conv_fixup_kernel(const IgemmParams p, int G) {
    constexpr int WM = 4 / WN, REGS = MB * NB * 16;
    __shared__ float red[WIDE ? 3 * 16 * 64 : 1];
    const int unit = WIDE ? blockIdx.x >> 2 : blockIdx.x, q = WIDE ? threadIdx.x >> 6 : 0;
    const int tid = WIDE ? (blockIdx.x & 3) * 64 + (threadIdx.x & 63) : threadIdx.x;     // the GEMM thread whose accumulators this lane sums
    const int lane = tid & 63, wv = tid >> 6, wm = wv / WN, wn = wv % WN;
    // hybrid split: tiles below p.whole were computed whole by one workgroup each -- the grid covers the split tiles only
    const int tile = p.whole + unit / (MB * NB), blk = unit % (MB * NB), bi = blk / NB, bj = blk - bi * NB;
    const Split sp = make_split(p.tilesM * p.tilesN, p.nslab, G, p.whole);
    const int first = tile * p.nslab, last = first + p.nslab - 1;
    const int g0 = split_owner(sp, first), g1 = split_owner(sp, last);
    if (g0 == g1 && split_lo(sp, g0) <= first && split_lo(sp, g0 + 1) > last) return;   // computed whole by one workgroup
    int tm, tn;
    tile_decode(p, tile, tm, tn);
    // column tiles are p.tn_stride columns apart: the tile width, except the k = 5 wgrad's 255 (51 whole channels) of 256
    const int nt0 = p.n_lo + tn * p.tn_stride, n0 = nt0 + (wn * NB + bj) * 32;
    // a 32-column block that starts past the problem's last column holds nothing: the epilogue would write nothing, and the kernels
    // that meet many such blocks (tall raw tile, conv_h3: few-column problems) did not write it either
    if (KIND != FIX_G && n0 >= p.B * (KIND == FIX_F ? p.Ly : p.U)) return;
    AccT<1, 1> acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc.c[0][0][r] = 0.f;
#pragma unroll 2
    for (int g = g0 + q; g <= g1; g += WIDE ? 4 : 1) {
        const int slot = (split_lo(sp, g) / p.nslab == tile) ? 0 : 1;     // the range's first segment, or its last
        const float* src = p.ws + ((long)(g * 2 + slot) * REGS) * NT + tid;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc.c[0][0][r] += src[(blk * 16 + r) * NT];
    }
    if (WIDE) {         // (the returns above are uniform over the workgroup here: all four waves stand for the same GEMM wave)
        if (q) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[((q - 1) * 16 + r) * 64 + lane] = acc.c[0][0][r];
        }
        __syncthreads();
        if (q) return;
#pragma unroll
        for (int qq = 0; qq < 3; ++qq)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc.c[0][0][r] += red[(qq * 16 + r) * 64 + lane];
    }
    // the block's origin; the epilogues take it as the origin of a 1 x 1-block tile of wave (0, 0)
    const int m0 = ((tm * WM + wm) * MB + bi) * 32;
    if (KIND == FIX_F) epilogue_f<0, 1, 1>(p, acc, m0, n0, lane, 0, 0);
    else if (KIND == FIX_T_PM) epilogue_t_pm<1, 1>(p, acc, (tm * WM + wm) * MB * 16 + (bi >> 1) * 32, n0, lane, bi & 1);
    else if (KIND == FIX_T) epilogue_t<0, 1, 1>(p, acc, m0, n0, lane, 0, 0);
    else epilogue_g<0, 1, 1>(p, acc, m0, n0, lane, 0, 0, nt0 + p.tn_stride);
}

}  // namespace
