// resample.hip -- sample-rate conversion by a rational factor (pg_resample): the rate change of the reference's get_mix_chunks
// (preproc_mdb.py:105-116: librosa.load(sr=44100), then librosa.resample(44100 -> 16000)), so that ordinary 44.1 kHz audio reaches
// the model's 16 kHz without a host DSP library.
//
// Filter.  A band-limited sinc interpolator under a Kaiser window with resampy's published kaiser_best / kaiser_fast parameters
// (Z zero crossings, beta, roll-off r):  h(t) = r sinc(r t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta) for |t| <= Z, else 0.
// up / down reduced by their gcd to U / D, s = min(1, U/D), W = Z / s, H = floor(W), taps = floor(W) + ceil(W) + 1.  Output t has
// n0 = (t D) div U, p = (t D) mod U and
//     y[t] = sum_{k < taps} bank[k U + p] x[n0 - H + k],     x[n] = 0 outside [0, n_in),
//     bank[k U + p] = float32(s h(s (p/U + H - k)))          evaluated in double on the HOST (pg_resample_bank),
//     n_out = ceil(n_in U / D).
// The bank is tap-major / phase-minor.  PARITY UNPINNED (like the STFT): resampy interpolates linearly in a 512-per-crossing table
// and truncates its index step, and is not available to pin against; this is the filter it approximates.  The last sample
// t = n_out - 1 is computed (old librosa zero-pads it when resampy returns floor), and equal rates are filtered like any other
// ratio here (the Python wrapper returns its input, as librosa does).
//
// Kernel.  One workgroup of 256 threads takes a tile of consecutive outputs of one signal and stages the input window the tile
// reaches -- tile D/U + taps samples -- in LDS, zero-filled BY INDEX wherever n is outside [0, n_in): the tap loop has no
// branches and nothing is ever read from a row's stride padding or from the next row.  The tile's (n0, p) base is formed once per
// workgroup in 64 bits (t D passes 2^31 within a five-minute track); per-lane offsets stay below 2^28.
// Outputs t and t + S with S a multiple of U have the same phase and windows exactly S D / U apart, so a lane owns R = 4 such
// outputs and loads each bank value (global memory; the bank is at most 226 KB and stays in L2) once for 4 multiply-adds on 4 LDS
// reads.  The tile is 4 S outputs, lane i takes the offsets i, i + 256, ... below S; the host picks S = m U so that few lanes
// idle (S = 480 for U = 160: 15 of 16) and the window stays within RS_WIN_MAX floats.  Ratios whose smallest such tile does not
// fit (4 D + taps beyond the window budget) take the R = 1 instantiation, whose tile is free of U.
// Order.  Every output is ONE chain acc = fmaf(bank[k U + p], x[n0 - H + k], acc) with k ascending from acc = 0, whatever the
// tile, R, the number of signals or the position in the batch: results are reproducible to the bit (-ffp-contract=off; the fused
// multiply-add is written out).
// What bounds it: per 4 wave-wide multiply-adds a CU serves 4 ds_read_b32 (2 LDS cycles each when conflict-free; neighbouring
// lanes' windows begin D / U = 2.76 samples apart at 441 / 160, which puts two addresses on the busiest bank: ~4) and one bank load
// whose 64 phases are scattered over a U-float row (5 cache lines at U = 160, 14 at U = 441: the address path, not the bytes).
// Letting neighbouring lanes take outputs c apart (c D / U near an odd integer) was modelled on the host and does not lower the
// busiest bank's load below two addresses, so it is not built.  Measurements in DESIGN.md section 4.2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_kaiser.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_KB = 8;            // taps whose bank values a lane fetches together
constexpr int RS_WIN_MAX = 12288;   // floats of LDS a workgroup's input window may take (48 KB: three workgroups per CU)
constexpr int RS_S_MAX = 4096;      // same-phase spacing S <= this: per-lane offsets (4 S) * D stay far below 2^31
constexpr int RS_U_MAX = 1024, RS_TAPS_MAX = 2048;

// the reduced ratio and everything that follows from it (host; pure function of up, down, quality)
struct RsPlan {
    int U, D, Z, H, taps;
    int R, S, slots, tile, win;     // launch shape: R outputs per lane S apart, `slots` offsets per lane, tile = R S, LDS window
};

long rs_gcd(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }

int rs_window(const RsPlan& p, int tile) { return (int)(((long)p.U - 1 + (long)(tile - 1) * p.D) / p.U) + p.taps; }

int rs_plan(int32_t up, int32_t down, int32_t quality, RsPlan& p) {
    if (up <= 0 || down <= 0) return pg_fail(PG_ERR_SHAPE, "resample: non-positive rate");
    if (quality != PG_RS_KAISER_BEST && quality != PG_RS_KAISER_FAST) return pg_fail(PG_ERR_UNSUPPORTED, "resample: unknown quality");
    const long g = rs_gcd(up, down);
    const long U = up / g, D = down / g;
    const long Z = RS_FILTERS[quality].Z;
    if (U > RS_U_MAX) return pg_fail(PG_ERR_UNSUPPORTED, "resample: more than 1024 phases after reducing up / down");
    // W = Z / min(1, U / D) as an exact fraction: floor and ceil in integers
    const long fl = U >= D ? Z : (Z * D) / U, ce = U >= D ? Z : (Z * D + U - 1) / U;
    if (fl + ce + 1 > RS_TAPS_MAX) return pg_fail(PG_ERR_UNSUPPORTED, "resample: more than 2048 taps (down / up too large)");
    p.U = (int)U; p.D = (int)D; p.Z = (int)Z; p.H = (int)fl; p.taps = (int)(fl + ce + 1);
    // R = 4 outputs per lane one multiple of U apart: the first spacing S = m U that keeps >= 90 % of the lanes busy, else the best
    p.R = 0;
    double best = 0.0;
    for (long S = U; S <= RS_S_MAX; S += U) {
        if (rs_window(p, (int)(4 * S)) > RS_WIN_MAX) break;
        const long slots = (S + RS_THREADS - 1) / RS_THREADS;
        const double eff = (double)S / (double)(slots * RS_THREADS);
        if (eff > best) { best = eff; p.R = 4; p.S = (int)S; }
        if (eff >= 0.9) break;
    }
    if (!p.R) {                                                  // no same-phase tile fits: one output per lane and offset
        p.R = 1; p.S = 1024;
        while (rs_window(p, p.S) > RS_WIN_MAX) p.S >>= 1;         // (ends: taps + 2 <= 2050 fits)
    }
    p.slots = (p.S + RS_THREADS - 1) / RS_THREADS;
    p.tile = p.R * p.S;
    p.win = rs_window(p, p.tile);
    return PG_OK;
}

struct RsKernelArgs {
    const float* x; float* y; const float* bank;
    long x_stride, y_stride, n_in, n_out, tiles;
    int U, D, H, taps, S, slots, win, dstep;                     // dstep = (S / U) D: window distance of a lane's R outputs
};

template <int R>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsKernelArgs a) {
    extern __shared__ float rs_win[];
    const long sig = (long)blockIdx.x / a.tiles, tile = (long)blockIdx.x - sig * a.tiles;
    const long t0 = tile * ((long)R * a.S);
    const long base = t0 * a.D;                                   // 64-bit: once per workgroup
    const long n0_base = base / a.U;
    const int p_base = (int)(base - n0_base * a.U);
    const long n_lo = n0_base - a.H;
    const float* xr = a.x + sig * a.x_stride;
    for (int i = threadIdx.x; i < a.win; i += RS_THREADS) {
        const long n = n_lo + i;
        const bool in = n >= 0 && n < a.n_in;
        const float v = xr[in ? n : 0];                           // branch-free; the index test decides, never the padding
        rs_win[i] = in ? v : 0.0f;
    }
    __syncthreads();
    float* yr = a.y + sig * a.y_stride;
    for (int s = 0; s < a.slots; ++s) {
        const int j = (int)threadIdx.x + s * RS_THREADS;
        if (j >= a.S) break;
        const int q = p_base + j * a.D;
        const int d = q / a.U, p = q - d * a.U;
        const float* bp = a.bank + p;
        const float* w = rs_win + d;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0f;
        // RS_KB taps at a time: their bank values are fetched together, the next group's while this one is summed (one
        // latency per group, not per tap); the order of every chain stays k ascending
        int k = 0;
        float b[RS_KB];
        if (a.taps >= RS_KB) {
#pragma unroll
            for (int u = 0; u < RS_KB; ++u) b[u] = bp[u * a.U];
        }
        for (; k + RS_KB <= a.taps; k += RS_KB) {
            float bn[RS_KB];
            const bool more = k + 2 * RS_KB <= a.taps;
#pragma unroll
            for (int u = 0; u < RS_KB; ++u) bn[u] = bp[(more ? k + RS_KB + u : 0) * a.U];
#pragma unroll
            for (int u = 0; u < RS_KB; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(b[u], w[r * a.dstep + k + u], acc[r]);
            }
#pragma unroll
            for (int u = 0; u < RS_KB; ++u) b[u] = bn[u];
        }
        for (; k < a.taps; ++k) {
            const float bk = bp[k * a.U];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fmaf(bk, w[r * a.dstep + k], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long t = t0 + j + (long)r * a.S;
            if (t < a.n_out) yr[t] = acc[r];
        }
    }
}

}  // namespace

extern "C" int64_t pg_resample_out_len(int64_t n_in, int32_t up, int32_t down) {
    if (n_in <= 0) return pg_fail(PG_ERR_SHAPE, "resample: non-positive length");
    if (up <= 0 || down <= 0) return pg_fail(PG_ERR_SHAPE, "resample: non-positive rate");
    const long g = rs_gcd(up, down);
    const __int128 v = ((__int128)n_in * (up / g) + (down / g) - 1) / (down / g);
    if (v > (__int128)INT64_MAX) return pg_fail(PG_ERR_SHAPE, "resample: output length beyond 2^63");
    return (int64_t)v;
}

extern "C" int32_t pg_resample_taps(int32_t up, int32_t down, int32_t quality) {
    RsPlan p;
    if (int e = rs_plan(up, down, quality, p)) return e;
    return p.taps;
}

extern "C" int64_t pg_resample_bank_elems(int32_t up, int32_t down, int32_t quality) {
    RsPlan p;
    if (int e = rs_plan(up, down, quality, p)) return e;
    return (int64_t)p.taps * p.U;
}

extern "C" int pg_resample_bank(float* bank_host, int32_t up, int32_t down, int32_t quality) {
    RsPlan p;
    if (int e = rs_plan(up, down, quality, p)) return e;
    if (!bank_host) return pg_fail(PG_ERR_NULL, "resample_bank: null buffer");
    const RsFilter f = RS_FILTERS[quality];
    const double s = p.U >= p.D ? 1.0 : (double)p.U / (double)p.D, i0b = rs_i0(f.beta);
    const double den = (double)(p.U >= p.D ? p.U : p.D);          // s (p/U + H - k) = (p + U (H - k)) / max(U, D): exact numerator
    for (int k = 0; k < p.taps; ++k)
        for (int ph = 0; ph < p.U; ++ph) {
            const double t = (double)((long)ph + (long)p.U * (p.H - k)) / den;
            const double h = rs_h(t, (double)f.Z, f.beta, f.rolloff, i0b);
            bank_host[(long)k * p.U + ph] = (float)(s * h);
        }
    return PG_OK;
}

extern "C" int pg_resample(const pg_resample_args* a, void* stream) {
    if (!a) return pg_fail(PG_ERR_NULL, "resample: null args");
    if (a->n_signals <= 0 || a->n_in <= 0) return pg_fail(PG_ERR_SHAPE, "resample: non-positive size");
    RsPlan p;
    if (int e = rs_plan(a->up, a->down, a->quality, p)) return e;
    if (a->n_out != pg_resample_out_len(a->n_in, a->up, a->down)) return pg_fail(PG_ERR_SHAPE, "resample: n_out is not ceil(n_in up / down)");
    if (a->x_stride < a->n_in || a->y_stride < a->n_out) return pg_fail(PG_ERR_SHAPE, "resample: row stride shorter than the row");
    if (!a->x || !a->y || !a->bank) return pg_fail(PG_ERR_NULL, "resample: x, y and bank required");
    RsKernelArgs k;
    k.x = a->x; k.y = a->y; k.bank = a->bank;
    k.x_stride = a->x_stride; k.y_stride = a->y_stride; k.n_in = a->n_in; k.n_out = a->n_out;
    k.tiles = (a->n_out + p.tile - 1) / p.tile;
    if (k.tiles > 0x7fffffffL / a->n_signals) return pg_fail(PG_ERR_SHAPE, "resample: n_signals * tiles beyond 2^31");
    k.U = p.U; k.D = p.D; k.H = p.H; k.taps = p.taps; k.S = p.S; k.slots = p.slots; k.win = p.win;
    k.dstep = p.R == 4 ? (p.S / p.U) * p.D : 0;
    const dim3 grid((unsigned)(k.tiles * a->n_signals)), block(RS_THREADS);
    const size_t lds = (size_t)p.win * sizeof(float);
    if (p.R == 4) hipLaunchKernelGGL(resample_kernel<4>, grid, block, lds, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(resample_kernel<1>, grid, block, lds, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PG_OK : pg_fail((int)e, "resample launch failed");
}
