// varispeed.hip -- a band-limited resampler whose read position and bandwidth vary along the output (pg_varispeed): the playback
// half of a pitch curve (phasegen/track.py, PitchCurve), where pg_resample takes one (up, down) for the whole row.  The reference
// has no counterpart; include/phasegen.h holds the contract.
//
// Filter.  Smith's table-driven band-limited interpolation: the Kaiser-windowed sinc h of pg_resample (pg_kaiser.h), sampled L times
// per zero crossing on the HOST in double (pg_varispeed_table: pairs (h_i, h_{i+1} - h_i)) and interpolated linearly on the device.
// Output t reads the source at p = P_j + q delta inside block j = t div step (positions are linear between the block ends of `pos`)
// with the bandwidth s = sc(scale[j]):  y[t] = sum over n in [0, n_in) with u = |p - n| s L < Z L of  s (h_i + eta d_i) x[n].
//
// Kernel.  One workgroup of 256 threads takes VS_TILE = 1024 consecutive outputs of one row, lane i the outputs i, i + 256, ...
// The workgroup folds the clamped block ends its tile touches into (min, max): positions are linear inside a block, so every p of
// the tile lies between them.  If [min - Z / 0.25 .. max + Z / 0.25] cut to the row fits VS_WIN_MAX floats the window is staged in
// LDS once and every tap is an LDS read; otherwise (a jump, a backward step, a hostile table) the taps come straight from global
// memory.  Either way an output runs vs_sum over [n_lo, n_hi], the integers within reach of p cut to [0, n_in): ONE chain
// acc = acc + (s (h_i + eta d_i)) x[n], n ascending from acc = 0, every operation a separate IEEE operation (-ffp-contract=off), a
// tap with u >= Z L skipped by a select -- so the result is a function of the set of taps alone, and both paths give the same
// bits.  An output whose [n_lo, n_hi] is not inside the staged window (it cannot happen by the reasoning above; the test costs two
// compares) takes the global path by itself.  Nothing is read outside [0, n_in) of a row, whatever the tables hold: the loop bounds
// are cut to the row and the staging loop reads in-row indices only; LDS words outside the cut window are never read.
// The filter pair (h_i, d_i) is ONE 8-byte load per tap from global memory (256 KB at Z = 64, L = 512: it stays in L2, as
// pg_resample's bank does).  VS_KB taps are fetched together, so a lane waits one latency per group and not per tap.  No atomics,
// no workspace, one launch on the caller's stream.
// What bounds it: per tap a lane does two double operations (p - n, the product with s L), a floor, three conversions, the 8-byte
// table load and four fp32 operations; consecutive taps of a lane are s L table entries (1 - 4 KB) apart and neighbouring lanes
// rate s L entries, so a wave's table load touches up to 64 cache lines: the address path of the vector memory unit, not the bytes.
// Measurements in DESIGN.md section 4.20.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_kaiser.h"

namespace {

constexpr int VS_THREADS = 256;
constexpr int VS_TILE = 1024;       // outputs per workgroup
constexpr int VS_WIN_MAX = 12288;   // floats of LDS the staged window may take (48 KB: three workgroups per CU, as pg_resample)
constexpr int VS_KB = 4;            // taps whose table pairs a lane fetches together
constexpr int VS_Z_MAX = 64, VS_L_MAX = 512, VS_STEP_MAX = 4096;

bool vs_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int vs_check_filter(int32_t zeros, int32_t per_zero, const char* who) {
    if (zeros < 1 || zeros > VS_Z_MAX) return pg_failf(PG_ERR_UNSUPPORTED, "%s: zeros %d outside [1, 64]", who, zeros);
    if (per_zero > VS_L_MAX || !vs_pow2(per_zero)) return pg_failf(PG_ERR_UNSUPPORTED, "%s: per_zero %d is not a power of two in [1, 512]", who, per_zero);
    return PG_OK;
}

struct VsKernelArgs {
    const double* pos; const float* scale; const float2* table; const float* x; float* y;
    long x_stride, y_stride;
    int n_in, n_out, step, shift, tiles, Z, L;                    // shift = log2(step)
};

// the mapped kernels' clamp (include/phasegen.h): NaN and negative positions count as 0, anything beyond 2^52 as 2^52
__device__ __forceinline__ double vs_pc(double p) { return !(p >= 0.0) ? 0.0 : (p > 4503599627370496.0 ? 4503599627370496.0 : p); }
__device__ __forceinline__ float vs_sc(float v) { return !(v >= 0.25f) ? 0.25f : (v > 1.0f ? 1.0f : v); }

// The chain of one output over the taps n_lo .. n_hi (inside [0, n_in); LDS: inside the staged window that begins at w_lo).
template <bool LDS>
__device__ __forceinline__ float vs_sum(const float* src, long w_lo, const float2* __restrict__ table, double p, double sL, double ZL, float s,
                                        long n_lo, long n_hi) {
    float acc = 0.0f;
    long n = n_lo;
    for (; n + VS_KB - 1 <= n_hi; n += VS_KB) {
        float2 hd[VS_KB];
        float eta[VS_KB], xv[VS_KB];
        bool in[VS_KB];
#pragma unroll
        for (int k = 0; k < VS_KB; ++k) {
            const double u = fabs(p - (double)(n + k)) * sL;
            const double fl = floor(u);
            in[k] = u < ZL;
            eta[k] = (float)(u - fl);
            hd[k] = table[in[k] ? (int)fl : 0];
            xv[k] = LDS ? src[n + k - w_lo] : src[n + k];
        }
#pragma unroll
        for (int k = 0; k < VS_KB; ++k) {
            const float w = (hd[k].x + eta[k] * hd[k].y) * s;
            const float next = acc + w * xv[k];
            acc = in[k] ? next : acc;
        }
    }
    for (; n <= n_hi; ++n) {
        const double u = fabs(p - (double)n) * sL;
        const double fl = floor(u);
        const bool in = u < ZL;
        const float eta = (float)(u - fl);
        const float2 hd = table[in ? (int)fl : 0];
        const float xv = LDS ? src[n - w_lo] : src[n];
        const float w = (hd.x + eta * hd.y) * s;
        const float next = acc + w * xv;
        acc = in ? next : acc;
    }
    return acc;
}

__global__ __launch_bounds__(VS_THREADS) void varispeed_kernel(const VsKernelArgs a) {
    __shared__ float vs_win[VS_WIN_MAX];
    __shared__ double vs_red[2][VS_THREADS / 64];
    const long sig = (long)blockIdx.x / a.tiles, tile = (long)blockIdx.x - sig * a.tiles;
    const long t0 = tile * VS_TILE;
    const long t_last = (t0 + VS_TILE < (long)a.n_out ? t0 + VS_TILE : (long)a.n_out) - 1;
    const float* xr = a.x + sig * a.x_stride;
    float* yr = a.y + sig * a.y_stride;
    // the tile's source span: the extremes of the clamped block ends j0 .. j1 + 1 (j1 + 1 <= nb: the table holds nb + 1 entries)
    const long j0 = t0 >> a.shift, j1 = t_last >> a.shift;
    double lo = 4503599627370496.0, hi = 0.0;
    for (long j = j0 + threadIdx.x; j <= j1 + 1; j += VS_THREADS) {
        const double P = vs_pc(a.pos[j]);
        lo = P < lo ? P : lo;
        hi = P > hi ? P : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) { vs_red[0][threadIdx.x >> 6] = lo; vs_red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < VS_THREADS / 64; ++w) {
        lo = vs_red[0][w] < lo ? vs_red[0][w] : lo;
        hi = vs_red[1][w] > hi ? vs_red[1][w] : hi;
    }
    // the widest reach is Z / 0.25; two samples of margin for the rounding of p and of the reach (0 <= lo <= hi <= 2^52: the
    // conversions are exact enough and cannot overflow)
    const long reach = 4L * a.Z + 2;
    long w_lo = (long)floor(lo) - reach, w_hi = (long)floor(hi) + 1 + reach;
    w_lo = w_lo < 0 ? 0 : w_lo;
    w_hi = w_hi > (long)a.n_in - 1 ? (long)a.n_in - 1 : w_hi;
    const bool staged = w_hi - w_lo + 1 <= (long)VS_WIN_MAX;      // (an empty window, w_hi < w_lo, is staged: no tap is in the row)
    if (staged) {
        for (long i = threadIdx.x; i <= w_hi - w_lo; i += VS_THREADS) vs_win[i] = xr[w_lo + i];
    }
    __syncthreads();
    const double ZL = (double)(a.Z * a.L), inv_step = 1.0 / (double)a.step;
#pragma unroll 1
    for (int r = 0; r < VS_TILE / VS_THREADS; ++r) {
        const long t = t0 + threadIdx.x + (long)r * VS_THREADS;
        if (t > t_last) break;
        const long j = t >> a.shift, q = t - (j << a.shift);
        const double P0 = vs_pc(a.pos[j]), P1 = vs_pc(a.pos[j + 1]);
        const double delta = (P1 - P0) * inv_step;
        const double p = P0 + (double)q * delta;
        const float s = vs_sc(a.scale[j]);
        const double sL = (double)s * (double)a.L;
        // every n with |p - n| s L < Z L lies within W = Z / s of p; one sample of margin for the rounding of W and of the test
        const double W = (double)a.Z / (double)s;
        long n_lo = (long)floor(p - W) - 1, n_hi = (long)floor(p + W) + 2;
        n_lo = n_lo < 0 ? 0 : n_lo;
        n_hi = n_hi > (long)a.n_in - 1 ? (long)a.n_in - 1 : n_hi;
        float acc;
        if (staged && n_lo >= w_lo && n_hi <= w_hi) acc = vs_sum<true>(vs_win, w_lo, a.table, p, sL, ZL, s, n_lo, n_hi);
        else acc = vs_sum<false>(xr, 0, a.table, p, sL, ZL, s, n_lo, n_hi);
        yr[t] = acc;
    }
}

}  // namespace

extern "C" int64_t pg_varispeed_table_elems(int32_t zeros, int32_t per_zero) {
    if (int e = vs_check_filter(zeros, per_zero, "varispeed_table")) return e;
    return 2 * ((int64_t)zeros * per_zero + 1);
}

extern "C" int pg_varispeed_table(float* table_host, int32_t zeros, int32_t per_zero, double beta, double rolloff) {
    if (!table_host) return pg_fail(PG_ERR_NULL, "varispeed_table: null buffer");
    if (int e = vs_check_filter(zeros, per_zero, "varispeed_table")) return e;
    if (!(beta >= 0.0 && beta <= 15.0)) return pg_fail(PG_ERR_SHAPE, "varispeed_table: beta outside [0, 15]");
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return pg_fail(PG_ERR_SHAPE, "varispeed_table: rolloff outside (0, 1]");
    const long n = (long)zeros * per_zero;
    const double i0b = rs_i0(beta);
    for (long i = 0; i <= n; ++i) table_host[2 * i] = (float)rs_h((double)i / (double)per_zero, (double)zeros, beta, rolloff, i0b);
    for (long i = 0; i < n; ++i) table_host[2 * i + 1] = table_host[2 * i + 2] - table_host[2 * i];   // on the rounded values
    table_host[2 * n + 1] = 0.0f;
    return PG_OK;
}

extern "C" int pg_varispeed(const pg_varispeed_args* a, void* stream) {
    if (!a) return pg_fail(PG_ERR_NULL, "varispeed: null args");
    if (a->n_sig <= 0 || a->n_in <= 0 || a->n_out <= 0) return pg_fail(PG_ERR_SHAPE, "varispeed: non-positive size");
    if (a->step > VS_STEP_MAX || !vs_pow2(a->step)) return pg_failf(PG_ERR_UNSUPPORTED, "varispeed: step %d is not a power of two in [1, 4096]", a->step);
    if (int e = vs_check_filter(a->zeros, a->per_zero, "varispeed")) return e;
    if (a->x_stride < a->n_in || a->y_stride < a->n_out) return pg_fail(PG_ERR_SHAPE, "varispeed: row stride shorter than the row");
    if (!a->pos || !a->scale || !a->table || !a->x || !a->y) return pg_fail(PG_ERR_NULL, "varispeed: pos, scale, table, x and y required");
    if (((uintptr_t)a->pos | (uintptr_t)a->table) & 7) return pg_fail(PG_ERR_ALIGN, "varispeed: pos and table must be 8-byte aligned");
    VsKernelArgs k;
    k.pos = a->pos; k.scale = a->scale; k.table = (const float2*)a->table; k.x = a->x; k.y = a->y;
    k.x_stride = a->x_stride; k.y_stride = a->y_stride;
    k.n_in = a->n_in; k.n_out = a->n_out; k.step = a->step; k.Z = a->zeros; k.L = a->per_zero;
    k.shift = 0;
    while ((1 << k.shift) < a->step) ++k.shift;
    k.tiles = (int)(((long)a->n_out + VS_TILE - 1) / VS_TILE);
    if (k.tiles > 0x7fffffff / a->n_sig) return pg_fail(PG_ERR_SHAPE, "varispeed: n_sig * tiles beyond 2^31");
    hipLaunchKernelGGL(varispeed_kernel, dim3((unsigned)(k.tiles * a->n_sig)), dim3(VS_THREADS), 0, (hipStream_t)stream, k);
    return pg_launch_ok("varispeed launch failed");
}
