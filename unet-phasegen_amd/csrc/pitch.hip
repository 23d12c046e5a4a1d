// pitch.hip -- a fundamental-frequency tracker (pg_pitch_track): YIN (de Cheveigne and Kawahara 2002) per frame, the measuring half
// of a pitch correction (phasegen/track.py, detect_pitch, PitchCurve.correcting, autotune).  The reference has no counterpart;
// include/phasegen.h holds the contract: every operation a separate IEEE float32 operation (-ffp-contract=off), the chain over j of
// the difference function ascending, the running sum ascending.
//
// Kernel.  One workgroup of 256 threads takes up to PT_FRAMES = 4 consecutive frames of one row and stages their common span of
// (frames - 1) hop + W + tau_max samples in LDS once (zeros past the row's end; the host takes fewer frames per workgroup when the
// span would pass PT_SPAN_MAX floats, so a long hop costs nothing).  The parallelism of a frame is its lags: a lane owns PT_R = 5
// CONSECUTIVE lags tau0 .. tau0 + 4 and walks j in steps of PT_U = 8 with a register window x[j + tau0 .. j + tau0 + 11], so eight
// steps of five chains cost 8 broadcast reads of x_j and 12 neighbour reads for 40 sub / mul / add triples.  Neighbouring lanes'
// windows begin 5 floats apart: 5 is odd, so the 32 lanes of a read group fall into 32 different banks.  The default 320 lags are 64
// lanes -- one wave per frame, four frames per workgroup, no lane idle; tau_max = 1024 takes 205 lanes (four waves, padded to whole
// waves so that a wave never straddles two frames and x_j is one broadcast).  d(tau) goes to LDS.
// Then wave g finishes frame g: lane 0 runs the serial chain S(tau) = S(tau - 1) + d(tau) out of LDS (unrolled by 8, the loads ahead
// of the adds; a tenth of the frame's time, hidden by the other resident workgroups), every lane normalises its share of cm(tau) in
// place, and the two searches of the pick are min-reductions over (index) and (value, index) by shuffles.  Exact comparisons only,
// so the reduction order cannot show.  Lane 0 writes the two results with plain stores.  No atomics, no global scratch, no state;
// one launch on the caller's stream.  LDS: span + 2 (tau_max + 1) floats per frame: 18.7 KB at 1024 / 16..320 / 256 -- eight
// workgroups per CU.
// What bounds it: three dependent-free VALU operations per (j, tau) -- 3 W tau_max per frame -- at half a read per triple.
// Measurements in DESIGN.md section 4.21.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_FRAMES = PT_THREADS / 64;   // frames per workgroup at most: wave g finishes frame g
constexpr int PT_R = 5;                      // consecutive lags per lane (odd: neighbouring windows fall into different banks)
constexpr int PT_U = 8;                      // steps of j per register window
constexpr int PT_SPAN_MAX = 6144;            // floats of LDS the staged span may take
constexpr int PT_W_MIN = 4, PT_W_MAX = 2048, PT_TAU_MIN = 2, PT_TAU_MAX = 1024;

struct PtKernelArgs {
    const float* x; float* period; float* ap;
    long x_stride, out_stride;
    int n_in, frames, hop, W, tau_min, tau_max;
    int per_wg, groups, span;                // frames per workgroup, workgroups per row, floats of the span of per_wg frames
    float theta;
};

// d(tau0 .. tau0 + PT_R - 1) of the frame that begins at xs (LDS): the chain acc = acc + (x_j - x_{j + tau})^2 over j ascending
__device__ __forceinline__ void pt_diff(const float* xs, int tau0, int W, float (&acc)[PT_R]) {
#pragma unroll
    for (int r = 0; r < PT_R; ++r) acc[r] = 0.0f;
    const float* xw = xs + tau0;
    int j = 0;
    for (; j + PT_U <= W; j += PT_U) {
        float xj[PT_U], w[PT_U + PT_R - 1];
#pragma unroll
        for (int u = 0; u < PT_U; ++u) xj[u] = xs[j + u];
#pragma unroll
        for (int k = 0; k < PT_U + PT_R - 1; ++k) w[k] = xw[j + k];
#pragma unroll
        for (int u = 0; u < PT_U; ++u) {
#pragma unroll
            for (int r = 0; r < PT_R; ++r) {
                const float e = xj[u] - w[u + r];
                acc[r] = acc[r] + e * e;
            }
        }
    }
    for (; j < W; ++j) {
        const float xj = xs[j];
#pragma unroll
        for (int r = 0; r < PT_R; ++r) {
            const float e = xj - xw[j + r];
            acc[r] = acc[r] + e * e;
        }
    }
}

__device__ __forceinline__ int pt_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(PT_THREADS) void pitch_track_kernel(const PtKernelArgs a) {
    extern __shared__ float pt_lds[];
    const int T1 = a.tau_max + 1;
    float* span = pt_lds;                                        // a.span + PT_R floats
    float* dbuf = pt_lds + a.span + PT_R;                        // per_wg rows of T1: d, then cm in place
    float* sbuf = dbuf + a.per_wg * T1;                          // per_wg rows of T1: S
    const long sig = (long)blockIdx.x / a.groups, grp = (long)blockIdx.x - sig * a.groups;
    const int f0 = (int)grp * a.per_wg;
    const int nf = a.frames - f0 < a.per_wg ? a.frames - f0 : a.per_wg;      // frames of this workgroup, 1 .. per_wg
    const float* xr = a.x + sig * a.x_stride;
    const long s0 = (long)f0 * a.hop;
    // the span of nf frames and PT_R floats the last lanes' windows run into: a sample at or beyond n_in is +0.0 and is not read
    const int len = (nf - 1) * a.hop + a.W + a.tau_max + PT_R;
    for (int i = threadIdx.x; i < len; i += PT_THREADS) {
        const long n = s0 + i;
        span[i] = (i < len - PT_R && n < (long)a.n_in) ? xr[n] : 0.0f;
    }
    __syncthreads();
    // the difference function: blocks of PT_R lags, a frame's blocks padded to whole waves
    const int nblk = (a.tau_max + PT_R - 1) / PT_R, padded = (nblk + 63) & ~63;
    for (int it = threadIdx.x; it < nf * padded; it += PT_THREADS) {
        const int g = it / padded, blk = it - g * padded;
        if (blk < nblk) {
            const int tau0 = 1 + blk * PT_R;
            float acc[PT_R];
            pt_diff(span + g * a.hop, tau0, a.W, acc);
#pragma unroll
            for (int r = 0; r < PT_R; ++r)
                if (tau0 + r <= a.tau_max) dbuf[g * T1 + tau0 + r] = acc[r];
        }
    }
    __syncthreads();
    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool mine = g < nf;
    float* d = dbuf + (mine ? g : 0) * T1;
    float* S = sbuf + (mine ? g : 0) * T1;
    if (mine && lane == 0) {                                     // the running sum: one serial chain, ascending
        float s = 0.0f;
        S[0] = 0.0f;
        int t = 1;
        for (; t + 7 <= a.tau_max; t += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = d[t + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) { s = s + v[k]; S[t + k] = s; }
        }
        for (; t <= a.tau_max; ++t) { s = s + d[t]; S[t] = s; }
    }
    __syncthreads();
    bool finite = false;
    if (mine) {
        const float total = S[a.tau_max];
        finite = fabsf(total) < INFINITY;                        // (false for a NaN)
        if (finite) {
            for (int t = lane; t <= a.tau_max; t += 64) {
                const float st = S[t];
                d[t] = (t >= 1 && st > 0.0f) ? (d[t] * (float)t) / st : 1.0f;
            }
        }
    }
    __syncthreads();
    if (!mine) return;
    float* pr = a.period + sig * a.out_stride + (f0 + g);
    float* pa = a.ap + sig * a.out_stride + (f0 + g);
    if (!finite) {
        if (lane == 0) { *pr = __builtin_nanf(""); *pa = __builtin_nanf(""); }
        return;
    }
    const float* cm = d;
    const int hi = a.tau_max - 1;                                // A = [tau_min, hi]
    int first = 0x7fffffff;
    for (int t = a.tau_min + lane; t <= hi; t += 64)
        if (cm[t] < a.theta) { first = t; break; }
    first = pt_wave_min(first);
    int pick;
    if (first != 0x7fffffff) {                                   // the walk down: the first tau >= first at which it stops
        int stop = 0x7fffffff;
        for (int t = first + lane; t <= hi; t += 64)
            if (t == hi || !(cm[t + 1] < cm[t])) { stop = t; break; }
        pick = pt_wave_min(stop);
    } else {                                                     // the smallest tau that attains the minimum over A
        float bv = INFINITY;
        int bt = 0x7fffffff;
        for (int t = a.tau_min + lane; t <= hi; t += 64) {
            const float v = cm[t];
            if (v < bv || (v == bv && t < bt)) { bv = v; bt = t; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int ot = __shfl_xor(bt, off, 64);
            if (ov < bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; }
        }
        pick = bt;
    }
    if (lane == 0) {
        const float ca = cm[pick - 1], cb = cm[pick], cc = cm[pick + 1];
        const float den = (ca + cc) - (2.0f * cb);
        float delta = 0.0f;
        if (den > 0.0f) {
            const float q = (0.5f * (ca - cc)) / den;
            delta = q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q);
        }
        *pr = (float)pick + delta;
        *pa = cb;
    }
}

}  // namespace

extern "C" int pg_pitch_track(const pg_pitch_track_args* a, void* stream) {
    if (!a) return pg_fail(PG_ERR_NULL, "pitch_track: null args");
    if (a->n_sig <= 0 || a->n_in <= 0 || a->frames <= 0 || a->hop <= 0) return pg_fail(PG_ERR_SHAPE, "pitch_track: non-positive size");
    if (a->window < PT_W_MIN || a->window > PT_W_MAX) return pg_failf(PG_ERR_UNSUPPORTED, "pitch_track: window %d outside [4, 2048]", a->window);
    if (a->tau_min < PT_TAU_MIN || a->tau_min >= a->tau_max || a->tau_max > PT_TAU_MAX)
        return pg_failf(PG_ERR_UNSUPPORTED, "pitch_track: lags %d .. %d outside 2 <= tau_min < tau_max <= 1024", a->tau_min, a->tau_max);
    if (a->x_stride < a->n_in || a->out_stride < a->frames) return pg_fail(PG_ERR_SHAPE, "pitch_track: row stride shorter than the row");
    if (!a->x || !a->period || !a->ap) return pg_fail(PG_ERR_NULL, "pitch_track: x, period and ap required");
    PtKernelArgs k;
    k.x = a->x; k.period = a->period; k.ap = a->ap;
    k.x_stride = a->x_stride; k.out_stride = a->out_stride;
    k.n_in = a->n_in; k.frames = a->frames; k.hop = a->hop; k.W = a->window; k.tau_min = a->tau_min; k.tau_max = a->tau_max;
    k.theta = a->threshold;
    const long one = (long)a->window + a->tau_max;
    long per = 1 + ((long)PT_SPAN_MAX - one) / a->hop;           // one <= 3072 < PT_SPAN_MAX: at least 1
    per = per > PT_FRAMES ? PT_FRAMES : per;
    per = per > a->frames ? a->frames : per;
    k.per_wg = (int)per;
    k.span = (int)((per - 1) * a->hop + one);
    k.groups = (int)(((long)a->frames + per - 1) / per);
    if (k.groups > 0x7fffffff / a->n_sig) return pg_fail(PG_ERR_SHAPE, "pitch_track: n_sig * frames beyond 2^31 workgroups");
    const size_t lds = sizeof(float) * ((size_t)k.span + PT_R + 2 * (size_t)k.per_wg * (a->tau_max + 1));
    hipLaunchKernelGGL(pitch_track_kernel, dim3((unsigned)(k.groups * a->n_sig)), dim3(PT_THREADS), lds, (hipStream_t)stream, k);
    return pg_launch_ok("pitch_track launch failed");
}
