// stitch.hip -- crossfaded overlap-add of equal-length clips into whole tracks (pg_stitch), with the finite check and the peak
// normalisation of utils.py:41-42 taken over the whole track instead of one clip.  Nothing in the reference does this (its demo.py
// stops at clips of `frames` columns); the arithmetic below is the contract and the tests restate it in float64.
//
// Geometry and value.  Clip k of a track (T = clip_len samples) begins at output sample k step and shares V = T - step samples with
// the next clip, 0 <= 2 V <= T; which clips cover a sample and where the crossfade reads them is pg_track.h's join (pg_phase_join
// cuts its frames by the same code), and a sample covered twice is st_blend of the two under the ramp
//     raw = (fl(a lo) + fl(b hi)) / fl(a + b)          fp32, no contraction (-ffp-contract=off), the lower clip's term first.
// step == T therefore concatenates, and all-ones clips give all ones: (a + b) / (a + b).  The output has n_out samples,
// (n_clips-1) step < n_out <= (n_clips-1) step + T: the last clip may be cut short, the others are used whole.
// Ramp.  ramp[j] = float32(sin^2(pi (j + 0.5) / (2 V))), 0 <= j < V, evaluated in double on the HOST (pg_stitch_ramp) and handed
// over as a device copy: strictly positive (2.3e-9 at V = 16384, a normal float), ramp[j] + ramp[V-1-j] within 2^-23 of 1.
// Peak / finiteness.  n_nonfinite = number of NaN / +-inf output samples of all tracks, peak = max |raw| over the FINITE samples of
// all tracks jointly (librosa.util.normalize(axis=None)); with normalize and peak > FLT_MIN, out = raw / peak.  A maximum and an
// integer count are exact in any order, so the two-stage reduction (per-workgroup partials in `workspace`, then a second launch
// whose every workgroup folds the partials for itself) does not depend on the grid.  No atomics.
//
// Kernel.  Element-wise and memory-bound: each clip sample is read once, each output written once (twice with normalize: the
// second launch scales in place).  A unit is 4 consecutive samples of one track where step, T, the three strides and the four
// pointers allow 16-byte accesses (join_four) and 1 sample otherwise (join_one); the arithmetic per sample is the same, so both
// paths give the same bits.  The last unit of a row with n_out % 4 != 0 is done sample by sample.  Units are walked grid-stride
// (pg_stream_grid, whose cap sizes the workspace on the host without asking a device).  All index arithmetic is 64-bit.
// Measurements in DESIGN.md section 4.7.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_track.h"

namespace {

constexpr int ST_THREADS = 256;

struct StPartial { float peak; int32_t bad; };

struct StKernelArgs {
    const float* clips; float* out; const float* ramp; StPartial* partial;
    float* peak; int32_t* n_nonfinite;
    long clip_stride, track_stride, out_stride, n_out, step, units_per_track, units;
    int n_clips, T, V, nparts, normalize;
};

// the blend of a sample covered twice: fp32, nothing contracted, the lower clip's term first
struct st_blend {
    __device__ __forceinline__ float operator()(float a, float b, float lo, float hi) const { return (a * lo + b * hi) / (a + b); }
};

__device__ __forceinline__ void st_note(float v, float& peak, int& bad) {
    if (pg_finite(v)) peak = fmaxf(peak, fabsf(v));
    else ++bad;
}

// block-wide maximum / sum through wave shuffles and 4 LDS slots; every thread gets the result
__device__ __forceinline__ void st_block_reduce(float& peak, int& bad) {
    __shared__ float s_peak[ST_THREADS / 64];
    __shared__ int s_bad[ST_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        peak = fmaxf(peak, __shfl_xor(peak, off, 64));
        bad += __shfl_xor(bad, off, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_peak[threadIdx.x >> 6] = peak; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    peak = 0.f; bad = 0;
#pragma unroll
    for (int i = 0; i < ST_THREADS / 64; ++i) { peak = fmaxf(peak, s_peak[i]); bad += s_bad[i]; }
}

// raw samples -> out; with a.partial, this workgroup's finite maximum and non-finite count -> partial[blockIdx.x]
template <int VEC>
__global__ __launch_bounds__(ST_THREADS) void stitch_kernel(const StKernelArgs a) {
    float peak = 0.f;
    int bad = 0;
    const pg_track::Join jn{a.ramp, a.step, a.clip_stride, a.n_clips, a.V};
    const long stride = (long)gridDim.x * ST_THREADS;
    for (long u = (long)blockIdx.x * ST_THREADS + threadIdx.x; u < a.units; u += stride) {
        const long r = u / a.units_per_track, t = (u - r * a.units_per_track) * VEC;
        const float* tr = a.clips + r * a.track_stride;
        float* op = a.out + r * a.out_stride + t;
        if (VEC == 4 && t + 4 <= a.n_out) {
            const f32x4 v = pg_track::join_four(jn, tr, t, st_blend());
            *(f32x4*)op = v;
#pragma unroll
            for (int i = 0; i < 4; ++i) st_note(v[i], peak, bad);
        } else {
            const long n = VEC == 1 ? 1 : a.n_out - t;            // (a 16-byte row's last, short unit)
            for (long i = 0; i < n; ++i) {
                const float v = pg_track::join_one(jn, tr, t + i, st_blend());
                op[i] = v;
                st_note(v, peak, bad);
            }
        }
    }
    if (a.partial) {
        st_block_reduce(peak, bad);
        if (threadIdx.x == 0) { a.partial[blockIdx.x].peak = peak; a.partial[blockIdx.x].bad = bad; }
    }
}

// second stage: every workgroup folds the partials (exact in any order), workgroup 0 publishes them, and with normalize all of
// them scale `out` in place
template <int VEC>
__global__ __launch_bounds__(ST_THREADS) void stitch_finish_kernel(const StKernelArgs a) {
    float peak = 0.f;
    int bad = 0;
    for (int i = threadIdx.x; i < a.nparts; i += ST_THREADS) { peak = fmaxf(peak, a.partial[i].peak); bad += a.partial[i].bad; }
    st_block_reduce(peak, bad);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.peak) *a.peak = peak;
        if (a.n_nonfinite) *a.n_nonfinite = bad;
    }
    if (!a.normalize || !(peak > FLT_MIN)) return;
    const long stride = (long)gridDim.x * ST_THREADS;
    for (long u = (long)blockIdx.x * ST_THREADS + threadIdx.x; u < a.units; u += stride) {
        const long r = u / a.units_per_track, t = (u - r * a.units_per_track) * VEC;
        float* op = a.out + r * a.out_stride + t;
        if (VEC == 4 && t + 4 <= a.n_out) {
            f32x4 v = *(const f32x4*)op;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] / peak;
            *(f32x4*)op = v;
        } else {
            const long n = VEC == 1 ? 1 : a.n_out - t;
            for (long i = 0; i < n; ++i) op[i] = op[i] / peak;
        }
    }
}

int st_check(const pg_stitch_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "stitch: null args");
    if (a->n_tracks <= 0 || a->n_clips <= 0 || a->clip_len <= 0 || a->step <= 0) return pg_fail(PG_ERR_SHAPE, "stitch: non-positive dimension");
    if (a->step > a->clip_len) return pg_fail(PG_ERR_SHAPE, "stitch: step beyond the clip length (clips would leave gaps)");
    if (2 * (int64_t)(a->clip_len - a->step) > a->clip_len) return pg_fail(PG_ERR_SHAPE, "stitch: overlap beyond half a clip (more than two clips per sample)");
    const int64_t lo = (int64_t)(a->n_clips - 1) * a->step;
    if (a->n_out <= lo || a->n_out > lo + a->clip_len) return pg_fail(PG_ERR_SHAPE, "stitch: n_out outside ((n_clips-1) step, (n_clips-1) step + clip_len]");
    if (a->n_out > INT64_MAX / 2 / a->n_tracks) return pg_fail(PG_ERR_SHAPE, "stitch: n_tracks * n_out beyond 2^62");
    return PG_OK;
}

}  // namespace

extern "C" int pg_stitch_ramp(float* ramp_host, int32_t overlap) {
    if (overlap < 0) return pg_fail(PG_ERR_SHAPE, "stitch_ramp: negative overlap");
    if (overlap == 0) return PG_OK;
    if (!ramp_host) return pg_fail(PG_ERR_NULL, "stitch_ramp: null buffer");
    for (int32_t j = 0; j < overlap; ++j) {
        const double s = sin(M_PI * ((double)j + 0.5) / (2.0 * (double)overlap));
        ramp_host[j] = (float)(s * s);
    }
    return PG_OK;
}

extern "C" int64_t pg_workspace_bytes_stitch(const pg_stitch_args* a) {
    if (int e = st_check(a)) return e;
    return (int64_t)PG_STREAM_MAX_BLOCKS * (int64_t)sizeof(StPartial);      // the most partials a call leaves
}

extern "C" int pg_stitch(const pg_stitch_args* a, void* stream) {
    if (int e = st_check(a)) return e;
    const int V = a->clip_len - a->step;
    if (a->clip_stride < a->clip_len) return pg_fail(PG_ERR_SHAPE, "stitch: clip_stride shorter than a clip");
    if (a->out_stride < a->n_out) return pg_fail(PG_ERR_SHAPE, "stitch: out_stride shorter than a row");
    if (!a->clips || !a->out) return pg_fail(PG_ERR_NULL, "stitch: clips and out required");
    if (V > 0 && !a->ramp) return pg_fail(PG_ERR_NULL, "stitch: ramp required when clips overlap");
    const bool reduce = a->normalize || a->peak || a->n_nonfinite;
    if (reduce && (!a->workspace || a->workspace_bytes < pg_workspace_bytes_stitch(a)))
        return pg_fail(PG_ERR_WORKSPACE, "stitch: normalize / peak / n_nonfinite need a workspace of pg_workspace_bytes_stitch() bytes");
    if (reduce && ((uintptr_t)a->workspace & 7)) return pg_fail(PG_ERR_ALIGN, "stitch: workspace must be 8-byte aligned");
    if (((uintptr_t)a->clips & 3) || ((uintptr_t)a->out & 3) || ((uintptr_t)a->ramp & 3) || ((uintptr_t)a->peak & 3) || ((uintptr_t)a->n_nonfinite & 3))
        return pg_fail(PG_ERR_ALIGN, "stitch: misaligned pointer");
    // (a stride that is never applied -- one clip, one track -- does not decide)
    const bool wide = (a->step & 3) == 0 && (a->clip_len & 3) == 0 && (a->n_clips == 1 || (a->clip_stride & 3) == 0)
                      && (a->n_tracks == 1 || ((a->track_stride & 3) == 0 && (a->out_stride & 3) == 0))
                      && pg_al16(a->clips) && pg_al16(a->out) && (V == 0 || pg_al16(a->ramp));
    StKernelArgs k;
    k.clips = a->clips; k.out = a->out; k.ramp = a->ramp; k.partial = reduce ? (StPartial*)a->workspace : nullptr;
    k.peak = a->peak; k.n_nonfinite = a->n_nonfinite;
    k.clip_stride = a->clip_stride; k.track_stride = a->n_tracks == 1 ? 0 : a->track_stride; k.out_stride = a->out_stride;
    k.n_out = a->n_out; k.step = a->step;
    k.units_per_track = wide ? (a->n_out + 3) / 4 : a->n_out;
    k.units = k.units_per_track * a->n_tracks;
    k.n_clips = a->n_clips; k.T = a->clip_len; k.V = V; k.normalize = a->normalize ? 1 : 0;
    const unsigned grid = pg_stream_grid(k.units, ST_THREADS);
    k.nparts = (int)grid;
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL(stitch_kernel<4>, dim3(grid), dim3(ST_THREADS), 0, st, k);
    else hipLaunchKernelGGL(stitch_kernel<1>, dim3(grid), dim3(ST_THREADS), 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pg_fail((int)e, "stitch launch failed");
    if (reduce) {
        const unsigned g2 = k.normalize ? grid : 1u;
        if (wide) hipLaunchKernelGGL(stitch_finish_kernel<4>, dim3(g2), dim3(ST_THREADS), 0, st, k);
        else hipLaunchKernelGGL(stitch_finish_kernel<1>, dim3(g2), dim3(ST_THREADS), 0, st, k);
        e = hipGetLastError();
        if (e != hipSuccess) return pg_fail((int)e, "stitch second-stage launch failed");
    }
    return PG_OK;
}
