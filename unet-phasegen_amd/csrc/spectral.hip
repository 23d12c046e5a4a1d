// spectral.hip -- the two streaming kernels of the spectral-domain track join (phasegen/track.py, join="spectral"): the clip windows
// of a whole-track spectrogram plane, optionally resampled along time (pg_spec_clips), and ONE phase per global frame from the
// overlapped clips' phases (pg_phase_join).  Nothing in the reference does this (its demo.py stops at clips of `frames` columns);
// the arithmetic below is the contract (include/phasegen.h states it) and tests/_spectral_ref.py restates it in float64.
//
// Geometry of both.  Clip k covers the global frames k sf .. k sf + frames - 1 of the track's frame grid, sf the frame stride between
// clips; Vf = frames - sf frames are shared with the next clip.
//
// pg_spec_clips.  Output frame f of clip k is global frame g = k sf + f; its source position p = (double)g * src_per_out and the two
// source frames i0, i1 around it are pg_track.h's time grid (the one pg_phase_vocoder and pg_phase_lock read A and M on);
// w = (float)(p - floor(p)); out = P[i0] bit for bit when w == 0, else fl(a + fl(w fl(b1 - a))) with a = P[i0], b1 = P[i1] in
// fp32, nothing contracted (-ffp-contract=off).  src_per_out == 1.0 is therefore a copy (clamped at the last source frame), and
// n_clips = 1 resamples a whole plane.  pg_spec_clips_map is the same kernel on pg_track.h's MappedGrid: p = pc(pos[g]) from a table
// of (n_clips - 1) sf + frames doubles (tests/_map_ref.py); it has the frame-by-frame path alone.
//
// pg_phase_join.  Which clips cover a global frame and where the crossfade reads them is pg_track.h's join, the code pg_stitch cuts
// its samples by; only the blend differs.  A shared frame, with a = ramp[Vf-1-j], b = ramp[j], lo = phi[k-1][j + sf], hi = phi[k][j]:
// zr = fl(fl(a cos lo) + fl(b cos hi)), zi likewise with sin, out = atan2(zi, zr); zr == zi == 0 or either not finite: out =
// (b >= a ? hi : lo).  sin / cos / atan2 are pg_fastmath.h's (pg_sincos, pg_atan2): the unit vectors blended here are the ones
// pg_istft mode 0 forms from the same angles, and ~85 VALU instructions per SHARED frame keep the kernel under its memory time
// (libm's: ~300).
//
// Kernels.  Element-wise and memory-bound, no LDS.  A unit is 4 consecutive frames of one (clip or channel, bin) row, one thread per
// unit; units are walked grid-stride (pg_stream_grid).  Where sf, frames, the row lengths, the strides and the pointers allow (and,
// for pg_spec_clips, src_per_out == 1.0) a unit moves as 16-byte accesses: sf and Vf are then multiples of 4, so a unit never
// straddles a clip boundary, the end of a shared region or the end of the source plane.  Otherwise the same unit is done frame by
// frame with the same per-frame arithmetic: both paths give the same bits.  All index arithmetic is 64-bit.  Measurements:
// DESIGN.md section 4.10.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_track.h"
#include "pg_fastmath.h"

namespace {

namespace tk = pg_track;
constexpr int SP_THREADS = 256;

struct ScKernelArgs {
    const float* P; float* out;
    double src_per_out; const double* pos;                        // the time grid (pg_track.h): Grid::of(args) takes its own
    long p_stride, F_src, sf, units_per_row, units;
    int n_ch, bins, frames;
};

// one output frame: global frame g of the source row `row`
template <typename Grid>
__device__ __forceinline__ float sc_one(const float* row, long g, const Grid& grid, long F_src) {
    const double p = grid.at(g);
    const long i0 = tk::i0(grid, g, F_src), i1 = tk::i1(i0, F_src);
    const float w = (float)(p - floor(p));
    const float a = row[i0];
    if (w == 0.0f) return a;
    const float d = row[i1] - a;
    const float m = w * d;
    return a + m;
}

template <typename Grid, bool VEC>
__global__ __launch_bounds__(SP_THREADS) void spec_clips_kernel(const ScKernelArgs a) {
    const Grid grid = Grid::of(a);
    const long stride = (long)gridDim.x * SP_THREADS;
    for (long u = (long)blockIdx.x * SP_THREADS + threadIdx.x; u < a.units; u += stride) {
        const long r = u / a.units_per_row, f0 = (u - r * a.units_per_row) * 4;         // r = (k n_ch + c) bins + b
        const long kc = r / a.bins, b = r - kc * a.bins, k = kc / a.n_ch, c = kc - k * a.n_ch;
        const float* row = a.P + c * a.p_stride + b * a.F_src;
        float* op = a.out + r * a.frames + f0;
        const long g = k * a.sf + f0;
        if (VEC) {                                                // rate 1: g and F_src are multiples of 4
            f32x4 v;
            if (g + 4 <= a.F_src) v = *(const f32x4*)(row + g);
            else { const float e = row[a.F_src - 1]; v = f32x4{e, e, e, e}; }
            *(f32x4*)op = v;
        } else {
            const int n = a.frames - f0 < 4 ? (int)(a.frames - f0) : 4;
            for (int i = 0; i < n; ++i) op[i] = sc_one(row, g + i, grid, a.F_src);
        }
    }
}

struct PjKernelArgs {
    const float* phi; float* out; const float* ramp;
    long clip_stride, ch_stride, row_pitch, F_out, sf, units_per_row, units;
    int n_clips, bins, Vf;
};

// the blend of a shared frame: the weighted circular mean of its two phases, the lower clip's term first
struct pj_blend {
    __device__ __forceinline__ float operator()(float a, float b, float lo, float hi) const {
        float sl, cl, sh, ch;
        pg_sincos(lo, sl, cl);
        pg_sincos(hi, sh, ch);
        const float zr = a * cl + b * ch, zi = a * sl + b * sh;
        if (!(pg_finite(zr) && pg_finite(zi)) || (zr == 0.0f && zi == 0.0f)) return b >= a ? hi : lo;
        return pg_atan2(zi, zr);
    }
};

template <bool VEC>
__global__ __launch_bounds__(SP_THREADS) void phase_join_kernel(const PjKernelArgs a) {
    const tk::Join jn{a.ramp, a.sf, a.clip_stride, a.n_clips, a.Vf};
    const long stride = (long)gridDim.x * SP_THREADS;
    for (long u = (long)blockIdx.x * SP_THREADS + threadIdx.x; u < a.units; u += stride) {
        const long r = u / a.units_per_row, g = (u - r * a.units_per_row) * 4;          // r = c bins + b
        const long c = r / a.bins, b = r - c * a.bins;
        const float* rp = a.phi + c * a.ch_stride + b * a.row_pitch;
        float* op = a.out + r * a.F_out + g;
        if (VEC) {                                                // sf, Vf, F_out are multiples of 4
            *(f32x4*)op = tk::join_four(jn, rp, g, pj_blend());
        } else {
            const int n = a.F_out - g < 4 ? (int)(a.F_out - g) : 4;
            for (int i = 0; i < n; ++i) op[i] = tk::join_one(jn, rp, g + i, pj_blend());
        }
    }
}

// What the two ABI structs of pg_spec_clips say differently: the grid, and the channel stride (in elements) under its own name.
struct ScGrid { double src_per_out; const double* pos; int64_t p_stride; const char* p_name; };
ScGrid sc_grid(const pg_spec_clips_args& a) { return ScGrid{a.src_per_out, nullptr, a.p_stride, "p_stride"}; }
ScGrid sc_grid(const pg_spec_clips_map_args& a) { return ScGrid{0.0, a.pos, (int64_t)a.p_ch_rows * a.F_src, "p_ch_rows"}; }

// The checks of pg_spec_clips and pg_spec_clips_map, each row once, and the kernel's arguments.  MAPPED: no src_per_out row, `pos` in
// the NULL and the ALIGN row (8 bytes), and never the 16-byte path, which is rate 1's.
template <bool MAPPED, typename Args>
int sc_plan(const char* op, const Args* a, ScKernelArgs& k, bool& wide) {
    if (!a || !a->P || !a->out || (MAPPED && !sc_grid(*a).pos)) return pg_failf(PG_ERR_NULL, "%s: args, P%s required", op, MAPPED ? ", out and pos" : " and out");
    const ScGrid g = sc_grid(*a);
    if (a->n_clips <= 0 || a->n_ch <= 0 || a->bins <= 0 || a->frames <= 0 || a->F_src <= 0) return pg_failf(PG_ERR_SHAPE, "%s: non-positive dimension", op);
    if (a->sf < 1) return pg_failf(PG_ERR_SHAPE, "%s: sf must be at least 1", op);
    if (!MAPPED && (!(g.src_per_out > 0.0) || !(g.src_per_out <= 1.7976931348623157e308))) return pg_failf(PG_ERR_SHAPE, "%s: src_per_out must be finite and positive", op);
    if (g.p_stride < (int64_t)a->bins * a->F_src) return pg_failf(PG_ERR_SHAPE, "%s: %s shorter than a plane", op, g.p_name);
    const int64_t rows = (int64_t)a->n_clips * a->n_ch * a->bins;
    if (rows > INT64_MAX / 2 / a->frames) return pg_failf(PG_ERR_SHAPE, "%s: output beyond 2^62 elements", op);
    if ((((uintptr_t)a->P) & 3) || (((uintptr_t)a->out) & 3) || (((uintptr_t)g.pos) & 7)) return pg_failf(PG_ERR_ALIGN, "%s: misaligned pointer", op);
    // (a stride that is never applied -- one channel -- does not decide)
    wide = !MAPPED && g.src_per_out == 1.0 && (a->sf & 3) == 0 && (a->frames & 3) == 0 && (a->F_src & 3) == 0
           && (a->n_ch == 1 || (g.p_stride & 3) == 0) && pg_al16(a->P) && pg_al16(a->out);
    k.P = a->P; k.out = a->out; k.src_per_out = g.src_per_out; k.pos = g.pos;
    k.p_stride = a->n_ch == 1 ? 0 : g.p_stride; k.F_src = a->F_src; k.sf = a->sf;
    k.units_per_row = ((long)a->frames + 3) / 4; k.units = k.units_per_row * rows;
    k.n_ch = a->n_ch; k.bins = a->bins; k.frames = a->frames;
    return PG_OK;
}

template <typename Kernel>
int sc_launch(const char* op, Kernel kernel, const ScKernelArgs& k, void* stream) {
    hipLaunchKernelGGL(kernel, dim3(pg_stream_grid(k.units, SP_THREADS)), dim3(SP_THREADS), 0, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PG_OK : pg_failf((int)e, "%s launch failed", op);
}

}  // namespace

extern "C" int pg_spec_clips(const pg_spec_clips_args* a, void* stream) {
    ScKernelArgs k;
    bool wide;
    if (int e = sc_plan<false>("spec_clips", a, k, wide)) return e;
    if (wide) return sc_launch("spec_clips", spec_clips_kernel<tk::UniformGrid, true>, k, stream);
    return sc_launch("spec_clips", spec_clips_kernel<tk::UniformGrid, false>, k, stream);
}

// pg_spec_clips over the positions of a table (tk::MappedGrid): the frame-by-frame path alone
extern "C" int pg_spec_clips_map(const pg_spec_clips_map_args* a, void* stream) {
    ScKernelArgs k;
    bool wide;
    if (int e = sc_plan<true>("spec_clips_map", a, k, wide)) return e;
    return sc_launch("spec_clips_map", spec_clips_kernel<tk::MappedGrid, false>, k, stream);
}

extern "C" int pg_phase_join(const pg_phase_join_args* a, void* stream) {
    if (!a || !a->phi || !a->out || !a->ramp) return pg_fail(PG_ERR_NULL, "phase_join: args, phi, out and ramp required");
    if (a->n_clips <= 0 || a->n_ch <= 0 || a->bins <= 0 || a->frames <= 0) return pg_fail(PG_ERR_SHAPE, "phase_join: non-positive dimension");
    if (a->sf < 1 || a->sf >= a->frames) return pg_fail(PG_ERR_SHAPE, "phase_join: need 1 <= sf < frames (neighbouring clips share Vf = frames - sf >= 1 frames)");
    const int Vf = a->frames - a->sf;
    if (2 * (int64_t)Vf > a->frames) return pg_fail(PG_ERR_SHAPE, "phase_join: overlap beyond half a clip (more than two clips per frame)");
    // (a stride that is never applied -- one bin, one channel, one clip -- is not checked)
    const int64_t pitch = a->bins == 1 ? a->frames : a->row_pitch, plane = (int64_t)(a->bins - 1) * pitch + a->frames;
    if (pitch < a->frames) return pg_fail(PG_ERR_SHAPE, "phase_join: row_pitch shorter than a row");
    if (a->n_ch > 1 && a->ch_stride < plane) return pg_fail(PG_ERR_SHAPE, "phase_join: ch_stride shorter than a channel");
    if (a->n_clips > 1 && a->clip_stride < plane) return pg_fail(PG_ERR_SHAPE, "phase_join: clip_stride shorter than a clip");
    const int64_t F_out = (int64_t)(a->n_clips - 1) * a->sf + a->frames, rows = (int64_t)a->n_ch * a->bins;
    if (rows > INT64_MAX / 2 / F_out) return pg_fail(PG_ERR_SHAPE, "phase_join: output beyond 2^62 elements");
    if ((((uintptr_t)a->phi) & 3) || (((uintptr_t)a->out) & 3) || (((uintptr_t)a->ramp) & 3)) return pg_fail(PG_ERR_ALIGN, "phase_join: misaligned pointer");
    const bool wide = (a->sf & 3) == 0 && (a->frames & 3) == 0 && (a->n_clips == 1 || (a->clip_stride & 3) == 0)
                      && (a->n_ch == 1 || (a->ch_stride & 3) == 0) && (a->bins == 1 || (a->row_pitch & 3) == 0)
                      && pg_al16(a->phi) && pg_al16(a->out) && pg_al16(a->ramp);
    PjKernelArgs k;
    k.phi = a->phi; k.out = a->out; k.ramp = a->ramp;
    k.clip_stride = a->clip_stride; k.ch_stride = a->n_ch == 1 ? 0 : a->ch_stride; k.row_pitch = a->bins == 1 ? 0 : a->row_pitch;
    k.F_out = F_out; k.sf = a->sf;
    k.units_per_row = (F_out + 3) / 4; k.units = k.units_per_row * rows;
    k.n_clips = a->n_clips; k.bins = a->bins; k.Vf = Vf;
    const unsigned grid = pg_stream_grid(k.units, SP_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL(phase_join_kernel<true>, dim3(grid), dim3(SP_THREADS), 0, st, k);
    else hipLaunchKernelGGL(phase_join_kernel<false>, dim3(grid), dim3(SP_THREADS), 0, st, k);
    return pg_launch_ok("phase_join launch failed");
}
