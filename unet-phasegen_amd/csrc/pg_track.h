// pg_track.h -- the rules the track kernels share (stitch.hip, spectral.hip, vocoder.hip, lock.hip, compare.hip; not part of the
// ABI).  include/phasegen.h states each of them once and promises bit-for-bit equalities between entry points that rest on them --
// pg_phase_lock with one bin equals pg_phase_vocoder, a stretch of 1 returns q(A), both joins cut a track at the same places -- so
// each is ONE piece of code here.  Everything on the device side is __forceinline__: the kernels compile to what they would with
// the text written out in place.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "pg_common.h"

// false for NaN and +-inf
__host__ __device__ __forceinline__ bool pg_finite(float v) { return fabsf(v) <= FLT_MAX; }

namespace pg_track {

// ---- The phase grid: a phase is a 32-bit unsigned fraction of a turn, so sums wrap and are exact in any order.  Each constant is
// the one double division the contract names.
constexpr double TWO_PI = 6.283185307179586;
constexpr double K = 4294967296.0 / TWO_PI;
constexpr double R = TWO_PI / 4294967296.0;

__device__ __forceinline__ uint32_t q(float x) {
    if (!(fabsf(x) <= 1048576.0f)) return 0u;               // NaN, +-inf and |x| > 2^20
    return (uint32_t)(int64_t)rint((double)x * K);
}

__device__ __forceinline__ float angle(uint32_t acc) { return (float)((double)(int32_t)acc * R); }

// ---- The time grid: output frame g (>= 0) sits at position p of the source, between the source frames
// i0 = min((int64)floor(p), F_src - 1) and i1 = min(i0 + 1, F_src - 1).  The grid is a TYPE, and every kernel that walks it is
// instantiated on both:
//   UniformGrid   p = (double)g * src_per_out: the stretched grid of pg_spec_clips, pg_phase_vocoder, pg_phase_lock(_linked).
//   MappedGrid    p = pc(pos[g]), pos a device table of doubles with one entry per output frame (the *_map entry points), and
//                 pc(p) = !(p >= 0) ? 0 : (p > 2^52 ? 2^52 : p): a NaN and a negative position count as 0, and beyond 2^52
//                 floor(p) == p.  From pc on everything is the uniform grid's arithmetic, word for word, so a table that holds
//                 (double)g * src_per_out gives the uniform grid's bits; whatever the table holds, 0 <= i0 <= i1 <= F_src - 1 and no
//                 read leaves a plane.  Positions need not be monotone: a frozen or backward table is legal.
// A kernel's argument struct holds both fields (src_per_out, pos) and Grid::of(args) picks its own.
struct UniformGrid {
    double spo;
    template <typename Args> static __device__ __forceinline__ UniformGrid of(const Args& a) { return UniformGrid{a.src_per_out}; }
    __device__ __forceinline__ double at(long g) const { return (double)g * spo; }
};

struct MappedGrid {
    const double* pos;
    template <typename Args> static __device__ __forceinline__ MappedGrid of(const Args& a) { return MappedGrid{a.pos}; }
    __device__ __forceinline__ double at(long g) const {
        const double p = pos[g];
        return !(p >= 0.0) ? 0.0 : (p > 4503599627370496.0 ? 4503599627370496.0 : p);
    }
};

template <typename Grid>
__device__ __forceinline__ long i0(const Grid& gr, long g, long F_src) {
    const double fl = floor(gr.at(g));
    return fl < (double)F_src ? (long)fl : F_src - 1;        // (also for a position beyond the int64 range)
}

__device__ __forceinline__ long i1(long i0, long F_src) { return i0 + 1 < F_src ? i0 + 1 : F_src - 1; }

// the advance into frame g is measured between i1(g - 1) and i0(g); frame 0 has none (i1p == i0)
struct Advance { long i0, i1p; };
template <typename Grid>
__device__ __forceinline__ Advance advance(const Grid& gr, long g, long F_src) {
    Advance s;
    s.i0 = i0(gr, g, F_src);
    s.i1p = g > 0 ? i1(i0(gr, g - 1, F_src), F_src) : s.i0;
    return s;
}

// ---- The two-clip crossfade join.  Clip k begins at element k step of the output row and shares its first V elements with the
// tail of clip k - 1 (2 V <= clip length: at most two clips cover an element).  Element t: k = min(t div step, n_clips - 1),
// j = t - k step; shared iff k >= 1 and j < V, and then blend(ramp[V-1-j], ramp[j], lo, hi) with hi = clip[k][j] and
// lo = clip[k-1][j + step], the lower clip's term first; every other element is clip[k][j] bit for bit.
struct Join { const float* ramp; long step, clip_stride; int n_clips, V; };
struct JoinAt { long k, j; const float* hp; };               // hp: clip[k] + j of the row whose clip 0 begins at `base`

__device__ __forceinline__ JoinAt join_locate(const Join& jn, const float* base, long t) {
    JoinAt at;
    at.k = t / jn.step;
    if (at.k > jn.n_clips - 1) at.k = jn.n_clips - 1;
    at.j = t - at.k * jn.step;
    at.hp = base + at.k * jn.clip_stride + at.j;
    return at;
}

template <typename Blend>
__device__ __forceinline__ float join_one(const Join& jn, const float* base, long t, Blend blend) {
    const JoinAt at = join_locate(jn, base, t);
    const float hi = *at.hp;
    if (at.k >= 1 && at.j < jn.V) return blend(jn.ramp[jn.V - 1 - at.j], jn.ramp[at.j], at.hp[jn.step - jn.clip_stride], hi);
    return hi;
}

// Elements t .. t + 3 as 16-byte accesses: step and V are multiples of 4 there, so the four never straddle a clip boundary or the
// end of a shared region, and the reversed ramp ramp[V-1-j-i] is the 16-byte load at V-4-j read backwards.
template <typename Blend>
__device__ __forceinline__ f32x4 join_four(const Join& jn, const float* base, long t, Blend blend) {
    const JoinAt at = join_locate(jn, base, t);
    f32x4 v = *(const f32x4*)at.hp;
    if (at.k >= 1 && at.j < jn.V) {
        const f32x4 lo = *(const f32x4*)(at.hp + (jn.step - jn.clip_stride));
        const f32x4 rb = *(const f32x4*)(jn.ramp + at.j), ra = *(const f32x4*)(jn.ramp + (jn.V - 4 - at.j));
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = blend(ra[3 - i], rb[i], lo[i], v[i]);
    }
    return v;
}

}  // namespace pg_track

// ---- Host side of a streaming launch
inline bool pg_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Units are walked grid-stride by at most 8 workgroups per CU, and never by more than PG_STREAM_MAX_BLOCKS (256 CUs x 8), which
// also sizes pg_stitch's workspace on the host without asking a device.
constexpr int PG_STREAM_MAX_BLOCKS = 2048;
inline unsigned pg_stream_grid(long units, int threads) {
    long cap = (long)pg_cu_count() * 8; if (cap > PG_STREAM_MAX_BLOCKS) cap = PG_STREAM_MAX_BLOCKS; if (cap < 1) cap = 1;
    const long grid = (units + threads - 1) / threads;
    return (unsigned)(grid > cap ? cap : grid);
}

// ---- The host side of a stretched-plane call: pg_phase_vocoder, pg_phase_lock, pg_phase_lock_linked and their *_map twins.  Six ABI
// structs, ONE description of the call and ONE list of checks.  A reader (pg_stretch_uniform / pg_stretch_mapped) turns a struct
// into a PgStretchCall: the sizes as int64, the channel strides in elements (a mapped struct's count of rows times F_src), the
// grid (src_per_out, or the table `pos`) and the names a message has to quote.  A NULL struct reads as a call without planes, so
// the NULL row answers for it.
enum PgStretchPlanes { PG_M_OPTIONAL, PG_M_REQUIRED, PG_REFERENCE };   // vocoder: M may be NULL; lock: M; linked: (Aref, Mref), no M
struct PgStretchCall {
    PgStretchPlanes planes;
    bool mapped;                                             // the grid: `pos` (8-byte aligned, required), else src_per_out
    double src_per_out; const double* pos;
    int64_t n_ch, bins, F_src, F_out, a_stride, m_stride;
    const char *a_name, *m_name;                             // the strides as the struct names them: a_stride or a_ch_rows
    float reset_below;
    const float *A, *M, *Aref, *Mref; float* out;
};

template <PgStretchPlanes P, typename Args>
void pg_stretch_planes(PgStretchCall& c, const Args* a) {   // the fields every one of the six names alike
    c.n_ch = a->n_ch; c.bins = a->bins; c.F_src = a->F_src; c.F_out = a->F_out; c.reset_below = a->reset_below;
    c.A = a->A; c.out = a->out;
    if constexpr (P == PG_REFERENCE) { c.Aref = a->Aref; c.Mref = a->Mref; } else c.M = a->M;
}

template <PgStretchPlanes P, typename Args>
PgStretchCall pg_stretch_uniform(const Args* a) {
    PgStretchCall c = {};
    c.planes = P; c.a_name = "a_stride"; c.m_name = "m_stride";
    if (!a) return c;
    pg_stretch_planes<P>(c, a);
    c.src_per_out = a->src_per_out; c.a_stride = a->a_stride;
    if constexpr (P != PG_REFERENCE) c.m_stride = a->m_stride;
    return c;
}

template <PgStretchPlanes P, typename Args>
PgStretchCall pg_stretch_mapped(const Args* a) {
    PgStretchCall c = {};
    c.planes = P; c.mapped = true; c.a_name = "a_ch_rows"; c.m_name = "m_ch_rows";
    if (!a) return c;
    pg_stretch_planes<P>(c, a);
    c.pos = a->pos; c.a_stride = (int64_t)a->a_ch_rows * a->F_src;
    if constexpr (P != PG_REFERENCE) c.m_stride = (int64_t)a->m_ch_rows * a->F_src;
    return c;
}

// The checks, each row once, in the order that decides which error a doubly-bad call reports -- NULL, shapes, ranges, strides, 2^62,
// alignment -- and the kernel arguments every such kernel takes: k.A .. k.reset_below and the grid, with the stride of a single
// channel 0.  `op` prefixes every message; max_bins: the op's own limit.  A mapped call has no src_per_out row, and `pos` in the
// NULL and the ALIGN row; its sizes are int32, so the 2^62 rows cannot answer for it.  wide: `out` takes 16-byte stores.
template <typename KernelArgs>
int pg_stretch_check(const char* op, int max_bins, const PgStretchCall& c, KernelArgs& k, bool& wide) {
    const bool planes = c.A && (c.planes != PG_M_REQUIRED || c.M) && (c.planes != PG_REFERENCE || (c.Aref && c.Mref));
    if (!planes || !c.out || (c.mapped && !c.pos))
        return pg_failf(PG_ERR_NULL, "%s: args, A%s%s required", op, c.planes == PG_M_REQUIRED ? ", M" : c.planes == PG_REFERENCE ? ", Aref, Mref" : "",
                        c.mapped ? ", out and pos" : " and out");
    if (c.n_ch <= 0 || c.bins <= 0 || c.F_src <= 0 || c.F_out <= 0) return pg_failf(PG_ERR_SHAPE, "%s: non-positive dimension", op);
    if (c.bins > max_bins) return pg_failf(PG_ERR_SHAPE, "%s: more than %d bins", op, max_bins);
    if (!c.mapped && (!(c.src_per_out > 0.0) || !(c.src_per_out <= DBL_MAX))) return pg_failf(PG_ERR_SHAPE, "%s: src_per_out must be finite and positive", op);
    if (!(c.reset_below >= 0.0f) || !pg_finite(c.reset_below)) return pg_failf(PG_ERR_SHAPE, "%s: reset_below must be finite and not negative", op);
    if (c.F_src > INT64_MAX / 2 / c.bins) return pg_failf(PG_ERR_SHAPE, "%s: plane beyond 2^62 elements", op);
    if (c.a_stride < c.bins * c.F_src) return pg_failf(PG_ERR_SHAPE, "%s: %s shorter than a plane", op, c.a_name);
    if (c.M && c.m_stride < c.bins * c.F_src) return pg_failf(PG_ERR_SHAPE, "%s: %s shorter than a plane", op, c.m_name);
    if (c.n_ch * c.bins > INT64_MAX / 2 / c.F_out) return pg_failf(PG_ERR_SHAPE, "%s: output beyond 2^62 elements", op);
    if (((uintptr_t)c.A | (uintptr_t)c.M | (uintptr_t)c.Aref | (uintptr_t)c.Mref | (uintptr_t)c.out) & 3 || ((uintptr_t)c.pos) & 7)
        return pg_failf(PG_ERR_ALIGN, "%s: misaligned pointer", op);
    wide = (c.F_out & 3) == 0 && pg_al16(c.out);
    k.A = c.A; k.M = c.M; k.out = c.out;
    k.src_per_out = c.src_per_out; k.pos = c.pos;
    k.a_stride = c.n_ch == 1 ? 0 : c.a_stride; k.m_stride = c.n_ch == 1 ? 0 : c.m_stride;
    k.F_src = c.F_src; k.F_out = c.F_out;
    k.bins = (int)c.bins; k.reset_below = c.reset_below;
    return PG_OK;
}
