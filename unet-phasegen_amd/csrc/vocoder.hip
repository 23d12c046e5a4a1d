// vocoder.hip -- pg_phase_vocoder: the phase-vocoder phase of a time-stretched spectrogram (phasegen/track.py, phase="vocoder"), the
// standard comparator of every time-stretch method.  Each bin's analysis phase is propagated along the OUTPUT frame grid by the
// frame-to-frame advance measured on the SOURCE grid at the output frame's position (librosa.phase_vocoder's recurrence); a bin that
// falls below a magnitude floor takes its analysis phase back (the transient / silence reset).  The reference has no counterpart; the
// arithmetic is the contract (include/phasegen.h states it) and tests/_vocoder_ref.py restates it in numpy, bit for bit.
//
// The phase grid q() / angle() and the positions i0(g), i1(g) are pg_track.h's.  Phase matters modulo 2 pi only and is kept as a
// 32-bit unsigned fraction of a turn: integer addition wraps and is associative, so the scan along time is EXACT in any order and
// the result cannot depend on the grid, the chunking or the wave size.
//   delta[g] = q(A[i1]) - q(A[i0])                            (uint32: the wrap IS the principal value of the advance)
//   reset[g] = g == 0 || (M != NULL && M[i0] < reset_below)
//   acc[g]   = reset[g] ? q(A[i0]) : acc[g-1] + delta[g-1]    (uint32)
//   out[g]   = angle(acc[g])
//
// Kernel.  One 256-thread workgroup per (channel, bin) row (rows are walked grid-stride), the row in chunks of 1024 output frames, 4
// consecutive frames per thread.  Element g of the scan is the pair (reset[g], reset[g] ? q(A[i0(g)]) : delta[g-1]) and the operator
// is the segmented sum (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2): in registers over a thread's 4 elements, across the 64
// lanes of a wave (6 shuffle steps), across the 4 waves through LDS (two buffers alternate, so one barrier per chunk), and a carry
// register into the next chunk.  Source reads are gathers at i0 / i1, monotone in g: they coalesce and hit cache.  Stores are 16-byte
// when `out` and F_out allow and frame by frame otherwise; both paths give the same bits.  All index arithmetic is 64-bit; q() is one
// double multiply (nothing to contract; the file is built with -ffp-contract=off like the rest).  Measurements: DESIGN.md section 4.11.
//
// pg_phase_vocoder_map is the same kernel on pg_track.h's MappedGrid: i0(g) comes from pc(pos[g]), pos a table of F_out doubles, and
// need not grow with g (the gathers are then no longer monotone; nothing else depends on it).  tests/_map_ref.py; DESIGN.md 4.19.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_track.h"

namespace {

namespace tk = pg_track;
constexpr int PV_THREADS = 256;
constexpr int PV_PER_THREAD = 4;
constexpr int PV_CHUNK = PV_THREADS * PV_PER_THREAD;      // 1024 output frames
constexpr int PV_WAVES = PV_THREADS / 64;

struct PvKernelArgs {
    const float* A; const float* M; float* out;
    double src_per_out; const double* pos;                    // the grid: Grid::of(args) takes its own
    long a_stride, m_stride, F_src, F_out, rows;
    int bins;
    float reset_below;
};

template <typename Grid, bool VEC>
__global__ __launch_bounds__(PV_THREADS) void phase_vocoder_kernel(const PvKernelArgs a) {
    const Grid grid = Grid::of(a);
    __shared__ uint32_t wave_v[2][PV_WAVES];
    __shared__ uint32_t wave_f[2][PV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const long c = r / a.bins, b = r - c * a.bins;
        const float* ar = a.A + c * a.a_stride + b * a.F_src;
        const float* mr = a.M ? a.M + c * a.m_stride + b * a.F_src : nullptr;
        float* orow = a.out + r * a.F_out;
        uint32_t carry = 0u;                                  // acc of the last frame of the previous chunk (frame 0 always resets)
        int buf = 0;
        for (long c0 = 0; c0 < a.F_out; c0 += PV_CHUNK, buf ^= 1) {
            const long g0 = c0 + (long)tid * PV_PER_THREAD;
            // 1. the thread's 4 elements, scanned in registers; frames past the end are the identity (0, 0).  The five frames
            // g0 - 1 .. g0 + 3 give the positions and quantised phases of all four elements: element g takes q(A[i0(g)]) when it
            // resets and delta[g-1] = q(A[i1(g-1)]) - q(A[i0(g-1)]) otherwise, and i1(g-1) is very often i0(g).  (Frames outside
            // 0 .. F_out - 1 are clamped into the row: what they read is valid and never used.)
            long i0[PV_PER_THREAD + 1];
            uint32_t q0[PV_PER_THREAD + 1];
#pragma unroll
            for (int j = 0; j <= PV_PER_THREAD; ++j) {
                long g = g0 - 1 + j;
                g = g < 0 ? 0 : (g < a.F_out ? g : a.F_out - 1);
                i0[j] = tk::i0(grid, g, a.F_src);
                q0[j] = tk::q(ar[i0[j]]);
            }
            uint32_t v[PV_PER_THREAD];
            bool f[PV_PER_THREAD];
            uint32_t tv = 0u;
            bool tf = false;
#pragma unroll
            for (int i = 0; i < PV_PER_THREAD; ++i) {
                const long g = g0 + i;
                uint32_t ev = 0u;
                bool ef = false;
                if (g < a.F_out) {
                    ef = g == 0 || (mr != nullptr && mr[i0[i + 1]] < a.reset_below);
                    if (ef) ev = q0[i + 1];
                    else {
                        const long j1 = tk::i1(i0[i], a.F_src);
                        ev = (j1 == i0[i + 1] ? q0[i + 1] : tk::q(ar[j1])) - q0[i];
                    }
                }
                tv = ef ? ev : tv + ev;
                tf = tf || ef;
                v[i] = tv; f[i] = tf;
            }
            // 2. inclusive segmented scan of the threads' totals across the wave
            uint32_t sv = tv, sf = tf ? 1u : 0u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t pv = __shfl_up(sv, off, 64), pf = __shfl_up(sf, off, 64);
                if (lane >= off) { sv = sf ? sv : pv + sv; sf |= pf; }
            }
            // the lanes before this one: (0, 0) for lane 0
            uint32_t xv = __shfl_up(sv, 1, 64), xf = __shfl_up(sf, 1, 64);
            if (lane == 0) { xv = 0u; xf = 0u; }
            // 3. the waves' totals through LDS
            if (lane == 63) { wave_v[buf][wave] = sv; wave_f[buf][wave] = sf; }
            __syncthreads();
            uint32_t pre = carry, tot = carry;                // carry o wave 0 o ... o wave (w - 1), and over all waves
#pragma unroll
            for (int w = 0; w < PV_WAVES; ++w) {
                const uint32_t wv = wave_v[buf][w], wf = wave_f[buf][w];
                tot = wf ? wv : tot + wv;
                if (w + 1 == wave) pre = tot;
            }
            carry = tot;
            pre = xf ? xv : pre + xv;                         // ... o the lanes before this one
            // 4. the thread's frames
            if (g0 < a.F_out) {
                if (VEC) {                                    // F_out % 4 == 0: the unit is whole and 16-byte aligned
                    f32x4 o;
#pragma unroll
                    for (int i = 0; i < PV_PER_THREAD; ++i) o[i] = tk::angle(f[i] ? v[i] : pre + v[i]);
                    *(f32x4*)(orow + g0) = o;
                } else {
#pragma unroll
                    for (int i = 0; i < PV_PER_THREAD; ++i)
                        if (g0 + i < a.F_out) orow[g0 + i] = tk::angle(f[i] ? v[i] : pre + v[i]);
                }
            }
        }
        // (the next row's first barrier orders its LDS writes after this row's last reads: the buffers alternate and every wave
        // passes a chunk's barrier before any wave reaches the chunk after the next)
        __syncthreads();
    }
}

// the checked call (pg_track.h) on the grid it names
template <typename Grid>
int pv_run(const char* op, const PgStretchCall& c, void* stream) {
    PvKernelArgs k;
    bool wide;
    if (int e = pg_stretch_check(op, INT32_MAX, c, k, wide)) return e;
    k.rows = c.n_ch * c.bins;
    const unsigned grid = pg_stream_grid(k.rows, 1);          // a workgroup per row
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL((phase_vocoder_kernel<Grid, true>), dim3(grid), dim3(PV_THREADS), 0, st, k);
    else hipLaunchKernelGGL((phase_vocoder_kernel<Grid, false>), dim3(grid), dim3(PV_THREADS), 0, st, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PG_OK : pg_failf((int)e, "%s launch failed", op);
}

}  // namespace

extern "C" int pg_phase_vocoder(const pg_phase_vocoder_args* a, void* stream) {
    return pv_run<tk::UniformGrid>("phase_vocoder", pg_stretch_uniform<PG_M_OPTIONAL>(a), stream);
}

// the same scan over the positions of a table (tk::MappedGrid)
extern "C" int pg_phase_vocoder_map(const pg_phase_vocoder_map_args* a, void* stream) {
    return pv_run<tk::MappedGrid>("phase_vocoder_map", pg_stretch_mapped<PG_M_OPTIONAL>(a), stream);
}
