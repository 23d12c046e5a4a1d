// lock.hip -- pg_phase_lock: the phase-vocoder phase with identity phase locking (Laroche & Dolson; phasegen/track.py,
// phase="vocoder_locked").  pg_phase_vocoder (vocoder.hip) advances every bin on its own, so the bins of one sinusoid's main lobe drift
// apart; here only the spectral PEAKS of a frame advance and every other bin takes the rotation of its nearest peak, so the analysis'
// phase relations inside a lobe survive the stretch.  The reference has no counterpart; the arithmetic is the contract
// (include/phasegen.h states it) and tests/_lock_ref.py restates it in numpy, bit for bit.
//
// pg_phase_spsi (single-pass spectrogram inversion; phase="spsi") is a second recurrence of the same shape and runs on the same
// scan: the peaks, the regions and the three launches below are its too, only the frame source differs -- it reads M alone, on the
// output grid itself, and a peak advances by its interpolated frequency instead of by a measured phase difference (LockSrc /
// SpsiSrc below; tests/_spsi_ref.py).  What follows describes pg_phase_lock; where pg_phase_spsi differs the sources say so.
//
// pg_phase_lock_linked (phase="vocoder_locked" with link_channels; tests/_link_ref.py) gives all channels ONE rotation, that of a
// reference plane pair (Aref, Mref): compose and carry are pg_phase_lock's on the reference, run once with a channel count of 1, and
// only apply runs per (channel, chunk) -- it rebuilds the chunk's maps from the reference, reads the one T slot of its chunk, which
// nothing writes after carry, and adds q(A[c]) at the output (LinkSrc: a third plane in the staged window).  T cancels in the
// uint32 difference of two channels, so the analysis' inter-channel phase differences survive the stretch exactly.  (One workgroup
// serving all channels of a chunk from one map would save the recomputation of the maps; it needs n_ch planes of the window or a
// pass per channel over stored maps, and is not done.)
//
// pg_phase_lock_map and pg_phase_lock_linked_map are the two above on pg_track.h's MappedGrid: the positions of the output frames
// come from a table, pc(pos[g]), and need not grow with g.  Only LkArgs and the two loaders (lk_load, lk_fetch) know the grid: the
// frame sources carry it as a type, LockSrc<Grid> / LinkSrc<Grid>, and the scan below is the same code for both (tests/_map_ref.py;
// DESIGN.md section 4.19).  On the host the four are ONE function, lk_stretch: pg_track.h reads each ABI struct into a PgStretchCall
// and checks it (the checker pg_phase_vocoder and its twin go through), the workspace rows are lk_workspace_check's -- pg_phase_spsi's
// too -- and the entry points only name their struct's reader, their grid and their frame sources.
//
// The recurrence (q(), angle(), i0(g), i1(g) and the advance into frame g are pg_track.h's, shared with vocoder.hip).  Per channel,
// T_g[b] (uint32, a fraction of a turn) is the rotation of bin b at output frame g against its analysis
// phase: T_0 = 0 and T_g[b] = reset ? 0 : T_{g-1}[p] + e_g[p] with p = P_g(b) the peak bin b belongs to, e_g[p] = q(A[p][i1(g-1)]) -
// q(A[p][i0(g)]) and reset = M[p][i0(g)] < reset_below; out[b][g] = angle(T_g[b] + q(A[b][i0(g)])).  Frame g is therefore a GATHER MAP
// (src_g, c_g): T_g[b] = T_{g-1}[src_g[b]] + c_g[b], where a reset is the source index `bins`, the zero source (T[bins] == 0).  Maps
// compose -- (s2, c2) o (s1, c1) = (s1[s2], c1[s2] + c2), the zero source stays the zero source -- composition is associative and the
// sums are integers modulo 2^32, so any split of the time axis gives the sequential loop's bits.
//
// Three launches, time in chunks of LK_CHUNK = 32 output frames:
//   compose  one workgroup per (channel, chunk but the last): folds the chunk's frame maps into one (S, C) pair in LDS (double
//            buffered, one gather per frame) and writes it to the workspace;
//   carry    one workgroup per channel: walks the chunk maps in order, one LDS gather per chunk, and writes T at every chunk's start;
//   apply    one workgroup per (channel, chunk): starts from its T, replays its frames and writes `out`.
// The peak maps are RECOMPUTED in apply: stored they would take 2 bytes per output cell, as much again as half of `out`, while the
// workspace as it is holds 12 bytes per bin and chunk (S, C, T), 3/32 of `out`.
//
// One frame, in a workgroup of up to 1024 threads with bin b = tid + j nt (j < BPT <= 4): every thread puts its bins' magnitude and
// advance into LDS; after a barrier it tests its bins against their four neighbours, and a wave's ballot IS the 64-bin word of the
// frame's peak bitmask (at most 64 words); after a second barrier every wave forms the mask of non-empty words with one more ballot,
// and the nearest peak below and above a bin is a count of leading / trailing zeros in its own word or in the nearest non-empty one.
// Two barriers per frame; the magnitude / advance buffers alternate by frame so that the next frame's writes cannot overtake this
// frame's gathers.
//
// Memory.  A and M are frames-fastest, so a frame is a column with stride F_src.  Threads that walk their own rows frame by frame
// fetch a whole cache line per 4-byte value and, the live lines of a CU's workgroups being many times its share of the L2, fetch it
// again for every frame: measured, that was 32 times the planes' bytes and 0.75 ms per launch.  So a WINDOW of wt consecutive source
// frames of all rows is staged through LDS instead (lk_fetch): read with the lanes along the frames, a row's segment per request,
// M as it is and A already quantised, and reloaded when a frame's positions leave it -- every 12 output frames at wt = 8 and a stretch
// of 1.5.  wt is the widest power of two that fits beside the maps (lk_window): 8 frames at 1024 bins, 4 at 2048, up to the whole chunk
// for narrow planes, none at 4096 bins, where the maps alone take 129 KiB and the rows are walked after all.  `out` is written along
// frames in a weak sense only: a thread collects four frames of a row and stores 16 bytes when F_out and `out` allow -- a row's
// 128-byte line is filled by eight stores over a chunk -- and frame by frame, 4 bytes per lane with the lanes F_out apart,
// otherwise; both paths give the same bits.  (Staging a chunk's 32 frames per row through LDS and storing whole lines is not done.)  All index arithmetic is 64-bit; no atomics.  Measurements: DESIGN.md section 4.12.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_track.h"

namespace {

namespace tk = pg_track;
constexpr int LK_CHUNK = 32;                                // L: output frames per chunk (a multiple of 4: chunks begin on a 16-byte unit)
constexpr int LK_MAX_BINS = 4096;
constexpr int LK_MAX_THREADS = 1024;
constexpr int LK_WORDS = LK_MAX_BINS / 64;                  // words of the peak bitmask
constexpr int LK_RING = 8;                                  // map words per thread in flight in the carry: 8 / BPT chunk maps
static_assert(PG_LOCK_REACH == 2, "the peak test below is written for a reach of 2");
static_assert(LK_CHUNK % 4 == 0, "16-byte stores need chunks of whole units");

struct LkArgs {
    const float* A; const float* M; float* out;
    uint32_t* ws;                                           // per (channel, chunk): S[bins], C[bins], T[bins]
    double src_per_out; const double* pos;                  // the time grid (pg_track.h): a frame source's Grid::of(args) takes its own
    long a_stride, m_stride, F_src, F_out, n_chunks;
    int bins, nb;                                           // nb = BPT * blockDim.x >= bins
    int wt_compose, wt_apply;                               // source frames in the staged window of either kernel (a power of two; 0: none)
    float reset_below;
    int bin0;                                               // SpsiSrc only: the FFT bin of row 0, and hop / n_fft in double
    double hop_per_fft;
    const float* X; long x_stride;                          // LinkSrc only: the channels' angle planes (A and M are the reference's)
};

// what a thread reads of frame g for its bins: the magnitude, the quantised analysis phase and the advance e_g (SpsiSrc: qa is
// the half turn of an odd FFT bin, and e is not known yet)
template <int BPT>
struct LkFrame { float m[BPT]; uint32_t qa[BPT]; uint32_t e[BPT]; };

template <typename Grid, int BPT, bool LINKED>
__device__ __forceinline__ void lk_load(const LkArgs& a, const float* Ac, const float* Mc, const float* Xc, long g, LkFrame<BPT>& f) {
    const tk::Advance adv = tk::advance(Grid::of(a), g, a.F_src);
    const long i0 = adv.i0, i1p = adv.i1p;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = (int)threadIdx.x + j * (int)blockDim.x;
        f.m[j] = __uint_as_float(0x7fc00000u);              // bins past the end: never a peak, never gathered
        f.qa[j] = 0u; f.e[j] = 0u;
        if (b < a.bins) {
            const long row = (long)b * a.F_src;
            f.m[j] = Mc[row + i0];
            f.qa[j] = tk::q(Ac[row + i0]);
            f.e[j] = (i1p == i0 ? f.qa[j] : tk::q(Ac[row + i1p])) - f.qa[j];
            if (LINKED) f.qa[j] = tk::q(Xc[row + i0]);      // (the advance is the reference's; the channel's own phase is what is added)
        }
    }
}

// The staged window: wt consecutive source frames of every row of M and of q(A), read with the lanes along the frames -- a row's
// segment is one request -- and kept transposed in LDS as win[b * (wt + 1) + k] (an odd pitch: a frame's column is read without bank
// conflicts).  ws0: the window's first source frame, -1 before the first load; uniform over the workgroup, as is every branch here.
// A frame whose two positions are further apart than a window (src_per_out >= wt), or a plane too wide for a window to fit into LDS
// beside the maps (wt == 0), is read by every thread from its own rows instead.  LINKED: a third plane, q(X) of the workgroup's
// channel, is staged beside the reference's two and is what f.qa holds.  Nothing here needs the positions to grow with g: under a
// mapped grid a frame behind the window reloads it and a jump wider than the window reads the rows.
template <typename Grid, int BPT, bool LINKED>
__device__ __forceinline__ void lk_fetch(const LkArgs& a, const float* Ac, const float* Mc, const float* Xc, long g, uint32_t* win, int wt,
                                         long& ws0, LkFrame<BPT>& f) {
    const tk::Advance adv = tk::advance(Grid::of(a), g, a.F_src);
    const long i0 = adv.i0, i1p = adv.i1p;
    const long lo = i0 < i1p ? i0 : i1p, hi = i0 < i1p ? i1p : i0;
    if (wt == 0 || hi - lo >= wt) { lk_load<Grid, BPT, LINKED>(a, Ac, Mc, Xc, g, f); return; }
    const int pitch = wt + 1, tid = threadIdx.x, nt = blockDim.x;
    uint32_t* winM = win;
    uint32_t* winA = win + a.nb * pitch;
    uint32_t* winX = winA + a.nb * pitch;                   // (LINKED only)
    if (ws0 < 0 || lo < ws0 || hi >= ws0 + wt) {
        // (every wave has left the previous frame's window reads behind: two barriers ago)
        ws0 = lo;
        const int shift = __builtin_ctz((unsigned)wt), n = a.bins << shift;
        for (int e = tid; e < n; e += nt) {
            const int r = e >> shift, k = e & (wt - 1);
            if (ws0 + k < a.F_src) {
                const long at = (long)r * a.F_src + ws0 + k;
                winM[r * pitch + k] = __float_as_uint(Mc[at]);
                winA[r * pitch + k] = tk::q(Ac[at]);
                if (LINKED) winX[r * pitch + k] = tk::q(Xc[at]);
            }
        }
        __syncthreads();
    }
    const int k0 = (int)(i0 - ws0), k1 = (int)(i1p - ws0);
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = tid + j * nt;
        f.m[j] = __uint_as_float(0x7fc00000u);
        f.qa[j] = 0u; f.e[j] = 0u;
        if (b < a.bins) {
            f.m[j] = __uint_as_float(winM[b * pitch + k0]);
            f.qa[j] = winA[b * pitch + k0];
            f.e[j] = winA[b * pitch + k1] - f.qa[j];
            if (LINKED) f.qa[j] = winX[b * pitch + k0];
        }
    }
}

// ---- The frame source.  The scan -- regions, compose, carry, apply -- is ONE piece of code over T_g[b] = T_{g-1}[P_g(b)] + c_g[P_g(b)];
// a frame source says where frame g's magnitudes come from (fetch: f.m), how the advance of a peak is formed (EARLY: f.e, known
// when the frame is fetched; otherwise advance(), from the frame's magnitudes in LDS after the first barrier of the region step),
// when a region starts again from zero (reset) and what is added at the output (f.qa).  PLANES: planes in the staged window.
// LINKED: every channel of the launch reads channel 0's T from the workspace and its own plane Xc beside the shared (Ac, Mc).

// pg_phase_lock: the time grid `Grid` (uniform, or pg_phase_lock_map's table) over M and q(A); the advance is measured on A; a quiet
// peak resets; q(A) is added.
template <typename Grid>
struct LockSrc {
    static constexpr int PLANES = 2;
    static constexpr bool EARLY = true;
    static constexpr bool LINKED = false;
    template <int BPT>
    static __device__ __forceinline__ void fetch(const LkArgs& a, const float* Ac, const float* Mc, const float*, long g, uint32_t* win, int wt,
                                                 long& ws0, LkFrame<BPT>& f) { lk_fetch<Grid, BPT, false>(a, Ac, Mc, nullptr, g, win, wt, ws0, f); }
    static __device__ __forceinline__ uint32_t advance(const LkArgs&, const uint32_t*, int) { return 0u; }
    static __device__ __forceinline__ bool reset(const LkArgs& a, long g, const uint32_t* msf, int p) {
        return g == 0 || __uint_as_float(msf[p]) < a.reset_below;
    }
};

// pg_phase_lock_linked, the apply launch alone: LockSrc on the reference's planes (Ac = Aref, Mc = Mref, shared by all channels:
// the maps, the advances and the resets are pg_phase_lock's of the reference, and compose and carry ARE LockSrc's, run once), but
// what is added at the output is q(X) of the workgroup's own channel, a third plane of the window.
template <typename Grid>
struct LinkSrc : LockSrc<Grid> {
    static constexpr int PLANES = 3;
    static constexpr bool LINKED = true;
    template <int BPT>
    static __device__ __forceinline__ void fetch(const LkArgs& a, const float* Ac, const float* Mc, const float* Xc, long g, uint32_t* win,
                                                 int wt, long& ws0, LkFrame<BPT>& f) { lk_fetch<Grid, BPT, true>(a, Ac, Mc, Xc, g, win, wt, ws0, f); }
};

// pg_phase_spsi: M on the output grid itself (frame g is column g; no A); the advance of bin p is its interpolated frequency times
// hop / n_fft of a turn (include/phasegen.h: the offset in fp32 with one IEEE division, the advance in double); only frame 0
// resets; the half turn of the odd FFT bins is added.
struct SpsiSrc {
    static constexpr int PLANES = 1;
    static constexpr bool EARLY = false;
    static constexpr bool LINKED = false;
    // The window holds frames [g - g % wt, + wt) of the one plane: wt divides LK_CHUNK and chunks begin on multiples of it, so it
    // is reloaded every wt frames whatever the data.  (Every wave has left the previous window's reads two barriers behind.)
    template <int BPT>
    static __device__ __forceinline__ void fetch(const LkArgs& a, const float*, const float* Mc, const float*, long g, uint32_t* win, int wt,
                                                 long&, LkFrame<BPT>& f) {
        const int tid = threadIdx.x, nt = blockDim.x, pitch = wt + 1, k = wt ? (int)(g & (long)(wt - 1)) : 0;
        if (wt && k == 0) {
            const int shift = __builtin_ctz((unsigned)wt), n = a.bins << shift;
            for (int e = tid; e < n; e += nt) {
                const int r = e >> shift, kk = e & (wt - 1);
                if (g + kk < a.F_src) win[r * pitch + kk] = __float_as_uint(Mc[(long)r * a.F_src + g + kk]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            const int b = tid + j * nt;
            f.m[j] = __uint_as_float(0x7fc00000u);
            f.qa[j] = (uint32_t)((b + a.bin0) & 1) << 31;
            f.e[j] = 0u;
            if (b < a.bins) f.m[j] = wt ? __uint_as_float(win[b * pitch + k]) : Mc[(long)b * a.F_src + g];
        }
    }
    // ms: the frame's magnitudes (bins past the end are NaN and never asked for)
    static __device__ __forceinline__ uint32_t advance(const LkArgs& a, const uint32_t* ms, int p) {
        float delta = 0.0f;
        if (p > 0 && p < a.bins - 1) {
            const float al = __uint_as_float(ms[p - 1]), be = __uint_as_float(ms[p]), ga = __uint_as_float(ms[p + 1]);
            const float d = (al - be) + (ga - be);
            const float n = 0.5f * (al - ga);
            if (d < 0.0f) delta = n / d;
            if (!(fabsf(delta) <= 0.5f)) delta = 0.0f;
        }
        const double x = ((double)(p + a.bin0) + (double)delta) * a.hop_per_fft;
        return (uint32_t)(int64_t)rint(x * 4294967296.0);
    }
    static __device__ __forceinline__ bool reset(const LkArgs&, long g, const uint32_t*, int) { return g == 0; }
};

// the nearest set bit of the bitmask to bin b (a tie goes to the lower one); b itself when no bit is set.  nz: the non-empty words.
__device__ __forceinline__ int lk_nearest(const uint64_t* pk, uint64_t nz, int b) {
    const int w = b >> 6, bit = b & 63;
    const uint64_t word = pk[w];
    int lp = -1, rp = -1;
    const uint64_t lo = word & ((2ull << bit) - 1ull);       // bits 0 .. bit
    if (lo) lp = (w << 6) + 63 - __builtin_clzll(lo);
    else {
        const uint64_t nzl = nz & ((1ull << w) - 1ull);
        if (nzl) { const int w2 = 63 - __builtin_clzll(nzl); lp = (w2 << 6) + 63 - __builtin_clzll(pk[w2]); }
    }
    const uint64_t hi = word & ~((1ull << bit) - 1ull);      // bits bit .. 63
    if (hi) rp = (w << 6) + __builtin_ctzll(hi);
    else {
        const uint64_t nzr = nz & ~((2ull << w) - 1ull);
        if (nzr) { const int w2 = __builtin_ctzll(nzr); rp = (w2 << 6) + __builtin_ctzll(pk[w2]); }
    }
    if (lp < 0) return rp < 0 ? b : rp;
    if (rp < 0) return lp;
    return (b - lp) <= (rp - b) ? lp : rp;
}

// One frame's regions: p[j] = P_g(bin j of this thread).  ms / es: this frame's magnitude and advance buffers (nb words each; written
// here, valid until the frame after the next writes them again); pk: the peak bitmask.  Two barriers.  A source whose advance is
// formed from the neighbours' magnitudes fills es between the two (for every bin: in a frame without peaks every bin is its own).
template <typename Src, int BPT>
__device__ __forceinline__ void lk_regions(const LkArgs& a, const LkFrame<BPT>& f, uint32_t* ms, uint32_t* es, uint64_t* pk, int (&p)[BPT]) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, bins = a.bins;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        ms[tid + j * nt] = __float_as_uint(f.m[j]);
        if (Src::EARLY) es[tid + j * nt] = f.e[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = tid + j * nt;
        const float mb = f.m[j];
        bool peak = b < bins && mb == mb;
#pragma unroll
        for (int d = 1; d <= PG_LOCK_REACH; ++d) {
            if (b - d >= 0 && b < bins) peak = peak && mb > __uint_as_float(ms[b - d]);
            if (b + d < bins) peak = peak && mb >= __uint_as_float(ms[b + d]);
        }
        const uint64_t word = __ballot(peak);
        if (lane == 0) pk[j * (nt >> 6) + wave] = word;
        if (!Src::EARLY && b < bins) es[b] = Src::advance(a, ms, b);
    }
    __syncthreads();
    const int n_words = BPT * (nt >> 6);
    const uint64_t mine = lane < n_words ? pk[lane] : 0ull;
    const uint64_t nz = __ballot(mine != 0ull);
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = tid + j * nt;
        p[j] = b < bins ? lk_nearest(pk, nz, b) : 0;
    }
}

extern __shared__ __attribute__((aligned(16))) uint32_t lk_lds[];

// LDS of compose: pk[64] (uint64), ms[2][nb], es[2][nb], S[2][nb + 1], C[2][nb + 1], win[Src::PLANES][nb][wt + 1]
template <typename Src, int BPT>
__global__ __launch_bounds__(LK_MAX_THREADS) void lock_compose_kernel(const LkArgs a) {
    const int tid = threadIdx.x, nt = blockDim.x, nb = a.nb, bins = a.bins;
    uint64_t* pk = (uint64_t*)lk_lds;
    uint32_t* ms = lk_lds + 2 * LK_WORDS;
    uint32_t* es = ms + 2 * nb;
    uint32_t* S = es + 2 * nb;
    uint32_t* Cm = S + 2 * (nb + 1);
    uint32_t* win = Cm + 2 * (nb + 1);
    const long per = a.n_chunks - 1;                         // the last chunk's map is never applied
    const long c = (long)blockIdx.x / per, k = (long)blockIdx.x - c * per;
    const float* Ac = a.A + c * a.a_stride;
    const float* Mc = a.M + c * a.m_stride;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = tid + j * nt;
        if (b < bins) { S[b] = (uint32_t)b; Cm[b] = 0u; }
    }
    if (tid == 0) { S[bins] = (uint32_t)bins; S[nb + 1 + bins] = (uint32_t)bins; Cm[bins] = 0u; Cm[nb + 1 + bins] = 0u; }
    const long g0 = k * LK_CHUNK, g1 = g0 + LK_CHUNK;        // (k is not the last chunk: the chunk is whole)
    long ws0 = -1;
    int cur = 0;
    for (long g = g0; g < g1; ++g) {
        LkFrame<BPT> f;
        Src::template fetch<BPT>(a, Ac, Mc, nullptr, g, win, a.wt_compose, ws0, f);
        const int par = (int)(g & 1);
        const uint32_t* msf = ms + par * nb;
        const uint32_t* esf = es + par * nb;
        int p[BPT];
        lk_regions<Src, BPT>(a, f, ms + par * nb, es + par * nb, pk, p);
        const uint32_t* Sc = S + cur * (nb + 1);
        const uint32_t* Cc = Cm + cur * (nb + 1);
        uint32_t* Sn = S + (cur ^ 1) * (nb + 1);
        uint32_t* Cn = Cm + (cur ^ 1) * (nb + 1);
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            const int b = tid + j * nt;
            if (b < bins) {
                const int pj = p[j];
                const bool reset = Src::reset(a, g, msf, pj);
                Sn[b] = reset ? (uint32_t)bins : Sc[pj];
                Cn[b] = reset ? 0u : Cc[pj] + esf[pj];
            }
        }
        cur ^= 1;
    }
    __syncthreads();
    uint32_t* w = a.ws + (c * a.n_chunks + k) * 3 * (long)bins;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = tid + j * nt;
        if (b < bins) { w[b] = S[cur * (nb + 1) + b]; w[bins + b] = Cm[cur * (nb + 1) + b]; }
    }
}

// LDS of carry: T[2][nb + 1].  (Chunk maps are chunk maps: the carry serves every frame source.)
template <int BPT>
__global__ __launch_bounds__(LK_MAX_THREADS) void lock_carry_kernel(const LkArgs a) {
    const int tid = threadIdx.x, nt = blockDim.x, nb = a.nb, bins = a.bins;
    uint32_t* T = lk_lds;
    const long c = blockIdx.x;
    uint32_t* w = a.ws + c * a.n_chunks * 3 * (long)bins;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = tid + j * nt;
        if (b < bins) T[b] = 0u;                             // (chunk 0 begins with frame 0, which resets every bin)
    }
    if (tid == 0) { T[bins] = 0u; T[nb + 1 + bins] = 0u; }   // the zero source, in both buffers
    __syncthreads();
    // The chunk maps travel through a ring of LK_DEPTH register slots, loaded LK_DEPTH steps ahead: a step is one LDS gather and one
    // barrier, far shorter than a load's latency.  LK_DEPTH = 8 / BPT in integers: 8, 4, 2 (6 of the 8 words) and 2 slots.  Every
    // slot starts as the map (0, 0) and is loaded only with a chunk's map that exists, so a slot that is gathered through without
    // one -- the last chunk's step, or any slot when n_chunks <= LK_DEPTH -- holds indices <= bins: zeros or an earlier chunk's map.
    constexpr int LK_DEPTH = LK_RING / BPT;
    uint32_t s[LK_DEPTH][BPT], cc[LK_DEPTH][BPT];
#pragma unroll
    for (int d = 0; d < LK_DEPTH; ++d) {
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            const int b = tid + j * nt;
            s[d][j] = 0u; cc[d][j] = 0u;
            if (b < bins && d + 1 < a.n_chunks) { s[d][j] = w[d * 3 * (long)bins + b]; cc[d][j] = w[d * 3 * (long)bins + bins + b]; }
        }
    }
    int cur = 0;
    for (long k0 = 0; k0 < a.n_chunks; k0 += LK_DEPTH) {
#pragma unroll
        for (int d = 0; d < LK_DEPTH; ++d) {
            const long k = k0 + d;
            if (k < a.n_chunks) {                            // (uniform over the workgroup)
                const uint32_t* Tc = T + cur * (nb + 1);
                uint32_t* Tn = T + (cur ^ 1) * (nb + 1);
                uint32_t* wk = w + k * 3 * (long)bins;
                const uint32_t* nw = wk + LK_DEPTH * 3 * (long)bins;
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int b = tid + j * nt;
                    if (b < bins) {
                        wk[2 * (long)bins + b] = Tc[b];
                        Tn[b] = Tc[s[d][j]] + cc[d][j];      // (the last chunk has no map: a stale one, whose result nobody reads)
                        if (k + LK_DEPTH + 1 < a.n_chunks) { s[d][j] = nw[b]; cc[d][j] = nw[bins + b]; }
                    }
                }
                __syncthreads();
                cur ^= 1;
            }
        }
    }
}

// LDS of apply: pk[64] (uint64), ms[2][nb], es[2][nb], T[2][nb], win[Src::PLANES][nb][wt + 1]
template <typename Src, int BPT, bool VEC>
__global__ __launch_bounds__(LK_MAX_THREADS) void lock_apply_kernel(const LkArgs a) {
    const int tid = threadIdx.x, nt = blockDim.x, nb = a.nb, bins = a.bins;
    uint64_t* pk = (uint64_t*)lk_lds;
    uint32_t* ms = lk_lds + 2 * LK_WORDS;
    uint32_t* es = ms + 2 * nb;
    uint32_t* T = es + 2 * nb;
    uint32_t* win = T + 2 * nb;
    const long c = (long)blockIdx.x / a.n_chunks, k = (long)blockIdx.x - c * a.n_chunks;
    const float* Ac = a.A + c * a.a_stride;
    const float* Mc = a.M + c * a.m_stride;
    const float* Xc = Src::LINKED ? a.X + c * a.x_stride : nullptr;
    float* oc = a.out + c * (long)bins * a.F_out;
    const uint32_t* w = a.ws + ((Src::LINKED ? 0 : c) * a.n_chunks + k) * 3 * (long)bins + 2 * (long)bins;   // (LINKED: one T for all channels)
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int b = tid + j * nt;
        if (b < bins) T[b] = w[b];
    }
    const long g0 = k * LK_CHUNK, g1 = g0 + LK_CHUNK < a.F_out ? g0 + LK_CHUNK : a.F_out;
    long ws0 = -1;
    int cur = 0;
    for (long gq = g0; gq < g1; gq += 4) {                   // VEC: F_out % 4 == 0, so every unit is whole
        f32x4 o[BPT];                                        // (filled by selects on u: the frame loop stays rolled, registers stay few)
#pragma unroll
        for (int j = 0; j < BPT; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int u = 0; u < 4; ++u) {
            const long g = gq + u;
            if (g < g1) {                                    // (uniform over the workgroup)
                LkFrame<BPT> f;
                Src::template fetch<BPT>(a, Ac, Mc, Xc, g, win, a.wt_apply, ws0, f);
                const int par = u & 1;                       // (gq is a multiple of 4)
                const uint32_t* msf = ms + par * nb;
                const uint32_t* esf = es + par * nb;
                int p[BPT];
                lk_regions<Src, BPT>(a, f, ms + par * nb, es + par * nb, pk, p);
                const uint32_t* Tc = T + cur * nb;
                uint32_t* Tn = T + (cur ^ 1) * nb;
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int b = tid + j * nt;
                    if (b < bins) {
                        const int pj = p[j];
                        const bool reset = Src::reset(a, g, msf, pj);
                        const uint32_t t = reset ? 0u : Tc[pj] + esf[pj];
                        Tn[b] = t;
                        const float v = tk::angle(t + f.qa[j]);
                        if (VEC) {
                            o[j][0] = u == 0 ? v : o[j][0]; o[j][1] = u == 1 ? v : o[j][1];
                            o[j][2] = u == 2 ? v : o[j][2]; o[j][3] = u == 3 ? v : o[j][3];
                        } else oc[(long)b * a.F_out + g] = v;
                    }
                }
                cur ^= 1;
            }
        }
        if (VEC) {
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                const int b = tid + j * nt;
                if (b < bins) *(f32x4*)(oc + (long)b * a.F_out + gq) = o[j];
            }
        }
    }
}

int lk_bpt(int bins) { return (bins + LK_MAX_THREADS - 1) / LK_MAX_THREADS; }
int lk_threads(int bins) { const int bpt = lk_bpt(bins); return (((bins + bpt - 1) / bpt) + 63) / 64 * 64; }

template <typename Kernel>
hipError_t lk_launch(Kernel kernel, long grid, int threads, int lds_bytes, hipStream_t st, const LkArgs& k) {
    if (lds_bytes > 65536) {                                 // (the attribute belongs to (function, current device): nothing cached)
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds_bytes, st, k);
    return hipGetLastError();
}

// The window of `planes` planes beside `base` bytes of LDS: the widest power of two up to the chunk's own span that fits into a
// CU's 160 KiB; 0 when not even 2 frames fit.  (Measured at 1024 bins and two planes: 8 frames with one workgroup per CU and 4
// frames with two take the same time within 1 %; the wider window fetches every line half as often.)  A source of one plane gets
// twice the frames in the same bytes.
int lk_window(int base, int nb, int planes) {
    int wt = 0;
    for (int t = 2; t <= LK_CHUNK; t *= 2)
        if (base + 4 * planes * nb * (t + 1) <= 160 * 1024) wt = t;
    return wt;
}

// Scan: the source of compose (and of the carry's maps), over n_scan channels; Src: the source of apply, over n_ch channels -- the
// same source and count but for pg_phase_lock_linked, whose scan is the reference's alone.
template <typename Scan, typename Src, int BPT>
hipError_t lk_run(LkArgs& k, int n_scan, int n_ch, int threads, bool wide, hipStream_t st) {
    const int nb = k.nb;
    int lds_compose = (2 * LK_WORDS + 4 * nb + 4 * (nb + 1)) * 4;
    const int lds_carry = 2 * (nb + 1) * 4;
    int lds_apply = (2 * LK_WORDS + 6 * nb) * 4;
    k.wt_compose = lk_window(lds_compose, nb, Scan::PLANES);
    k.wt_apply = lk_window(lds_apply, nb, Src::PLANES);
    if (k.wt_compose) lds_compose += 4 * Scan::PLANES * nb * (k.wt_compose + 1);
    if (k.wt_apply) lds_apply += 4 * Src::PLANES * nb * (k.wt_apply + 1);
    hipError_t e = hipSuccess;
    if (k.n_chunks > 1) {
        e = lk_launch(lock_compose_kernel<Scan, BPT>, (long)n_scan * (k.n_chunks - 1), threads, lds_compose, st, k);
        if (e != hipSuccess) return e;
    }
    e = lk_launch(lock_carry_kernel<BPT>, n_scan, threads, lds_carry, st, k);
    if (e != hipSuccess) return e;
    if (wide) return lk_launch(lock_apply_kernel<Src, BPT, true>, (long)n_ch * k.n_chunks, threads, lds_apply, st, k);
    return lk_launch(lock_apply_kernel<Src, BPT, false>, (long)n_ch * k.n_chunks, threads, lds_apply, st, k);
}

// shapes the workspace depends on -> bytes, or a negative error code.  linked: one channel's worth whatever n_ch -- the scan is the
// reference's alone (n_ch still has to be positive, and the apply grid's (channel, chunk) pairs to fit).
int64_t lk_workspace_bytes(const char* op, int64_t n_ch, int64_t bins, int64_t F_out, bool linked = false) {
    if (n_ch <= 0 || bins <= 0 || F_out <= 0) return pg_failf(PG_ERR_SHAPE, "%s: non-positive dimension", op);
    if (bins > LK_MAX_BINS) return pg_failf(PG_ERR_SHAPE, "%s: more than %d bins", op, LK_MAX_BINS);
    const int64_t n_chunks = (F_out - 1) / LK_CHUNK + 1;
    if (n_chunks > (int64_t)0x7fffffff / n_ch) return pg_failf(PG_ERR_SHAPE, "%s: more than 2^31 - 1 (channel, chunk) pairs", op);
    return (linked ? 1 : n_ch) * n_chunks * 3 * bins * 4;      // < 2^31 * 3 * 2^12 * 4
}

// The workspace rows of every entry point, after its own checks: alignment, then the size the query pg_workspace_bytes_<op>() states
// (which may refuse the shapes), then presence and size.
int lk_workspace_check(const char* op, int64_t n_ch, int64_t bins, int64_t F_out, bool linked, const void* workspace, int64_t workspace_bytes) {
    if (((uintptr_t)workspace) & 3) return pg_failf(PG_ERR_ALIGN, "%s: misaligned pointer", op);
    const int64_t need = lk_workspace_bytes(op, n_ch, bins, F_out, linked);
    if (need < 0) return (int)need;
    if (!workspace || workspace_bytes < need) return pg_failf(PG_ERR_WORKSPACE, "%s: workspace missing or smaller than pg_workspace_bytes_%s()", op, op);
    return PG_OK;
}

// the three launches for the sources Scan (compose, carry: n_scan channels) and Src (apply: n_ch); k holds everything but the plan
template <typename Scan, typename Src>
int lk_scan(const char* op, LkArgs& k, int n_scan, int n_ch, int64_t F_out, void* workspace, bool wide, void* stream) {
    const int bpt = lk_bpt(k.bins), threads = lk_threads(k.bins);
    k.ws = (uint32_t*)workspace;
    k.n_chunks = (F_out - 1) / LK_CHUNK + 1;
    k.nb = bpt * threads;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    switch (bpt) {
        case 1: e = lk_run<Scan, Src, 1>(k, n_scan, n_ch, threads, wide, st); break;
        case 2: e = lk_run<Scan, Src, 2>(k, n_scan, n_ch, threads, wide, st); break;
        case 3: e = lk_run<Scan, Src, 3>(k, n_scan, n_ch, threads, wide, st); break;
        default: e = lk_run<Scan, Src, 4>(k, n_scan, n_ch, threads, wide, st); break;
    }
    return e == hipSuccess ? PG_OK : pg_failf((int)e, "%s launch failed", op);
}

// pg_phase_lock and pg_phase_lock_linked on either grid (Scan, Src: as in lk_scan): the checked call (pg_track.h), the workspace of
// `a`, the scan.  A linked call scans the reference's planes once, as one channel (strides 0), and hands the channels' own planes to
// apply as X.
template <typename Scan, typename Src, typename Args>
int lk_stretch(const char* op, const PgStretchCall& c, const Args* a, void* stream) {
    LkArgs k;
    bool wide;
    if (int e = pg_stretch_check(op, LK_MAX_BINS, c, k, wide)) return e;
    if (int e = lk_workspace_check(op, c.n_ch, c.bins, c.F_out, Src::LINKED, a->workspace, a->workspace_bytes)) return e;
    k.bin0 = 0; k.hop_per_fft = 0.0; k.X = nullptr; k.x_stride = 0;
    if (Src::LINKED) {
        k.X = k.A; k.x_stride = k.a_stride;
        k.A = c.Aref; k.M = c.Mref; k.a_stride = 0;
    }
    return lk_scan<Scan, Src>(op, k, Src::LINKED ? 1 : (int)c.n_ch, (int)c.n_ch, c.F_out, a->workspace, wide, stream);
}

}  // namespace

extern "C" int64_t pg_workspace_bytes_phase_lock(const pg_phase_lock_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "phase_lock: args required");
    return lk_workspace_bytes("phase_lock", a->n_ch, a->bins, a->F_out);
}

extern "C" int pg_phase_lock(const pg_phase_lock_args* a, void* stream) {
    return lk_stretch<LockSrc<tk::UniformGrid>, LockSrc<tk::UniformGrid>>("phase_lock", pg_stretch_uniform<PG_M_REQUIRED>(a), a, stream);
}

// pg_phase_lock over the positions of a table: the same three launches on LockSrc<tk::MappedGrid>, the same workspace
extern "C" int64_t pg_workspace_bytes_phase_lock_map(const pg_phase_lock_map_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "phase_lock_map: args required");
    return lk_workspace_bytes("phase_lock_map", a->n_ch, a->bins, a->F_out);
}

extern "C" int pg_phase_lock_map(const pg_phase_lock_map_args* a, void* stream) {
    return lk_stretch<LockSrc<tk::MappedGrid>, LockSrc<tk::MappedGrid>>("phase_lock_map", pg_stretch_mapped<PG_M_REQUIRED>(a), a, stream);
}

extern "C" int64_t pg_workspace_bytes_phase_lock_linked(const pg_phase_lock_linked_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "phase_lock_linked: args required");
    return lk_workspace_bytes("phase_lock_linked", a->n_ch, a->bins, a->F_out, true);
}

extern "C" int pg_phase_lock_linked(const pg_phase_lock_linked_args* a, void* stream) {
    return lk_stretch<LockSrc<tk::UniformGrid>, LinkSrc<tk::UniformGrid>>("phase_lock_linked", pg_stretch_uniform<PG_REFERENCE>(a), a, stream);
}

extern "C" int64_t pg_workspace_bytes_phase_lock_linked_map(const pg_phase_lock_linked_map_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "phase_lock_linked_map: args required");
    return lk_workspace_bytes("phase_lock_linked_map", a->n_ch, a->bins, a->F_out, true);
}

extern "C" int pg_phase_lock_linked_map(const pg_phase_lock_linked_map_args* a, void* stream) {
    return lk_stretch<LockSrc<tk::MappedGrid>, LinkSrc<tk::MappedGrid>>("phase_lock_linked_map", pg_stretch_mapped<PG_REFERENCE>(a), a, stream);
}

extern "C" int64_t pg_workspace_bytes_phase_spsi(const pg_phase_spsi_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "phase_spsi: args required");
    return lk_workspace_bytes("phase_spsi", a->n_ch, a->bins, a->F);
}

// (the checks in the order of pg_stretch_check: NULL, shapes, ranges, strides, alignment, then the workspace)
extern "C" int pg_phase_spsi(const pg_phase_spsi_args* a, void* stream) {
    if (!a || !a->M || !a->out) return pg_fail(PG_ERR_NULL, "phase_spsi: args, M and out required");
    if (a->n_ch <= 0 || a->bins <= 0 || a->F <= 0) return pg_fail(PG_ERR_SHAPE, "phase_spsi: non-positive dimension");
    if (a->bins > LK_MAX_BINS) return pg_failf(PG_ERR_SHAPE, "phase_spsi: more than %d bins", LK_MAX_BINS);
    if (a->n_fft < 1 || a->hop < 1 || a->hop > a->n_fft) return pg_fail(PG_ERR_SHAPE, "phase_spsi: need 1 <= hop <= n_fft");
    if (a->bin0 < 0 || a->bin0 > 65536) return pg_fail(PG_ERR_SHAPE, "phase_spsi: bin0 must be within [0, 65536]");
    if (a->F > INT64_MAX / 2 / a->bins) return pg_fail(PG_ERR_SHAPE, "phase_spsi: plane beyond 2^62 elements");
    if (a->m_stride < (int64_t)a->bins * a->F) return pg_fail(PG_ERR_SHAPE, "phase_spsi: m_stride shorter than a plane");
    if ((int64_t)a->n_ch * a->bins > INT64_MAX / 2 / a->F) return pg_fail(PG_ERR_SHAPE, "phase_spsi: output beyond 2^62 elements");
    if ((((uintptr_t)a->M) & 3) || (((uintptr_t)a->out) & 3)) return pg_fail(PG_ERR_ALIGN, "phase_spsi: misaligned pointer");
    if (int e = lk_workspace_check("phase_spsi", a->n_ch, a->bins, a->F, false, a->workspace, a->workspace_bytes)) return e;
    LkArgs k;
    k.A = nullptr; k.M = a->M; k.out = a->out;
    k.src_per_out = 1.0; k.pos = nullptr;                    // the identity grid: frame g of `out` is column g of M
    k.a_stride = 0; k.m_stride = a->n_ch == 1 ? 0 : a->m_stride;
    k.F_src = a->F; k.F_out = a->F;
    k.bins = a->bins; k.reset_below = 0.0f;
    k.bin0 = a->bin0; k.hop_per_fft = (double)a->hop / (double)a->n_fft; k.X = nullptr; k.x_stride = 0;
    const bool wide = (a->F & 3) == 0 && pg_al16(a->out);
    return lk_scan<SpsiSrc, SpsiSrc>("phase_spsi", k, a->n_ch, a->n_ch, a->F, a->workspace, wide, stream);
}
