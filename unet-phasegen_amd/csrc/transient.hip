// transient.hip -- the two kernels of the transient-preserving stretch (phasegen/track.py, transients="ola"; Driedger, Mueller &
// Ewert 2014): pg_hpss splits a log-magnitude plane into a harmonic and a percussive plane by median filtering (Fitzgerald 2010,
// binary masks), and pg_ola_stretch relocates a time-domain signal by plain overlap-add with a short window.  The harmonic plane
// goes through whichever phase source the caller chose; the percussive plane is inverted on the SOURCE grid and its clicks are
// moved, not stretched.  The reference has no counterpart; the arithmetic is the contract (include/phasegen.h states it) and
// tests/_transient_ref.py restates both in numpy, bit for bit.
//
// pg_hpss.  key(x) = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000) is the IEEE total order as an unsigned integer; the staged
// tile holds KEYS, so a median is a selection among uint32 values and a cell's own bits are key^-1 of its key.  One 256-thread
// workgroup per (channel, 32 bins, 64 frames) tile, tiles walked grid-stride with a 64-bit index.  The tile and its halos of hf
// rows and ht frames are staged once: wave w loads the LDS rows w, w + 4, ..., its lanes run along the frames (coalesced), and the
// edge replication is the clamp of the row and the frame index on that load, so LDS position (r, c) holds exactly the element the
// contract's window names.  The row pitch is 64 + 2 ht rounded up to 1 modulo 4: a thread owns 4 consecutive frames of a row and a
// wave 4 rows of 16 such threads, and with that pitch the 64 lanes of every ds_read_b32 hit 64 different banks, along time (stride
// 1 per window element) and along frequency (stride one pitch) alike.  At most 62 x 97 keys = 24 056 bytes: six workgroups per CU.
//
// The median of W keys: W ds_reads into registers, then a selection network of min_u32 / max_u32 pairs.  The network is Batcher's
// odd-even merge sort for W inputs (the loop form that is valid for any W), built at compile time and pruned backwards from the
// one output that is used, rank (W - 1) / 2: 1, 3, 5, ..., 31 inputs need 0, 3, 8, 14, 24, 32, 39, 49, 70, 79, 91, 104, 113, 126, 138
// and 152 comparators (17 inputs: 70 of the sort's 85), against W^2 comparisons for rank counting.  The list is a constexpr table and the loop over it is unrolled, so
// every index is an immediate and nothing is spilled (tests/test_abi_host.py reads the code object's notes: no scratch).  The window
// sizes are runtime arguments: a uniform switch picks the instantiation, once for time and once for frequency.  The result cannot
// depend on the method: the element of rank r has well-defined bits.
//
// pg_ola_stretch.  A thread owns 4 consecutive output samples t0 .. t0 + 3 (t0 % 4 == 0) and walks the output frames that cover any
// of them in ascending g; the frame's centre c_g (one double multiply, one rint) is formed once for the four.  For one frame the
// four samples read x[s .. s + 3] and neighbouring threads the neighbouring quadruples: coalesced.  den and num are plain fp32
// accumulators per sample, so the order of the additions is the contract's whatever the launch looks like.  The window table is
// copied to LDS once per workgroup (at most 16 KiB).  16-byte stores where y and its row stride allow, sample by sample otherwise
// and for the last, partial quadruple of a row; the same function forms every sample on both paths.  No atomics, no workspace.
// Built with -ffp-contract=off like the rest; all index arithmetic is 64-bit.  Measurements: DESIGN.md section 4.15.
// pg_ola_stretch_map is the same kernel with the centre read from a table, one double per frame (OlMapped below; tests/_map_ref.py;
// DESIGN.md section 4.19).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_track.h"

namespace {

// ---- pg_hpss ---------------------------------------------------------------------------------------------------------------------
constexpr int HP_THREADS = 256;
constexpr int HP_TB = 32, HP_TF = 64;                                 // bins and frames of a tile
constexpr int HP_MAX_H = (PG_HPSS_MAX_WIN - 1) / 2;                   // 15
constexpr int HP_MAX_PITCH = HP_TF + 2 * HP_MAX_H + 3;                // 97
constexpr int HP_LDS = (HP_TB + 2 * HP_MAX_H) * HP_MAX_PITCH;

__device__ __forceinline__ uint32_t hp_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float hp_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// The comparators (a < b: the smaller key goes to a) that the output of rank (W - 1) / 2 depends on, in order.
template <int W>
struct HpNet { int n; unsigned char a[192], b[192]; };

template <int W>
constexpr HpNet<W> hp_make_net() {
    HpNet<W> all{}, net{};
    for (int p = 1; p < W; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k <= W - 1; j += 2 * k)
                for (int i = 0; i <= k - 1 && i <= W - j - k - 1; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        all.a[all.n] = (unsigned char)(i + j); all.b[all.n] = (unsigned char)(i + j + k); ++all.n;
                    }
    bool need[W] = {};
    bool keep[192] = {};
    need[(W - 1) / 2] = true;
    for (int c = all.n - 1; c >= 0; --c)
        if (need[all.a[c]] || need[all.b[c]]) { keep[c] = true; need[all.a[c]] = true; need[all.b[c]] = true; }
    for (int c = 0; c < all.n; ++c)
        if (keep[c]) { net.a[net.n] = all.a[c]; net.b[net.n] = all.b[c]; ++net.n; }
    return net;
}

template <int W>
__device__ __forceinline__ uint32_t hp_median(const uint32_t* p, int stride) {
    constexpr HpNet<W> net = hp_make_net<W>();
    uint32_t v[W];
#pragma unroll
    for (int d = 0; d < W; ++d) v[d] = p[d * stride];
#pragma unroll
    for (int c = 0; c < net.n; ++c) {
        const uint32_t x = v[net.a[c]], y = v[net.b[c]];
        v[net.a[c]] = x < y ? x : y;
        v[net.b[c]] = x < y ? y : x;
    }
    return v[(W - 1) / 2];
}

// the element of rank h among the 2 h + 1 keys p[0], p[stride], ...
__device__ __forceinline__ uint32_t hp_median_of(int h, const uint32_t* p, int stride) {
    switch (h) {
        case 0: return p[0];
        case 1: return hp_median<3>(p, stride);
        case 2: return hp_median<5>(p, stride);
        case 3: return hp_median<7>(p, stride);
        case 4: return hp_median<9>(p, stride);
        case 5: return hp_median<11>(p, stride);
        case 6: return hp_median<13>(p, stride);
        case 7: return hp_median<15>(p, stride);
        case 8: return hp_median<17>(p, stride);
        case 9: return hp_median<19>(p, stride);
        case 10: return hp_median<21>(p, stride);
        case 11: return hp_median<23>(p, stride);
        case 12: return hp_median<25>(p, stride);
        case 13: return hp_median<27>(p, stride);
        case 14: return hp_median<29>(p, stride);
        default: return hp_median<31>(p, stride);
    }
}

struct HpKernelArgs {
    const float* M; float* harm; float* perc;
    long m_stride, F, tiles_f, tiles_b, tiles;
    int bins, ht, hf, pitch;
};

template <bool VEC>
__global__ __launch_bounds__(HP_THREADS) void hpss_kernel(const HpKernelArgs a) {
    __shared__ uint32_t keys[HP_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows = HP_TB + 2 * a.hf, cols = HP_TF + 2 * a.ht;
    const int tx = (tid & 15) * 4, ty = tid >> 4;                     // the thread's 4 frames and its row in each half of the tile
    for (long t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const long tf = t % a.tiles_f, cb = t / a.tiles_f, tb = cb % a.tiles_b, c = cb / a.tiles_b;
        const long g0 = tf * HP_TF;
        const int b0 = (int)tb * HP_TB;
        const float* plane = a.M + c * a.m_stride;
        __syncthreads();                                              // the previous tile's reads are done
        for (int r = wave; r < rows; r += HP_THREADS / 64) {
            int b = b0 - a.hf + r;
            b = b < 0 ? 0 : (b < a.bins ? b : a.bins - 1);
            const float* row = plane + (long)b * a.F;
            for (int cc = lane; cc < cols; cc += 64) {
                long g = g0 - a.ht + cc;
                g = g < 0 ? 0 : (g < a.F ? g : a.F - 1);
                keys[r * a.pitch + cc] = hp_key(row[g]);
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            const int y = ty + half * (HP_TB / 2);
            const int b = b0 + y;
            const long g = g0 + tx;
            if (b >= a.bins || g >= a.F) continue;
            const int n = a.F - g < 4 ? (int)(a.F - g) : 4;
            f32x4 h = {0.0f, 0.0f, 0.0f, 0.0f}, p = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
            for (int i = 0; i < n; ++i) {
                // the cell is at LDS (y + hf, tx + i + ht); its time window begins ht columns before it, its frequency window hf rows above it
                const uint32_t* cell = keys + (y + a.hf) * a.pitch + (tx + i + a.ht);
                const uint32_t kh = hp_median_of(a.ht, cell - a.ht, 1);
                const uint32_t kp = hp_median_of(a.hf, cell - a.hf * a.pitch, a.pitch);
                const float m = hp_unkey(*cell);
                const bool harmonic = kh >= kp;
                const float hv = harmonic ? m : 0.0f, pv = harmonic ? 0.0f : m;
                // (a select per lane of the vector: i is a loop counter, not an immediate)
                h[0] = i == 0 ? hv : h[0]; h[1] = i == 1 ? hv : h[1]; h[2] = i == 2 ? hv : h[2]; h[3] = i == 3 ? hv : h[3];
                p[0] = i == 0 ? pv : p[0]; p[1] = i == 1 ? pv : p[1]; p[2] = i == 2 ? pv : p[2]; p[3] = i == 3 ? pv : p[3];
            }
            const long o = ((c * a.bins + b) * a.F) + g;
            if (VEC) {                                                // F % 4 == 0: the quadruple is whole and 16-byte aligned
                *(f32x4*)(a.harm + o) = h;
                *(f32x4*)(a.perc + o) = p;
            } else {
                if (n > 0) { a.harm[o] = h[0]; a.perc[o] = p[0]; }
                if (n > 1) { a.harm[o + 1] = h[1]; a.perc[o + 1] = p[1]; }
                if (n > 2) { a.harm[o + 2] = h[2]; a.perc[o + 2] = p[2]; }
                if (n > 3) { a.harm[o + 3] = h[3]; a.perc[o + 3] = p[3]; }
            }
        }
    }
}

// ---- pg_ola_stretch --------------------------------------------------------------------------------------------------------------
constexpr int OL_THREADS = 256;
constexpr int OL_MAX_WIN = 4096;

struct OlKernelArgs {
    const float* x; const float* win; const float* base; float* y;
    double src_per_out; const double* pos;                            // the grain grid below: Grid::of(args) takes its own
    long x_stride, base_stride, y_stride, n_in, n_out, units_per_row, units;
    int w, hop;
};

// The sample-grid twin of pg_track.h's time grid: where grain g, centred on output sample g hop, has its centre in the input.
//   OlUniform   cd = rint((double)(g hop) * src_per_out); never negative, so "beyond 2^62" is one comparison.
//   OlMapped    cd = rint(pos[g]), pos one double per grain: a centre that is NaN or beyond +-2^62 is outside every signal.  The
//               table ends with the last grain that covers an output sample, (n_out + w/2) / hop; a thread's unit of four may
//               reach one grain further, which covers only samples past the row's end, and last() stops there.
struct OlUniform {
    double spo;
    static __device__ __forceinline__ OlUniform of(const OlKernelArgs& a) { return OlUniform{a.src_per_out}; }
    __device__ __forceinline__ double centre(long g, long gh) const { return rint((double)gh * spo); }
    static __device__ __forceinline__ bool inside(double cd) { return cd < 4611686018427387904.0; }
    __device__ __forceinline__ long last(long g_hi, const OlKernelArgs&) const { return g_hi; }
};

struct OlMapped {
    const double* pos;
    static __device__ __forceinline__ OlMapped of(const OlKernelArgs& a) { return OlMapped{a.pos}; }
    __device__ __forceinline__ double centre(long g, long) const { return rint(pos[g]); }
    static __device__ __forceinline__ bool inside(double cd) { return fabs(cd) < 4611686018427387904.0; }   // (false for a NaN)
    __device__ __forceinline__ long last(long g_hi, const OlKernelArgs& a) const {
        const long end = (a.n_out + a.w / 2) / a.hop;
        return g_hi < end ? g_hi : end;
    }
};

// floor(a / b) for b > 0
__device__ __forceinline__ long ol_floor_div(long a, long b) { const long q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }

template <typename Grid, bool VEC>
__global__ __launch_bounds__(OL_THREADS) void ola_stretch_kernel(const OlKernelArgs a) {
    const Grid grid = Grid::of(a);
    __shared__ float win[OL_MAX_WIN];
    for (int j = threadIdx.x; j < a.w; j += OL_THREADS) win[j] = a.win[j];
    __syncthreads();
    const long stride = (long)gridDim.x * OL_THREADS;
    const long half = a.w / 2;
    for (long u = (long)blockIdx.x * OL_THREADS + threadIdx.x; u < a.units; u += stride) {
        const long r = u / a.units_per_row, t0 = (u - r * a.units_per_row) * 4;
        const float* xr = a.x + r * a.x_stride;
        const int n = a.n_out - t0 < 4 ? (int)(a.n_out - t0) : 4;
        // the frames that cover t: g hop - w/2 <= t <= g hop + w/2 - 1, g >= 0
        long g_lo = ol_floor_div(t0 - half + a.hop, a.hop);           // ceil((t0 - w/2 + 1) / hop)
        if (g_lo < 0) g_lo = 0;
        const long g_hi = grid.last((t0 + 3 + half) / a.hop, a);
        float den[4] = {0.0f, 0.0f, 0.0f, 0.0f}, num[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (long g = g_lo; g <= g_hi; ++g) {
            const long gh = g * a.hop;
            const double cd = grid.centre(g, gh);
            const bool inside = Grid::inside(cd);                     // a centre beyond 2^62 is outside every signal
            const long cg = inside ? (long)cd : 0;
            const long j0 = t0 - gh + half;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long j = j0 + i;
                if (j >= 0 && j < a.w) {
                    const float wv = win[j];
                    den[i] = den[i] + wv;
                    const long s = cg + j - half;
                    if (inside && s >= 0 && s < a.n_in) {
                        const float term = wv * xr[s];
                        num[i] = num[i] + term;
                    }
                }
            }
        }
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = den[i] > 0.0f ? num[i] / den[i] : 0.0f;
            if (a.base != nullptr && i < n) v = a.base[r * a.base_stride + t0 + i] + v;
            o[i] = v;
        }
        float* yp = a.y + r * a.y_stride + t0;
        if (VEC && n == 4) *(f32x4*)yp = o;
        else {
            if (n > 0) yp[0] = o[0];
            if (n > 1) yp[1] = o[1];
            if (n > 2) yp[2] = o[2];
            if (n > 3) yp[3] = o[3];
        }
    }
}

bool ol_window_ok(int32_t w) { return w >= 2 && w <= OL_MAX_WIN && (w & 1) == 0; }

// What the two ABI structs of pg_ola_stretch say differently: the grid (every other field has one name; the sizes and strides are
// int64 in the one and int32 in the other).
struct OlGrid { double src_per_out; const double* pos; };
OlGrid ol_grid(const pg_ola_stretch_args& a) { return OlGrid{a.src_per_out, nullptr}; }
OlGrid ol_grid(const pg_ola_stretch_map_args& a) { return OlGrid{0.0, a.pos}; }

// The checks of pg_ola_stretch and pg_ola_stretch_map, each row once, the kernel's arguments and the launch on Grid.  MAPPED: no
// src_per_out row, `pos` in the NULL and the ALIGN row (8 bytes); no int32 size reaches the 2^62 row.
template <typename Grid, bool MAPPED, typename Args>
int ol_plan(const char* op, const Args* a, void* stream) {
    if (!a || !a->x || !a->win || !a->y || (MAPPED && !ol_grid(*a).pos)) return pg_failf(PG_ERR_NULL, "%s: args, x, win%s required", op, MAPPED ? ", y and pos" : " and y");
    const OlGrid g = ol_grid(*a);
    if (a->n_sig <= 0 || a->n_in <= 0 || a->n_out <= 0) return pg_failf(PG_ERR_SHAPE, "%s: non-positive dimension", op);
    if (!ol_window_ok(a->win_len)) return pg_failf(PG_ERR_SHAPE, "%s: win_len must be even and within 2 .. %d", op, OL_MAX_WIN);
    if (a->hop < 1 || a->hop > a->win_len / 2) return pg_failf(PG_ERR_SHAPE, "%s: need 1 <= hop <= win_len / 2", op);
    if (!MAPPED && (!(g.src_per_out > 0.0) || !(g.src_per_out <= DBL_MAX))) return pg_failf(PG_ERR_SHAPE, "%s: src_per_out must be finite and positive", op);
    if (a->n_in > INT64_MAX / 2 || a->n_out > INT64_MAX / 2 / a->n_sig) return pg_failf(PG_ERR_SHAPE, "%s: signals beyond 2^62 elements", op);
    if (a->x_stride < a->n_in) return pg_failf(PG_ERR_SHAPE, "%s: x_stride shorter than a row", op);
    if (a->y_stride < a->n_out) return pg_failf(PG_ERR_SHAPE, "%s: y_stride shorter than a row", op);
    if (a->base && a->base_stride < a->n_out) return pg_failf(PG_ERR_SHAPE, "%s: base_stride shorter than a row", op);
    if ((((uintptr_t)a->x) & 3) || (((uintptr_t)a->win) & 3) || (((uintptr_t)a->base) & 3) || (((uintptr_t)a->y) & 3) || (((uintptr_t)g.pos) & 7))
        return pg_failf(PG_ERR_ALIGN, "%s: misaligned pointer", op);
    OlKernelArgs k;
    k.x = a->x; k.win = a->win; k.base = a->base; k.y = a->y;
    k.src_per_out = g.src_per_out; k.pos = g.pos;
    const bool one = a->n_sig == 1;                                   // (a stride that is never applied does not decide)
    k.x_stride = one ? 0 : a->x_stride; k.base_stride = one ? 0 : a->base_stride; k.y_stride = one ? 0 : a->y_stride;
    k.n_in = a->n_in; k.n_out = a->n_out;
    k.units_per_row = ((long)a->n_out + 3) / 4; k.units = k.units_per_row * a->n_sig;
    k.w = a->win_len; k.hop = a->hop;
    const bool wide = pg_al16(a->y) && (one || (a->y_stride & 3) == 0);
    const unsigned grid = pg_stream_grid(k.units, OL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL((ola_stretch_kernel<Grid, true>), dim3(grid), dim3(OL_THREADS), 0, st, k);
    else hipLaunchKernelGGL((ola_stretch_kernel<Grid, false>), dim3(grid), dim3(OL_THREADS), 0, st, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PG_OK : pg_failf((int)e, "%s launch failed", op);
}

}  // namespace

extern "C" int pg_hpss(const pg_hpss_args* a, void* stream) {
    if (!a || !a->M || !a->harm || !a->perc) return pg_fail(PG_ERR_NULL, "hpss: args, M, harm and perc required");
    if (a->n_ch <= 0 || a->bins <= 0 || a->F <= 0) return pg_fail(PG_ERR_SHAPE, "hpss: non-positive dimension");
    if (a->win_t < 1 || a->win_t > PG_HPSS_MAX_WIN || !(a->win_t & 1) || a->win_f < 1 || a->win_f > PG_HPSS_MAX_WIN || !(a->win_f & 1))
        return pg_failf(PG_ERR_SHAPE, "hpss: win_t and win_f must be odd and within 1 .. %d", PG_HPSS_MAX_WIN);
    if (a->F > INT64_MAX / 2 / a->bins) return pg_fail(PG_ERR_SHAPE, "hpss: plane beyond 2^62 elements");
    if (a->m_stride < (int64_t)a->bins * a->F) return pg_fail(PG_ERR_SHAPE, "hpss: m_stride shorter than a plane");
    if ((int64_t)a->n_ch * a->bins > INT64_MAX / 2 / a->F) return pg_fail(PG_ERR_SHAPE, "hpss: output beyond 2^62 elements");
    if ((((uintptr_t)a->M) & 3) || (((uintptr_t)a->harm) & 3) || (((uintptr_t)a->perc) & 3)) return pg_fail(PG_ERR_ALIGN, "hpss: misaligned pointer");
    HpKernelArgs k;
    k.M = a->M; k.harm = a->harm; k.perc = a->perc;
    k.m_stride = a->n_ch == 1 ? 0 : a->m_stride; k.F = a->F;
    k.tiles_f = (a->F + HP_TF - 1) / HP_TF; k.tiles_b = (a->bins + HP_TB - 1) / HP_TB; k.tiles = k.tiles_f * k.tiles_b * a->n_ch;
    k.bins = a->bins; k.ht = (a->win_t - 1) / 2; k.hf = (a->win_f - 1) / 2;
    k.pitch = HP_TF + 2 * k.ht + 1;                                   // 64 + 2 ht is even: + 1 or + 3 makes it 1 modulo 4
    if ((k.pitch & 3) != 1) k.pitch += 2;
    const bool wide = (a->F & 3) == 0 && pg_al16(a->harm) && pg_al16(a->perc);
    const unsigned grid = pg_stream_grid(k.tiles, 1);                 // a workgroup per tile
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL(hpss_kernel<true>, dim3(grid), dim3(HP_THREADS), 0, st, k);
    else hipLaunchKernelGGL(hpss_kernel<false>, dim3(grid), dim3(HP_THREADS), 0, st, k);
    return pg_launch_ok("hpss launch failed");
}

extern "C" int pg_ola_window(float* win_host, int32_t win_len) {
    if (!win_host) return pg_fail(PG_ERR_NULL, "ola_window: win_host required");
    if (!ol_window_ok(win_len)) return pg_failf(PG_ERR_SHAPE, "ola_window: win_len must be even and within 2 .. %d", OL_MAX_WIN);
    for (int j = 0; j < win_len; ++j) win_host[j] = (float)(0.5 - 0.5 * cos(2.0 * 3.141592653589793 * (double)j / (double)win_len));
    return PG_OK;
}

extern "C" int pg_ola_stretch(const pg_ola_stretch_args* a, void* stream) { return ol_plan<OlUniform, false>("ola_stretch", a, stream); }

// pg_ola_stretch with one source centre per grain (OlMapped)
extern "C" int pg_ola_stretch_map(const pg_ola_stretch_map_args* a, void* stream) { return ol_plan<OlMapped, true>("ola_stretch_map", a, stream); }
