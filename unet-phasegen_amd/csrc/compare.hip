// compare.hip -- how far a reconstruction is from its source, reduced on the device: pg_wave_compare (two sets of signals) and
// pg_spec_compare (two sets of spectrograms in pg_stft's layout).  Each call leaves six doubles per signal from which the host
// forms SI-SDR / SNR and spectral convergence / log-spectral distance (phasegen/metrics.py).  The reference has no counterpart (its
// validate.py takes mean absolute waveform errors of dataset clips on the host); the contract in include/phasegen.h is the
// specification and tests/test_compare_gpu.py restates it in float64.
//
// Both are HBM-bound reductions with the house rules of pg_moments and pg_stitch: per-workgroup partials in the caller's workspace,
// later launches fold them in a fixed order, sums in double, no floating-point atomics, 64-bit index arithmetic, validation on the
// host before any launch.  The partition and every summation tree are functions of the shapes alone -- constants below, never the
// grid, the CU count, n_signals or a signal's position -- so signal s of a batch has the bits of the same signal run alone.
//
// Lanes and loads.  A lane always owns 4 consecutive elements of the contiguous axis (samples / frames).  Where base pointers,
// strides (and for spectrograms frames % 4) allow, it fetches them as one 16-byte load, otherwise one by one (and the last, short
// group of a row always one by one); the arithmetic and its order per lane are the same, so both paths give the same bits.
//
// pg_wave_compare.  Row s is cut into chunks of WC_CHUNK = 8192 samples, one workgroup each: thread t of 256 takes the groups
// 4 (t + 256 i), i = 0..7, ascending, in double; xor-shuffle tree per wave, the four waves as (w0 + w1) + (w2 + w3); the chunk's six
// values go to the workspace.  compare_fold_kernel, one workgroup per signal, adds the chunks: thread t takes chunks t, t + 256, ...
// ascending, then the same tree.  Slot 4 is a maximum (exact in any order), slot 5 an integer count carried as a double.
//
// pg_spec_compare.  A workgroup takes SC_FRAMES = 256 frames (64 lanes x 4) by SC_BINS = 64 bins of one signal; its wave w walks
// bins 16 w .. 16 w + 15 of the block in ascending order, so lanes run along the contiguous frames and bins are split over the
// waves.  Per cell the four floats are widened first: mR, mE0, mE = g mE0, their products and (mR - mE)^2 are formed and added in
// double (no product of two inputs can overflow or vanish); L(m) = 10 log10f(max((float)(m m), floor)) and (L - L)^2 stay fp32.
// The per-frame sums of (L(mR) - L(mE))^2 of the four waves meet in LDS and are added in ascending bin order; the block's 256
// per-frame sums go to the workspace, its cell sums (slots 0-3, 5) through the tree above as well.  spec_tile_kernel (one
// workgroup per signal and frame tile) adds each frame's bin blocks in ascending order, takes sqrt(sum / bins), reduces the 256
// frames through the tree, and adds the tile's cell sums in ascending block order; compare_fold_kernel adds the tiles.
// Measurements and the compiler's resource report: DESIGN.md section 4.8.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_track.h"

namespace {

constexpr int CMP_THREADS = 256;
constexpr int WC_CHUNK = 8192;             // samples per workgroup of pg_wave_compare: 8 groups of 4 per thread
constexpr int SC_FRAMES = 256;             // frames per workgroup of pg_spec_compare: 64 lanes x 4
constexpr int SC_WBINS = 16;               // bins per wave
constexpr int SC_BINS = 4 * SC_WBINS;      // bins per workgroup

// Block-wide fold of six values; with MAX4 slot 4 is a maximum, else a sum.  Thread 0's copy is the result (every thread gets it).
template <bool MAX4>
__device__ __forceinline__ void cmp_block_reduce(double (&v)[6], double (*red)[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(v[k], off, 64);
            v[k] = (MAX4 && k == 4) ? fmax(v[k], o) : v[k] + o;
        }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; ++k)
        v[k] = (MAX4 && k == 4) ? fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k])) : (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// ---- pg_wave_compare ------------------------------------------------------------------------------------------------------------
struct WcKernelArgs {
    const float* x; const float* y; const double* gain; double* partial;
    long n, x_stride, y_stride;
    int nchunks;
};

template <int VEC>
__global__ __launch_bounds__(CMP_THREADS) void wave_compare_kernel(const WcKernelArgs a) {
    __shared__ double red[4][6];
    const long s = blockIdx.x / a.nchunks, c = blockIdx.x - s * a.nchunks;
    const float* xp = a.x + s * a.x_stride;
    const float* yp = a.y + s * a.y_stride;
    const double g = a.gain ? a.gain[s] : 1.0;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int bad = 0;
#pragma unroll 4
    for (int i = 0; i < WC_CHUNK / (4 * CMP_THREADS); ++i) {
        const long t = c * WC_CHUNK + 4L * (i * CMP_THREADS + (int)threadIdx.x);
        if (t < a.n) {
            float xv[4], yv[4];
            if (VEC == 4 && t + 4 <= a.n) {
                const f32x4 X = *(const f32x4*)(xp + t), Y = *(const f32x4*)(yp + t);
#pragma unroll
                for (int j = 0; j < 4; ++j) { xv[j] = X[j]; yv[j] = Y[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {                      // (samples past the row's end: zeros, which change no slot)
                    const bool in = t + j < a.n;
                    xv[j] = in ? xp[t + j] : 0.f;
                    yv[j] = in ? yp[t + j] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float xf = xv[j], yf = yv[j];
                if (!(pg_finite(xf) && pg_finite(yf))) { ++bad; xf = 0.f; yf = 0.f; }
                const double xd = (double)xf, yd = (double)yf;
                v[0] += xd * xd;
                v[1] += yd * yd;
                v[2] += xd * yd;
                const double d = xd - g * yd;
                v[3] += d * d;
                v[4] = fmax(v[4], fabs(d));
            }
        }
    }
    v[5] = (double)bad;
    cmp_block_reduce<true>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.partial[(long)blockIdx.x * 6 + k] = v[k];
    }
}

// out[s] = fold of partial[s][0 .. nparts): one workgroup per signal
template <bool MAX4>
__global__ __launch_bounds__(CMP_THREADS) void compare_fold_kernel(const double* __restrict__ partial, int nparts, double* __restrict__ out) {
    __shared__ double red[4][6];
    const double* p = partial + (long)blockIdx.x * nparts * 6;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nparts; i += CMP_THREADS) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double o = p[(long)i * 6 + k];
            v[k] = (MAX4 && k == 4) ? fmax(v[k], o) : v[k] + o;
        }
    }
    cmp_block_reduce<MAX4>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[(long)blockIdx.x * 6 + k] = v[k];
    }
}

// ---- pg_spec_compare ------------------------------------------------------------------------------------------------------------
struct ScKernelArgs {
    const float* R; const float* E; const double* gain;
    double* cellpart;      // (n_signals, ntiles, nblocks, 6): slots 0-3 and 5 of one workgroup (slot 4 unused)
    double* framepart;     // (n_signals, nblocks, frames): per-frame sums of (L(mR) - L(mE))^2 over one bin block
    double* tilepart;      // (n_signals, ntiles, 6)
    long r_stride, e_stride, plane;
    int bins, frames, ntiles, nblocks;
    float floor_power;
};

// the level stays an fp32 logarithm of the power rounded to fp32: it needs m m <= FLT_MAX (include/phasegen.h, "Magnitude range")
__device__ __forceinline__ float sc_level(double m, float floor_power) { return 10.f * log10f(fmaxf((float)(m * m), floor_power)); }

template <int VEC>
__global__ __launch_bounds__(CMP_THREADS) void spec_compare_kernel(const ScKernelArgs a) {
    __shared__ double red[4][6];
    __shared__ double fsum[4][SC_FRAMES];
    const int blk = blockIdx.x % a.nblocks, rest = blockIdx.x / a.nblocks;
    const int tile = rest % a.ntiles;
    const long s = rest / a.ntiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* Rp = a.R + s * a.r_stride;
    const float* Ep = a.E + s * a.e_stride;
    const float gf = a.gain ? (float)a.gain[s] : 1.f;
    const long f = (long)tile * SC_FRAMES + 4 * lane;
    const long nf = a.frames - f;                                    // frames of this lane's group that exist (<= 0: none)
    const int b_lo = blk * SC_BINS + wave * SC_WBINS;
    const int b_hi = min(b_lo + SC_WBINS, a.bins);
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double fs[4] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    if (nf > 0) {
#pragma unroll 2
        for (int b = b_lo; b < b_hi; ++b) {
            const long o = (long)b * a.frames + f;
            float rr[4], ri[4], er[4], ei[4];
            if (VEC == 4 && nf >= 4) {
                const f32x4 A = *(const f32x4*)(Rp + o), B = *(const f32x4*)(Rp + a.plane + o);
                const f32x4 C = *(const f32x4*)(Ep + o), D = *(const f32x4*)(Ep + a.plane + o);
#pragma unroll
                for (int j = 0; j < 4; ++j) { rr[j] = A[j]; ri[j] = B[j]; er[j] = C[j]; ei[j] = D[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {                      // (frames past the end: zero cells, which change no slot)
                    const bool in = j < nf;
                    rr[j] = in ? Rp[o + j] : 0.f;
                    ri[j] = in ? Rp[a.plane + o + j] : 0.f;
                    er[j] = in ? Ep[o + j] : 0.f;
                    ei[j] = in ? Ep[a.plane + o + j] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!(pg_finite(rr[j]) && pg_finite(ri[j]) && pg_finite(er[j]) && pg_finite(ei[j]))) {
                    ++bad;
                    rr[j] = ri[j] = er[j] = ei[j] = 0.f;
                }
                // widened BEFORE any product (as wave_compare_kernel does): the squares of two floats are exact doubles at every
                // exponent, so nothing overflows above 2^63.5 or vanishes below 2^-75 on its way into the sums
                const double rrd = (double)rr[j], rid = (double)ri[j], erd = (double)er[j], eid = (double)ei[j];
                const double mR = sqrt(rrd * rrd + rid * rid);
                const double mE0 = sqrt(erd * erd + eid * eid);
                const double mE = (double)gf * mE0;
                const double d = mR - mE;
                v[0] += mR * mR;
                v[1] += mE0 * mE0;
                v[2] += mR * mE0;
                v[3] += d * d;
                const float dl = sc_level(mR, a.floor_power) - sc_level(mE, a.floor_power);
                fs[j] += (double)(dl * dl);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) fsum[wave][4 * lane + j] = fs[j];
    v[5] = (double)bad;
    cmp_block_reduce<false>(v, red);                                 // (its barriers also publish fsum)
    const long ft = (long)tile * SC_FRAMES + (int)threadIdx.x;
    if (ft < a.frames)                                               // the four waves' bins in ascending order
        a.framepart[(s * a.nblocks + blk) * a.frames + ft] = ((fsum[0][threadIdx.x] + fsum[1][threadIdx.x]) + fsum[2][threadIdx.x]) + fsum[3][threadIdx.x];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.cellpart[(long)blockIdx.x * 6 + k] = v[k];
    }
}

// one workgroup per (signal, frame tile): per frame the bin blocks in ascending order, sqrt(sum / bins), the 256 frames through the
// tree; the tile's cell sums in ascending block order
__global__ __launch_bounds__(CMP_THREADS) void spec_tile_kernel(const ScKernelArgs a) {
    __shared__ double red[4][6];
    const int tile = blockIdx.x % a.ntiles;
    const long s = blockIdx.x / a.ntiles;
    const long ft = (long)tile * SC_FRAMES + (int)threadIdx.x;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ft < a.frames) {
        double sum = 0.0;
        for (int b = 0; b < a.nblocks; ++b) sum += a.framepart[(s * a.nblocks + b) * a.frames + ft];
        v[4] = sqrt(sum / (double)a.bins);
    }
    if (threadIdx.x == 0) {
        const double* cp = a.cellpart + (long)blockIdx.x * a.nblocks * 6;
        for (int b = 0; b < a.nblocks; ++b) {
#pragma unroll
            for (int k = 0; k < 6; ++k) if (k != 4) v[k] += cp[b * 6 + k];
        }
    }
    cmp_block_reduce<false>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.tilepart[(long)blockIdx.x * 6 + k] = v[k];
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int wc_check(const pg_wave_compare_args* a, int64_t* nchunks) {
    if (!a) return pg_fail(PG_ERR_NULL, "wave_compare: null args");
    if (a->n_signals <= 0 || a->n <= 0) return pg_fail(PG_ERR_SHAPE, "wave_compare: non-positive dimension");
    const int64_t nc = (a->n + WC_CHUNK - 1) / WC_CHUNK;
    if (nc > INT32_MAX / a->n_signals) return pg_fail(PG_ERR_SHAPE, "wave_compare: n_signals * ceil(n / 8192) beyond 2^31");
    *nchunks = nc;
    return PG_OK;
}

struct ScPlan { int64_t ntiles, nblocks, cell_elems, tile_elems, frame_elems; };

int sc_check(const pg_spec_compare_args* a, ScPlan* p) {
    if (!a) return pg_fail(PG_ERR_NULL, "spec_compare: null args");
    if (a->n_signals <= 0 || a->bins <= 0 || a->frames <= 0) return pg_fail(PG_ERR_SHAPE, "spec_compare: non-positive dimension");
    if (!(a->floor_power > 0.f) || !pg_finite(a->floor_power)) return pg_fail(PG_ERR_SHAPE, "spec_compare: floor_power must be positive and finite");
    p->ntiles = ((int64_t)a->frames + SC_FRAMES - 1) / SC_FRAMES;
    p->nblocks = ((int64_t)a->bins + SC_BINS - 1) / SC_BINS;
    if (p->ntiles * p->nblocks > INT32_MAX / a->n_signals) return pg_fail(PG_ERR_SHAPE, "spec_compare: more than 2^31 workgroups");
    p->cell_elems = (int64_t)a->n_signals * p->ntiles * p->nblocks * 6;
    p->tile_elems = (int64_t)a->n_signals * p->ntiles * 6;
    p->frame_elems = (int64_t)a->n_signals * p->nblocks * a->frames;
    return PG_OK;
}

}  // namespace

extern "C" int64_t pg_workspace_bytes_wave_compare(const pg_wave_compare_args* a) {
    int64_t nc;
    if (int e = wc_check(a, &nc)) return e;
    return (int64_t)a->n_signals * nc * 6 * (int64_t)sizeof(double);
}

extern "C" int pg_wave_compare(const pg_wave_compare_args* a, void* stream) {
    int64_t nc;
    if (int e = wc_check(a, &nc)) return e;
    if (a->x_stride < a->n) return pg_fail(PG_ERR_SHAPE, "wave_compare: x_stride shorter than a row");
    if (a->y_stride < a->n) return pg_fail(PG_ERR_SHAPE, "wave_compare: y_stride shorter than a row");
    if (!a->x || !a->y || !a->out) return pg_fail(PG_ERR_NULL, "wave_compare: x, y and out required");
    if (((uintptr_t)a->x & 3) || ((uintptr_t)a->y & 3) || ((uintptr_t)a->out & 7) || ((uintptr_t)a->gain & 7))
        return pg_fail(PG_ERR_ALIGN, "wave_compare: misaligned pointer");
    if (!a->workspace || a->workspace_bytes < pg_workspace_bytes_wave_compare(a))
        return pg_fail(PG_ERR_WORKSPACE, "wave_compare: needs a workspace of pg_workspace_bytes_wave_compare() bytes");
    if ((uintptr_t)a->workspace & 7) return pg_fail(PG_ERR_ALIGN, "wave_compare: workspace must be 8-byte aligned");
    // (a stride that is never applied -- one signal -- does not decide)
    const bool wide = pg_al16(a->x) && pg_al16(a->y) && (a->n_signals == 1 || ((a->x_stride & 3) == 0 && (a->y_stride & 3) == 0));
    WcKernelArgs k;
    k.x = a->x; k.y = a->y; k.gain = a->gain; k.partial = (double*)a->workspace;
    k.n = a->n; k.x_stride = a->n_signals == 1 ? 0 : a->x_stride; k.y_stride = a->n_signals == 1 ? 0 : a->y_stride;
    k.nchunks = (int)nc;
    const unsigned grid = (unsigned)(nc * a->n_signals);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL(wave_compare_kernel<4>, dim3(grid), dim3(CMP_THREADS), 0, st, k);
    else hipLaunchKernelGGL(wave_compare_kernel<1>, dim3(grid), dim3(CMP_THREADS), 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pg_fail((int)e, "wave_compare launch failed");
    hipLaunchKernelGGL(compare_fold_kernel<true>, dim3((unsigned)a->n_signals), dim3(CMP_THREADS), 0, st, (const double*)k.partial, k.nchunks, a->out);
    e = hipGetLastError();
    if (e != hipSuccess) return pg_fail((int)e, "wave_compare second-stage launch failed");
    return PG_OK;
}

extern "C" int64_t pg_workspace_bytes_spec_compare(const pg_spec_compare_args* a) {
    ScPlan p;
    if (int e = sc_check(a, &p)) return e;
    return (p.cell_elems + p.tile_elems + p.frame_elems) * (int64_t)sizeof(double);
}

extern "C" int pg_spec_compare(const pg_spec_compare_args* a, void* stream) {
    ScPlan p;
    if (int e = sc_check(a, &p)) return e;
    const int64_t plane = (int64_t)a->bins * a->frames;
    if (a->r_stride < 2 * plane) return pg_fail(PG_ERR_SHAPE, "spec_compare: r_stride shorter than a signal (2 * bins * frames)");
    if (a->e_stride < 2 * plane) return pg_fail(PG_ERR_SHAPE, "spec_compare: e_stride shorter than a signal (2 * bins * frames)");
    if (!a->R || !a->E || !a->out) return pg_fail(PG_ERR_NULL, "spec_compare: R, E and out required");
    if (((uintptr_t)a->R & 3) || ((uintptr_t)a->E & 3) || ((uintptr_t)a->out & 7) || ((uintptr_t)a->gain & 7))
        return pg_fail(PG_ERR_ALIGN, "spec_compare: misaligned pointer");
    if (!a->workspace || a->workspace_bytes < pg_workspace_bytes_spec_compare(a))
        return pg_fail(PG_ERR_WORKSPACE, "spec_compare: needs a workspace of pg_workspace_bytes_spec_compare() bytes");
    if ((uintptr_t)a->workspace & 7) return pg_fail(PG_ERR_ALIGN, "spec_compare: workspace must be 8-byte aligned");
    const bool wide = (a->frames & 3) == 0 && pg_al16(a->R) && pg_al16(a->E)
                      && (a->n_signals == 1 || ((a->r_stride & 3) == 0 && (a->e_stride & 3) == 0));
    ScKernelArgs k;
    k.R = a->R; k.E = a->E; k.gain = a->gain;
    k.cellpart = (double*)a->workspace; k.tilepart = k.cellpart + p.cell_elems; k.framepart = k.tilepart + p.tile_elems;
    k.r_stride = a->n_signals == 1 ? 0 : a->r_stride; k.e_stride = a->n_signals == 1 ? 0 : a->e_stride; k.plane = plane;
    k.bins = a->bins; k.frames = a->frames; k.ntiles = (int)p.ntiles; k.nblocks = (int)p.nblocks;
    k.floor_power = a->floor_power;
    const unsigned grid = (unsigned)(p.ntiles * p.nblocks * a->n_signals);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL(spec_compare_kernel<4>, dim3(grid), dim3(CMP_THREADS), 0, st, k);
    else hipLaunchKernelGGL(spec_compare_kernel<1>, dim3(grid), dim3(CMP_THREADS), 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pg_fail((int)e, "spec_compare launch failed");
    hipLaunchKernelGGL(spec_tile_kernel, dim3((unsigned)(p.ntiles * a->n_signals)), dim3(CMP_THREADS), 0, st, k);
    e = hipGetLastError();
    if (e != hipSuccess) return pg_fail((int)e, "spec_compare second-stage launch failed");
    hipLaunchKernelGGL(compare_fold_kernel<false>, dim3((unsigned)a->n_signals), dim3(CMP_THREADS), 0, st, (const double*)k.tilepart, k.ntiles, a->out);
    e = hipGetLastError();
    if (e != hipSuccess) return pg_fail((int)e, "spec_compare third-stage launch failed");
    return PG_OK;
}
