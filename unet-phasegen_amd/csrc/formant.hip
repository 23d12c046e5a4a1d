// formant.hip -- pg_formant_shift: the spectral envelope of every frame of a log1p-magnitude plane and, optionally, the plane with
// that envelope re-imposed at `ratio` times each bin's frequency (phasegen/track.py, formant_semitones / pitch_shift(formants="keep")).
// The reference has no counterpart; include/phasegen.h states the arithmetic and tests/_formant_ref.py restates it in float64.
//
// The estimator is a peak hold along frequency followed by 1 + iters passes of a liftered cosine smoother S = T' diag(s) T, T the
// order x bins table pg_formant_basis fills.  Frames are the contiguous axis of the plane, so with N = frames both halves of a pass
// are plain GEMMs without a transpose, C (order x N) = T (order x bins) V (bins x N) and E (bins x N) = T' (bins x order) C, and
// they run on the fp32 MFMA (v_mfma_f32_32x32x2f32, the fragments of conv_common.h).
//
// One 256-thread workgroup owns a tile of FT consecutive frames x ALL bins of one channel; tiles are walked grid-stride with a 64-bit
// index.  LDS holds ONE plane of the tile, H (bins rounded up to 32 rows x FT, rows past `bins` zero), and 24 KiB beside it:
//   1. peak hold: the tile of x goes into H with 16-byte global loads, eight in flight per thread, and h replaces it IN PLACE, 64
//      rows at a time: a thread forms 4 consecutive rows x 4 frames from the part their windows share plus three rows on either
//      side (2 hold + 4 LDS reads for four results, row indices clamped: edge replication) into one of three 8 KiB slots beside H,
//      and a slot is written back one round later, when the round after it has read the rows it replaces (hold <= 64 rows).  A
//      maximum is exact in any order.
//   2. first product: wave w owns the 32-bin blocks w, w + 4, ...  It reads a block of H in the MFMA ACCUMULATOR layout (register r
//      of lane l: bin (r & 3) + 8 (r >> 2) + 4 (l >> 5), frame l & 31), which serves as the B operand of 16 k-steps in the order
//      the registers have; the A operand, T[q][those bins], is four 16-byte loads per lane from L2.  Each wave keeps its part of C
//      in registers; the four parts are added through LDS in wave order ((w0 + w1) + w2) + w3 and scaled by s[q] there.
//   3. second product and the next pass's first, fused: for a block of its own a wave forms E = T' C (A: 32 consecutive bins of a
//      table row per half wave, coalesced; B: C from LDS), takes v = max(h, E) against H in the same layout IN REGISTERS and feeds
//      it straight back as the B operand of step 2 for the next pass.  The envelope never touches LDS between passes.
//   4. the last pass writes E over H (nobody needs h any more), and after a barrier the epilogue walks the tile row by row, four
//      frames per thread: env gets E, out gets log1p(expm1(x) a / b) with the envelope read at the warped position from LDS and x
//      re-read from the plane (the tile was read moments ago: L2).  16-byte stores where pointers and F allow.
// The order of every sum along K is a function of (bins, order): block b belongs to wave b % 4 whatever the tile, MFMA columns do
// not mix, and a column's arithmetic does not depend on which column it is -- so a frame's bits depend on nothing but the frame,
// and a non-finite cell stays in its own (channel, frame).  Rows of the table past `order` and columns past `bins` are read as
// zero and the matching rows of H and C are written as zero, so no uninitialised LDS word is ever multiplied.
// FT = 32 up to 1024 bins (H = 128 KiB), 16 up to 2048, 8 up to 4096: the MFMA is 32 columns wide, columns past FT compute on
// zeros and are dropped.  Built with -ffp-contract=off like the rest.  Measurements: DESIGN.md section 4.18.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_track.h"
#include "pg_fastmath.h"
#include "conv_common.h"

namespace {

constexpr int FM_THREADS = 256;
constexpr int FM_MAX_BINS = 4096, FM_MAX_ORDER = 64, FM_MAX_HOLD = 64, FM_MAX_ITERS = 16;
constexpr int FM_CH = 64;                                             // rows of H one round of the peak hold replaces
constexpr int FM_AUX = 3 * FM_CH * 32;                                // floats beside H: three slots of held rows, later C (64 x 32)

struct FmKernelArgs {
    const float* M; const float* basis; float* env; float* out;
    double ratio;
    long m_stride, F, tiles_f, tiles;
    float eps;
    int bins, order, hold, iters, ft, nb;
    int vec_in, vec_tab, vec_env, vec_out;
};

// bin (inside its 32-bin block) that accumulator register r of a lane in half hh holds
__device__ __forceinline__ int fm_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

__device__ __forceinline__ f32x4 fm_max4(f32x4 a, f32x4 b) {
    f32x4 r;
    r[0] = fmaxf(a[0], b[0]); r[1] = fmaxf(a[1], b[1]); r[2] = fmaxf(a[2], b[2]); r[3] = fmaxf(a[3], b[3]);
    return r;
}

// frames g .. g + 3 of a row of F frames; a frame past the end reads as zero
template <bool VEC>
__device__ __forceinline__ f32x4 fm_load4(const float* row, long g, long F) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC) { if (g < F) v = *(const f32x4*)(row + g); }             // F % 4 == 0, g % 4 == 0: the quadruple is whole
    else {
        if (g < F) v[0] = row[g];
        if (g + 1 < F) v[1] = row[g + 1];
        if (g + 2 < F) v[2] = row[g + 2];
        if (g + 3 < F) v[3] = row[g + 3];
    }
    return v;
}

__device__ __forceinline__ void fm_store4(float* p, f32x4 v, int n, bool vec) {
    if (vec) *(f32x4*)p = v;                                          // (n == 4 there)
    else {
        if (n > 0) p[0] = v[0];
        if (n > 1) p[1] = v[1];
        if (n > 2) p[2] = v[2];
        if (n > 3) p[3] = v[3];
    }
}

// table entries T[q][k .. k + 3] (k % 4 == 0); a column past `bins` and a row past `order` (ok false) read as zero
__device__ __forceinline__ f32x4 fm_tab4(const float* trow, int k, int bins, bool ok, bool vec) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!ok) return v;
    if (vec) { if (k < bins) v = *(const f32x4*)(trow + k); }         // bins % 4 == 0
    else {
        if (k < bins) v[0] = trow[k];
        if (k + 1 < bins) v[1] = trow[k + 1];
        if (k + 2 < bins) v[2] = trow[k + 2];
        if (k + 3 < bins) v[3] = trow[k + 3];
    }
    return v;
}

// One 32-bin block b of a pass.  FIRST: v = h, the block of H in the accumulator layout.  Otherwise E = T'[block b, :] C (C: 64 x 32 in
// LDS, rows past `order` zero; k-steps of two coefficients, q = 2 s + hh) and then, on the last pass, E goes to H and nothing else
// happens; on the others v = max(h, E).  Then C' += T[:, block b] v (k-step r: the bin fm_row(r, hh) of the block), per wave, in
// `cacc`.  The table entries of BOTH products are loaded together (fm_tab_load) before the block's first MFMA: one memory latency
// per block, not one per k-step.
// An order of at most 32 runs half the k-steps of the second product and one row block of the first.
struct FmTab { f32x4 t1[2][4]; float t2[8][4]; };

template <bool FIRST>
__device__ __forceinline__ void fm_tab_load(const FmKernelArgs& a, int b, FmTab& tb, int nmb, int col, int hh, bool last) {
    if (FIRST || !last) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            if (mb >= nmb) continue;
            const int q = 32 * mb + col;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) tb.t1[mb][r4] = fm_tab4(a.basis + (long)q * a.bins, 32 * b + 8 * r4 + 4 * hh, a.bins, q < a.order, a.vec_tab);
        }
    }
    if (!FIRST) {
        const int k = 32 * b + col;
        const bool kok = k < a.bins;
        const float* tcol = a.basis + k;
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) {
            if (s4 >= 4 * nmb) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 8 * s4 + 2 * j + hh;
                tb.t2[s4][j] = (kok && q < a.order) ? tcol[(long)q * a.bins] : 0.0f;
            }
        }
    }
}

template <bool FIRST>
__device__ __forceinline__ void fm_block(const FmKernelArgs& a, int b, const FmTab& tb, float* H, const float* C, f32x16 (&cacc)[2], int nmb, int ft,
                                         int col, int hh, bool colok, bool last) {
    f32x16 v;
    if (FIRST) {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = colok ? H[(32 * b + fm_row(r, hh)) * ft + col] : 0.0f;
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = 0.0f;
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) {
            if (s4 >= 4 * nmb) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) v = __builtin_amdgcn_mfma_f32_32x32x2f32(tb.t2[s4][j], C[(8 * s4 + 2 * j + hh) * 32 + col], v, 0, 0, 0);
        }
        if (last) {
            if (colok) {
#pragma unroll
                for (int r = 0; r < 16; ++r) H[(32 * b + fm_row(r, hh)) * ft + col] = v[r];
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = fmaxf(colok ? H[(32 * b + fm_row(r, hh)) * ft + col] : 0.0f, v[r]);
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        if (mb >= nmb) continue;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
            for (int i = 0; i < 4; ++i) cacc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(tb.t1[mb][r4][i], v[4 * r4 + i], cacc[mb], 0, 0, 0);
    }
}

template <bool FIRST>
__device__ __forceinline__ void fm_walk(const FmKernelArgs& a, float* H, const float* C, f32x16 (&cacc)[2], int nmb, int ft, int wave, int col, int hh,
                                        bool colok, bool last) {
    for (int b = wave; b < a.nb; b += FM_THREADS / 64) {
        FmTab tb;
        fm_tab_load<FIRST>(a, b, tb, nmb, col, hh, last);
        fm_block<FIRST>(a, b, tb, H, C, cacc, nmb, ft, col, hh, colok, last);
    }
}

// the four waves' parts of C, added in wave order and scaled: C[q] = s[q] (((w0 + w1) + w2) + w3), rows past `order` zero
__device__ __forceinline__ void fm_reduce(const FmKernelArgs& a, float* C, const f32x16 (&cacc)[2], int nmb, int wave, int col, int hh) {
    __syncthreads();                                                  // the previous pass's reads of C (or of the staged rows) are done
    for (int w = 0; w < FM_THREADS / 64; ++w) {
        if (wave == w) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                if (mb >= nmb) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int q = 32 * mb + fm_row(r, hh);
                    float s = cacc[mb][r];
                    if (w > 0) s = C[q * 32 + col] + s;
                    if (w == FM_THREADS / 64 - 1) s = q < a.order ? a.basis[(long)a.order * a.bins + q] * s : 0.0f;
                    C[q * 32 + col] = s;
                }
            }
        }
        __syncthreads();
    }
}

template <bool VIN>
__global__ __launch_bounds__(FM_THREADS) void formant_kernel(const FmKernelArgs a) {
    extern __shared__ __attribute__((aligned(16))) float fm_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, hh = lane >> 5;
    const int ft = a.ft, qpr = ft >> 2, qsh = ft == 32 ? 3 : (ft == 16 ? 2 : 1), rows_pad = a.nb * 32;   // qpr = 1 << qsh quadruples per row
    float* H = fm_lds;
    float* AUX = fm_lds + rows_pad * ft;
    const int nmb = (a.order + 31) >> 5;
    const bool colok = col < ft;
    for (long t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const long c = t / a.tiles_f, g0 = (t - c * a.tiles_f) * ft;
        const float* plane = a.M + c * a.m_stride;
        __syncthreads();                                              // the previous tile's epilogue is done with H
        // ---- 1. peak hold -------------------------------------------------------------------------------------------------------
        // the tile of x into H (rows past `bins` zero), then h over it in place: 64 rows at a time into one of three slots beside H,
        // written back one round later, when the round after them has read the rows they replace (hold <= 64: its lowest row)
        const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int base = tid; base < rows_pad * qpr; base += 8 * FM_THREADS) {           // eight loads in flight per thread
            f32x4 buf[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int u = base + i * FM_THREADS, k = u >> qsh, qd = u & (qpr - 1);
                buf[i] = k < a.bins ? fm_load4<VIN>(plane + (long)k * a.F, g0 + 4 * qd, a.F) : zero;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int u = base + i * FM_THREADS;
                if (u < rows_pad * qpr) *(f32x4*)(H + u * 4) = buf[i];
            }
        }
        __syncthreads();
        if (a.hold > 0) {
            const int nchunk = (rows_pad + FM_CH - 1) / FM_CH, top = a.bins - 1;
            for (int ch = 0; ch <= nchunk; ++ch) {
                if (ch < nchunk) {
                    float* slot = AUX + (ch % 3) * FM_CH * ft;
                    for (int u = tid; u < (FM_CH / 4) * qpr; u += FM_THREADS) {
                        const int rg = u >> qsh, qd = u & (qpr - 1), kf = FM_CH * ch + 4 * rg;    // the group's first bin
                        const float* X = H + 4 * qd;
#define FM_X(j) (*(const f32x4*)(X + (kf + (j) < 0 ? 0 : (kf + (j) < top ? kf + (j) : top)) * ft))
                        f32x4 h[4];
                        if (a.hold >= 2) {                            // what the four windows share, then three rows on either side
                            f32x4 cm = FM_X(3 - a.hold);
                            int j = 4 - a.hold;
                            for (; j + 3 <= a.hold; j += 4) {         // four reads in flight
                                const f32x4 x0 = FM_X(j), x1 = FM_X(j + 1), x2 = FM_X(j + 2), x3 = FM_X(j + 3);
                                cm = fm_max4(cm, fm_max4(fm_max4(x0, x1), fm_max4(x2, x3)));
                            }
                            for (; j <= a.hold; ++j) cm = fm_max4(cm, FM_X(j));
                            const f32x4 a2 = FM_X(2 - a.hold);
                            const f32x4 a1 = fm_max4(a2, FM_X(1 - a.hold));
                            const f32x4 a0 = fm_max4(a1, FM_X(-a.hold));
                            const f32x4 b1 = FM_X(a.hold + 1);
                            const f32x4 b2 = fm_max4(b1, FM_X(a.hold + 2));
                            const f32x4 b3 = fm_max4(b2, FM_X(a.hold + 3));
                            h[0] = fm_max4(cm, a0);
                            h[1] = fm_max4(fm_max4(cm, a1), b1);
                            h[2] = fm_max4(fm_max4(cm, a2), b2);
                            h[3] = fm_max4(cm, b3);
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i) h[i] = fm_max4(fm_max4(FM_X(i), FM_X(i - 1)), FM_X(i + 1));
                        }
#undef FM_X
#pragma unroll
                        for (int i = 0; i < 4; ++i) *(f32x4*)(slot + (4 * rg + i) * ft + 4 * qd) = h[i];
                    }
                }
                __syncthreads();
                if (ch >= 1) {
                    const float* slot = AUX + ((ch - 1) % 3) * FM_CH * ft;
                    for (int u = tid; u < FM_CH * qpr; u += FM_THREADS) {
                        const int r = u >> qsh, qd = u & (qpr - 1), k = FM_CH * (ch - 1) + r;
                        if (k < a.bins) *(f32x4*)(H + k * ft + 4 * qd) = *(const f32x4*)(slot + r * ft + 4 * qd);
                    }
                }
            }
            __syncthreads();
        }
        // ---- 2. C = T h ---------------------------------------------------------------------------------------------------------
        f32x16 cacc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { cacc[0][r] = 0.0f; cacc[1][r] = 0.0f; }
        fm_walk<true>(a, H, AUX, cacc, nmb, ft, wave, col, hh, colok, false);
        // ---- 3. passes: e = T' diag(s) C, and C = T max(h, e) for the next one ---------------------------------------------------------
        for (int pass = 0; ; ++pass) {
            fm_reduce(a, AUX, cacc, nmb, wave, col, hh);
            const bool last = pass == a.iters;
#pragma unroll
            for (int r = 0; r < 16; ++r) { cacc[0][r] = 0.0f; cacc[1][r] = 0.0f; }
            fm_walk<false>(a, H, AUX, cacc, nmb, ft, wave, col, hh, colok, last);
            if (last) break;
        }
        __syncthreads();
        // ---- 4. epilogue: H holds the envelope ------------------------------------------------------------------------------------------
        for (int base = tid; base < a.bins * qpr; base += 4 * FM_THREADS) {               // four rows' reads of x in flight per thread
          f32x4 xs[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
              const int u = base + i * FM_THREADS, k = u >> qsh, qd = u & (qpr - 1);
              xs[i] = (a.out != nullptr && k < a.bins) ? fm_load4<VIN>(plane + (long)k * a.F, g0 + 4 * qd, a.F) : zero;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int u = base + i * FM_THREADS, k = u >> qsh, qd = u & (qpr - 1);
            const long g = g0 + 4 * qd;
            if (k >= a.bins || g >= a.F) continue;
            const int n = a.F - g < 4 ? (int)(a.F - g) : 4;
            const f32x4 e = *(const f32x4*)(H + k * ft + 4 * qd);
            const long o = (c * a.bins + k) * a.F + g;
            if (a.env) fm_store4(a.env + o, e, n, a.vec_env);
            if (a.out) {
                const f32x4 x = xs[i];
                f32x4 y = x;                                          // ratio == 1.0: the plane's bits
                if (a.ratio != 1.0) {
                    double p = (double)(k + 1) * a.ratio - 1.0;
                    p = p < 0.0 ? 0.0 : (p < (double)(a.bins - 1) ? p : (double)(a.bins - 1));
                    const int i0 = (int)floor(p), i1 = i0 + 1 < a.bins ? i0 + 1 : a.bins - 1;
                    const float w = (float)(p - (double)i0);
                    const f32x4 e0 = *(const f32x4*)(H + i0 * ft + 4 * qd), e1 = *(const f32x4*)(H + i1 * ft + 4 * qd);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float ew = e0[i] + w * (e1[i] - e0[i]);
                        const float aa = pg_expm1_ref(fmaxf(ew, 0.0f)) + a.eps;
                        const float bb = pg_expm1_ref(fmaxf(e[i], 0.0f)) + a.eps;
                        const float lin = pg_expm1_ref(x[i]) * (aa / bb);
                        y[i] = x[i] == 0.0f ? 0.0f : pg_log1p_pos(lin);
                    }
                }
                fm_store4(a.out + o, y, n, a.vec_out);
            }
          }
        }
    }
}

bool fm_basis_ok(int32_t bins, int32_t order) { return bins >= 1 && bins <= FM_MAX_BINS && order >= 1 && order <= FM_MAX_ORDER && order <= bins; }

}  // namespace

extern "C" int64_t pg_formant_basis_elems(int32_t bins, int32_t order) {
    if (!fm_basis_ok(bins, order)) return pg_failf(PG_ERR_SHAPE, "formant_basis: need 1 <= bins <= %d and 1 <= order <= min(bins, %d)", FM_MAX_BINS, FM_MAX_ORDER);
    return (int64_t)order * bins + order;
}

extern "C" int pg_formant_basis(float* basis_host, int32_t bins, int32_t order) {
    if (!basis_host) return pg_fail(PG_ERR_NULL, "formant_basis: basis_host required");
    if (!fm_basis_ok(bins, order)) return pg_failf(PG_ERR_SHAPE, "formant_basis: need 1 <= bins <= %d and 1 <= order <= min(bins, %d)", FM_MAX_BINS, FM_MAX_ORDER);
    const double pi = 3.141592653589793;
    for (int q = 0; q < order; ++q)
        for (int k = 0; k < bins; ++k) basis_host[(long)q * bins + k] = (float)cos(pi * (double)q * ((double)k + 0.5) / (double)bins);
    for (int q = 0; q < order; ++q) {
        const double cq = (q == 0 ? 1.0 : 2.0) / (double)bins, wq = 0.5 * (1.0 + cos(pi * (double)q / (double)order));
        basis_host[(long)order * bins + q] = (float)(cq * wq);
    }
    return PG_OK;
}

extern "C" int pg_formant_shift(const pg_formant_args* a, void* stream) {
    if (!a || !a->M || !a->basis || (!a->env && !a->out)) return pg_fail(PG_ERR_NULL, "formant_shift: args, M, basis and one of env and out required");
    if (a->n_ch <= 0 || a->bins <= 0 || a->F <= 0) return pg_fail(PG_ERR_SHAPE, "formant_shift: non-positive dimension");
    if (a->bins > FM_MAX_BINS) return pg_failf(PG_ERR_SHAPE, "formant_shift: more than %d bins", FM_MAX_BINS);
    if (a->m_ch_rows < a->bins) return pg_fail(PG_ERR_SHAPE, "formant_shift: m_ch_rows shorter than a plane");
    if (a->order < 1 || a->order > FM_MAX_ORDER || a->order > a->bins) return pg_failf(PG_ERR_SHAPE, "formant_shift: order must be within 1 .. min(bins, %d)", FM_MAX_ORDER);
    if (a->hold < 0 || a->hold > FM_MAX_HOLD) return pg_failf(PG_ERR_SHAPE, "formant_shift: hold must be within 0 .. %d", FM_MAX_HOLD);
    if (a->iters < 0 || a->iters > FM_MAX_ITERS) return pg_failf(PG_ERR_SHAPE, "formant_shift: iters must be within 0 .. %d", FM_MAX_ITERS);
    if ((int64_t)a->n_ch * a->m_ch_rows > INT64_MAX / 2 / a->F) return pg_fail(PG_ERR_SHAPE, "formant_shift: plane beyond 2^62 elements");
    if (!(a->ratio >= 0.25) || !(a->ratio <= 4.0)) return pg_fail(PG_ERR_SHAPE, "formant_shift: ratio must be finite and within [0.25, 4]");
    if (!(a->eps > 0.0f) || !pg_finite(a->eps)) return pg_fail(PG_ERR_SHAPE, "formant_shift: eps must be finite and positive");
    if ((((uintptr_t)a->M) & 3) || (((uintptr_t)a->basis) & 3) || (((uintptr_t)a->env) & 3) || (((uintptr_t)a->out) & 3))
        return pg_fail(PG_ERR_ALIGN, "formant_shift: misaligned pointer");
    FmKernelArgs k;
    k.M = a->M; k.basis = a->basis; k.env = a->env; k.out = a->out;
    k.ratio = a->ratio; k.eps = a->eps;
    k.F = a->F; k.m_stride = a->n_ch == 1 ? 0 : (long)a->m_ch_rows * a->F;
    k.bins = a->bins; k.order = a->order; k.hold = a->hold; k.iters = a->iters;
    k.nb = (a->bins + 31) / 32;
    k.ft = k.nb * 32 <= 1024 ? 32 : (k.nb * 32 <= 2048 ? 16 : 8);    // H is at most 128 KiB
    k.tiles_f = (k.F + k.ft - 1) / k.ft; k.tiles = k.tiles_f * a->n_ch;
    const bool f4 = (a->F & 3) == 0;                                  // (then every row of every plane begins a multiple of 16 bytes after its base)
    k.vec_in = f4 && pg_al16(a->M); k.vec_env = f4 && pg_al16(a->env); k.vec_out = f4 && pg_al16(a->out);
    k.vec_tab = (a->bins & 3) == 0 && pg_al16(a->basis);
    const int lds_bytes = (k.nb * 32 * k.ft + FM_AUX) * (int)sizeof(float);
    const unsigned grid = pg_stream_grid(k.tiles, 1);                 // a workgroup per tile
    // dynamic LDS above 64 KB: the attribute belongs to (function, current device); set on every call, nothing cached
    void (*kernel)(const FmKernelArgs) = k.vec_in ? formant_kernel<true> : formant_kernel<false>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return pg_fail((int)e, "formant_shift: LDS attribute refused");
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(FM_THREADS), lds_bytes, (hipStream_t)stream, k);
    return pg_launch_ok("formant_shift launch failed");
}
