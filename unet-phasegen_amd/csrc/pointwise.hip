// pointwise.hip -- the HBM-bound side of the path that is not a normalisation layer (those are norm.hip): the fused cos/sin/
// magnitude loss with its gradient, whole-array moments and standardisation, Adam over the flat parameter arena, the polar
// transform, and the bf16-resident path's weight shadow and row cast.
// All are streaming kernels: coalesced frame-contiguous reads, wavefront shuffle reductions, no atomics
// (every reduction has a fixed order => bit-reproducible run to run).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"
#include "pg_fastmath.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// Loss (train.py:45-60) fused with d loss / d pred.  One thread per (b, c, l); stage 1 leaves 3 partial sums
// per workgroup in the workspace, stage 2 (one workgroup) adds them in double in a fixed order.
// ---------------------------------------------------------------------------------------------------------
constexpr int LOSS_BLOCKS = 1024;

__global__ __launch_bounds__(256) void loss_partial_kernel(const pg_loss_args a, float* partial) {
    __shared__ float scratch[16];
    const long CL = (long)a.C * a.L, N = (long)a.B * CL;
    const float scale = 2.0f / (float)N;
    float s_cos = 0.f, s_sin = 0.f, s_mag = 0.f;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < N; e += (long)gridDim.x * blockDim.x) {
        const long b = e / CL, r = e - b * CL;
        const float ph = a.pred[b * 2 * CL + r], mh = a.pred[b * 2 * CL + CL + r];
        const float m = a.batch[b * 2 * CL + r], th = a.batch[b * 2 * CL + CL + r];
        float sp, cp, st, ct;
        sincosf(ph, &sp, &cp);
        sincosf(th, &st, &ct);
        const float dc = cp - ct, ds = sp - st, dm = mh - m;
        s_cos += dc * dc; s_sin += ds * ds; s_mag += dm * dm;
        if (a.dpred) {
            // autograd of MSE(cos p, cos th) + MSE(sin p, sin th):  2/N * (dc * -sin p + ds * cos p)
            a.dpred[b * 2 * CL + r] = scale * (ds * cp - dc * sp);
            a.dpred[b * 2 * CL + CL + r] = a.mag_weight * scale * dm;
        }
    }
    s_cos = pg_block_sum(s_cos, scratch);
    s_sin = pg_block_sum(s_sin, scratch);
    s_mag = pg_block_sum(s_mag, scratch);
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 3 + 0] = s_cos; partial[blockIdx.x * 3 + 1] = s_sin; partial[blockIdx.x * 3 + 2] = s_mag;
    }
}

__global__ __launch_bounds__(64) void loss_final_kernel(const float* partial, int nblocks, double n, float mag_weight, float* losses) {
    // lane i adds partials i, i + 64, ... in double, then a fixed shuffle tree: deterministic, 64x shorter than one lane alone
    double c = 0, s = 0, m = 0;
    for (int i = threadIdx.x; i < nblocks; i += 64) { c += partial[i * 3]; s += partial[i * 3 + 1]; m += partial[i * 3 + 2]; }
    c = pg_group_sum<64>(c); s = pg_group_sum<64>(s); m = pg_group_sum<64>(m);
    if (threadIdx.x == 0) {
        const float cos_l = (float)(c / n), sin_l = (float)(s / n), mag_l = (float)(m / n);
        const float ang = cos_l + sin_l;
        losses[0] = ang + mag_l * mag_weight; losses[1] = ang; losses[2] = mag_l;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Whole-array standardisation of the feature set (preproc_mdb.py:182): moments in double (fixed reduction order:
// per-thread grid-stride sums, wave shuffle tree, per-workgroup partials summed by one wave), then one in-place pass.
// ---------------------------------------------------------------------------------------------------------
constexpr int MOM_BLOCKS = 1024;

// pass 0: sum of x; pass 1: sum of (x - mean)^2 with the mean read from stats[0] (two-pass, like numpy's std)
__global__ __launch_bounds__(256) void moments_partial_kernel(const float* __restrict__ x, long n, const double* stats, int pass, double* partial) {
    __shared__ double red[4];
    const double mean = pass ? stats[0] : 0.0;
    double acc = 0;
    const long stride = (long)gridDim.x * 256;
    const bool vec = (((uintptr_t)x) & 15) == 0;
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f32x4 v = ((const f32x4*)x)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double d = (double)v[j] - mean; acc += pass ? d * d : d; }
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const double d = (double)x[i] - mean; acc += pass ? d * d : d;
    }
    acc = pg_group_sum<64>(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void moments_final_kernel(const double* partial, int nblocks, double n, int pass, double* stats) {
    double acc = 0;
    for (int i = threadIdx.x; i < nblocks; i += 64) acc += partial[i];
    acc = pg_group_sum<64>(acc);
    if (threadIdx.x == 0) stats[pass] = pass ? sqrt(acc / n) : acc / n;
}

__global__ __launch_bounds__(256) void standardize_kernel(float* __restrict__ x, long n, const double* stats) {
    const float mean = (float)stats[0], std = (float)stats[1];             // float32 arithmetic, as numpy on a float32 array
    const long stride = (long)gridDim.x * 256;
    const bool vec = (((uintptr_t)x) & 15) == 0;
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        f32x4 v = ((f32x4*)x)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (v[j] - mean) / std;
        ((f32x4*)x)[i] = v;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] = (x[i] - mean) / std;
}

// ---------------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam defaults, single-tensor path of torch 2.x): m.lerp_(g, 1-b1); v = b2 v + (1-b2) g g;
// p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps).  28 B of HBM traffic per parameter.
// ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float omb1, float b2, float omb2,
                                                   float step_size, float bc2_sqrt, float eps, float gs) {
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i], gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a = pp[k], b = mm[k], c = vv[k];
            pg_adam_one(a, gg[k], b, c, omb1, b2, omb2, step_size, bc2_sqrt, eps, gs);
            pp[k] = a; mm[k] = b; vv[k] = c;
        }
        reinterpret_cast<f32x4*>(p)[i] = pp; reinterpret_cast<f32x4*>(m)[i] = mm; reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        pg_adam_one(p[i], g[i], m[i], v[i], omb1, b2, omb2, step_size, bc2_sqrt, eps, gs);
    }
}

// "Thin" variant for running BESIDE the MFMA-bound convolution kernels of backward (pg_adam_args.thin; phasegen.trainer):
// one 256-thread workgroup per CU at most, <= 32 VGPRs so that its four waves fit into the registers the conv kernels
// leave free (2 waves x <= 240 of 512 per SIMD), non-temporal loads and stores so that the 28 B per parameter it streams do
// not evict the conv kernels' operands from L2 / Infinity Cache.  Slower than adam_kernel on an idle chip (fewer bytes in
// flight), which does not matter in the shadow of ~100 ms of convolutions.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256)
void adam_thin_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                      float omb1, float b2, float omb2, float step_size, float bc2_sqrt, float eps, float gs) {
    const long n2 = n >> 1;          // two parameters per thread and iteration: 23 VGPRs (four need 41)
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
        f32x2 pp = __builtin_nontemporal_load(reinterpret_cast<f32x2*>(p) + i), gg = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(g) + i);
        f32x2 mm = __builtin_nontemporal_load(reinterpret_cast<f32x2*>(m) + i), vv = __builtin_nontemporal_load(reinterpret_cast<f32x2*>(v) + i);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float a = pp[k], b = mm[k], c = vv[k];
            pg_adam_one(a, gg[k], b, c, omb1, b2, omb2, step_size, bc2_sqrt, eps, gs);
            pp[k] = a; mm[k] = b; vv[k] = c;
        }
        __builtin_nontemporal_store(pp, reinterpret_cast<f32x2*>(p) + i);
        __builtin_nontemporal_store(mm, reinterpret_cast<f32x2*>(m) + i);
        __builtin_nontemporal_store(vv, reinterpret_cast<f32x2*>(v) + i);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) pg_adam_one(p[n - 1], g[n - 1], m[n - 1], v[n - 1], omb1, b2, omb2, step_size, bc2_sqrt, eps, gs);
}

// ---------------------------------------------------------------------------------------------------------
// data.py:39-47: [re; im] -> [log1p(|z|); angle(z)], 16 B of traffic per bin-frame.
// ---------------------------------------------------------------------------------------------------------
// (the arithmetic is pg_polar_one, pg_fastmath.h: shared with the STFT kernel's fused epilogue, so the two stay bit-identical)
__device__ __forceinline__ void polar_one(float re, float im, int use_exp, float& mag, float& ang) { pg_polar_one(re, im, use_exp, mag, ang); }

// VEC = 4: 16-B loads/stores (inner % 4 == 0 and 16-B aligned planes); VEC = 1: any shape
template <int VEC>
__global__ __launch_bounds__(256) void polar_kernel(const float* __restrict__ in, float* __restrict__ out, long n_items, long inner, int use_exp) {
    const long per = inner / VEC, total = n_items * per;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long it = e / per, r = (e - it * per) * VEC;
        const float* pre = in + it * 2 * inner + r;
        float* pm = out + it * 2 * inner + r;
        if (VEC == 4) {
            const f32x4 re = *reinterpret_cast<const f32x4*>(pre), im = *reinterpret_cast<const f32x4*>(pre + inner);
            f32x4 mg, an;
#pragma unroll
            for (int k = 0; k < 4; ++k) { float a, b; polar_one(re[k], im[k], use_exp, a, b); mg[k] = a; an[k] = b; }
            *reinterpret_cast<f32x4*>(pm) = mg;
            *reinterpret_cast<f32x4*>(pm + inner) = an;
        } else {
            float a, b;
            polar_one(pre[0], pre[inner], use_exp, a, b);
            pm[0] = a; pm[inner] = b;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// bf16-resident path helpers (conv_h.hip): the weight shadow and the fp32 -> bf16 row cast.
// ---------------------------------------------------------------------------------------------------------
// Conv1d weights (Cout, Cin, k) are already [row = o][K = (q, j)]: a plain cast.  ConvTranspose1d weights (Cin, Cout, k) become
// A[(o * s + phi)][q * KJ + jj'] = W[q][o][s * (KJ - 1 - jj') + phi]  (KJ = taps per phase, ceil(k / s) rounded up to a power
// of two with zero weights for the taps that do not exist -- k = 5, s = 2 is stored as 4 taps per phase; taps are stored so
// that window positions ASCEND with jj', the order conv_h_kernel's T form reads them in).
__global__ __launch_bounds__(256) void shadow_kernel(const float* __restrict__ w, unsigned short* __restrict__ wh, int Cin, int Cout, int k, int s, int transposed, int KJ) {
    const long n = transposed ? (long)Cin * Cout * s * KJ : (long)Cin * Cout * k;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        if (!transposed) { wh[e] = pg_bf16_bits(w[e]); continue; }
        const long Ktot = (long)Cin * KJ;
        const long row = e / Ktot; const int kk = (int)(e - row * Ktot);
        const int o = (int)(row / s), phi = (int)(row - (long)o * s), q = kk / KJ, jj = kk - q * KJ;
        const int j = s * (KJ - 1 - jj) + phi;            // taps past k (KJ rounded up to a power of two; k = 5: 3 -> 4) are zero
        wh[e] = j < k ? pg_bf16_bits(w[((long)q * Cout + o) * k + j]) : (unsigned short)0;
    }
}

// (B, C, L) fp32 rows -> (B, C, pitch) bf16 rows, activation applied first; the tail [L, pitch) of every row is zeroed.
// The activation is the select x >= 0 ? x : slope * x, not pg_act_apply's fmaxf(x, slope * x): the two agree bit for bit on every
// finite x, on +inf and on NaN, but under ReLU fmaxf(-inf, 0 * -inf) hands -inf through as a "rectified" value where the select
// stores the NaN of 0 * -inf (tests/test_z_pointwise_gpu.py).
__global__ __launch_bounds__(256) void cast_rows_kernel(const pg_cast_args a) {
    const long rows = (long)a.B * a.C, total = rows * a.pitch;
    const float slope = pg_act_slope(a.act);
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long row = e / a.pitch; const int l = (int)(e - row * a.pitch);
        const long b = row / a.C, c = row - b * a.C;
        float v = 0.f;
        if (l < a.L) { v = a.x[b * a.x_bs + c * a.L + l]; v = v >= 0.f ? v : slope * v; }
        a.y[b * a.y_bs + c * a.pitch + l] = pg_bf16_bits(v);
    }
}

}  // namespace

// taps per output phase of a transposed conv in the shadow layout: ceil(k / stride) rounded up to a power of two
int pg_shadow_taps(int k, int stride) { int kj = (k + stride - 1) / stride, p2 = 1; while (p2 < kj) p2 <<= 1; return p2; }
extern "C" int64_t pg_shadow_elems(int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t transposed) {
    return transposed ? (int64_t)Cin * Cout * stride * pg_shadow_taps(k, stride) : (int64_t)Cin * Cout * k;
}

extern "C" int pg_shadow_weights(const float* w, uint16_t* wh, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t transposed, void* stream) {
    if (!w || !wh) return pg_fail(PG_ERR_NULL, "shadow_weights: w, wh required");
    if (Cin <= 0 || Cout <= 0 || k <= 0 || stride <= 0) return pg_fail(PG_ERR_SHAPE, "shadow_weights: non-positive dimension");
    const int KJ = pg_shadow_taps(k, stride);
    const long n = transposed ? (long)Cin * Cout * stride * KJ : (long)Cin * Cout * k;
    long blocks = (n + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(shadow_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, wh, Cin, Cout, k, stride, transposed, KJ);
    return pg_launch_ok("shadow_weights launch failed");
}

extern "C" int pg_cast_rows_bf16(const pg_cast_args* a, void* stream) {
    if (!a || !a->x || !a->y) return pg_fail(PG_ERR_NULL, "cast_rows_bf16: x, y required");
    if (a->B <= 0 || a->C <= 0 || a->L <= 0 || a->pitch < a->L) return pg_fail(PG_ERR_SHAPE, "cast_rows_bf16: bad sizes");
    const long total = (long)a->B * a->C * a->pitch;
    long blocks = (total + 255) / 256; if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(cast_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *a);
    return pg_launch_ok("cast_rows_bf16 launch failed");
}

extern "C" int64_t pg_workspace_bytes_loss(const pg_loss_args*) { return (int64_t)LOSS_BLOCKS * 3 * sizeof(float); }

extern "C" int pg_loss_fwd_bwd(const pg_loss_args* a, void* stream) {
    if (!a || !a->pred || !a->batch || !a->losses || !a->workspace) return pg_fail(PG_ERR_NULL, "loss: pred, batch, losses, workspace required");
    if (a->B <= 0 || a->C <= 0 || a->L <= 0) return pg_fail(PG_ERR_SHAPE, "loss: non-positive dimension");
    if (a->workspace_bytes < pg_workspace_bytes_loss(a)) return pg_fail(PG_ERR_WORKSPACE, "loss: workspace too small");
    const long N = (long)a->B * a->C * a->L;
    int blocks = (int)((N + 255) / 256); if (blocks > LOSS_BLOCKS) blocks = LOSS_BLOCKS;
    float* partial = (float*)a->workspace;
    hipLaunchKernelGGL(loss_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *a, partial);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, blocks, (double)N, a->mag_weight, a->losses);
    return pg_launch_ok("loss launch failed");
}

extern "C" int64_t pg_workspace_bytes_moments(void) { return (int64_t)MOM_BLOCKS * (int64_t)sizeof(double); }

extern "C" int pg_moments(const pg_moments_args* a, void* stream) {
    if (!a || !a->x || !a->stats || !a->workspace) return pg_fail(PG_ERR_NULL, "moments: x, stats, workspace required");
    if (a->n <= 0) return pg_fail(PG_ERR_SHAPE, "moments: non-positive size");
    if (a->workspace_bytes < pg_workspace_bytes_moments()) return pg_fail(PG_ERR_WORKSPACE, "moments: workspace too small");
    if (((uintptr_t)a->x & 3) || ((uintptr_t)a->stats & 7) || ((uintptr_t)a->workspace & 7)) return pg_fail(PG_ERR_ALIGN, "moments: misaligned pointer");
    long blocks = ((a->n >> 2) + 255) / 256; if (blocks > MOM_BLOCKS) blocks = MOM_BLOCKS; if (blocks < 1) blocks = 1;
    double* partial = (double*)a->workspace;
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(moments_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a->x, (long)a->n, a->stats, pass, partial);
        hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, (int)blocks, (double)a->n, pass, a->stats);
    }
    return pg_launch_ok("moments launch failed");
}

extern "C" int pg_standardize(float* x, int64_t n, const double* stats, void* stream) {
    if (!x || !stats) return pg_fail(PG_ERR_NULL, "standardize: x, stats required");
    if (n <= 0) return pg_fail(PG_ERR_SHAPE, "standardize: non-positive size");
    if (((uintptr_t)x & 3) || ((uintptr_t)stats & 7)) return pg_fail(PG_ERR_ALIGN, "standardize: misaligned pointer");
    long blocks = ((n >> 2) + 255) / 256; if (blocks > 256 * 16) blocks = 256 * 16; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)n, stats);
    return pg_launch_ok("standardize launch failed");
}

// Python floats -> the fp32 scalars of the update, rounded exactly where torch rounds them (one definition for the streaming
// kernel and the wgrad epilogue)
PgAdamScalars pg_adam_scalars(const pg_adam_args* a) {
    const double bc1 = 1.0 - pow(a->beta1, a->step), bc2 = 1.0 - pow(a->beta2, a->step);
    return { (float)(1.0 - a->beta1), (float)a->beta2, (float)(1.0 - a->beta2), (float)(a->lr / bc1), (float)sqrt(bc2), (float)a->eps,
             (float)a->grad_scale };
}

extern "C" int pg_adam_step(const pg_adam_args* a, void* stream) {
    if (!a || !a->p || !a->g || !a->m || !a->v) return pg_fail(PG_ERR_NULL, "adam: p, g, m, v required");
    if (a->n <= 0) return PG_OK;
    if (a->step < 1) return pg_fail(PG_ERR_SHAPE, "adam: step is 1-based");
    if (((uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v) & 15) return pg_fail(PG_ERR_ALIGN, "adam: pointers must be 16-byte aligned");
    const PgAdamScalars h = pg_adam_scalars(a);
    long blocks = ((a->n >> 2) + 255) / 256; if (blocks > 256 * 16) blocks = 256 * 16; if (blocks < 1) blocks = 1;
    if (a->thin) {
        const long cus = pg_cu_count();
        if (blocks > cus) blocks = cus;
        hipLaunchKernelGGL(adam_thin_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m, a->v, (long)a->n,
                           h.omb1, h.b2, h.omb2, h.step_size, h.bc2_sqrt, h.eps, h.gs);
        return pg_launch_ok("adam launch failed");
    }
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m, a->v, (long)a->n,
                       h.omb1, h.b2, h.omb2, h.step_size, h.bc2_sqrt, h.eps, h.gs);
    return pg_launch_ok("adam launch failed");
}

extern "C" int pg_polar(const pg_polar_args* a, void* stream) {
    if (!a || !a->in || !a->out) return pg_fail(PG_ERR_NULL, "polar: in, out required");
    if (a->n_items <= 0 || a->inner <= 0) return pg_fail(PG_ERR_SHAPE, "polar: non-positive size");
    const bool vec = (a->inner & 3) == 0 && (((uintptr_t)a->in | (uintptr_t)a->out) & 15) == 0;
    long blocks = (a->n_items * a->inner / (vec ? 4 : 1) + 255) / 256; if (blocks > 256 * 16) blocks = 256 * 16; if (blocks < 1) blocks = 1;
    if (vec) hipLaunchKernelGGL(polar_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a->in, a->out, (long)a->n_items, (long)a->inner, a->use_exp);
    else hipLaunchKernelGGL(polar_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a->in, a->out, (long)a->n_items, (long)a->inner, a->use_exp);
    return pg_launch_ok("polar launch failed");
}
