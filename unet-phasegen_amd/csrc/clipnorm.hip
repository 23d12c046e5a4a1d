// clipnorm.hip -- BatchNorm with PER-CLIP statistics (pg_clipnorm_fwd): every row (b, c) of L frames is normalised by its own
// mean and biased variance, which is what the reference's batch-of-one inference forwards compute (demo.py:33-45, train.py:76-83:
// no .eval() anywhere), for B clips in one launch.  The running buffers end up exactly as after B batch-of-one calls in clip order.
//
// Mapping.  Rows are short (29 ... 256 frames in the U-Net) and there are B * C of them; consecutive channels of a sample are
// contiguous.  A row gets a power-of-two lane GROUP (16 / 32 / 64 lanes by L), a wave covers the 4 / 2 / 1 adjacent rows -- one
// contiguous span of memory --, lane j of a group holds units j, j + G, j + 2 G, ... of its row in registers (a unit = 1 float,
// or 4 where L % 4 == 0).  One HBM read; mean, centred squares and the outputs come from the registers (the two-pass arithmetic of
// bn_fwd_reg_kernel); the group sums are __shfl_xor butterflies.  No LDS, no barrier, no atomics: waves are independent and walk
// the rows grid-stride.  A wave's pass over its rows is one latency chain (load, reduce, store), so the groups are kept NARROW --
// up to 8 units per lane before the next width -- to have 1-2 KB per wave in flight (one 129-frame row per wave on 64 lanes runs
// at half the rate; measurements in DESIGN.md section 4.6).
// Reduction order.  Group width, units per lane and unit size are functions of L ALONE (where 16-byte accesses are not possible
// the same units are moved as scalars), so a row's statistics and outputs do not depend on B, the grid, the alignment of the
// tensors or on which rows share its wave: a clip normalised inside a batch is bit-identical to the same clip normalised alone.
// Rows longer than CN_REG_MAX frames take a looping kernel (one wave per row, three passes over the row).
// Running buffers.  The main kernel leaves every row's mean and biased variance in the caller's workspace; a second small kernel
// (launched only when a running buffer or the counter is given) walks b = 0 .. B-1 per channel: one momentum step per clip.
// Built with -ffp-contract=off like the rest of the library: the chain is reproducible to the bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"

namespace {

constexpr int CN_REG_MAX = 1024;   // longest row the register-resident kernels hold (16 values per lane on 64 lanes)
constexpr int CN_CHAIN = 16;       // clips whose statistics the running-buffer kernel fetches at a time

typedef float cnf4 __attribute__((ext_vector_type(4)));
typedef unsigned short cnus4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float cn_slope(int act) { return act == PG_ACT_LEAKY02 ? 0.2f : (act == PG_ACT_RELU ? 0.0f : 1.0f); }
__device__ __forceinline__ unsigned short cn_bf16_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

// sum over the G lanes of a group (G = 16 / 32 / 64 consecutive lanes of the wave); every lane of the group gets it
template <int G>
__device__ __forceinline__ float cn_group_sum(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// all outputs for VEC consecutive elements of row (b, c) starting at frame l: fp32 y / y2 and the bf16 copies, each with its own
// activation (slope 1 = identity, 0.2 = LeakyReLU, 0 = ReLU) -- the store logic of pg_bn_fwd.  WIDE: 16-byte (fp32) / 8-byte
// (bf16) stores; the host has checked that every given tensor allows them.
template <int VEC, bool WIDE>
__device__ __forceinline__ void cn_store(const pg_clipnorm_args& a, long b, long c, int l, const float* o) {
    if (a.y) {
        const float s = cn_slope(a.y_act); float* p = a.y + b * a.y_bs + c * a.L + l;
        if (WIDE) { cnf4 t; for (int k = 0; k < 4; ++k) t[k] = fmaxf(o[k], s * o[k]); *(cnf4*)p = t; }
        else for (int k = 0; k < VEC; ++k) p[k] = fmaxf(o[k], s * o[k]);
    }
    if (a.y2) {
        const float s = cn_slope(a.y2_act); float* p = a.y2 + b * a.y2_bs + c * a.L + l;
        if (WIDE) { cnf4 t; for (int k = 0; k < 4; ++k) t[k] = fmaxf(o[k], s * o[k]); *(cnf4*)p = t; }
        else for (int k = 0; k < VEC; ++k) p[k] = fmaxf(o[k], s * o[k]);
    }
    if (a.yh) {
        const float s = cn_slope(a.yh_act); uint16_t* p = a.yh + b * a.yh_bs + c * a.yh_pitch + l;
        if (WIDE) { cnus4 t; for (int k = 0; k < 4; ++k) t[k] = cn_bf16_bits(fmaxf(o[k], s * o[k])); *(cnus4*)p = t; }
        else for (int k = 0; k < VEC; ++k) p[k] = cn_bf16_bits(fmaxf(o[k], s * o[k]));
    }
    if (a.yh2) {
        const float s = cn_slope(a.yh2_act); uint16_t* p = a.yh2 + b * a.yh2_bs + c * a.yh2_pitch + l;
        if (WIDE) { cnus4 t; for (int k = 0; k < 4; ++k) t[k] = cn_bf16_bits(fmaxf(o[k], s * o[k])); *(cnus4*)p = t; }
        else for (int k = 0; k < VEC; ++k) p[k] = cn_bf16_bits(fmaxf(o[k], s * o[k]));
    }
}

// per-row statistics out: save_mean / save_invstd (B, C) for the caller, mean / biased variance for the running-buffer chain
__device__ __forceinline__ void cn_save(const pg_clipnorm_args& a, long r, float mean, float var, float invstd) {
    if (a.save_mean) a.save_mean[r] = mean;
    if (a.save_invstd) a.save_invstd[r] = invstd;
    if (a.workspace) {
        float* ws = (float*)a.workspace;
        ws[r] = mean;
        ws[(long)a.B * a.C + r] = var;
    }
}

// Register-resident rows: G lanes per row, UPL units of VEC floats per lane (G * UPL * VEC >= L), 64 / G rows per wave.
template <int G, int UPL, int VEC, bool WIDE>
__global__ __launch_bounds__(256) void clipnorm_reg_kernel(const pg_clipnorm_args a) {
    static_assert(VEC == 4 || !WIDE, "16-byte accesses move 4-float units");
    constexpr int RPW = 64 / G;
    const int lane = threadIdx.x & 63, sub = lane & (G - 1), grp = lane / G;
    const long rows = (long)a.B * a.C;
    const long nwave = (long)gridDim.x * (blockDim.x >> 6);
    const int Lu = a.L / VEC;
    for (long w = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w * RPW < rows; w += nwave) {     // wave-uniform trip count
        const long r = w * RPW + grp;
        const bool rok = r < rows;
        const long b = rok ? r / a.C : 0, c = rok ? r - b * a.C : 0;
        const float* xr = a.x + b * a.x_bs + c * a.L;
        float v[UPL][VEC];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < UPL; ++i) {
            const int u = sub + i * G;
            const bool ok = rok && u < Lu;
            const float* p = xr + (ok ? VEC * u : 0);            // branch-free: a lane without a unit re-reads the row's first one
            if (WIDE) {
                const cnf4 t = *(const cnf4*)p;
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[i][k] = ok ? t[k] : 0.f;
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { const float t = p[k]; v[i][k] = ok ? t : 0.f; }
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) s += v[i][k];
        }
        const float mean = cn_group_sum<G>(s) / (float)a.L;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < UPL; ++i)
            if (rok && sub + i * G < Lu) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { const float d = v[i][k] - mean; q += d * d; }
            }
        const float var = cn_group_sum<G>(q) / (float)a.L;
        const float invstd = 1.0f / sqrtf(var + a.eps);
        const float ga = a.gamma[c], be = a.beta[c];
#pragma unroll
        for (int i = 0; i < UPL; ++i)
            if (rok && sub + i * G < Lu) {
                float o[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) o[k] = (v[i][k] - mean) * invstd * ga + be;
                cn_store<VEC, WIDE>(a, b, c, VEC * (sub + i * G), o);
            }
        if (rok && sub == 0) cn_save(a, r, mean, var, invstd);
    }
}

// Long rows (L > CN_REG_MAX): one wave per row, lane j takes frames j, j + 64, ...; three passes over the row (the second and
// third come from the caches).  Same arithmetic; the order again depends on L alone.
__global__ __launch_bounds__(256) void clipnorm_loop_kernel(const pg_clipnorm_args a) {
    const int lane = threadIdx.x & 63;
    const long rows = (long)a.B * a.C;
    const long nwave = (long)gridDim.x * (blockDim.x >> 6);
    for (long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < rows; r += nwave) {
        const long b = r / a.C, c = r - b * a.C;
        const float* xr = a.x + b * a.x_bs + c * a.L;
        float s = 0.f;
        for (int l = lane; l < a.L; l += 64) s += xr[l];
        const float mean = cn_group_sum<64>(s) / (float)a.L;
        float q = 0.f;
        for (int l = lane; l < a.L; l += 64) { const float d = xr[l] - mean; q += d * d; }
        const float var = cn_group_sum<64>(q) / (float)a.L;
        const float invstd = 1.0f / sqrtf(var + a.eps);
        const float ga = a.gamma[c], be = a.beta[c];
        for (int l = lane; l < a.L; l += 64) {
            const float o = (xr[l] - mean) * invstd * ga + be;
            cn_store<1, false>(a, b, c, l, &o);
        }
        if (lane == 0) cn_save(a, r, mean, var, invstd);
    }
}

// The running buffers after B batch-of-one BatchNorm calls in clip order: one thread per channel walks b = 0 .. B-1 (the
// arithmetic of pg_bn_fwd's update with n = L); nn.BatchNorm's counter advances by B.
__global__ __launch_bounds__(64) void clipnorm_running_kernel(const pg_clipnorm_args a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += a.B;
    if (c >= a.C || !a.workspace) return;                        // (no workspace: only the counter was asked for)
    const float* mean = (const float*)a.workspace;
    const float* var = mean + (long)a.B * a.C;
    const float unb = (float)a.L / (float)(a.L > 1 ? a.L - 1 : 1);
    // the chain is serial, its loads are not: CN_CHAIN clips' statistics are fetched together, then folded in clip order
    float rm = a.running_mean ? a.running_mean[c] : 0.f, rv = a.running_var ? a.running_var[c] : 0.f;
    for (int b0 = 0; b0 < a.B; b0 += CN_CHAIN) {
        float m[CN_CHAIN], v[CN_CHAIN];
#pragma unroll
        for (int j = 0; j < CN_CHAIN; ++j) {
            const long at = (long)(b0 + j < a.B ? b0 + j : b0) * a.C + c;
            m[j] = mean[at]; v[j] = var[at];
        }
#pragma unroll
        for (int j = 0; j < CN_CHAIN; ++j)
            if (b0 + j < a.B) {
                rm = (1.f - a.momentum) * rm + a.momentum * m[j];
                rv = (1.f - a.momentum) * rv + a.momentum * (v[j] * unb);
            }
    }
    if (a.running_mean) a.running_mean[c] = rm;
    if (a.running_var) a.running_var[c] = rv;
}

struct CnPlan { int G, upl, vec; bool wide; };

// group width, units per lane and unit size from L alone; `wide` (how the units are moved) from the tensors
bool cn_plan(const pg_clipnorm_args* a, CnPlan& p) {
    if (a->L > CN_REG_MAX) return false;
    p.vec = (a->L & 3) == 0 ? 4 : 1;
    const int units = a->L / p.vec;
    p.G = units <= 128 ? 16 : (units <= 256 ? 32 : 64);
    const int need = (units + p.G - 1) / p.G;                    // 1 .. 8 (16 lanes), 5 .. 8 (32 lanes), 5 .. 16 (64 lanes)
    p.upl = need <= 6 ? need : (need <= 8 ? 8 : 16);
    auto ok16 = [](const void* q, long bs) { return q == nullptr || ((((uintptr_t)q) & 15) == 0 && (bs & 3) == 0); };
    auto ok8 = [](const void* q, long bs, int pitch) { return q == nullptr || ((((uintptr_t)q) & 7) == 0 && (bs & 3) == 0 && (pitch & 3) == 0); };
    p.wide = p.vec == 4 && ok16(a->x, a->x_bs) && ok16(a->y, a->y_bs) && ok16(a->y2, a->y2_bs)
             && ok8(a->yh, a->yh_bs, a->yh_pitch) && ok8(a->yh2, a->yh2_bs, a->yh2_pitch);
    return true;
}

template <int G, int UPL>
void cn_launch_gu(const pg_clipnorm_args* a, const CnPlan& p, unsigned grid, hipStream_t st) {
    if (p.vec == 1) hipLaunchKernelGGL((clipnorm_reg_kernel<G, UPL, 1, false>), dim3(grid), dim3(256), 0, st, *a);
    else if constexpr (G * UPL * 4 <= CN_REG_MAX) {             // (4-float units: at most CN_REG_MAX / 4 of them)
        if (p.wide) hipLaunchKernelGGL((clipnorm_reg_kernel<G, UPL, 4, true>), dim3(grid), dim3(256), 0, st, *a);
        else hipLaunchKernelGGL((clipnorm_reg_kernel<G, UPL, 4, false>), dim3(grid), dim3(256), 0, st, *a);
    }
}

void cn_launch_reg(const pg_clipnorm_args* a, const CnPlan& p, unsigned grid, hipStream_t st) {
#define PG_CN_CASE(G, U) case U: cn_launch_gu<G, U>(a, p, grid, st); break;
    if (p.G == 16) switch (p.upl) { PG_CN_CASE(16, 1) PG_CN_CASE(16, 2) PG_CN_CASE(16, 3) PG_CN_CASE(16, 4) PG_CN_CASE(16, 5) PG_CN_CASE(16, 6) PG_CN_CASE(16, 8) }
    else if (p.G == 32) switch (p.upl) { PG_CN_CASE(32, 5) PG_CN_CASE(32, 6) PG_CN_CASE(32, 8) }
    else switch (p.upl) { PG_CN_CASE(64, 5) PG_CN_CASE(64, 6) PG_CN_CASE(64, 8) PG_CN_CASE(64, 16) }
#undef PG_CN_CASE
}

int cn_check(const pg_clipnorm_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "clipnorm: null args");
    if (a->B <= 0 || a->C <= 0 || a->L <= 0) return pg_fail(PG_ERR_SHAPE, "clipnorm: non-positive dimension");
    if ((long)a->B * a->C > 0x7fffffffL) return pg_fail(PG_ERR_SHAPE, "clipnorm: B*C too large");
    return PG_OK;
}

}  // namespace

extern "C" int64_t pg_workspace_bytes_clipnorm(const pg_clipnorm_args* a) {
    if (int e = cn_check(a)) return e;
    return (int64_t)2 * a->B * a->C * (int64_t)sizeof(float);
}

extern "C" int pg_clipnorm_fwd(const pg_clipnorm_args* a, void* stream) {
    if (int e = cn_check(a)) return e;
    if (!a->x || (!a->y && !a->yh) || !a->gamma || !a->beta)
        return pg_fail(PG_ERR_NULL, "clipnorm_fwd: x, y (or yh), gamma, beta required");
    if ((a->yh && a->yh_pitch < a->L) || (a->yh2 && a->yh2_pitch < a->L)) return pg_fail(PG_ERR_SHAPE, "clipnorm_fwd: bf16 output pitch below L");
    const bool chain = a->running_mean || a->running_var;
    if (chain && (!a->workspace || a->workspace_bytes < pg_workspace_bytes_clipnorm(a)))
        return pg_fail(PG_ERR_WORKSPACE, "clipnorm_fwd: running buffers need a workspace of pg_workspace_bytes_clipnorm() bytes");
    pg_clipnorm_args k = *a;
    if (!chain) k.workspace = nullptr;                           // nobody reads the per-row statistics: do not write them
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)k.B * k.C;
    const long cap = (long)pg_cu_count() * 8;                    // 8 workgroups of 4 waves per CU fill it; the rest is grid-stride
    CnPlan p;
    if (cn_plan(&k, p)) {
        const long waves = (rows * p.G + 63) / 64;
        long grid = (waves + 3) / 4; if (grid > cap) grid = cap;
        cn_launch_reg(&k, p, (unsigned)grid, st);
    } else {
        long grid = (rows + 3) / 4; if (grid > cap) grid = cap;
        hipLaunchKernelGGL(clipnorm_loop_kernel, dim3((unsigned)grid), dim3(256), 0, st, k);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pg_fail((int)e, "clipnorm_fwd launch failed");
    if (chain || k.num_batches_tracked) {
        hipLaunchKernelGGL(clipnorm_running_kernel, dim3((unsigned)((k.C + 63) / 64)), dim3(64), 0, st, k);
        e = hipGetLastError();
        if (e != hipSuccess) return pg_fail((int)e, "clipnorm_fwd running-buffer launch failed");
    }
    return PG_OK;
}
