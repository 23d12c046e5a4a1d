// norm.hip -- the normalisation layers: train-mode BatchNorm (pg_bn_fwd / pg_bn_bwd) and BatchNorm with PER-CLIP statistics
// (pg_clipnorm_fwd).  HBM-bound streaming kernels: coalesced frame-contiguous accesses, shuffle reductions in a fixed order, no
// atomics => bit-reproducible run to run.  Built with -ffp-contract=off like the rest of the library.
// pg_bn_args and pg_clipnorm_args name their outputs alike, so the output epilogue (norm_store) and the alignment rule of wide
// accesses (wide_ok) exist once, as templates on the argument struct, and so does the running-statistics step (norm_running_step).
// The reductions do NOT: BatchNorm gives a channel a workgroup (block sums), clipnorm gives a row a lane group (butterflies), and
// both orders are pinned by bitwise tests.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "phasegen.h"
#include "pg_common.h"

namespace {

// All outputs for VEC consecutive elements of row (b, c) starting at frame l: fp32 y / y2 and the bf16 copies yh / yh2 of the
// bf16-resident path, each with its own activation (slope 1 = identity, 0.2 = LeakyReLU, 0 = ReLU).  WIDE: one 16-byte (fp32) /
// 8-byte (bf16) store per tensor -- the host has checked that every given tensor allows them (wide_ok) --, else VEC scalar stores.
template <int VEC, bool WIDE, typename Args>
__device__ __forceinline__ void norm_store(const Args& a, long b, long c, int l, const float* o) {
    static_assert(VEC == 4 || !WIDE, "wide stores move 4-float units");
    auto f32 = [&](float* y, long bs, int act) {
        if (!y) return;
        const float s = pg_act_slope(act); float* p = y + b * bs + c * a.L + l;
        if (WIDE) { f32x4 t; for (int k = 0; k < 4; ++k) t[k] = pg_act_apply(o[k], s); *(f32x4*)p = t; }
        else for (int k = 0; k < VEC; ++k) p[k] = pg_act_apply(o[k], s);
    };
    auto bf16 = [&](uint16_t* y, long bs, int pitch, int act) {
        if (!y) return;
        const float s = pg_act_slope(act); uint16_t* p = y + b * bs + c * pitch + l;
        if (WIDE) { u16x4 t; for (int k = 0; k < 4; ++k) t[k] = pg_bf16_bits(pg_act_apply(o[k], s)); *(u16x4*)p = t; }
        else for (int k = 0; k < VEC; ++k) p[k] = pg_bf16_bits(pg_act_apply(o[k], s));
    };
    f32(a.y, a.y_bs, a.y_act);
    f32(a.y2, a.y2_bs, a.y2_act);
    bf16(a.yh, a.yh_bs, a.yh_pitch, a.yh_act);
    bf16(a.yh2, a.yh2_bs, a.yh2_pitch, a.yh2_act);
}

// One momentum step of nn.BatchNorm's running buffers rm[c] / rv[c] (either may be NULL) with a batch of n values per channel of
// this mean and BIASED variance (the buffer gets the unbiased one)
__device__ __forceinline__ void norm_running_step(float* rm, float* rv, long c, float momentum, float mean, float var, int n) {
    if (rm) rm[c] = (1.f - momentum) * rm[c] + momentum * mean;
    if (rv) {
        const float unbiased = var * ((float)n / (float)(n > 1 ? n - 1 : 1));
        rv[c] = (1.f - momentum) * rv[c] + momentum * unbiased;
    }
}

// ---------------------------------------------------------------------------------------------------------
// BatchNorm, one workgroup per channel.  Tensor element (b, c, l) = base[b*bs + c*L + l].
// model.py:81,83 (nn.BatchNorm on (B, C, L)): mean / biased var over (B, L), eps inside the sqrt,
// running_var gets the unbiased variance, momentum 0.1.
// ---------------------------------------------------------------------------------------------------------
// what thread 0 of channel c's workgroup leaves behind after a forward: the statistics for the backward, the running buffers, and
// nn.BatchNorm's counter (no separate launch for it)
__device__ __forceinline__ void bn_fwd_tail(const pg_bn_args& a, int c, int n, float mean, float var, float invstd) {
    a.save_mean[c] = mean;
    a.save_invstd[c] = invstd;
    norm_running_step(a.running_mean, a.running_var, c, a.momentum, mean, var, n);
    if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
}

__global__ __launch_bounds__(256) void bn_fwd_kernel(const pg_bn_args a) {
    __shared__ float scratch[16];
    const int c = blockIdx.x, n = a.B * a.L;
    const float* xc = a.x + (long)c * a.L;
    float s = 0.f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int b = e / a.L, l = e - b * a.L;
        s += xc[(long)b * a.x_bs + l];
    }
    const float mean = pg_block_sum(s, scratch) / (float)n;
    float q = 0.f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int b = e / a.L, l = e - b * a.L;
        const float d = xc[(long)b * a.x_bs + l] - mean;
        q += d * d;
    }
    const float var = pg_block_sum(q, scratch) / (float)n;
    const float invstd = 1.0f / sqrtf(var + a.eps);
    const float g = a.gamma[c], be = a.beta[c];
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int b = e / a.L, l = e - b * a.L;
        const float o = (xc[(long)b * a.x_bs + l] - mean) * invstd * g + be;
        norm_store<1, false>(a, b, c, l, &o);
    }
    if (threadIdx.x == 0) bn_fwd_tail(a, c, n, mean, var, invstd);
}

// Register-resident variants (every shape of the U-Net: B * L <= 64 * 256): the channel's B x L values are read from HBM ONCE
// into registers and mean, variance and the normalised / activated outputs are all computed from there: 1 read + 1-2 writes
// instead of 3 reads.  The channel is walked FLAT: unit e = tid + 256 i of the B * L / VEC units (VEC = 4: float4 units when
// frames and strides allow 16-byte accesses -- one wave instruction moves 1 KB --, else single floats), (sample, position)
// advanced incrementally (no division in the loop), so every lane works whatever L is (129 frames used to idle 127 of 256
// lanes of a power-of-two row map).  Same two-pass arithmetic (mean first, then the centred squares), block sums in a fixed
// order: bit-reproducible.
template <int VEC> struct BnVec;
template <> struct BnVec<1> { typedef float T; };
template <> struct BnVec<4> { typedef f32x4 T; };
typedef float bnf2 __attribute__((ext_vector_type(2)));
template <> struct BnVec<2> { typedef bnf2 T; };
template <int VEC> __device__ __forceinline__ float bn_lane(const typename BnVec<VEC>::T& v, int k);
template <> __device__ __forceinline__ float bn_lane<1>(const float& v, int) { return v; }
template <> __device__ __forceinline__ float bn_lane<4>(const f32x4& v, int k) { return v[k]; }
template <> __device__ __forceinline__ float bn_lane<2>(const bnf2& v, int k) { return v[k]; }

struct BnWalk { int b, u, db, du, Lu; };
__device__ __forceinline__ BnWalk bn_walk(int L, int vec) {
    BnWalk w; w.Lu = L / vec;
    w.b = threadIdx.x / w.Lu; w.u = threadIdx.x - w.b * w.Lu;
    w.db = 256 / w.Lu; w.du = 256 - w.db * w.Lu;
    return w;
}
__device__ __forceinline__ void bn_next(BnWalk& w) {
    w.u += w.du; w.b += w.db;
    if (w.u >= w.Lu) { w.u -= w.Lu; w.b += 1; }
}

// The walk runs ONCE: unit i's (sample, position) is kept packed in one register (pk = b << 16 | u, -1 = past the end) and the
// later passes decode it -- re-walking made the compiler keep every intermediate of three identical walks alive.
template <int UPT, int VEC>          // UPT units of VEC floats per thread
__global__ __launch_bounds__(256) void bn_fwd_reg_kernel(const pg_bn_args a) {
    typedef typename BnVec<VEC>::T V;
    __shared__ float scratch[16];
    const int c = blockIdx.x, n = a.B * a.L;
    const float* xc = a.x + (long)c * a.L;
    V v[UPT];
    int pk[UPT];
    float s = 0.f;
    BnWalk w = bn_walk(a.L, VEC);
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        const bool ok = w.b < a.B;
        pk[i] = ok ? (w.b << 16) | w.u : -1;
        v[i] = *(const V*)(xc + (ok ? (long)w.b * a.x_bs + VEC * w.u : 0L));      // branch-free: all loads issue back to back
        if (!ok) v[i] = V(0.f);
#pragma unroll
        for (int k = 0; k < VEC; ++k) s += bn_lane<VEC>(v[i], k);
        bn_next(w);
    }
    const float mean = pg_block_sum(s, scratch) / (float)n;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < UPT; ++i)
        if (pk[i] >= 0) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) { const float d = bn_lane<VEC>(v[i], k) - mean; q += d * d; }
        }
    const float var = pg_block_sum(q, scratch) / (float)n;
    const float invstd = 1.0f / sqrtf(var + a.eps);
    const float ga = a.gamma[c], be = a.beta[c];
#pragma unroll
    for (int i = 0; i < UPT; ++i)
        if (pk[i] >= 0) {
            float o[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) o[k] = (bn_lane<VEC>(v[i], k) - mean) * invstd * ga + be;
            norm_store<VEC, VEC == 4>(a, pk[i] >> 16, c, VEC * (pk[i] & 0xffff), o);     // (a float2 unit is stored as scalars)
        }
    if (threadIdx.x == 0) bn_fwd_tail(a, c, n, mean, var, invstd);
}

template <int UPT, int VEC>
__global__ __launch_bounds__(256) void bn_bwd_reg_kernel(const pg_bn_args a) {
    typedef typename BnVec<VEC>::T V;
    __shared__ float scratch[16];
    const int c = blockIdx.x, n = a.B * a.L;
    const float* xc = a.x + (long)c * a.L;
    const float* dyc = a.dy + (long)c * a.L;
    const float mean = a.save_mean[c], invstd = a.save_invstd[c];
    V xh[UPT], dy[UPT];
    int pk[UPT];
    float s1 = 0.f, s2 = 0.f;
    BnWalk w = bn_walk(a.L, VEC);
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
        const bool ok = w.b < a.B;
        pk[i] = ok ? (w.b << 16) | w.u : -1;
        dy[i] = *(const V*)(dyc + (ok ? (long)w.b * a.dy_bs + VEC * w.u : 0L));   // branch-free: all loads issue back to back
        const V xv = *(const V*)(xc + (ok ? (long)w.b * a.x_bs + VEC * w.u : 0L));
        xh[i] = (xv - mean) * invstd;
        if (!ok) { dy[i] = V(0.f); xh[i] = V(0.f); }
#pragma unroll
        for (int k = 0; k < VEC; ++k) { s1 += bn_lane<VEC>(dy[i], k); s2 += bn_lane<VEC>(dy[i], k) * bn_lane<VEC>(xh[i], k); }
        bn_next(w);
    }
    const float sum_dy = pg_block_sum(s1, scratch);
    const float sum_dy_xhat = pg_block_sum(s2, scratch);
    const float kk = a.gamma[c] * invstd, m1 = sum_dy / (float)n, m2 = sum_dy_xhat / (float)n;
    float* dxc = a.dx + (long)c * a.L;
#pragma unroll
    for (int i = 0; i < UPT; ++i)
        if (pk[i] >= 0) *(V*)(dxc + (long)(pk[i] >> 16) * a.dx_bs + VEC * (pk[i] & 0xffff)) = kk * (dy[i] - m1 - xh[i] * m2);
    if (threadIdx.x == 0) {
        a.dgamma[c] = sum_dy_xhat;
        a.dbeta[c] = sum_dy;
    }
}

// dx = gamma * invstd * (dy - mean(dy) - xhat * mean(dy * xhat));  dgamma = sum(dy * xhat);  dbeta = sum(dy)
__global__ __launch_bounds__(256) void bn_bwd_kernel(const pg_bn_args a) {
    __shared__ float scratch[16];
    const int c = blockIdx.x, n = a.B * a.L;
    const float* xc = a.x + (long)c * a.L;
    const float* dyc = a.dy + (long)c * a.L;
    const float mean = a.save_mean[c], invstd = a.save_invstd[c];
    float s1 = 0.f, s2 = 0.f;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int b = e / a.L, l = e - b * a.L;
        const float dy = dyc[(long)b * a.dy_bs + l];
        s1 += dy;
        s2 += dy * (xc[(long)b * a.x_bs + l] - mean) * invstd;
    }
    const float sum_dy = pg_block_sum(s1, scratch);
    const float sum_dy_xhat = pg_block_sum(s2, scratch);
    const float k = a.gamma[c] * invstd, m1 = sum_dy / (float)n, m2 = sum_dy_xhat / (float)n;
    float* dxc = a.dx + (long)c * a.L;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int b = e / a.L, l = e - b * a.L;
        const float xhat = (xc[(long)b * a.x_bs + l] - mean) * invstd;
        dxc[(long)b * a.dx_bs + l] = k * (dyc[(long)b * a.dy_bs + l] - m1 - xhat * m2);
    }
    if (threadIdx.x == 0) {
        a.dgamma[c] = sum_dy_xhat;
        a.dbeta[c] = sum_dy;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Per-clip statistics: every row (b, c) of L frames is normalised by its own mean and biased variance, which is what the
// reference's batch-of-one inference forwards compute (demo.py:33-45, train.py:76-83: no .eval() anywhere), for B clips in one
// launch.  The running buffers end up exactly as after B batch-of-one calls in clip order.
//
// Mapping.  Rows are short (29 ... 256 frames in the U-Net) and there are B * C of them; consecutive channels of a sample are
// contiguous.  A row gets a power-of-two lane GROUP (16 / 32 / 64 lanes by L), a wave covers the 4 / 2 / 1 adjacent rows -- one
// contiguous span of memory --, lane j of a group holds units j, j + G, j + 2 G, ... of its row in registers (a unit = 1 float,
// or 4 where L % 4 == 0).  One HBM read; mean, centred squares and the outputs come from the registers (the two-pass arithmetic of
// bn_fwd_reg_kernel); the group sums are butterflies (pg_group_sum).  No LDS, no barrier, no atomics: waves are independent and walk
// the rows grid-stride.  A wave's pass over its rows is one latency chain (load, reduce, store), so the groups are kept NARROW --
// up to 8 units per lane before the next width -- to have 1-2 KB per wave in flight (one 129-frame row per wave on 64 lanes runs
// at half the rate; measurements in DESIGN.md section 4.6).
// Reduction order.  Group width, units per lane and unit size are functions of L ALONE (where 16-byte accesses are not possible
// the same units are moved as scalars), so a row's statistics and outputs do not depend on B, the grid, the alignment of the
// tensors or on which rows share its wave: a clip normalised inside a batch is bit-identical to the same clip normalised alone.
// Rows longer than CN_REG_MAX frames take a looping kernel (one wave per row, three passes over the row).
// Running buffers.  The main kernel leaves every row's mean and biased variance in the caller's workspace; a second small kernel
// (launched only when a running buffer or the counter is given) walks b = 0 .. B-1 per channel: one momentum step per clip.
// ---------------------------------------------------------------------------------------------------------
constexpr int CN_REG_MAX = 1024;   // longest row the register-resident kernels hold (16 values per lane on 64 lanes)
constexpr int CN_CHAIN = 16;       // clips whose statistics the running-buffer kernel fetches at a time

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
                const f32x4 t = *(const f32x4*)p;
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[i][k] = ok ? t[k] : 0.f;
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { const float t = p[k]; v[i][k] = ok ? t : 0.f; }
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) s += v[i][k];
        }
        const float mean = pg_group_sum<G>(s) / (float)a.L;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < UPL; ++i)
            if (rok && sub + i * G < Lu) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { const float d = v[i][k] - mean; q += d * d; }
            }
        const float var = pg_group_sum<G>(q) / (float)a.L;
        const float invstd = 1.0f / sqrtf(var + a.eps);
        const float ga = a.gamma[c], be = a.beta[c];
#pragma unroll
        for (int i = 0; i < UPL; ++i)
            if (rok && sub + i * G < Lu) {
                float o[VEC];
#pragma unroll
                for (int k = 0; k < VEC; ++k) o[k] = (v[i][k] - mean) * invstd * ga + be;
                norm_store<VEC, WIDE>(a, b, c, VEC * (sub + i * G), o);
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
        const float mean = pg_group_sum<64>(s) / (float)a.L;
        float q = 0.f;
        for (int l = lane; l < a.L; l += 64) { const float d = xr[l] - mean; q += d * d; }
        const float var = pg_group_sum<64>(q) / (float)a.L;
        const float invstd = 1.0f / sqrtf(var + a.eps);
        const float ga = a.gamma[c], be = a.beta[c];
        for (int l = lane; l < a.L; l += 64) {
            const float o = (xr[l] - mean) * invstd * ga + be;
            norm_store<1, false>(a, b, c, l, &o);
        }
        if (lane == 0) cn_save(a, r, mean, var, invstd);
    }
}

// The running buffers after B batch-of-one BatchNorm calls in clip order: one thread per channel walks b = 0 .. B-1 (one
// norm_running_step with n = L per clip); nn.BatchNorm's counter advances by B.
__global__ __launch_bounds__(64) void clipnorm_running_kernel(const pg_clipnorm_args a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += a.B;
    if (c >= a.C || !a.workspace) return;                        // (no workspace: only the counter was asked for)
    const float* mean = (const float*)a.workspace;
    const float* var = mean + (long)a.B * a.C;
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
            if (b0 + j < a.B) norm_running_step(&rm, &rv, 0, a.momentum, m[j], v[j], a.L);
    }
    if (a.running_mean) a.running_mean[c] = rm;
    if (a.running_var) a.running_var[c] = rv;
}

// ---------------------------------------------------------------------------------------------------------
// Host side: launch plans
// ---------------------------------------------------------------------------------------------------------
// 16-byte accesses to an fp32 tensor, 8-byte ones to a bf16 tensor (a tensor that is not given allows everything)
bool ok16(const void* p, long bs) { return p == nullptr || ((((uintptr_t)p) & 15) == 0 && (bs & 3) == 0); }
bool ok8(const void* p, long bs, int pitch) { return p == nullptr || ((((uintptr_t)p) & 7) == 0 && (bs & 3) == 0 && (pitch & 3) == 0); }
// does every given output tensor of a forward allow them?
template <typename Args>
bool wide_ok(const Args* a) {
    return ok16(a->y, a->y_bs) && ok16(a->y2, a->y2_bs) && ok8(a->yh, a->yh_bs, a->yh_pitch) && ok8(a->yh2, a->yh2_bs, a->yh2_pitch);
}

int bn_check(const pg_bn_args* a) {
    if (!a) return pg_fail(PG_ERR_NULL, "bn: null args");
    if (a->B <= 0 || a->C <= 0 || a->L <= 0) return pg_fail(PG_ERR_SHAPE, "bn: non-positive dimension");
    if ((long)a->B * a->L > 0x7fffffffL) return pg_fail(PG_ERR_SHAPE, "bn: B*L too large");
    return PG_OK;
}

// register-resident BN: the channel's B * L values fit 64 registers per thread; 16-byte units where every tensor allows them
bool bn_reg_plan(const pg_bn_args* a, bool bwd, int& vec, int& upt) {
    const long n = (long)a->B * a->L;
    if (n > 64L * 256) return false;
    bool v4 = (a->L & 3) == 0 && ok16(a->x, a->x_bs);
    if (bwd) v4 = v4 && ok16(a->dy, a->dy_bs) && ok16(a->dx, a->dx_bs);
    else v4 = v4 && wide_ok(a);
    auto ok8f = [](const void* p, long bs) { return p == nullptr || ((((uintptr_t)p) & 7) == 0 && (bs & 1) == 0); };
    bool v2 = (a->L & 1) == 0 && ok8f(a->x, a->x_bs);
    if (bwd) v2 = v2 && ok8f(a->dy, a->dy_bs) && ok8f(a->dx, a->dx_bs);      // (forward stores of a float2 unit are scalar)
    vec = v4 ? 4 : (v2 ? 2 : 1);
    const long units = n / vec;
    upt = (int)((units + 255) / 256);
    return true;
}

template <bool BWD>
void bn_launch_reg(const pg_bn_args* a, int vec, int upt, hipStream_t st) {
#define PG_BN_LAUNCH(U, V) { if (BWD) hipLaunchKernelGGL((bn_bwd_reg_kernel<U, V>), dim3(a->C), dim3(256), 0, st, *a); \
                             else hipLaunchKernelGGL((bn_fwd_reg_kernel<U, V>), dim3(a->C), dim3(256), 0, st, *a); }
    // (units-per-thread values are the ones hipcc allocates sanely: <8, 4> and <16, 2> take 180-245 VGPRs and spill)
    // (the small ones are for single clips -- demo.py's batch of one: 64 values per channel -- where walking 16 or 32 empty units
    // per thread made a 2048-channel layer take 12-26 us)
    if (vec == 4) { if (upt <= 1) PG_BN_LAUNCH(1, 4) else if (upt <= 4) PG_BN_LAUNCH(4, 4) else PG_BN_LAUNCH(16, 4) }
    else if (vec == 2) { if (upt <= 2) PG_BN_LAUNCH(2, 2) else PG_BN_LAUNCH(32, 2) }
    else { if (upt <= 2) PG_BN_LAUNCH(2, 1) else if (upt <= 16) PG_BN_LAUNCH(16, 1) else if (upt <= 33) PG_BN_LAUNCH(33, 1) else PG_BN_LAUNCH(64, 1) }
#undef PG_BN_LAUNCH
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
    p.wide = p.vec == 4 && ok16(a->x, a->x_bs) && wide_ok(a);
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

extern "C" int pg_bn_fwd(const pg_bn_args* a, void* stream) {
    if (int e = bn_check(a)) return e;
    if (!a->x || (!a->y && !a->yh) || !a->gamma || !a->beta || !a->save_mean || !a->save_invstd)
        return pg_fail(PG_ERR_NULL, "bn_fwd: x, y (or yh), gamma, beta, save_mean, save_invstd required");
    if ((a->yh && a->yh_pitch < a->L) || (a->yh2 && a->yh2_pitch < a->L)) return pg_fail(PG_ERR_SHAPE, "bn_fwd: bf16 output pitch below L");
    int vec, upt;
    if (bn_reg_plan(a, false, vec, upt)) bn_launch_reg<false>(a, vec, upt, (hipStream_t)stream);
    else hipLaunchKernelGGL(bn_fwd_kernel, dim3(a->C), dim3(256), 0, (hipStream_t)stream, *a);
    return pg_launch_ok("bn_fwd launch failed");
}

extern "C" int pg_bn_bwd(const pg_bn_args* a, void* stream) {
    if (int e = bn_check(a)) return e;
    if (!a->x || !a->dy || !a->dx || !a->gamma || !a->save_mean || !a->save_invstd || !a->dgamma || !a->dbeta)
        return pg_fail(PG_ERR_NULL, "bn_bwd: x, dy, dx, gamma, save_mean, save_invstd, dgamma, dbeta required");
    int vec, upt;
    if (bn_reg_plan(a, true, vec, upt)) bn_launch_reg<true>(a, vec, upt, (hipStream_t)stream);
    else hipLaunchKernelGGL(bn_bwd_kernel, dim3(a->C), dim3(256), 0, (hipStream_t)stream, *a);
    return pg_launch_ok("bn_bwd launch failed");
}

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
    if (int e = pg_launch_ok("clipnorm_fwd launch failed")) return e;
    if (chain || k.num_batches_tracked) {
        hipLaunchKernelGGL(clipnorm_running_kernel, dim3((unsigned)((k.C + 63) / 64)), dim3(64), 0, st, k);
        return pg_launch_ok("clipnorm_fwd running-buffer launch failed");
    }
    return PG_OK;
}
