/* phasegen.h -- C ABI of libphasegen.so: the MI355X (gfx950) hot path of UNet-PhaseGen.
 *
 * The reference (LemonATsu/UNet-PhaseGen) is pure Python and has no FFI of its own; what it binds on
 * this path is torch.nn.Conv1d / ConvTranspose1d / BatchNorm / (Leaky)ReLU / cat (model.py:77-113),
 * MSELoss + Adam (train.py:26-28,45-62), np.abs/np.angle (data.py:39-47) and librosa.stft / istft
 * (preproc_mdb.py:93, utils.py:40) and librosa.resample (preproc_mdb.py:114).  Each entry point below replaces one of those and cites it.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, scalars; no torch types.  All tensors fp32.
 *   - activations are (B, channels, frames), frames fastest; a tensor is given as {ptr, batch_stride}
 *     (elements) so a channel slice of a wider buffer (the U-Net's concat halves) is passed without copy.
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library allocates nothing and keeps
 *     no mutable global state besides a thread-local last-error string: every knob (MFMA operand precision,
 *     work-split schedule, FFT schedule) is a field of the call's argument struct, so calls on different
 *     streams / threads are independent.  A workspace belongs to ONE stream at a time.
 *   - every call is asynchronous on the hipStream_t passed as `void* stream`; no internal syncs.
 *   - return 0 on success, <0 = PG_ERR_* (bad argument), >0 = hipError_t from the launch.
 *
 * Non-finite values
 *   A NaN or +-inf in an input is ordinary data to every entry point: no call fails on it, and what it does to the outputs is
 *   part of the contract.  The entry points that state a rule of their own keep it (pg_stitch's count, pg_phase_join's fallback,
 *   pg_phase_vocoder's q(x) and "a NaN in M does not reset", pg_phase_lock / _linked / pg_phase_spsi, slot 5 of the compare kernels,
 *   pg_hpss's total order, pg_formant_shift's confinement: a non-finite or out-of-domain cell of its plane affects only the outputs
 *   of its own (channel, frame), and every other frame has the bits of the clean call).
 *   For every other one -- the conv entry points, pg_conv_fwd_h, pg_bn_fwd / _bwd, pg_clipnorm_fwd, pg_loss_fwd_bwd, pg_adam_step,
 *   pg_cast_rows_bf16, pg_stft, pg_stft_crops, pg_polar, pg_istft, pg_gl_project, pg_ola_nt, pg_moments / pg_standardize,
 *   pg_resample, pg_spec_clips, pg_ola_stretch -- let ref(x) be the entry point's documented formula evaluated in IEEE arithmetic on the input
 *   with ONE element replaced by NaN, +inf or -inf, where
 *     - an activation is the select x >= 0 ? x : slope * x, its derivative x > 0 ? 1 : slope (a NaN in a dgrad's mask source is a
 *       comparison that fails: the factor is the slope, nothing else happens);
 *     - zero padding, the zeros between the frames of a transposed convolution and the samples outside a signal's ends are "no term",
 *       not a product with zero;
 *     - a maximum (the peak of pg_istft / pg_ola_nt with normalize) that sees a NaN is a NaN: the whole signal becomes NaN;
 *     - z = re + 1j * im of pg_polar / pg_gl_project is data.py:40's arithmetic: an infinite im makes the real part NaN on its way;
 *     - a term of a transform whose coefficient is exactly zero (cos or sin of a multiple of pi / 2: every bin at taps 0 and n_fft / 2,
 *       the imaginary part of the Nyquist bin) may carry the non-finite value or not: a fast transform never forms that product.
 *   R1, nothing is swallowed: an output element that is non-finite in ref is non-finite on the device.  No exceptions.  (Finite
 *       against non-finite is what is promised, not NaN against inf: the bf16x3 split answers NaN for inf, inf - inf.)
 *   R2, nothing spreads: an output element that is finite in ref and equal there to ref of the clean input has the bits of the same
 *       call on the clean input, and a clean call after a poisoned one on the same workspace has the clean bits.  Exceptions:
 *     C1  zeros that are multiplied in.  The convolution kernels read padding, inserted zeros and the frames past the end of the
 *         partner operand as 0.0 and multiply, and 0 * NaN = 0 * inf = NaN.  A non-finite WEIGHT w[o, c, j] may therefore turn
 *         every frame of every sample of its output channel o (forward) or input channel c (dgrad) into NaN, not only the frames
 *         whose window holds tap j on a real sample; a non-finite x[b, c, t] (dy[b, o, t]) of a WGRAD may turn every tap of
 *         dw[., c, .] (dw[o, ., .]) into NaN, not only the taps that pair frame t with a frame of dy (x).  Never another channel
 *         (pair).  All kernel families, all precisions, pg_conv_fwd_h included.  Skipping those products would put a select on
 *         every fragment load of the benchmarked kernels.
 *     C2  zero-weight phantom taps.  The im2col transposed form (conv_t: the ConvTranspose1d forward and the Conv1d dgrad where the
 *         raw-window kernels do not apply) runs its taps phase by phase and rounds k up to stride * ceil(k / stride) taps of zero
 *         weight where the stride does not divide k.  A non-finite input frame t (x of the forward, dy of the dgrad) may turn the
 *         frames t stride - pad + j, j = k .. stride ceil(k / stride) - 1, of every channel of its sample into NaN: the one or two
 *         frames behind its window.
 *   Cones (what ref makes non-finite), for orientation: conv forward / dgrad -- the frames of one sample whose window holds the
 *   element, every channel (a weight: one channel, every sample); wgrad -- one channel's taps; BatchNorm -- the channel (clipnorm:
 *   the row) with its save_* and running buffers; loss -- two of the three losses and one element of dpred; Adam -- that element's
 *   p / m / v; STFT -- every bin of the frames that hold the sample; ISTFT -- the samples the frame overlaps (normalize: the
 *   signal); resample -- the outputs whose taps hold the sample; spec_clips -- the output frames that read the source frame with
 *   a non-zero weight; ola_stretch -- the outputs one of whose covering frames reads the sample; moments / standardize -- everything.
 *   tests/_nonfinite.py, tests/test_nonfinite_host.py and tests/test_z_nonfinite_gpu.py hold every entry point to it.
 *
 * Magnitude range
 *   Every finite fp32 value, denormals and FLT_MAX included, is ordinary data: no call faults on it.  What the exponent of the data
 *   does to the outputs is contract, in four rules for the entry points that are compositions of additions, products with constants,
 *   FMAs, maxima, selects and positively homogeneous activations, and as a stated domain for the others.  ref64 is the entry point's
 *   documented formula in float64 on the fp32 values actually stored; B is the error bound the entry point meets on data of order
 *   one (for a convolution: 4 x that of sequential fp32 accumulation of the same operands, per element, relative to sum |a b|).
 *   M1, scale equivariance.  Multiply every operand by an exact power of two.  While every operand element and every output of ref64
 *       stays a normal fp32 number (or an exact zero; and a normal bf16 number where the mode casts), the outputs are the outputs of
 *       the unscaled call times the product of the powers, BIT FOR BIT.  Outputs the formula makes scale-free keep their bits: a
 *       normalised pg_istft / pg_ola_nt, pg_gl_project in S, the angle of pg_polar, pg_standardize, and the phases of pg_phase_vocoder,
 *       pg_phase_lock, pg_phase_lock_linked (magnitude plane and reset_below scaled together) and pg_phase_spsi.  No kernel holds an
 *       absolute epsilon, a narrower intermediate or a flush on these paths.
 *   M2, gradual underflow.  Operands normal, outputs of ref64 below FLT_MIN: |out - ref64| <= B 2^e + R 2^-150, 2^e the total scale
 *       and R the number of roundings on the output's path ((2 t + 1) K + 3 for a convolution whose GEMM is K deep, t = 3 for the
 *       bf16x3 split and 1 otherwise).  Nothing is flushed to zero.
 *   M3, denormal operands.  The fp32 paths read them as they are: M1 / M2's bound against ref64 on the stored values.
 *       The bf16, bf16x3 and pg_conv_fwd_h paths KEEP them as well (measured on an MI355X, gfx950, 2026-10-20: every element of every
 *       row, no operand flushed to zero): the conversion rounds a denormal fp32 operand to the bf16 denormal (RNE; the smallest is
 *       2^-133) and the bf16 MFMA multiplies it as it is, so the outputs are ref64 on the bf16-rounded operands within B.  For bf16x3
 *       that is float32(hi) + float32(lo) with lo = bf16(x - hi), which has no bits below 2^-133 either: a denormal operand is carried
 *       at bf16's precision by the split, not fp32's.  pg_cast_rows_bf16 rounds the same way.
 *   M4, overflow.  With S = sum |a b| in float64 along an output's sum: S < FLT_MAX / 2 -- the output is finite and within B S;
 *       |ref64| > FLT_MAX (1 + B) -- the output is +-inf with ref64's sign (bf16x3: or NaN, as R1 says).  In between (a partial sum
 *       of a split-K or stream-K tile may overflow where the total does not) nothing is promised.  A store activation sees the
 *       overflowed sum; these two zones are stated for the sum.
 *   Which rule holds where:
 *     M1 - M4  pg_conv1d_* / pg_convt1d_* forward, dgrad (with addend and mask) and wgrad (without the fused Adam epilogue, which is
 *              not homogeneous) at fp32, bf16 and bf16x3; pg_conv_fwd_h (yh / yh2 are y activated and rounded once to bf16).
 *     M1       pg_stft and pg_stft_crops without stats or polar, pg_istft mode 1, pg_ola_nt, pg_gl_project (equivariant in mag,
 *              invariant in S), pg_resample, pg_stitch (normalize: invariant), pg_spec_clips, pg_ola_stretch (x and base scaled
 *              together), pg_hpss (both planes), pg_bn_bwd in dy, pg_cast_rows_bf16 (a denormal input is rounded to the bf16
 *              denormal, RNE, not flushed), pg_moments (in double), pg_standardize, |z| of pg_polar with use_exp = 0, the phase
 *              kernels above; pg_wave_compare and pg_spec_compare: slots 0 - 3 scale with 2^(2 e) (pg_wave_compare's slot 4 with
 *              2^e), as doubles, at every fp32 exponent of the inputs -- both kernels widen before they multiply.
 *     M3 / M2  the same linear kernels (pg_stft, pg_istft mode 1, pg_ola_nt, pg_resample, pg_stitch, pg_spec_clips, pg_ola_stretch,
 *              pg_hpss) on inputs below FLT_MIN: their gain is one or more, so outputs below FLT_MIN come from such inputs; these
 *              are read as they are and the outputs are within B 2^e + R 2^-150 of ref64 (R = 16 n_fft for a transform: every
 *              rounding in an output's cone), nothing flushed; pg_spec_clips, pg_ola_stretch and pg_hpss keep the bits of their
 *              fp32 restatements there.
 *   Domains of the entry points that are not homogeneous; outside them the result is unspecified (finite or not), inside them the
 *   entry point meets its float64 restatement at its usual bound:
 *     pg_polar           every finite (re, im): |z| within 6e-7 relative plus one rounding where |z| < FLT_MIN, the angle within 3e-7
 *                        rad; |z| > FLT_MAX gives +inf, so use_exp = 1 wants |z| <= FLT_MAX (log1p of it would be finite, 88.7).
 *     pg_spec_compare    slots 0 - 3 and 5: every finite cell.  Slot 4 rounds m^2 to fp32 inside the logarithm: it wants
 *                        m^2 <= FLT_MAX (|z| < 2^64) for both magnitudes, and floor_power scaled along with the data.
 *     pg_adam_step       |grad_scale g| < 2^63 (g^2 is formed in fp32) and v < 2^126.  Below, everything is IEEE arithmetic with
 *                        denormals kept: g^2 and v underflow gradually, bit for bit as an fp32 restatement does.
 *     pg_bn_fwd, pg_clipnorm_fwd   |x - mean| < 2^63 (the centred squares are formed in fp32); y2 / yh / yh2 are the fp32 y activated
 *                        and, for the bf16 rows, rounded once, at every scale.  Data so small that the squares are
 *                        denormals or zero is normalised by eps alone, as the formula says.
 *     pg_loss_fwd_bwd    |m^ - m| < 2^63 per element and B C L (m^ - m)^2 summable in fp32; phases: |p| < 2^31 pi (pg_sincos's
 *                        reduction), the angle terms are bounded by 4 at any magnitude.
 *     pg_istft mode 0    the sum over a frame's bins of exp(m) below FLT_MAX / 4 (the butterflies add a frame's bins before the 1 / n_fft;
 *                        a single cell may reach m = 87, exp(m) = 2^125.5); pg_sincos wants |phi| < 2^31 pi.
 *     pg_formant_shift   the plane is a logarithm: no scale rule applies, and its stated domain (finite, 0 <= M <= 80) is the rule.
 *     normalize (pg_istft, pg_ola_nt, pg_stitch)   a peak <= FLT_MIN leaves the signal as it is (the early return): scale-free
 *                        outputs are promised for peaks above FLT_MIN.
 *   tests/_range.py, tests/test_range_host.py and tests/test_z_range_gpu.py hold the rows named there; DESIGN.md section 4.17 lists
 *   what was measured and what is not yet held.
 */
#ifndef PHASEGEN_H
#define PHASEGEN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_VERSION 400 /* 0.4.0: pg_bn_args.num_batches_tracked; (0.3.0: pg_conv_fwd_h reads its zero padding from the rows' tails and a
                        * PG_H_HEAD zero head; 0.2.0: knobs in the argument structs).  Argument structs GROW between minor versions
                        * (new fields are appended, and a zero / NULL there means the old behaviour), so their SIZE is part of the ABI:
                        * a caller compiled against an older header passes a shorter struct and the library would read past its end.
                        * Callers check pg_version() / 100 == PG_VERSION / 100 at load time and are rebuilt when it differs. */

enum { PG_OK = 0, PG_ERR_NULL = -1, PG_ERR_SHAPE = -2, PG_ERR_ALIGN = -3, PG_ERR_UNSUPPORTED = -4,
       PG_ERR_WORKSPACE = -5 };

/* activation fused on operand load / derivative mask fused in a dgrad epilogue */
enum { PG_ACT_NONE = 0, PG_ACT_LEAKY02 = 1 /* nn.LeakyReLU(0.2), model.py:80 */, PG_ACT_RELU = 2 /* model.py:82 */ };

/* One descriptor serves the six convolution entry points.  Geometry is always that of the FORWARD op:
 *   Conv1d          x (B,Cin,Lin) * w (Cout,Cin,k)  -> y (B,Cout,Lout),  Lout = (Lin + 2 pad - k)/stride + 1
 *   ConvTranspose1d x (B,Cin,Lin) * w (Cin,Cout,k)  -> y (B,Cout,Lout),  Lout = (Lin - 1) stride - 2 pad + k
 * bias is never used (model.py:65-69: use_bias == False under BatchNorm).
 * Every tensor a kernel READS through a buffer descriptor must span less than 2 GiB - 16 bytes from its pointer, the batch stride
 * included ((B - 1) * bs + C * L) * 4 < 0x7ffffff0: x and dy where they are gathered, w, and the dgrad's dx_add and dx_ref (dx_ref
 * only where dx_mask uses it).  A larger one is refused before any launch with PG_ERR_SHAPE ("... exceeds 2 GiB (31-bit buffer
 * offsets)").  The tensors a call WRITES (y, y2, dx) are addressed with 64-bit arithmetic: their batch strides have no such limit. */
struct pg_adam_args;
typedef struct pg_conv_args {
    int32_t B, Cin, Cout, Lin, Lout, k, stride, pad;
    const float* x;  int64_t x_bs;   /* forward input; read by *_fwd and *_wgrad                           */
    int32_t x_act;                   /* PG_ACT_* applied to x as it is read (the in-place (Leaky)ReLU that  */
                                     /*   precedes the conv in model.py:91,96,103 is never materialised)    */
    int32_t precision;               /* PG_PREC_*: operand precision of the MFMA contraction (below)        */
    const float* w;                  /* weights (layout above); read by *_fwd and *_dgrad                  */
    float* y;        int64_t y_bs;   /* forward output; written by *_fwd                                   */
    const float* dy; int64_t dy_bs;  /* grad wrt y; read by *_dgrad and *_wgrad                            */
    float* dx;       int64_t dx_bs;  /* grad wrt the tensor x was read from; written by *_dgrad            */
    const float* dx_add; int64_t dx_add_bs; /* optional (NULL): added to the dgrad result before masking (skip grad) */
    const float* dx_ref; int64_t dx_ref_bs; /* optional (NULL): dx *= act'(dx_ref) with act = dx_mask              */
    int32_t dx_mask;
    int32_t schedule;                /* 0 = automatic; otherwise PG_SCHED_* bits (tests and measurements)   */
    float* dw;                       /* grad wrt w, same layout as w; OVERWRITTEN by *_wgrad (beta = 0:     */
                                     /*   optim.zero_grad(), train.py:41, is folded into the write)         */
    int32_t y_act; int32_t y2_act;   /* *_fwd only: activation applied to the result as it is STORED (producers can */
    float* y2;       int64_t y2_bs;  /*   hand consumers pre-activated tensors); y2 = optional second copy with its */
                                     /*   own activation (the skip tensor is read as LeakyReLU by the next down conv */
                                     /*   and as ReLU by the up path, model.py:80,82,113)                           */
    void* workspace; int64_t workspace_bytes; /* optional scratch (pg_workspace_bytes_conv()): lets tile counts   */
                                     /*   that quantise badly over the CUs be split evenly (stream-K);      */
                                     /*   contents are garbage between calls; NULL = always one tile per WG. */
                                     /*   *_wgrad at fp32 also packs its operands here, behind that region: */
                                     /*   it needs pg_workspace_bytes_wgrad(a, op) bytes (else              */
                                     /*   PG_ERR_WORKSPACE); more than pg_workspace_bytes_conv() never      */
                                     /*   changes how a call splits its work                                 */
    const struct pg_adam_args* adam; /* *_wgrad only, optional (NULL): the optimiser step of THIS weight fused into the   */
                                     /*   wgrad epilogue (train.py:61-62 in one kernel): adam->p / m / v are the weight,   */
                                     /*   exp_avg and exp_avg_sq tensors (layout of w), updated from the gradient value the */
                                     /*   epilogue stores to dw -- same arithmetic as pg_adam_step, bit for bit; adam->g   */
                                     /*   and adam->n are ignored.  Callers order the layer's dgrad (which reads w) BEFORE */
                                     /*   this call on the stream.  Not for data-parallel runs (reduce first).             */
} pg_conv_args;
int64_t pg_workspace_bytes_conv(void);
/* Workspace one wgrad call needs (op: PG_OP_CONV1D_WGRAD / PG_OP_CONVT1D_WGRAD, below): pg_workspace_bytes_conv() plus the fp32
 * raw-window kernels' packed operands (Q rows with zero halos, P with K contiguous per row; activation applied).  A pure host
 * function of the geometry, precision and schedule (pointers are not read); a negative value is the call's error code. */
int64_t pg_workspace_bytes_wgrad(const pg_conv_args* a, int32_t op);
/* pg_conv_args.precision (BASELINE config 5): PG_PREC_FP32 (0, default) = fp32 operands, v_mfma_f32_32x32x2_f32, the 1e-4
 * parity path; PG_PREC_BF16 = operands rounded to bf16 (RNE, after the fused activation) at fragment load,
 * v_mfma_f32_32x32x16_bf16, fp32 accumulate -- tensors and master weights in HBM stay fp32; PG_PREC_BF16X3 = every fp32
 * operand is split exactly into hi + lo bf16 parts and each product is taken as hi*hi' + hi*lo' + lo*hi' on the bf16 pipe
 * (three MFMAs at 1/16 of the fp32 cost; ~5e-6 from exact against fp32 MFMA's ~1e-6: inside the 1e-4 parity bound, not fp32). */
enum { PG_PREC_FP32 = 0, PG_PREC_BF16 = 1, PG_PREC_BF16X3 = 2 };
/* pg_conv_args.schedule: bits 0-1 work split (0 automatic, 1 one tile per workgroup, 2 force stream-K); bit 2: no raw-window
 * kernels (im2col kernels); bit 3: no tall (256 x 128) raw tile; bit 4: other kernels (RCCL collectives) share the chip --
 * keep the fine stream-K split even where the tile count quantises perfectly; bits 8-11: stream-K grid = that many x the
 * resident workgroup slots (1..8; 0 = default 4; > 1 bounds the tail when other kernels such as RCCL's share the chip); bit 7: the
 * wgrad keeps the flat-K kernel; bit 13: never the one-wave-per-SIMD fp32 F / T kernels (conv_raw3.hip); bit 14: those kernels wherever they cover the problem;
 * bits 15-16: their tile order (1: row-major, 2 / 3: super-rows of 2 / 4 tile rows; 0: automatic) -- measurements only.
 * PG_SCHED_NO_COLSPLIT (bit 17): the conv_raw3 launches keep a short column tail (<= 128 columns past the last full 256-wide tile)
 * instead of handing it to a second launch of the tall-tile kernel (pg_conv_describe shows the second launch as |tail=...);
 * PG_SCHED_COLSPLIT (bit 18): the tail launch wherever the geometry allows, whatever the cost model says (tests).
 * PG_SCHED_SLOTS(n) (bits 19-23, n = 1..31; 0 = the device's own count; additive, PG_VERSION unchanged): plan this call as if the device had n compute
 * units.  Host side only: the grid, the whole / split classes of workgroups and the pricing of the column tail follow n, the kernels
 * are the ones every call runs.  Tests use it to put a small problem through the work splits a full-size layer takes on 256 CUs
 * (several whole tiles per workgroup, ranges that hold whole tiles between two partial ones, the hybrid split). */
enum { PG_SCHED_AUTO = 0, PG_SCHED_TILE_PER_WG = 1, PG_SCHED_FORCE_STREAMK = 2, PG_SCHED_NO_RAW = 4, PG_SCHED_NO_TALL = 8,
       PG_SCHED_CONTENDED = 16, PG_SCHED_NO_PS = 128, PG_SCHED_NO_RAW3 = 0x2000, PG_SCHED_ALL_RAW3 = 0x4000, PG_SCHED_NO_COLSPLIT = 0x20000, PG_SCHED_COLSPLIT = 0x40000 };
#define PG_SCHED_OVERSUB(f) (((f) & 15) << 8)
#define PG_SCHED_SLOTS(n) (((n) & 31) << 19)

/* nn.Conv1d forward / backward (model.py:77-78; autograd of train.py:61) */
int pg_conv1d_fwd(const pg_conv_args* a, void* stream);
int pg_conv1d_dgrad(const pg_conv_args* a, void* stream);
int pg_conv1d_wgrad(const pg_conv_args* a, void* stream);
/* nn.ConvTranspose1d forward / backward (model.py:88-89,94-95,101-102) */
int pg_convt1d_fwd(const pg_conv_args* a, void* stream);
int pg_convt1d_dgrad(const pg_conv_args* a, void* stream);
int pg_convt1d_wgrad(const pg_conv_args* a, void* stream);
/* The launch plan of one of the six calls above WITHOUT launching it (measurement aid; pure function of the arguments):
 * buf receives "kernel<template args>|grid=G|tiles=T|slabs=S|split=0/1|whole=W|fixup=none/plain/wide", the kernel named as rocprofv3 reports it. */
enum { PG_OP_CONV1D_FWD = 0, PG_OP_CONV1D_DGRAD = 1, PG_OP_CONV1D_WGRAD = 2,
       PG_OP_CONVT1D_FWD = 3, PG_OP_CONVT1D_DGRAD = 4, PG_OP_CONVT1D_WGRAD = 5 };
int pg_conv_describe(const pg_conv_args* a, int32_t op, char* buf, int32_t buflen);

/* ---- bf16-RESIDENT forward convolutions (BASELINE configs[4]: "bf16 MFMA convs") ----------------------------------------
 * Same two forward ops, but the operands already live in HBM as bf16: activations (B, C, pitch) whose rows are `pitch`
 * elements apart (pitch and batch stride even, pitch > L, elements [L, pitch) of every row ZERO -- allocate zero-filled once;
 * producers never write the tail), weights as a bf16 shadow of the fp32 master weights in the kernels' GEMM layout
 * (pg_shadow_weights, rebuilt whenever the masters change).
 * Zero-padding contract of x (v0.3): the kernels gather row windows as unchecked 16-byte pieces, so the convolution's zero
 * padding is READ from memory: (1) every row's zero tail must cover what a window reaches in front of the NEXT row and behind
 * this row's last frame (pg_conv_fwd_h_supported checks the layer's need; 40 elements cover every layer of the U-Net), and
 * (2) the PG_H_HEAD elements (64 bytes) in front of x must be readable and zero -- for a channel slice of a larger tensor
 * they are the previous channel's tail; a tensor of its own is allocated with that many zero elements in front.  v_mfma_f32_32x32x16_bf16, fp32 accumulate.  Outputs: the fp32 result as is (y, optional: what
 * pg_bn_fwd normalises) and / or up to two bf16 copies stored already activated for the next layer.  Geometries: the U-Net's
 * (k, stride) pairs with Cin a multiple of 32 / min(taps per phase, 32); others return PG_ERR_UNSUPPORTED (use pg_conv*_fwd). */
#define PG_H_HEAD 32
typedef struct pg_convh_args {
    int32_t B, Cin, Cout, Lin, Lout, k, stride, pad;
    int32_t transposed;              /* 0: nn.Conv1d forward (model.py:77-78), 1: nn.ConvTranspose1d forward (model.py:88-102) */
    int32_t schedule;                /* work-split bits of pg_conv_args.schedule (0-1, 4, 8-11, 19-23).  One tile family since 0.4 (256 x 256 on 4
                                      * waves, one per SIMD); bits 5-6, which selected the removed ones, return PG_ERR_UNSUPPORTED */
    const uint16_t* x; int64_t x_bs; /* bf16 (B, Cin, x_pitch), batch stride in elements */
    int32_t x_pitch; int32_t _pad0;
    const uint16_t* w;               /* pg_shadow_weights output for this layer */
    float* y; int64_t y_bs;          /* optional fp32 (B, Cout, Lout) */
    uint16_t* yh; int64_t yh_bs; int32_t yh_pitch; int32_t yh_act;       /* optional bf16 (B, Cout, yh_pitch) = PG_ACT(result) */
    uint16_t* yh2; int64_t yh2_bs; int32_t yh2_pitch; int32_t yh2_act;   /* optional second bf16 copy with its own activation */
    void* workspace; int64_t workspace_bytes;   /* pg_workspace_bytes_conv() */
} pg_convh_args;
int pg_conv_fwd_h(const pg_convh_args* a, void* stream);
int pg_conv_fwd_h_supported(const pg_convh_args* a);   /* 1 / 0: geometry (sizes, strides, pitches; pointers ignored) is covered */
int pg_conv_fwd_h_describe(const pg_convh_args* a, char* buf, int32_t buflen);   /* launch plan without launching, as pg_conv_describe */
/* bf16 shadow of one conv layer's weights: Conv1d (Cout, Cin, k) -> [o][(q, j)] (a cast); ConvTranspose1d (Cin, Cout, k) ->
 * [(o, phase)][(q, tap)] with the taps of a phase in the order the gather-form kernel reads them, ceil(k / stride) taps per
 * phase rounded up to a power of two with zero weights (k = 5, stride 2: 4).  wh holds pg_shadow_elems(...) elements. */
int64_t pg_shadow_elems(int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t transposed);
int pg_shadow_weights(const float* w, uint16_t* wh, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t transposed, void* stream);
/* fp32 (B, C, L) -> bf16 (B, C, pitch) with PG_ACT applied and the row tails zeroed (the network input of the bf16 path). */
typedef struct pg_cast_args { int32_t B, C, L, pitch, act, _pad0; const float* x; int64_t x_bs; uint16_t* y; int64_t y_bs; } pg_cast_args;
int pg_cast_rows_bf16(const pg_cast_args* a, void* stream);

/* Train-mode batch norm over (B, L) per channel (model.py:81,83 applied to 3-D tensors; eps 1e-5, momentum
 * 0.1; biased variance normalises, unbiased variance goes to running_var). */
typedef struct pg_bn_args {
    int32_t B, C, L; float eps, momentum;
    const float* x;  int64_t x_bs;       /* raw conv output                                  */
    float* y;        int64_t y_bs;       /* fwd: normalised + affine output                  */
    const float* gamma; const float* beta;
    float* save_mean; float* save_invstd;     /* (C) written by fwd, read by bwd             */
    float* running_mean; float* running_var;  /* (C) updated in place by fwd; may be NULL    */
    const float* dy; int64_t dy_bs;      /* bwd: grad wrt y                                  */
    float* dx;       int64_t dx_bs;      /* bwd: grad wrt x                                  */
    float* dgamma; float* dbeta;         /* bwd: (C), overwritten                            */
    int32_t y_act; int32_t y2_act;       /* fwd: activation applied as y is stored; optional second output y2 with  */
    float* y2;       int64_t y2_bs;      /*   its own activation (same purpose as in pg_conv_args)                  */
    /* fwd, bf16-resident path: optional bf16 outputs (B, C, pitch) with their own activations (tails stay untouched);  */
    /* y may then be NULL                                                                                               */
    uint16_t* yh;  int64_t yh_bs;  int32_t yh_pitch;  int32_t yh_act;
    uint16_t* yh2; int64_t yh2_bs; int32_t yh2_pitch; int32_t yh2_act;
    int64_t* num_batches_tracked;        /* fwd, optional (NULL): the layer's nn.BatchNorm counter, incremented by one on the device */
} pg_bn_args;
int pg_bn_fwd(const pg_bn_args* a, void* stream);
int pg_bn_bwd(const pg_bn_args* a, void* stream);

/* BatchNorm forward with PER-CLIP statistics: the reference runs inference one clip at a time and never calls .eval()
 * (demo.py:33-45, train.py:76-83), so each clip is normalised by its own statistics.  This entry point does that for B clips in
 * one launch: every row (b, c) of L frames is normalised by ITS mean and biased variance (two-pass, eps inside the sqrt), i.e.
 * what B calls of pg_bn_fwd with a batch of one compute.  A row's result does not depend on B or on its position in the batch
 * (bit for bit).  Tensor conventions and the output fields (y / y2 fp32 with their activations, yh / yh2 bf16 (B, C, pitch) with
 * theirs, row tails untouched; at least one of y, yh) are those of pg_bn_args.  save_mean / save_invstd are optional and (B, C).
 * running_mean / running_var (C, each optional) end up as after B batch-of-one calls in the order b = 0 .. B-1:
 * rm = (1 - m) rm + m mean_b, rv = (1 - m) rv + m var_b L / max(L - 1, 1), one step per clip; *num_batches_tracked += B.
 * They need `workspace`: pg_workspace_bytes_clipnorm() bytes (2 B C floats: the per-row means and variances between the two
 * launches), else PG_ERR_WORKSPACE; without running buffers the workspace is not touched.  No backward exists: inference only. */
typedef struct pg_clipnorm_args {
    int32_t B, C, L; float eps, momentum; int32_t _pad0;
    const float* x;  int64_t x_bs;       /* raw conv output                                                    */
    float* y;        int64_t y_bs;       /* normalised + affine output, stored as PG_ACT(y_act); may be NULL if yh is given */
    float* y2;       int64_t y2_bs;      /* optional second fp32 copy with its own activation                   */
    int32_t y_act; int32_t y2_act;
    uint16_t* yh;  int64_t yh_bs;  int32_t yh_pitch;  int32_t yh_act;      /* optional bf16 outputs, as in pg_bn_args */
    uint16_t* yh2; int64_t yh2_bs; int32_t yh2_pitch; int32_t yh2_act;
    const float* gamma; const float* beta;    /* (C)                                                            */
    float* save_mean; float* save_invstd;     /* optional (NULL): (B, C), the statistics of every row           */
    float* running_mean; float* running_var;  /* optional (NULL): (C), updated in place, one step per clip      */
    int64_t* num_batches_tracked;             /* optional (NULL): incremented by B on the device                */
    void* workspace; int64_t workspace_bytes; /* required with running_mean / running_var                       */
} pg_clipnorm_args;
int64_t pg_workspace_bytes_clipnorm(const pg_clipnorm_args* a);   /* host function of B and C; negative = error code */
int pg_clipnorm_fwd(const pg_clipnorm_args* a, void* stream);

/* train.py:45-60: loss = MSE(cos p, cos th) + MSE(sin p, sin th) + mag_weight * MSE(m, logmag), fused with its
 * gradient wrt pred.  pred (B,2C,L) = [phase ; magnitude]; batch (B,2,C,L) = [logmag ; angle].
 * losses[0..2] = {loss, ang, mag}.  Deterministic two-stage reduction through `workspace`. */
typedef struct pg_loss_args {
    int32_t B, C, L; float mag_weight;
    const float* pred; const float* batch;
    float* dpred;      /* may be NULL (evaluation only) */
    float* losses;     /* 3 floats, device */
    void* workspace; int64_t workspace_bytes;
} pg_loss_args;
int64_t pg_workspace_bytes_loss(const pg_loss_args* a);
int pg_loss_fwd_bwd(const pg_loss_args* a, void* stream);

/* torch.optim.Adam.step with defaults (train.py:27,62) over one flat parameter arena: p -= lr/bc1 * m/(sqrt(v)/sqrt(bc2)+eps).
 * grad_scale multiplies g first (1/world for data-parallel averaging); step is 1-based. */
typedef struct pg_adam_args {
    int64_t n; float* p; const float* g; float* m; float* v;
    double lr, beta1, beta2, eps, grad_scale;   /* Python floats, rounded to fp32 exactly where torch rounds them */
    int32_t step;
    int32_t thin;    /* 0: full-rate streaming launch (the chip is idle); 1: at most one small workgroup per CU, <= 32 VGPRs,  */
                     /*    non-temporal accesses -- for running BESIDE the MFMA-bound conv kernels of backward on another stream */
} pg_adam_args;
int pg_adam_step(const pg_adam_args* a, void* stream);

/* librosa.stft(y, n_fft, hop) + DC drop + [re; im] stacking (preproc_mdb.py:84-97), optionally fused with
 * data.py:39-47 (polar = 1 -> out = [log1p|z| ; angle z]).  y (n_signals, n_samples) -> out (n_signals, 2, n_fft/2, n_frames),
 * n_frames = 1 + n_samples / hop, reflect padding n_fft/2, periodic Hann.  n_fft: power of two in [32, 4096]. */
typedef struct pg_stft_args {
    int32_t n_signals, n_samples, n_fft, hop, n_frames, polar;
    int32_t single_frame;   /* transform schedule: 0 (default) = 4 frames per workgroup, real FFT through an n_fft/2-point radix-4 */
    int32_t _pad0;          /*   transform (n_fft <= 2048; longer always take the other path); 1 = one frame per workgroup,       */
    const float* y; float* out; /* full-length radix-2.  Same framing; they differ in fp32 rounding only (tests, measurements).   */
    /* Chunked source (preproc_mdb.py:66-97 without a gathered copy).  chunk_start == NULL: signal s is row s of y
     * (n_signals, n_samples).  Otherwise signal s is the n_samples-long chunk of source row chunk_row[s] (NULL: row 0) of
     * y (rows, src_stride) that begins at sample chunk_start[s] (0 <= start); samples at or beyond src_len read as zero --
     * the reference's zero-padded tail (preproc_mdb.py:86-88).  Both arrays are device pointers of n_signals entries. */
    const int64_t* chunk_start; const int32_t* chunk_row; int64_t src_len; int64_t src_stride;
} pg_stft_args;
int pg_stft(const pg_stft_args* a, void* stream);
/* The launch plan of a pg_stft call WITHOUT launching it (measurement aid, as pg_conv_describe: the same checks as the call, buf of at
 * least 128 bytes, pointers non-NULL but not read): one entry per launch in launch order, joined by '|', each
 * "kernel<template args>,grid=X[xY],block=T,lds=B" with the kernel named as rocprofv3 reports it and B the dynamic LDS bytes. */
int pg_stft_describe(const pg_stft_args* a, char* buf, int32_t buflen);
/* The integer framing map alone (bit-exact contract): idx[t, k] = sample index of tap k of frame t. */
int pg_stft_frame_index(int32_t n_samples, int32_t n_fft, int32_t hop, int32_t n_frames, int32_t* idx, void* stream);

/* Training batches straight from raw audio: pg_stft of n_signals CROPS of one flat device buffer that holds every track (every
 * channel) back to back, fused with the data set's standardisation (preproc_mdb.py:182) and data.py:39-47.  An entry point of its
 * own with a struct of its own (pg_stft_args keeps its 80 bytes); PG_VERSION is unchanged.
 *   Framing: pg_stft's, applied to the crop: signal s is n_samples samples long, sample q of it is src[crop_begin[s] + q] for
 *   q < lim = clamp(crop_end[s] - crop_begin[s], 0, n_samples) and ZERO for q >= lim -- the reference's zero-padded tail
 *   (preproc_mdb.py:86-88), applied first; the reflect padding of n_fft/2 then happens inside the crop's n_samples.  Window, DC
 *   drop and [re; im] stacking are pg_stft's.
 *   Memory contract: for signal s no address outside [crop_begin[s], crop_begin[s] + lim) is ever read, so a crop that runs off the
 *   end of its track never sees the next track.  The CALLER guarantees 0 <= crop_begin[s] and crop_end[s] <= the number of floats
 *   in src for every s: the arrays live on the device and the host cannot check them.
 *   Arithmetic contract: the bits of pg_stft (same single_frame) on the gathered, zero-padded crops, then -- with stats --
 *   pg_standardize with the same stats: v = (v - (float)mean) / (float)std in fp32, an IEEE division, nothing contracted, on re AND
 *   im of every cell (the Nyquist bin's zero imaginary part becomes (0 - mean) / std), then -- with polar -- pg_polar (use_exp = 1).
 *   stats == NULL and polar == 0 give the bits of the chunked pg_stft.  A row's result does not depend on n_signals or on its
 *   position in the batch.  Kernel families and selection rules are pg_stft's (pg_stft_crops_describe names the launch).
 *   Errors (host side): NULL src / out / crop_begin / crop_end PG_ERR_NULL; n_fft PG_ERR_UNSUPPORTED; sizes, n_frames PG_ERR_SHAPE;
 *   stats not 8-byte or out not 4-byte aligned PG_ERR_ALIGN. */
typedef struct pg_stft_crops_args {
    int32_t n_signals, n_samples, n_fft, hop, n_frames, polar;  /* as pg_stft_args; n_samples = crop length                  */
    int32_t single_frame, _pad0;                                /* transform schedule, as pg_stft_args                        */
    const float* src;                 /* ONE flat device buffer holding every track (every channel) back to back             */
    const int64_t* crop_begin;        /* n_signals device entries: index in src of sample 0 of crop s                        */
    const int64_t* crop_end;          /* n_signals device entries: index one past the last sample crop s may read (the end   */
                                      /*   of ITS track).  lim = clamp(end - begin, 0, n_samples); samples q >= lim are 0    */
    const double* stats;              /* optional (NULL): device {mean, std}; v = (v - (float)mean) / (float)std on re AND im */
    float* out;                       /* (n_signals, 2, n_fft/2, n_frames), dense                                            */
} pg_stft_crops_args;                 /* 72 bytes */
int pg_stft_crops(const pg_stft_crops_args* a, void* stream);
int pg_stft_crops_describe(const pg_stft_crops_args* a, char* buf, int32_t buflen);   /* launch plan without launching, as pg_stft_describe */

/* data.py:39-47 on its own: in (N,2,...) [re; im] -> out (N,2,...) [log1p|z| ; angle]; inner = bins*frames. */
typedef struct pg_polar_args { int64_t n_items; int64_t inner; const float* in; float* out;
                               int32_t use_exp; /* data.py:39 use_exp: 1 -> log1p|z|, 0 -> |z| */ int32_t _pad0; } pg_polar_args;
int pg_polar(const pg_polar_args* a, void* stream);

/* demo.py:39 + utils.py:34-42: z = (exp(logmag) - 1) e^{j phase} (mode 0) or re + j im (mode 1); zero DC row prepended;
 * librosa.istft (irfft x Hann, overlap-add, / window-sum-square, trim n_fft/2); optional peak normalisation.
 * a, b: (n_signals, bins, n_frames) with the given batch strides; audio (n_signals, hop * (n_frames - 1)). */
typedef struct pg_istft_args {
    int32_t n_signals, bins, n_frames, hop, mode, normalize;
    int32_t single_frame; int32_t _pad0;   /* transform schedule, as in pg_stft_args */
    const float* a; int64_t a_bs; const float* b; int64_t b_bs;
    float* audio;
    void* workspace; int64_t workspace_bytes;
} pg_istft_args;
int64_t pg_workspace_bytes_istft(const pg_istft_args* a);   /* host function of n_signals, bins, n_frames, hop (pointers are not read); negative = error code */
int pg_istft(const pg_istft_args* a, void* stream);
int pg_istft_describe(const pg_istft_args* a, char* buf, int32_t buflen);   /* launch plan without launching, as pg_stft_describe */

/* Griffin-Lim building blocks (utils.py:112-134).  pg_gl_project: S (2,bins,frames) = [re; im] of the current estimate's
 * STFT and the target magnitudes mag (bins,frames) -> new_spec = mag * exp(j angle(S)) written as (2,bins,frames) to
 * spec_out (may be NULL) and, laid out as the operand of the inverse-DFT GEMM, to x (2*bins-2, frames): rows 0..bins-1
 * real parts, rows bins.. imaginary parts of bins 1..bins-2 (DC/Nyquist imaginary parts are ignored by an irfft).
 * pg_ola_nt: overlap-add of windowed frames given as (n_fft, frames) [n][t], any even n_fft (the reference inverts the
 * DC-dropped matrix, n_fft = 2*(bins-1) = 2046), / window-sum-square, trim n_fft/2, optional peak normalisation. */
typedef struct pg_gl_args { int32_t bins, frames; const float* S; const float* mag; float* x; float* spec_out;
                            int32_t n, _pad0; } pg_gl_args;       /* n clips (0 = 1): every tensor gains a leading clip axis */
int pg_gl_project(const pg_gl_args* a, void* stream);
typedef struct pg_ola_args { int32_t n_fft, frames, hop, normalize; const float* fr; float* audio; void* workspace; int64_t workspace_bytes;
                             int32_t n, _pad0; } pg_ola_args;     /* n clips (0 = 1, at most 64): fr (n, n_fft, frames), audio (n, len) */
int pg_ola_nt(const pg_ola_args* a, void* stream);   /* workspace: 256 bytes */

/* preproc_mdb.py:182: x = (x - x.mean()) / x.std() over the WHOLE array (population std).  pg_moments reduces in double and
 * writes stats[0] = mean, stats[1] = std (device doubles); pg_standardize applies them in place.  Two launches + one
 * elementwise pass: 4 B read for the moments, 8 B for the update, per element. */
typedef struct pg_moments_args { int64_t n; const float* x; double* stats; void* workspace; int64_t workspace_bytes; } pg_moments_args;
int64_t pg_workspace_bytes_moments(void);
int pg_moments(const pg_moments_args* a, void* stream);
int pg_standardize(float* x, int64_t n, const double* stats, void* stream);

/* Sample-rate conversion by up / down (target rate / original rate): the rate change of preproc_mdb.py:105-116 (librosa.load at
 * 44.1 kHz, librosa.resample to 16 kHz).  A band-limited sinc interpolator under a Kaiser window, resampy's published parameters:
 *   quality                Z (zero crossings)   beta                  roll-off r
 *   PG_RS_KAISER_BEST      64                   14.769656459379492    0.9475937167399596
 *   PG_RS_KAISER_FAST      16                   8.555504641634386     0.85
 *   h(t) = r sinc(r t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta) for |t| <= Z, else 0          (sinc(x) = sin(pi x) / (pi x))
 * up / down are reduced by their gcd to U / D; s = min(1, U/D), W = Z / s, H = floor(W), taps = floor(W) + ceil(W) + 1
 * (160 / 441, best: H = 176, taps = 354).  Output t has n0 = (t D) div U, p = (t D) mod U and
 *   y[t] = sum_{k < taps} bank[k U + p] x[n0 - H + k]        x[n] = 0 outside [0, n_in); k ascending, one fmaf per tap
 *   bank[k U + p] = float32(s h(s (p/U + H - k)))            tap-major, phase-minor; evaluated in double
 *   n_out = ceil(n_in U / D)
 * Parity with resampy is UNPINNED (as the STFT's with librosa): resampy interpolates linearly in a 512-per-crossing table and
 * truncates its index step; this is the filter that table samples.  Two known deviations: the last sample t = n_out - 1 is
 * computed (old librosa zero-pads it when resampy returns floor), and equal rates are filtered like any other ratio (callers
 * that want librosa's pass-through skip the call).
 * The filter bank is built by the caller ON THE HOST (pg_resample_bank writes pg_resample_bank_elems() floats to a host buffer)
 * and handed to pg_resample as a DEVICE copy: the library allocates nothing and keeps nothing.  Limits after reduction: U <= 1024
 * and taps <= 2048, else PG_ERR_UNSUPPORTED (of the pairs of 8 / 11.025 / 16 / 22.05 / 32 / 44.1 / 48 kHz only 11.025 -> 32 kHz,
 * 1280 phases, is outside; go through 22.05 kHz).  The argument of h is formed as (p + U (H - k)) /
 * max(U, D), one division of exact integers, so |t| <= Z is decided exactly at the edge of the support.  A row's
 * result does not depend on n_signals or its position in the batch (bit for bit); nothing outside [0, n_in) of a row is used. */
enum { PG_RS_KAISER_BEST = 0, PG_RS_KAISER_FAST = 1 };
int64_t pg_resample_out_len(int64_t n_in, int32_t up, int32_t down);            /* host; <0 = error code            */
int32_t pg_resample_taps(int32_t up, int32_t down, int32_t quality);             /* host; <0 = error code            */
int64_t pg_resample_bank_elems(int32_t up, int32_t down, int32_t quality);       /* host: taps * U; <0 = error code  */
int pg_resample_bank(float* bank_host, int32_t up, int32_t down, int32_t quality);   /* HOST buffer, double arithmetic */
typedef struct pg_resample_args {
    int32_t n_signals, up, down, quality;
    int64_t n_in, n_out;                 /* n_out == pg_resample_out_len(...) else PG_ERR_SHAPE */
    const float* x; int64_t x_stride;    /* (n_signals, n_in), rows x_stride >= n_in apart      */
    float* y;       int64_t y_stride;    /* (n_signals, n_out), rows y_stride >= n_out apart    */
    const float* bank;                   /* DEVICE copy of pg_resample_bank's output            */
} pg_resample_args;
int pg_resample(const pg_resample_args* a, void* stream);

/* Whole tracks from overlapped clips: crossfaded overlap-add of n_clips equal-length clips per track, plus the finite check and the
 * peak normalisation of utils.py:41-42 taken over the WHOLE result (all tracks jointly: librosa.util.normalize(axis=None)).  The
 * reference has no counterpart (its demo.py stops at clips of `frames` columns); the arithmetic below is the contract.
 *   T = clip_len; clip k begins at output sample k step; V = T - step samples are shared with the next clip (0 <= 2 V <= T: at most
 *   two clips cover a sample); (n_clips-1) step < n_out <= (n_clips-1) step + T (the last clip may be cut short).
 *   ramp[j] = float32(sin^2(pi (j + 0.5) / (2 V))), 0 <= j < V, evaluated in double on the HOST (pg_stitch_ramp): every entry is
 *   strictly positive and ramp[j] + ramp[V-1-j] is within 2^-23 of 1.  pg_stitch takes a DEVICE copy, as pg_resample its bank: the
 *   library allocates nothing and keeps nothing.
 *   Output sample t of a track: k = min(t div step, n_clips-1), j = t - k step.  If k >= 1 and j < V, with a = ramp[V-1-j],
 *   b = ramp[j], lo = clip[k-1][j + step], hi = clip[k][j]:   raw = (fl(a lo) + fl(b hi)) / fl(a + b)   -- all fp32, nothing
 *   contracted, the lower clip's term first.  Otherwise raw = clip[k][j], copied bit for bit (the head of clip 0 and the tail of the
 *   last clip are never faded).  Hence step == T concatenates the clips and all-ones clips give all ones, bit for bit.
 *   *n_nonfinite = number of output samples of all tracks that are NaN or +-inf; *peak = max |raw| over the finite samples of all
 *   tracks; with normalize = 1 and peak > FLT_MIN, out = raw / peak, else out = raw.  The reduction is two-stage through `workspace`
 *   (per-workgroup partials, then a second launch; no float atomics) and exact in any order: the result does not depend on the grid.
 *   The workspace (pg_workspace_bytes_stitch() bytes, else PG_ERR_WORKSPACE) is needed only when normalize, peak or n_nonfinite is set.
 * Samples move 16 bytes per lane when step, T, the three strides and the pointers allow it and one by one otherwise; both paths give
 * the same bits.  Index arithmetic is 64-bit.  pg_stitch_ramp: overlap == 0 writes nothing (PG_OK), overlap < 0 is PG_ERR_SHAPE. */
int     pg_stitch_ramp(float* ramp_host, int32_t overlap);   /* HOST buffer of `overlap` floats, double arithmetic */
typedef struct pg_stitch_args {
    int32_t n_tracks, n_clips, clip_len, step;   /* T = clip_len; V = T - step is the overlap; 0 <= 2 V <= T, step >= 1 */
    int64_t n_out;                               /* (n_clips-1)*step < n_out <= (n_clips-1)*step + T                      */
    const float* clips; int64_t clip_stride, track_stride;   /* clip k of track r: clips + r*track_stride + k*clip_stride, T contiguous samples */
    float* out; int64_t out_stride;              /* (n_tracks, n_out), rows out_stride >= n_out apart                    */
    const float* ramp;                           /* DEVICE copy of pg_stitch_ramp(V); may be NULL iff V == 0             */
    int32_t normalize, _pad0;
    float* peak; int32_t* n_nonfinite;           /* optional device outputs, one value each                              */
    void* workspace; int64_t workspace_bytes;
} pg_stitch_args;                                /* 112 bytes */
int64_t pg_workspace_bytes_stitch(const pg_stitch_args* a);  /* host; negative = error code */
int     pg_stitch(const pg_stitch_args* a, void* stream);

/* The spectral-domain track join (phasegen/track.py, join="spectral"): instead of inverting every clip and crossfading waveforms
 * (pg_stitch), the clips' PHASES are joined on the track's global frame grid and the track is inverted by ONE pg_istft with the exact
 * magnitudes.  Two streaming entry points with structs of their own; PG_VERSION is unchanged.  The reference has no counterpart; the
 * arithmetic below is the contract.  Common geometry: clip k covers the global frames k sf .. k sf + frames - 1 (sf = frame stride
 * between clips).  Both kernels move 4 frames of a row per thread, as 16-byte accesses where sf, frames, the row lengths, the strides
 * and the pointers allow (pg_spec_clips: and src_per_out == 1.0) and frame by frame otherwise; both paths give the same bits.  Index
 * arithmetic is 64-bit.  The library allocates nothing and keeps nothing.
 *
 * pg_spec_clips: clip windows of a plane P (n_ch, bins, F_src) fp32, frames fastest, channels p_stride >= bins F_src elements apart
 *   (the log-magnitude or the angle plane of a (n_ch, 2, bins, F) polar tensor by pointer and stride), optionally resampled along
 *   time -> out (n_clips, n_ch, bins, frames), dense: the model's input order (clip, channel).
 *   Output frame f of clip k is global output frame g = k sf + f; its source position is p = (double)g * src_per_out (src_per_out =
 *   1 / stretch); i0 = min((int64)floor(p), F_src - 1), i1 = min(i0 + 1, F_src - 1), w = (float)(p - floor(p)).  With a = P[c, b, i0]
 *   and b1 = P[c, b, i1]: out = a bit for bit when w == 0, otherwise out = fl(a + fl(w fl(b1 - a))) in fp32, nothing contracted.
 *   Hence src_per_out == 1.0 is a pure copy (frames past the source's end repeat its last frame), and n_clips = 1, frames = F_out
 *   resamples a whole plane.  A (clip, channel) result does not depend on n_clips, n_ch or its position, bit for bit.
 *   Errors (host side, before any launch): NULL args / P / out PG_ERR_NULL; non-positive sizes, sf < 1, src_per_out not finite or
 *   <= 0, p_stride < bins F_src PG_ERR_SHAPE; P or out not 4-byte aligned PG_ERR_ALIGN.
 *
 * pg_phase_join: phi (n_clips, n_ch, bins, frames) with clip stride, channel stride and row pitch in elements (the first `bins` rows
 *   of a model output (n, 2 bins, frames) are read in place) -> out (n_ch, bins, F_out) dense, F_out = (n_clips - 1) sf + frames.
 *   Vf = frames - sf frames are shared by neighbouring clips, 1 <= Vf and 2 Vf <= frames (at most two clips cover a frame); ramp is
 *   a DEVICE copy of pg_stitch_ramp(Vf) (any Vf positive floats will do).
 *   Global frame g: k = min(g div sf, n_clips - 1), j = g - k sf.  If k >= 1 and j < Vf the frame is shared: with a = ramp[Vf-1-j],
 *   b = ramp[j], lo = phi[k-1][j + sf], hi = phi[k][j]:   zr = fl(fl(a cos lo) + fl(b cos hi)), zi = fl(fl(a sin lo) + fl(b sin hi)),
 *   out = atan2(zi, zr) -- the weighted circular mean, in (-pi, pi]; if zr == 0 and zi == 0, or either is not finite, out =
 *   (b >= a ? hi : lo).  Every other frame is phi[k][j] copied bit for bit (NOT wrapped: pg_istft mode 0 takes any angle).  sin, cos
 *   and atan2 are the library's own (csrc/pg_fastmath.h: those pg_istft mode 0 and pg_polar use; absolute errors 2.5e-7 + 6e-8 |phi|
 *   and 3e-7).  The result does not depend on n_ch or on the channel's position, bit for bit.
 *   Errors (host side, before any launch): NULL args / phi / out / ramp PG_ERR_NULL; non-positive sizes, sf < 1, Vf < 1, 2 Vf >
 *   frames, row_pitch < frames, a channel or clip stride (where applied) shorter than its rows PG_ERR_SHAPE; phi, out or ramp not
 *   4-byte aligned PG_ERR_ALIGN. */
typedef struct pg_spec_clips_args {
    int32_t n_clips, n_ch, bins, frames;         /* output (n_clips, n_ch, bins, frames)                                */
    int32_t sf, _pad0;                           /* clip k begins at global output frame k sf; sf >= 1                  */
    int64_t F_src;                               /* frames per row of P                                                 */
    double  src_per_out;                         /* source frames per output frame = 1 / stretch; finite, > 0          */
    const float* P; int64_t p_stride;            /* (n_ch, bins, F_src), channels p_stride >= bins F_src elements apart */
    float* out;
} pg_spec_clips_args;                            /* 64 bytes */
int pg_spec_clips(const pg_spec_clips_args* a, void* stream);
typedef struct pg_phase_join_args {
    int32_t n_clips, n_ch, bins, frames;
    int32_t sf, _pad0;                           /* Vf = frames - sf; 1 <= Vf, 2 Vf <= frames                           */
    const float* phi; int64_t clip_stride, ch_stride, row_pitch;   /* phi[k][c][b][f] = phi[k clip_stride + c ch_stride + b row_pitch + f] */
    float* out;                                  /* (n_ch, bins, (n_clips-1) sf + frames), dense                        */
    const float* ramp;                           /* DEVICE copy of pg_stitch_ramp(Vf)                                   */
} pg_phase_join_args;                            /* 72 bytes */
int pg_phase_join(const pg_phase_join_args* a, void* stream);

/* pg_phase_vocoder: the phase-vocoder phase of a time-stretched spectrogram (phasegen/track.py, phase="vocoder"): each bin's analysis
 * phase is propagated along the OUTPUT frame grid by the frame-to-frame advance measured on the source grid (the recurrence of
 * librosa.phase_vocoder), and a bin below a magnitude floor takes its analysis phase back.  One streaming kernel with a struct of its
 * own; PG_VERSION is unchanged.  The reference has no counterpart; the arithmetic below is the contract.
 *   A: the angle plane (n_ch, bins, F_src) fp32, frames fastest, channels a_stride >= bins F_src elements apart (pol[:, 1] of a
 *   (n_ch, 2, bins, F) polar tensor by pointer and stride).  M: optional (may be NULL), the log-magnitude plane of the same shape with
 *   its own channel stride m_stride (pol[:, 0]).  src_per_out = 1 / stretch, a double, finite and > 0.  reset_below: a float, finite
 *   and >= 0, in the units of M.  F_out >= 1.  -> out (n_ch, bins, F_out), dense fp32.
 *   Phase matters modulo 2 pi only and is kept as a 32-bit unsigned fraction of a turn; integer addition wraps and is associative, so
 *   the scan along time is exact in any order.  Constants (each one double division): TWO_PI = 6.283185307179586,
 *   K = 4294967296.0 / TWO_PI, R = TWO_PI / 4294967296.0.
 *   Quantisation: q(x) = 0 if x is not finite or |x| > 2^20, otherwise q(x) = (uint32)(int64) rint((double)x * K): one double
 *   multiply, round half to even, two's-complement wrap.
 *   Positions (pg_spec_clips's), for output frame g: p = (double)g * src_per_out, i0 = min((int64)floor(p), F_src - 1),
 *   i1 = min(i0 + 1, F_src - 1).
 *   Scan, per (channel, bin) row:
 *     delta[g] = q(A[i1(g)]) - q(A[i0(g)])   in uint32: the wrap is the principal value of the analysis phase advance.  The expected
 *                advance 2 pi hop k / n_fft of librosa.phase_vocoder cancels modulo 2 pi, so no bin frequency, hop or n_fft enters.
 *     reset[g] = (g == 0) || (M != NULL && M[i0(g)] < reset_below)          (a NaN in M does not reset)
 *     acc[g]   = reset[g] ? q(A[i0(g)]) : acc[g-1] + delta[g-1]             in uint32
 *     out[g]   = (float)((double)(int32)acc[g] * R)
 *   so every value lies in [-pi, pi) before the one rounding to fp32 (which may deliver the fp32 next to -pi or pi).
 *   Consequences.  With src_per_out == 1.0 the sum telescopes: acc[g] = q(A[g]) exactly for g < F_src, so a stretch of 1 returns the
 *   analysis phase (modulo 2 pi) to within one quantisation step (2 pi / 2^33) plus one fp32 rounding.  A bin whose magnitude is below
 *   the floor carries its analysis phase and resumes accumulating from that phase the moment it rises above the floor: the transient
 *   and silence phase reset that restores coherence between neighbouring bins at onsets; reset_below == 0 or M == NULL never resets
 *   after frame 0.  At the end of the source i1 == i0 and the advance is zero.  A row's result does not depend on n_ch, bins or the
 *   row's position, bit for bit, nor on how the kernel splits the scan.
 *   Kernel: one 256-thread workgroup per row, chunks of 1024 output frames, 4 per thread; a segmented scan in registers, across the
 *   wave and across the waves through LDS; 16-byte stores where out and F_out allow, frame by frame otherwise (same bits); 64-bit
 *   index arithmetic.  The library allocates nothing and keeps nothing.
 *   Errors (host side, before any launch): NULL args / A / out PG_ERR_NULL; non-positive sizes, src_per_out not finite or <= 0,
 *   reset_below not finite or < 0, a_stride (or, with M, m_stride) < bins F_src PG_ERR_SHAPE; A, M or out not 4-byte aligned
 *   PG_ERR_ALIGN. */
typedef struct pg_phase_vocoder_args {
    int32_t n_ch, bins;
    int64_t F_src, F_out;                        /* frames per row of A (and M), frames per row of out                  */
    double  src_per_out;                         /* source frames per output frame = 1 / stretch; finite, > 0          */
    float   reset_below; int32_t _pad0;          /* a frame whose M is below this takes its analysis phase; finite, >= 0 */
    const float* A; int64_t a_stride;            /* (n_ch, bins, F_src), channels a_stride >= bins F_src elements apart */
    const float* M; int64_t m_stride;            /* optional (NULL: no reset after frame 0), same shape, own stride    */
    float* out;                                  /* (n_ch, bins, F_out), dense                                          */
} pg_phase_vocoder_args;                         /* 80 bytes */
int pg_phase_vocoder(const pg_phase_vocoder_args* a, void* stream);

/* pg_phase_lock: the phase-vocoder phase with IDENTITY PHASE LOCKING (Laroche & Dolson 1999; phasegen/track.py,
 * phase="vocoder_locked").  A plain vocoder moves every bin on its own and the bins of one sinusoid's main lobe drift apart; here only
 * the spectral peaks of a frame advance, and every other bin takes its peak's rotation, so the analysis' phase relations inside a
 * lobe survive.  Struct of its own, PG_VERSION unchanged; the reference has no counterpart; the arithmetic below is the contract.
 *   A, M, src_per_out, reset_below, F_src, F_out, out, q(), K, R, i0(g), i1(g): those of pg_phase_vocoder, but M is REQUIRED.
 *   Per channel, with m_g[b] = M[b][i0(g)] and a_g[b] = q(A[b][i0(g)]):
 *   Peaks of frame g.  Bin b is a peak iff m_g[b] is not NaN and, for d = 1 .. PG_LOCK_REACH (= 2):
 *     (b - d < 0 or m_g[b] > m_g[b-d]) and (b + d >= bins or m_g[b] >= m_g[b+d])         plain IEEE fp32 comparisons
 *   so the first bin of a plateau is the peak and a NaN neighbour within reach disqualifies a bin.
 *   Region.  P_g(b) = the peak nearest to b in |b - p|, a tie going to the lower peak; in a frame without any peak P_g(b) = b.
 *   Rotation T (uint32, wrapping).  T_0[b] = 0.  For g >= 1, with p = P_g(b):
 *     e_g[p]  = q(A[p][i1(g-1)]) - q(A[p][i0(g)])                    (zero whenever i1(g-1) == i0(g))
 *     reset   = m_g[p] < reset_below                                 (a NaN does not reset)
 *     T_g[b]  = reset ? 0 : T_{g-1}[p] + e_g[p]
 *     out[b][g] = (float)((double)(int32)(T_g[b] + a_g[b]) * R)      (also for g = 0)
 *   T is constant over a peak's region: that is identity locking.
 *   Consequences.  Where every bin is its own region -- bins == 1, or an M that is NaN everywhere -- the result equals
 *   pg_phase_vocoder's with that same M, bit for bit.  src_per_out == 1.0 returns q(A) exactly for g < F_src.  A channel's result
 *   does not depend on n_ch or on the channel's position, nor on how the scan is split: frame g is the gather map T_g[b] =
 *   T_{g-1}[P_g(b)] + c_g[b], c_g[b] = e_g[P_g(b)], a reset being the source index `bins` with T[bins] == 0; maps compose as
 *   (P2, c2) o (P1, c1) = (P1[P2], c1[P2] + c2), associatively and in integers.
 *   Kernels: time in chunks of 32 output frames; compose (one workgroup per channel and chunk folds the chunk's maps in LDS), carry
 *   (one workgroup per channel walks the chunk maps), apply (one workgroup per channel and chunk replays its frames; the peak maps
 *   are recomputed, not stored); both stage a window of source frames of all rows through LDS, read along the frames (at 4096
 *   bins, where no window fits beside the maps, every thread walks its own rows).  16-byte stores where out and F_out allow, frame by frame otherwise (same bits); 64-bit index
 *   arithmetic; no atomics.  workspace: pg_workspace_bytes_phase_lock() bytes = 12 n_ch bins ceil(F_out / 32), a function of n_ch,
 *   bins and F_out alone.  The library allocates nothing and keeps nothing.
 *   Errors (host side, before any launch): those of pg_phase_vocoder, and M NULL PG_ERR_NULL; bins > 4096 PG_ERR_SHAPE; workspace
 *   NULL or smaller than the query's answer PG_ERR_WORKSPACE. */
#define PG_LOCK_REACH 2
typedef struct pg_phase_lock_args {
    int32_t n_ch, bins;                          /* bins <= 4096                                                        */
    int64_t F_src, F_out;                        /* frames per row of A and M, frames per row of out                    */
    double  src_per_out;                         /* source frames per output frame = 1 / stretch; finite, > 0          */
    float   reset_below; int32_t _pad0;          /* a peak whose M is below this resets its region; finite, >= 0        */
    const float* A; int64_t a_stride;            /* (n_ch, bins, F_src), channels a_stride >= bins F_src elements apart */
    const float* M; int64_t m_stride;            /* required, same shape, own stride                                    */
    float* out;                                  /* (n_ch, bins, F_out), dense                                          */
    void* workspace; int64_t workspace_bytes;
} pg_phase_lock_args;                            /* 96 bytes */
int64_t pg_workspace_bytes_phase_lock(const pg_phase_lock_args* a);   /* host function of n_ch, bins, F_out; negative = error code */
int     pg_phase_lock(const pg_phase_lock_args* a, void* stream);

/* pg_phase_lock_linked: pg_phase_lock with the channels LINKED (phasegen/track.py, phase="vocoder_locked", link_channels=True).
 * pg_phase_lock gives every channel its own peaks and its own rotation T, so the phases of one source in two channels drift apart by
 * an arbitrary angle and the stereo image (and the mono sum) is lost; here all channels take ONE rotation, that of a reference plane
 * pair (the channel mean, in the track layer).  Struct of its own, PG_VERSION unchanged; the reference has no counterpart; the
 * arithmetic below is the contract.
 *   A: the channels' angle planes (n_ch, bins, F_src), as pg_phase_lock's A.  Aref, Mref: the angle and the log-magnitude plane of
 *   the reference, (bins, F_src) each, dense, both REQUIRED.  src_per_out, reset_below, F_src, F_out, q(), R, i0(g): pg_phase_lock's.
 *   Rotation.  T_g[b] is, word for word, the rotation pg_phase_lock forms for the single channel (Aref, Mref): its peaks, its
 *   regions P_g(b), its advance e_g[p] = q(Aref[p][i1(g-1)]) - q(Aref[p][i0(g)]), its reset below reset_below, and T_0 = 0.
 *   Output.  For every channel c: out[c][b][g] = (float)((double)(int32)(T_g[b] + q(A[c][b][i0(g)])) * R).
 *   Consequences.  n_ch == 1 with A == Aref gives the bits of pg_phase_lock(Aref, Mref); more generally any channel whose plane
 *   equals Aref gets those bits.  src_per_out == 1.0 returns q(A[c]) for every channel (T is zero).  Before the final rounding
 *   (T + a_c) - (T + a_d) == a_c - a_d holds in uint32: the inter-channel phase difference of the analysis survives in every cell.
 *   A channel's result does not depend on n_ch or on the channel's position.
 *   Kernels: pg_phase_lock's compose and carry run ONCE, on the reference, as for one channel; apply runs per (channel, chunk),
 *   rebuilds the chunk's maps from (Mref, q(Aref)) and adds q(A[c]); its staged window holds three planes (8 source frames at 1024
 *   bins, 2 at 2048, none at 4096).  All channels of a chunk read the same T slot, which nothing writes after carry.  16-byte stores
 *   where out and F_out allow, frame by frame otherwise (same bits); 64-bit index arithmetic; no atomics.
 *   workspace: pg_workspace_bytes_phase_lock_linked() bytes = 12 bins ceil(F_out / 32): one channel's worth, a function of bins and
 *   F_out alone.  The library allocates nothing and keeps nothing.
 *   Errors (host side, before any launch, in this order): NULL args / A / Aref / Mref / out PG_ERR_NULL; non-positive sizes, bins >
 *   4096, src_per_out not finite or <= 0, reset_below not finite or < 0, a plane or output beyond 2^62 elements, a_stride < bins F_src,
 *   more than 2^31 - 1 (channel, chunk) pairs PG_ERR_SHAPE; A, Aref, Mref, out or workspace not 4-byte aligned PG_ERR_ALIGN;
 *   workspace NULL or smaller than the query's answer PG_ERR_WORKSPACE. */
typedef struct pg_phase_lock_linked_args {
    int32_t n_ch, bins;                          /* bins <= 4096                                                        */
    int64_t F_src, F_out;                        /* frames per row of A, Aref and Mref, frames per row of out           */
    double  src_per_out;                         /* source frames per output frame = 1 / stretch; finite, > 0          */
    float   reset_below; int32_t _pad0;          /* a peak whose Mref is below this resets its region; finite, >= 0     */
    const float* A; int64_t a_stride;            /* (n_ch, bins, F_src): the channels' angle planes, a_stride >= bins F_src apart */
    const float* Aref;                           /* (bins, F_src): angle plane of the reference                         */
    const float* Mref;                           /* (bins, F_src): log-magnitude plane of the reference, required       */
    float* out;                                  /* (n_ch, bins, F_out), dense                                          */
    void* workspace; int64_t workspace_bytes;
} pg_phase_lock_linked_args;                     /* 96 bytes */
int64_t pg_workspace_bytes_phase_lock_linked(const pg_phase_lock_linked_args* a);   /* host function of bins, F_out; negative = error code */
int     pg_phase_lock_linked(const pg_phase_lock_linked_args* a, void* stream);

/* pg_phase_spsi: a phase from the magnitudes ALONE, in one pass (single-pass spectrogram inversion; Beauregard, Harish & Wyse 2015;
 * phasegen/track.py, phase="spsi"): the peaks of every frame advance by their interpolated frequency and every other bin follows its
 * peak.  No analysis phase, no weights, no iteration: the comparator a predicted phase has to beat, and the only one that uses
 * nothing a stretched spectrogram does not have.  Struct of its own, PG_VERSION unchanged; the reference has no counterpart; the
 * arithmetic below is the contract.
 *   M: the log-magnitude plane (n_ch, bins, F) fp32 ON THE OUTPUT GRID (no time mapping here), frames fastest, channels m_stride >=
 *   bins F elements apart (pol[:, 0] of a polar tensor by pointer and stride).  n_fft, hop: 1 <= hop <= n_fft.  bin0: the FFT bin of
 *   row 0 (1 for the project's DC-dropped planes), 0 <= bin0 <= 65536.  -> out (n_ch, bins, F), dense fp32.
 *   Per channel, with m_g[b] = M[b][g]:
 *   Peaks and regions.  The peaks of frame g and P_g(b) are pg_phase_lock's, word for word: PG_LOCK_REACH, the plateau rule, NaN,
 *   and P_g(b) = b in a frame without any peak.
 *   Offset of p = P_g(b), in fp32, nothing contracted, one IEEE division: alpha = m_g[p-1], beta = m_g[p], gamma = m_g[p+1],
 *     d = fl(fl(alpha - beta) + fl(gamma - beta)),  n = 0.5f * fl(alpha - gamma),
 *     delta = n / d if 0 < p < bins - 1 and d < 0, otherwise 0; and if not (|delta| <= 0.5), which covers NaN, delta = 0.
 *   Advance, in double: x = ((double)(p + bin0) + (double)delta) * ((double)hop / (double)n_fft),
 *     adv_g[p] = (uint32)(int64) rint(x * 4294967296.0)             round half to even, two's-complement wrap
 *   Scan (uint32, wrapping).  Theta_0[b] = 0.  For g >= 1: Theta_g[b] = Theta_{g-1}[P_g(b)] + adv_g[P_g(b)].
 *   Output.  out[b][g] = (float)((double)(int32)(Theta_g[b] + (((b + bin0) & 1) << 31)) * R), R as in pg_phase_vocoder.  The half turn
 *   on odd FFT bins is the (-1)^k of a Hann window that starts at the frame's first sample (the project's and librosa's centred
 *   framing).  Theta carries no parity, so a peak that moves to the next bin continues without a jump.
 *   Consequences.  A plane whose columns are all equal gives Theta_g[b] = g adv[P(b)] exactly.  A channel's result does not depend
 *   on n_ch, on its position, or on how the scan is split (frame g is a gather map, as in pg_phase_lock).  There is no reset_below.
 *   Kernels: pg_phase_lock's three launches (compose, carry, apply; chunks of 32 frames) over another frame source: the staged
 *   window holds the one plane, twice as wide in the same LDS, and is reloaded every window's width of frames; the advance is
 *   formed from the frame's magnitudes in LDS.  16-byte stores where out and F allow, frame by frame otherwise (same bits).
 *   workspace: pg_workspace_bytes_phase_spsi() bytes = 12 n_ch bins ceil(F / 32), as pg_phase_lock's.  The library allocates
 *   nothing and keeps nothing.
 *   Errors (host side, before any launch, in this order): NULL args / M / out PG_ERR_NULL; non-positive sizes, bins > 4096, hop or
 *   n_fft outside 1 <= hop <= n_fft, bin0 outside [0, 65536], a plane or output beyond 2^62 elements, m_stride < bins F
 *   PG_ERR_SHAPE; M, out or workspace not 4-byte aligned PG_ERR_ALIGN; workspace NULL or smaller than the query's answer
 *   PG_ERR_WORKSPACE. */
typedef struct pg_phase_spsi_args {
    int32_t n_ch, bins;                          /* bins <= 4096                                                        */
    int64_t F;                                   /* frames per row of M and of out                                      */
    int32_t n_fft, hop;                          /* 1 <= hop <= n_fft                                                   */
    int32_t bin0, _pad0;                         /* FFT bin of row 0; 0 <= bin0 <= 65536                                */
    const float* M; int64_t m_stride;            /* (n_ch, bins, F), channels m_stride >= bins F elements apart         */
    float* out;                                  /* (n_ch, bins, F), dense                                              */
    void* workspace; int64_t workspace_bytes;
} pg_phase_spsi_args;                            /* 72 bytes */
int64_t pg_workspace_bytes_phase_spsi(const pg_phase_spsi_args* a);   /* host function of n_ch, bins, F; negative = error code */
int     pg_phase_spsi(const pg_phase_spsi_args* a, void* stream);

/* pg_hpss: harmonic / percussive split of a log-magnitude plane by median filtering (Fitzgerald 2010, binary masks), the first half
 * of the transient-preserving stretch (Driedger, Mueller & Ewert 2014; phasegen/track.py, transients="ola"): the harmonic plane goes
 * through the chosen phase source, the percussive plane through pg_ola_stretch.  Struct of its own, PG_VERSION unchanged; the
 * reference has no counterpart; the arithmetic below is the contract.
 *   M: (n_ch, bins, F) fp32, frames fastest, rows F apart, channels m_stride >= bins F elements apart (pol[:, 0] of a polar tensor by
 *   pointer and stride).  win_t, win_f: the window along time and along frequency, odd, 1 <= win <= PG_HPSS_MAX_WIN (= 31).
 *   -> harm, perc (n_ch, bins, F) each, dense fp32.
 *   Order.  key(x) = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000) as a uint32: the IEEE total order on the bit pattern.  -0
 *   sorts below +0, a positive NaN above +inf, a negative NaN below -inf; equal keys are equal bits, so "the element of rank r" of
 *   a window has well-defined bits.
 *   Medians, per channel, with ht = (win_t - 1) / 2 and hf = (win_f - 1) / 2:
 *     H[b][g] = the element of rank ht by key among M[b][clamp(g + d, 0, F - 1)], d = -ht .. ht,
 *     P[b][g] = the element of rank hf by key among M[clamp(b + d, 0, bins - 1)][g], d = -hf .. hf
 *   (edge replication keeps every window odd).
 *   Split.  A cell is harmonic iff key(H[b][g]) >= key(P[b][g]).  A harmonic cell gives harm = M[b][g] (its bits) and perc = +0.0f;
 *   any other cell gives perc = M[b][g] and harm = +0.0f.  The planes are the project's log1p magnitudes, so a zero is silence, and
 *   a median commutes with any increasing map, so the decision is the one a linear-magnitude HPSS with binary masks makes.
 *   Consequences.  Every cell lands in exactly one plane, bit for bit.  win_t == win_f == 1 makes everything harmonic.  A plane
 *   constant along time with win_f == 1 is all harmonic, and so is a plane constant along frequency with win_t == 1 (the tie goes
 *   to harm).  A channel's result does not depend on n_ch, on its position, or on how the kernel tiles the plane.  Non-finite
 *   values are ordered data (the Order above): nothing else happens to them.
 *   Kernel: one workgroup per (channel, 32 bins, 64 frames) tile, walked grid-stride; the tile and its halos of hf rows and ht frames
 *   are staged through LDS once, as keys, with global reads along the frames; both medians are selection networks over LDS reads.
 *   16-byte stores where harm, perc and F allow, element by element otherwise (same bits); 64-bit index arithmetic; no atomics.
 *   There is no workspace: the library allocates nothing and keeps nothing.
 *   Errors (host side, before any launch, in this order): NULL args / M / harm / perc PG_ERR_NULL; non-positive sizes, an even or
 *   out-of-range window, a plane or output beyond 2^62 elements, m_stride < bins F PG_ERR_SHAPE; M, harm or perc not 4-byte aligned
 *   PG_ERR_ALIGN. */
#define PG_HPSS_MAX_WIN 31
typedef struct pg_hpss_args {
    int32_t n_ch, bins;
    int64_t F;                                   /* frames per row                                                      */
    int32_t win_t, win_f;                        /* odd, 1 <= win <= PG_HPSS_MAX_WIN                                    */
    const float* M; int64_t m_stride;            /* (n_ch, bins, F), channels m_stride >= bins F elements apart         */
    float* harm;                                 /* (n_ch, bins, F), dense                                              */
    float* perc;                                 /* (n_ch, bins, F), dense                                              */
} pg_hpss_args;                                  /* 56 bytes */
int     pg_hpss(const pg_hpss_args* a, void* stream);

/* pg_ola_stretch: time-domain overlap-add at a time ratio, the second half of the transient-preserving stretch: the frames of a
 * short window are RELOCATED, not stretched, so a click stays a click.  Struct of its own, PG_VERSION unchanged; the reference has no
 * counterpart; the arithmetic below is the contract.
 *   x: (n_sig, n_in) fp32, rows x_stride >= n_in apart.  win: a DEVICE table of w = win_len floats, each finite and >= 0
 *   (pg_ola_window fills a host copy of the default; the table is not read on the host: a negative or non-finite entry is the
 *   caller's error and the formula says what happens).  base: optional (NULL), (n_sig, n_out), rows base_stride >= n_out apart,
 *   added to the result.  -> y (n_sig, n_out), rows y_stride >= n_out apart.
 *   Frames.  Output frame g >= 0 covers the output samples g hop - w/2 .. g hop + w/2 - 1; its centre in the input is
 *     c_g = (int64) rint((double)(g hop) * src_per_out)             round half to even; a centre beyond 2^62 is outside every signal.
 *   There is no upper limit on g, so y[t] does not depend on n_out.
 *   Output sample t.  Over the covering frames in ascending g, with j = t - g hop + w/2 and s = c_g + j - w/2, in fp32, nothing
 *   contracted:
 *     den = fl(den + win[j])                       for every covering frame,
 *     num = fl(num + fl(win[j] * x[s]))            only where 0 <= s < n_in: a sample outside the signal is "no term";
 *     r = den > 0 ? num / den : 0                  one IEEE division;       y[t] = base ? fl(base[t] + r) : r.
 *   Consequences.  At most w / hop + 1 frames cover a sample.  With src_per_out == 1 every term reads x[t], so
 *   |r - x[t]| <= (2 k + 2) 2^-24 |x[t]| for k covering frames (k products and k - 1 additions above, k - 1 additions below, the
 *   division; all weights non-negative): at most 12 2^-24 at the default 256 / 64 (k = 4 where hop divides w).  A row's result does not depend on n_sig or on its
 *   position.  A non-finite x[s] reaches exactly the outputs whose covering frames read it: R1 and R2 of the Non-finite section
 *   hold, with "no term" outside the ends.
 *   Kernel: 4 output samples per thread, 16-byte stores where y and y_stride allow and sample by sample otherwise (same bits); the
 *   window table is kept in LDS; neighbouring threads of one frame read neighbouring s.  64-bit index arithmetic; no atomics; no
 *   workspace: the library allocates nothing and keeps nothing.
 *   Errors (host side, before any launch, in this order): NULL args / x / win / y PG_ERR_NULL; non-positive sizes, win_len odd or
 *   outside 2 .. 4096, hop outside 1 .. win_len / 2, src_per_out not finite or <= 0, signals beyond 2^62 elements, x_stride < n_in,
 *   y_stride < n_out, (with base) base_stride < n_out PG_ERR_SHAPE; x, win, base or y not 4-byte aligned PG_ERR_ALIGN.
 * pg_ola_window (HOST): win_host[j] = (float)(0.5 - 0.5 cos(2 pi j / win_len)), j < win_len, the periodic Hann window, formed in
 *   double and rounded once; NULL PG_ERR_NULL, win_len odd or outside 2 .. 4096 PG_ERR_SHAPE.  At hop = win_len / 4 its shifted
 *   copies sum to 2 wherever every covering frame exists. */
typedef struct pg_ola_stretch_args {
    int32_t n_sig, win_len, hop, _pad0;          /* win_len even, 2 <= win_len <= 4096; 1 <= hop <= win_len / 2         */
    int64_t n_in, n_out;
    double  src_per_out;                         /* input samples per output sample = 1 / stretch; finite, > 0         */
    const float* x;    int64_t x_stride;         /* (n_sig, n_in)                                                       */
    const float* win;                            /* DEVICE table of win_len floats, each finite and >= 0                */
    const float* base; int64_t base_stride;      /* optional (NULL): (n_sig, n_out), added to the result                */
    float* y;          int64_t y_stride;         /* (n_sig, n_out)                                                      */
} pg_ola_stretch_args;                           /* 96 bytes */
int     pg_ola_stretch(const pg_ola_stretch_args* a, void* stream);
int     pg_ola_window(float* win_host, int32_t win_len);

/* Tempo maps: the five stretch kernels over a TABLE of positions instead of one rate (phasegen/track.py, TimeMap).  Each entry
 * point below is the twin of the one it is named after, with `pos`, a DEVICE table of doubles, in place of src_per_out: the kernels
 * are the twins' own, instantiated on a second time grid (csrc/pg_track.h), and everything the twin's comment says holds word for
 * word once "p = (double)g * src_per_out" is read as "p = pc(pos[g])".  Structs of their own, PG_VERSION unchanged; the reference has
 * no counterpart; the arithmetic below is the contract.
 *   A mapped position.  pc(p) = !(p >= 0) ? 0 : (p > 2^52 ? 2^52 : p): a NaN and a negative position count as 0, +inf and anything
 *   beyond 2^52 as 2^52, where floor(p) == p.  From pc on everything is the twin's arithmetic: i0 = min((int64)floor(pc), F_src - 1),
 *   i1 = min(i0 + 1, F_src - 1); in pg_spec_clips_map w = (float)(pc - floor(pc)) and out = a when w == 0 (so -0.0 survives),
 *   otherwise fl(a + fl(w fl(b1 - a))); in the three phase kernels the advance into frame g lies between i1(g - 1) and i0(g).
 *   Hence no read leaves a plane, whatever the table holds, and a NaN in `pos` reads source frame 0 (with w == 0).  Positions need
 *   not be monotone: a frozen table holds a frame's magnitudes while its phase goes on advancing by the step measured there, and a
 *   backward step or a jump takes the advance between i1(g-1) and i0(g) as it stands (a wrapped difference, whatever lies between;
 *   the planner in phasegen/track.py restricts slopes, the kernels do not).  A table that holds (double)g * src_per_out reproduces the twin BIT
 *   FOR BIT at any src_per_out, and the frames before a table's first departure from such a line have the twin's bits (the scans
 *   are causal; pg_spec_clips_map cell by cell).
 *   Tables.  pg_spec_clips_map: (n_clips - 1) sf + frames source-frame positions, one per global output frame.  pg_phase_vocoder_map,
 *   pg_phase_lock_map, pg_phase_lock_linked_map: F_out source-frame positions.  pg_ola_stretch_map: one source CENTRE per grain, in
 *   samples, (n_out + win_len / 2) / hop + 1 entries (grain g is centred on output sample g hop; no grain beyond the table covers an
 *   output sample); c_g = (int64) rint(pos[g]), round half to even, and a centre that is NaN or beyond +-2^62 is outside every
 *   signal: it counts in den and not in num.
 *   Sizes.  Every size is an int32_t, a channel stride is a count of ROWS (p_ch_rows, a_ch_rows, m_ch_rows >= bins: channels
 *   ch_rows F_src elements apart; 2 bins for a plane of a polar tensor) and a row stride of pg_ola_stretch_map a count of samples;
 *   all index arithmetic inside is 64-bit.  The only 64-bit integer field is workspace_bytes.
 *   NaN cells in A or M, the workspaces (pg_workspace_bytes_phase_lock_map / _linked_map return what the twins' queries return for
 *   equal shapes), the kernels, the 16-byte store paths: the twins'.  pg_spec_clips_map has no 16-byte path (the twin's is rate 1's).
 *   The library allocates nothing and keeps nothing.
 *   Errors (host side, before any launch): the twin's rows in the twin's order, without the src_per_out row and the rows no int32
 *   size can reach (a plane beyond 2^62 elements), with pos NULL in the PG_ERR_NULL row and pos not 8-byte aligned in the
 *   PG_ERR_ALIGN row; a ch_rows < bins is the twin's "stride shorter than a plane" (PG_ERR_SHAPE). */
typedef struct pg_spec_clips_map_args {
    int32_t n_clips, n_ch, bins, frames;         /* output (n_clips, n_ch, bins, frames)                                */
    int32_t sf, F_src;                           /* clip k begins at global output frame k sf; frames per row of P      */
    int32_t p_ch_rows, _pad0;                    /* channels p_ch_rows F_src elements apart, p_ch_rows >= bins          */
    const double* pos;                           /* DEVICE: (n_clips - 1) sf + frames source-frame positions            */
    const float* P;                              /* (n_ch, bins, F_src)                                                 */
    float* out;
} pg_spec_clips_map_args;                        /* 56 bytes */
int pg_spec_clips_map(const pg_spec_clips_map_args* a, void* stream);
typedef struct pg_phase_vocoder_map_args {
    int32_t n_ch, bins, F_src, F_out;
    float   reset_below; int32_t a_ch_rows;      /* channels of A a_ch_rows F_src elements apart, a_ch_rows >= bins     */
    int32_t m_ch_rows, _pad0;                    /* the same for M (unused when M is NULL)                              */
    const double* pos;                           /* DEVICE: F_out source-frame positions                                */
    const float* A;                              /* (n_ch, bins, F_src)                                                 */
    const float* M;                              /* optional (NULL: no reset after frame 0)                             */
    float* out;                                  /* (n_ch, bins, F_out), dense                                          */
} pg_phase_vocoder_map_args;                     /* 64 bytes */
int pg_phase_vocoder_map(const pg_phase_vocoder_map_args* a, void* stream);
typedef struct pg_phase_lock_map_args {
    int32_t n_ch, bins, F_src, F_out;            /* bins <= 4096                                                        */
    float   reset_below; int32_t a_ch_rows;
    int32_t m_ch_rows, _pad0;
    const double* pos;                           /* DEVICE: F_out source-frame positions                                */
    const float* A;
    const float* M;                              /* required                                                            */
    float* out;                                  /* (n_ch, bins, F_out), dense                                          */
    void* workspace; int64_t workspace_bytes;
} pg_phase_lock_map_args;                        /* 80 bytes */
int64_t pg_workspace_bytes_phase_lock_map(const pg_phase_lock_map_args* a);   /* host function of n_ch, bins, F_out; negative = error code */
int     pg_phase_lock_map(const pg_phase_lock_map_args* a, void* stream);
typedef struct pg_phase_lock_linked_map_args {
    int32_t n_ch, bins, F_src, F_out;            /* bins <= 4096                                                        */
    float   reset_below; int32_t a_ch_rows;      /* channels of A a_ch_rows F_src elements apart, a_ch_rows >= bins     */
    int32_t _pad0, _pad1;
    const double* pos;                           /* DEVICE: F_out source-frame positions                                */
    const float* A;                              /* (n_ch, bins, F_src): the channels' angle planes                     */
    const float* Aref;                           /* (bins, F_src): angle plane of the reference                         */
    const float* Mref;                           /* (bins, F_src): log-magnitude plane of the reference, required       */
    float* out;                                  /* (n_ch, bins, F_out), dense                                          */
    void* workspace; int64_t workspace_bytes;
} pg_phase_lock_linked_map_args;                 /* 88 bytes */
int64_t pg_workspace_bytes_phase_lock_linked_map(const pg_phase_lock_linked_map_args* a);   /* host function of bins, F_out; negative = error code */
int     pg_phase_lock_linked_map(const pg_phase_lock_linked_map_args* a, void* stream);
typedef struct pg_ola_stretch_map_args {
    int32_t n_sig, win_len, hop, n_in;           /* win_len even, 2 <= win_len <= 4096; 1 <= hop <= win_len / 2         */
    int32_t n_out, x_stride, base_stride, y_stride;   /* rows x_stride >= n_in, base_stride, y_stride >= n_out samples apart */
    const double* pos;                           /* DEVICE: (n_out + win_len / 2) / hop + 1 source centres, in samples  */
    const float* x;                              /* (n_sig, n_in)                                                       */
    const float* win;                            /* DEVICE table of win_len floats, each finite and >= 0                */
    const float* base;                           /* optional (NULL): (n_sig, n_out), added to the result                */
    float* y;                                    /* (n_sig, n_out)                                                      */
} pg_ola_stretch_map_args;                       /* 72 bytes */
int     pg_ola_stretch_map(const pg_ola_stretch_map_args* a, void* stream);

/* pg_varispeed: a band-limited resampler whose read position and bandwidth vary along the output -- the playback half of a pitch
 * curve (phasegen/track.py, PitchCurve), where pg_resample takes one (up, down) for the whole row.  Struct of its own, PG_VERSION
 * unchanged; the reference has no counterpart; the arithmetic below is the contract.
 *   Filter.  Smith's table-driven band-limited interpolation with pg_resample's Kaiser-windowed sinc
 *   h(t) = r sinc(r t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta), |t| <= Z, sampled L = per_zero times per zero crossing and interpolated
 *   linearly (the scheme resampy uses, with the table built exactly).  pg_varispeed_table_elems(Z, L) = 2 (Z L + 1) (negative = error
 *   code).  pg_varispeed_table (HOST, in double, as pg_resample_bank) fills pairs (h_i, d_i), i = 0 .. Z L: h_i = float32(h(i / L)),
 *   d_i = fl32(h_{i+1} - h_i) of the ROUNDED values, d_{ZL} = 0.  The caller passes a DEVICE copy as `table`; the kernel reads no other
 *   coefficients.  Limits: Z in [1, 64], L a power of two in [1, 512], beta in [0, 15], r in (0, 1].
 *   Tables.  step is a power of two, 1 <= step <= 4096; nb = ceil(n_out / step) blocks of step outputs.  pos: nb + 1 source positions
 *   in samples, one per block end; scale: nb bandwidths, one per block.
 *   Per output t of a row, every operation a separate IEEE operation (nothing contracted):
 *     j = t div step, q = t - j step
 *     P_j = pc(pos[j]), the mapped kernels' clamp above: a NaN or a negative position counts as 0, anything above 2^52 as 2^52
 *     delta = (P_{j+1} - P_j) (1.0 / step);   p = P_j + (double)q delta                        (double)
 *     s = sc(scale[j]),  sc(v) = !(v >= 0.25f) ? 0.25f : (v > 1.0f ? 1.0f : v): a NaN, zero or tiny scale counts as 0.25
 *     for every integer n in [0, n_in), ascending:
 *       u = fabs(p - (double)n) ((double)s L)                                                   (double; the product s L is exact)
 *       the tap belongs to the sum iff u < Z L;   i = (int)floor(u),  eta = (float)(u - floor(u))
 *       w = fl(fl(h_i + fl(eta d_i)) s);   acc = fl(acc + fl(w x[n])), from acc = 0.0f           (float)
 *     y[t] = acc
 *   Consequences.  A tap outside the support or outside the row is not read and not added: the result depends on the set of taps
 *   alone, never on the loop bounds the kernel chooses.  A NaN in x reaches exactly the outputs whose support contains it.  Row
 *   padding and the next row are never read.  Positions need not be monotone (a frozen table repeats a sample, a backward step plays
 *   backwards).  A row's bits do not depend on n_sig or on its place in the batch.  An output whose support misses the row is +0.0.
 *   Sizes.  Every size is an int32_t and the row strides are counts of samples; all index arithmetic inside is 64-bit.  There is no
 *   workspace: the library allocates nothing and keeps nothing.
 *   Kernel: one workgroup per 1024 consecutive outputs of one row.  It folds the clamped block ends its tile touches into a source
 *   span; a span that, with the filter's widest reach 4 Z on either side, fits 48 KB of LDS is staged once and summed from there,
 *   any other (jumps, backward steps, hostile tables) is summed straight from global memory with the same chain: the same bits.
 *   One 8-byte load of (h_i, d_i) per tap; no atomics; one launch on the caller's stream.
 *   Errors (host side, before any launch, in this order): NULL args PG_ERR_NULL; non-positive n_sig / n_in / n_out PG_ERR_SHAPE;
 *   step, zeros or per_zero outside the limits or not a power of two where one is required PG_ERR_UNSUPPORTED; a stride shorter
 *   than its row PG_ERR_SHAPE; pos, scale, table, x or y NULL PG_ERR_NULL; pos or table not 8-byte aligned PG_ERR_ALIGN.  Messages
 *   begin "varispeed: ".  pg_varispeed_table: NULL PG_ERR_NULL, zeros / per_zero as above, beta or rolloff outside the limits
 *   PG_ERR_SHAPE. */
int64_t pg_varispeed_table_elems(int32_t zeros, int32_t per_zero);   /* 2 (Z L + 1); negative = error code */
int     pg_varispeed_table(float* table_host, int32_t zeros, int32_t per_zero, double beta, double rolloff);  /* HOST, double arithmetic */
typedef struct pg_varispeed_args {
    int32_t n_sig, n_in, n_out, step;            /* step: a power of two, 1 <= step <= 4096                             */
    int32_t zeros, per_zero;                     /* Z in [1, 64]; L a power of two in [1, 512]                          */
    int32_t x_stride, y_stride;                  /* rows x_stride >= n_in, y_stride >= n_out samples apart              */
    const double* pos;                           /* DEVICE: nb + 1 source positions in samples, nb = ceil(n_out / step) */
    const float*  scale;                         /* DEVICE: nb bandwidths, one per block                                */
    const float*  table;                         /* DEVICE copy of pg_varispeed_table's output                          */
    const float*  x;                             /* (n_sig, n_in)                                                       */
    float*        y;                             /* (n_sig, n_out)                                                      */
} pg_varispeed_args;                             /* 72 bytes */
int     pg_varispeed(const pg_varispeed_args* a, void* stream);

/* pg_pitch_track: a fundamental-frequency tracker, YIN (de Cheveigne and Kawahara 2002) per frame -- the measuring half of a pitch
 * correction (phasegen/track.py, detect_pitch, PitchCurve.correcting, autotune).  Struct of its own, PG_VERSION unchanged; the
 * reference has no counterpart; the arithmetic below is the contract: every operation a separate IEEE float32 operation (nothing
 * contracted, division correctly rounded), so a numpy restatement reproduces the kernel bit for bit.
 *   Frame f of a row holds the samples x_j = x[f hop + j], j = 0 .. W + tau_max - 1.  A sample at or beyond n_in counts as +0.0f
 *   and is not read; the next row and the stride padding are never read.  Index arithmetic is 64-bit inside.
 *   1. Difference function.  d(0) = 0.  For tau = 1 .. tau_max: acc = 0; for j = 0 .. W - 1 ascending: e = fl(x_j - x_{j+tau}),
 *      acc = fl(acc + fl(e e)); d(tau) = acc.
 *   2. Running sum.  S(0) = 0, S(tau) = fl(S(tau - 1) + d(tau)), ascending.
 *   3. Non-finite gate.  If S(tau_max) is not finite, period[f] = ap[f] = NaN (quiet, positive: 0x7fc00000) and the frame is done.
 *      This covers a NaN or an Inf anywhere in the frame's W + tau_max samples (every one of them enters some d(tau)) and an
 *      overflow of the squares.  No other frame is affected.
 *   4. Normalised difference.  cm(0) = 1; for tau >= 1: cm(tau) = S(tau) > 0 ? fl(fl(d(tau) (float)tau) / S(tau)) : 1.0f.
 *   5. Pick.  A = [tau_min, tau_max - 1].  If some tau in A has cm(tau) < threshold, take the smallest; then, while tau + 1 is in A
 *      and cm(tau + 1) < cm(tau), step to tau + 1.  Otherwise take the smallest tau in A that attains min cm over A.  A NaN
 *      threshold never matches.  Both searches are exact comparisons, so any reduction order gives the same tau^.
 *   6. Refine.  a = cm(tau^ - 1), b = cm(tau^), c = cm(tau^ + 1) (both neighbours exist: tau_min >= 2, cm is defined up to
 *      tau_max).  den = fl(fl(a + c) - fl(2 b)); delta = den > 0 ? clamp(fl(fl(0.5f fl(a - c)) / den), -1, 1) : 0, with
 *      clamp(q) = q < -1 ? -1 : (q > 1 ? 1 : q); period[f] = fl((float)tau^ + delta), ap[f] = b.
 *   Consequences.  A frame's bits depend on its own W + tau_max samples and on nothing else: not on n_sig, the row's place, frames,
 *   or how frames share a workgroup.  Silence, a constant row and values whose squares underflow give S = 0, so cm = 1 everywhere,
 *   period = tau_min and ap = 1.  Scaling a row by a power of two that causes neither overflow nor underflow leaves both outputs
 *   bit-identical.  Voicing is the caller's decision (ap < threshold): the kernel always writes both values.
 *   Sizes.  Every size is an int32_t and the strides are counts of elements.  There is no workspace: the library allocates nothing
 *   and keeps nothing.
 *   Kernel: one workgroup per up to four consecutive frames of a row, their common span staged in LDS once; a lane owns five
 *   consecutive lags and a sliding register window; the running sum is one serial chain in one lane; the searches are shuffle
 *   reductions.  No atomics, no global scratch; one launch on the caller's stream.
 *   Errors (host side, before any launch, in this order): NULL args PG_ERR_NULL; non-positive n_sig / n_in / frames / hop
 *   PG_ERR_SHAPE; window, tau_min or tau_max outside the limits PG_ERR_UNSUPPORTED; a stride shorter than its row PG_ERR_SHAPE;
 *   x, period or ap NULL PG_ERR_NULL.  Messages begin "pitch_track: ". */
typedef struct pg_pitch_track_args {
    int32_t n_sig, n_in, frames, hop;            /* frame f of a row begins at sample f * hop                        */
    int32_t window, tau_min, tau_max;            /* W in [4, 2048]; 2 <= tau_min < tau_max <= 1024                   */
    int32_t x_stride, out_stride;                /* rows x_stride >= n_in samples, out_stride >= frames values apart */
    float   threshold;                           /* theta of the absolute threshold; any float                       */
    const float* x;                              /* (n_sig, n_in)                                                    */
    float* period;                               /* (n_sig, frames): the period in samples                           */
    float* ap;                                   /* (n_sig, frames): the aperiodicity d'(tau^)                       */
} pg_pitch_track_args;                           /* 64 bytes */
int     pg_pitch_track(const pg_pitch_track_args* a, void* stream);

/* pg_formant_shift: the spectral envelope of every frame of a log1p-magnitude plane and, optionally, the plane with that envelope
 * re-imposed at `ratio` times each bin's frequency -- formant preservation for a pitch shift (phasegen/track.py, formant_semitones,
 * pitch_shift(formants="keep")): the resampling that moves the partials moves the envelope with them, and this moves it back.
 * Struct of its own, PG_VERSION unchanged; the reference has no counterpart; the arithmetic below is the contract.
 *   M: (n_ch, bins, F) fp32, frames fastest, rows F apart, channels m_ch_rows F elements apart with m_ch_rows >= bins: a count of
 *   ROWS (2 bins for pol[:, 0] of a polar tensor, bins for a dense plane).  All sizes are int32_t and all address arithmetic inside
 *   is 64-bit.  Limits: 1 <= bins <= 4096, 1 <= order <= min(bins, 64), 0 <= hold <= 64, 0 <= iters <= 16, F >= 1, n_ch >= 1.
 *   Domain: cells finite with 0 <= M <= 80 (the project's log1p magnitudes; expm1 stays finite).  Outside it only the confinement
 *   below is promised.
 *   Basis.  pg_formant_basis_elems(bins, order) = order bins + order (negative = error code).  pg_formant_basis (HOST, in double,
 *   rounded once) fills T[q][k] = cos(pi q (k + 1/2) / bins), q < order, k < bins, k fastest, and then s[q] = c_q w_q with c_0 = 1 / bins,
 *   c_q = 2 / bins for q >= 1 and the Hann lifter w_q = (1 + cos(pi q / order)) / 2 (with it the smoother's infinity norm is 1.04 at
 *   every order; with a rectangular lifter it is 2.4 .. 2.9 and the iterations would amplify rounding).  The caller passes a DEVICE
 *   copy of the table as `basis`; the kernel reads no other coefficients.
 *   Per (channel c, frame g), with x[k] = M[c][k][g]:
 *     1. peak hold     h[k] = max over d = -hold .. hold of x[clamp(k + d, 0, bins - 1)]: exact; hold = 0 copies.
 *     2. smoothing     S(v)[k] = sum_q T[q][k] (s[q] sum_j T[q][j] v[j]), in fp32, the order of each sum the kernel's own;  e = S(h).
 *     3. iterations    `iters` times: e = S(max(h, e)).
 *     4. env (optional, dense (n_ch, bins, F)):  env[c][k][g] = e[k].
 *     5. out (optional, dense (n_ch, bins, F)):  p = (double)(k + 1) ratio - 1 clamped to [0, bins - 1] (bin k is FFT bin k + 1: DC is
 *        dropped), i0 = floor(p), i1 = min(i0 + 1, bins - 1), w = (float)(p - i0), ew = e[i0] + w (e[i1] - e[i0]),
 *        a = expm1(max(ew, 0)) + eps, b = expm1(max(e[k], 0)) + eps, out = log1p(expm1(x[k]) (a / b)), with the library's expm1
 *        (2^(m log2 e) - 1) and log1p; one IEEE division, nothing contracted.  ratio == 1.0 copies M to out bit for bit (as
 *        pg_spec_clips does at w == 0), and x[k] == 0 gives +0.0: the zeros pg_hpss writes as silence stay silence.
 *   At least one of env and out is required.
 *   Consequences.  A frame's result does not depend on n_ch, on F, on the frame's position or on how the kernel tiles the plane,
 *   bit for bit.  A plane constant along frequency has itself as its envelope, to rounding (the rows of S sum to one).
 *   Confinement: a non-finite or out-of-domain cell affects only outputs of its own (channel, frame); every other frame has the
 *   bits of the clean call.
 *   Kernel: one workgroup per tile of 32 consecutive frames (16 above 1024 bins, 8 above 2048) x ALL bins of one channel, kept in
 *   LDS across the hold, the 1 + iters passes and the epilogue; both products of a pass run on the fp32 MFMA with the table
 *   streamed from L2; the order of every sum is a function of (bins, order) alone.  16-byte loads and stores where the pointers and
 *   F allow, element by element otherwise (same bits); no atomics.  There is no workspace: the library allocates nothing and
 *   keeps nothing.
 *   Errors (host side, before any launch, in this order): NULL args / M / basis, or env and out both NULL, PG_ERR_NULL; non-positive
 *   sizes, bins > 4096, m_ch_rows < bins, order / hold / iters outside their limits, a plane beyond 2^62 elements, ratio not finite
 *   or outside [0.25, 4], eps not finite or <= 0 PG_ERR_SHAPE; M, basis, env or out not 4-byte aligned PG_ERR_ALIGN.  Messages begin
 *   "formant_shift: ".  pg_formant_basis / _elems: NULL PG_ERR_NULL, bins or order outside the limits PG_ERR_SHAPE. */
typedef struct pg_formant_args {
    int32_t n_ch, bins, F, m_ch_rows;            /* channels m_ch_rows * F elements apart, m_ch_rows >= bins            */
    int32_t order, hold, iters, _pad0;           /* 1 <= order <= min(bins, 64), 0 <= hold <= 64, 0 <= iters <= 16      */
    double  ratio;                               /* finite, in [0.25, 4]; 1.0 copies M to out                           */
    float   eps, _pad1;                          /* finite, > 0: the floor under both linear envelopes                  */
    const float* M;                              /* (n_ch, bins, F), see above                                          */
    const float* basis;                          /* DEVICE copy of pg_formant_basis's table, order bins + order floats  */
    float* env;                                  /* optional (NULL): (n_ch, bins, F), dense                             */
    float* out;                                  /* optional (NULL): (n_ch, bins, F), dense                             */
} pg_formant_args;                               /* 80 bytes */
int     pg_formant_shift(const pg_formant_args* a, void* stream);
int64_t pg_formant_basis_elems(int32_t bins, int32_t order);
int     pg_formant_basis(float* basis_host, int32_t bins, int32_t order);

/* How far a reconstruction is from its source, reduced on the device: the sums from which SI-SDR / SNR (waveforms) and spectral
 * convergence / log-spectral distance (spectrograms) are formed on the host (phasegen/metrics.py).  The reference has no counterpart
 * (validate.py takes mean absolute waveform errors of three dataset clips on the host); the arithmetic below is the contract.
 * Common to both calls: `out` is (n_signals, 6) DEVICE doubles, row s for signal s; `gain` is NULL (= 1.0) or n_signals device
 * doubles; sums are kept in double and reduced in two or three launches through `workspace` (pg_workspace_bytes_*() bytes, else
 * PG_ERR_WORKSPACE; no floating-point atomics; the library allocates nothing and keeps nothing).  The partition of the work and every
 * summation tree are functions of the shapes (n; bins, frames) alone -- not of the grid, the CU count, n_signals or the signal's
 * position -- so row s of a batch has the bits of the same signal run alone.  Elements move 16 bytes per lane where the base
 * pointers and the strides (and, for spectrograms, frames % 4 == 0) allow and one by one otherwise; both paths give the same bits.
 * Index arithmetic is 64-bit.
 *
 * pg_wave_compare: x (reference) and y (estimate), (n_signals, n) fp32, rows x_stride / y_stride >= n apart; g = gain[s].
 *   A sample where x or y is NaN or +-inf is counted in slot 5 and taken as 0 in BOTH inputs.  Element arithmetic is in double: the
 *   products x x, y y, x y of two floats are exact; g y is rounded, x - g y is rounded, its square is rounded.
 *     out[s] = { sum x^2, sum y^2, sum x y, sum (x - g y)^2, max |x - g y|, number of non-finite samples }
 *
 * pg_spec_compare: R (reference) and E (estimate) in the layout pg_stft writes, (n_signals, 2, bins, frames) fp32 = [re; im] planes
 *   bins * frames apart, signals r_stride / e_stride >= 2 bins frames apart; bins and frames are any positive integers.
 *   Per cell the four floats are widened to double BEFORE any product (as pg_wave_compare does), with g_f = (float)gain[s]:
 *     mR = sqrt(re^2 + im^2) of R, mE0 = sqrt(re^2 + im^2) of E, mE = g_f mE0, all in double;
 *     L(m) = 10 log10f(fmaxf((float)(m m), floor_power)) in fp32
 *   A cell where any of its four floats is NaN or +-inf is counted in slot 5 and taken as zero in both inputs.  The products mR mR,
 *   mE0 mE0, mR mE0 and (mR - mE)^2 are formed and added in double, so no finite cell overflows or vanishes in slots 0 - 3;
 *   (L(mR) - L(mE))^2 is formed in fp32 and promoted (slot 4's domain: "Magnitude range" above).
 *     out[s] = { sum mR^2, sum mE0^2, sum mR mE0, sum (mR - mE)^2,
 *                sum over frames of sqrt((sum over bins of (L(mR) - L(mE))^2) / bins), number of non-finite cells }
 *   Slot 4 / frames is the log-spectral distance in dB; a cell that is zero in both inputs adds 0 to it (both levels are the floor's).
 *   floor_power must be positive and finite (PG_ERR_SHAPE). */
typedef struct pg_wave_compare_args {
    int32_t n_signals, _pad0;
    int64_t n;
    const float* x; int64_t x_stride;
    const float* y; int64_t y_stride;
    const double* gain;                          /* optional (NULL = 1.0): n_signals device doubles */
    double* out;                                 /* (n_signals, 6) device doubles                   */
    void* workspace; int64_t workspace_bytes;
} pg_wave_compare_args;                          /* 80 bytes */
int64_t pg_workspace_bytes_wave_compare(const pg_wave_compare_args* a);   /* host function of n_signals and n; negative = error code */
int     pg_wave_compare(const pg_wave_compare_args* a, void* stream);
typedef struct pg_spec_compare_args {
    int32_t n_signals, bins, frames; float floor_power;
    const float* R; int64_t r_stride;
    const float* E; int64_t e_stride;
    const double* gain;                          /* optional (NULL = 1.0): n_signals device doubles */
    double* out;                                 /* (n_signals, 6) device doubles                   */
    void* workspace; int64_t workspace_bytes;
} pg_spec_compare_args;                          /* 80 bytes */
int64_t pg_workspace_bytes_spec_compare(const pg_spec_compare_args* a);   /* host function of n_signals, bins, frames; negative = error code */
int     pg_spec_compare(const pg_spec_compare_args* a, void* stream);

/* small helpers the training step needs on device */
int pg_fill(float* p, int64_t n, float value, void* stream);

int pg_version(void);
const char* pg_last_error_string(void);

#ifdef __cplusplus
}
#endif
#endif /* PHASEGEN_H */
