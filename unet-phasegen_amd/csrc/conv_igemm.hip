// conv_igemm.hip -- the six 1-D convolution passes of the U-Net as three implicit-GEMM kernels on the
// gfx950 matrix cores (default v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain; optional bf16-pipe operand
// modes, pg_conv_args.precision).
//
//   F ("forward-shaped"):  Y[b,m,t]  = sum_{q,j}               W[m][q][j] * act(X[b,q,s*t+j-p])
//        = nn.Conv1d forward (model.py:77-78)            and nn.ConvTranspose1d dgrad
//   T ("transposed"):      Y[b,m,tau] = sum_{q,j: s*i+j-p=tau} W[q][m][j] * act(X[b,q,i])
//        = nn.ConvTranspose1d forward (model.py:88-102)  and nn.Conv1d dgrad
//        computed in gather form: output phase phi = (tau+p) mod s only sees taps j = s*jj + phi, so the GEMM
//        rows are (m,phi) pairs, K = (q,jj), N = (b,u) with tau = s*u + phi - p.  No col2im scatter, no atomics.
//   G ("gradient of W"):   dW[m][q][j] = sum_{b,i} actP(P[b,m,i]) * actQ(Q[b,q,s*i+j-p])
//        = wgrad of both (conv: P=dy, Q=x; convT: P=x, Q=dy); beta = 0 write (zero_grad folded in).
//
// Two generations of kernels, selected per call by the host's launch plan (plan_conv() below); sources:
//   conv_common.h        problem descriptor, LDS-DMA helpers, MFMA operand modes, stream-K split, epilogues
//   conv_raw_impl.h      RAW-WINDOW F/T kernel template; conv_raw.hip instantiates the 128 x 256 tile (training), conv_raw_tall.hip the
//                        256 x 128 tile (few columns: small-batch inference)
//   conv_raw*.hip        RAW-WINDOW F/T kernels  } the fast path for every layer geometry of the U-Net except k = 5:
//   conv_raw_wgrad.hip   RAW-WINDOW G kernel     } workgroup tile 128 (M) x 256 (N), 4 waves of 64 x 128 (128 accumulator
//                        registers, 2 waves/SIMD).  The weight / P tile is gathered by LDS-DMA into a swizzled K-contiguous
//                        image; the ACTIVATION operand is staged as raw row windows (every element once) and the im2col
//                        overlap is resolved when fragments are read: ~60 % fewer global->LDS bytes and far fewer gather
//                        instructions per MFMA than an im2col tile.
//   conv_im2col.hip      IM2COL kernels (conv_f/t/g_kernel): 256 x 128 tile, both operands gathered element by element by
//                        LDS-DMA with per-lane source addresses (im2col, phase split, zero padding and the XOR swizzle all
//                        live in the address).  They serve k = 5, generic (k, s) and shapes whose windows do not fit, and
//                        stay covered by the tests (schedule bit 2).
//   conv_w1.h            what the two one-wave-per-SIMD families share: conv_raw3.hip (fp32 raw-window F / T) and conv_h3.hip
//                        (bf16-resident forward), 256 x 256 tiles
//   conv_fixup.h         fixup kernel of the stream-K split, for every family
//   conv_igemm.hip       (this file) instantiates the fixup kernel; host side: geometry checks, grid policy and the launch
//                        plan of a call (kernel family, tiles, grid, fixup form, column tail, packed wgrad operands), which
//                        pg_conv_describe formats, pg_workspace_bytes_wgrad sizes and the C ABI entry points execute.
//
// Common to both: operands reach LDS through buffer_load ... lds (no staging registers, no ds_write; out-of-range lanes
// write 0.0, which implements conv padding, tile edges and K tails); (Leaky)ReLU in front of every conv is applied
// branch-free on the MFMA fragments, so the in-place activations (model.py:80,82) and torch.cat (model.py:113) are
// never materialised; phase order per slab is pinned with sched_barrier(0): gathers for slab s+1, then fragment reads
// + MFMAs of slab s, then one __syncthreads() whose vmcnt(0) therefore sits behind the matrix work; double-buffered
// LDS.  Work decomposition is a persistent stream-K split over (tile, slab) with a deterministic fixup kernel (below).
// Each output element is accumulated in a fixed order: results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <cstring>
#include <cmath>
#include <algorithm>
#include "conv_fixup.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
constexpr int WG_PER_CU = 2;                    // <= 256 VGPR+AGPR per lane -> 2 waves per SIMD; 48 KB LDS per workgroup
constexpr int MAX_STREAMK_WG = 2048;            // bound on the persistent grid (sizes the caller's workspace)
constexpr long WS_PER_WG = 2L * ACC_REGS * NT * 4;   // two partial tiles of 256x128 fp32 per workgroup
constexpr long WS_STREAMK = (long)MAX_STREAMK_WG * WS_PER_WG;   // pg_workspace_bytes_conv(): the stream-K region of the workspace

// Per-call knobs decoded from pg_conv_args.precision / .schedule (no process-wide state: two streams or threads can run
// different precisions and schedules concurrently).
struct Knobs {
    int prec;         // PG_PREC_*: 0 fp32 MFMA, 1 bf16 operands, 2 bf16x3 split (all fp32 accumulate)
    int force_mode;   // work split: 0 automatic, 1 one tile per workgroup, 2 force stream-K
    int no_raw;       // 1 = never use the raw-window kernels (exercise the im2col kernels)
    int no_tall;      // 1 = never use the tall 256 x 128 raw tile
    int oversub;      // stream-K grid = up to oversub x resident workgroup slots
    int contended;    // other kernels (RCCL collectives) are expected to hold part of the chip: always take the finer split
    int no_ps;        // wgrad: 1 = never the per-sample-slab kernel (A/B, tests)
    int no_raw3;      // 1 = never the one-wave-per-SIMD fp32 kernels (conv_raw3.hip; schedule bit 13: A/B, tests of the older kernels)
    int all_raw3;     // 1 = the one-wave-per-SIMD kernels wherever they cover the problem (bit 14), also where auto prefers the older ones
    int sr;           // conv_raw3 tile order: super-row height forced by schedule bits 15-16 (0 = default)
    int force_colsplit;   // 1 = split wherever the geometry allows, whatever the cost model says (bit 18: tests reach the tail launch on small problems)
    int no_colsplit;  // 1 = never split the columns past the last full 256-wide tile off into a tail launch (bit 17: A/B, tests)
    int slots;        // PG_SCHED_SLOTS (bits 19-23): plan as if the device had this many compute units (0 = pg_cu_count(): tests reach the
                      // multi-tile work splits of the bench shape on small problems)
};
int decode_knobs(const pg_conv_args* a, Knobs& k) {
    if (a->precision < 0 || a->precision > 2) return pg_fail(PG_ERR_UNSUPPORTED, "conv: precision must be PG_PREC_FP32, PG_PREC_BF16 or PG_PREC_BF16X3");
    const int sc = a->schedule;
    if (sc < 0 || (sc & ~0xffffff) || ((sc >> 17) & 3) == 3 || (sc & 3) == 3 || ((sc >> 8) & 15) > 8) return pg_fail(PG_ERR_SHAPE, "conv: bad schedule bits");
    k.prec = a->precision;
    k.force_mode = sc & 3; k.no_raw = (sc >> 2) & 1; k.no_tall = (sc >> 3) & 1;
    k.oversub = (sc >> 8) & 15; if (!k.oversub) k.oversub = 4;
    k.contended = (sc >> 4) & 1;
    // bits 5-6 selected the two-waves-per-SIMD / eight-wave tile families of pg_conv_fwd_h until 0.3 (conv_h.hip, conv_h2.hip): no
    // automatic choice reached them once conv_h3 was the default for every layer, and they are gone (0.4); bit 12 (conv_h3) is a no-op
    if ((sc >> 5) & 3) return pg_fail(PG_ERR_UNSUPPORTED, "conv: schedule bits 5-6 (tile families removed in 0.4)");
    k.no_ps = (sc >> 7) & 1;
    k.no_raw3 = (sc >> 13) & 1;
    k.all_raw3 = (sc >> 14) & 1;
    k.sr = ((sc >> 15) & 3) ? 1 << (((sc >> 15) & 3) - 1) : 0;      // bits 15-16: 1 -> R = 1 (row-major), 2 -> 2, 3 -> 4; 0 = default
    k.no_colsplit = (sc >> 17) & 1;
    k.force_colsplit = (sc >> 18) & 1;
    k.slots = (sc >> 19) & 31;
    if (k.no_raw3 && k.all_raw3) return pg_fail(PG_ERR_SHAPE, "conv: schedule bits 13 and 14 exclude each other");
    return PG_OK;
}

// the wide fixup (four workgroups per 32 x 32 block, segments summed four abreast) from 8 segments per split tile on
bool fixup_wide(int grid, long split_tiles) { return split_tiles > 0 && grid >= 8 * split_tiles; }

// Grid policy.  Default: a persistent stream-K grid of up to oversub (4) x the resident workgroup slots, each
// workgroup owning an equal contiguous range of the (tile, slab) space, plus the fixup launch.  Measured on MI355X
// (tools/contention.py): the oversubscribed split costs nothing on a free chip, removes tile-count quantisation, and --
// what matters for data-parallel training, where RCCL's collective kernels hold part of the chip during backward --
// degrades gracefully when slots are taken (16 of 512 slots held: 1x split 33 -> 58 ms, one-tile-per-workgroup 32 -> 43 ms,
// 4x split 33 -> 37 ms).  Small problems (less than 8 slabs per resident slot, or no workspace) run one tile per
// workgroup.  kn.force_mode: 0 auto, 1 force one tile per workgroup, 2 force stream-K (tests).  one_wave: the one-wave-per-SIMD
// kernels (one workgroup per CU, partial tiles of 256 x 256).  kn.slots: the compute units to plan for instead of the device's
// (PG_SCHED_SLOTS); the only place the conv launch plan reads the CU count, so split_columns' pricing follows it too.
int pick_grid(long tiles, int nslab, IgemmParams& p, long ws_bytes, const Knobs& kn, bool one_wave) {
    const long total = tiles * (long)nslab;
    const long slots = (long)(kn.slots ? kn.slots : pg_cu_count()) * (one_wave ? 1 : WG_PER_CU), ws_per_wg = one_wave ? 2 * WS_PER_WG : WS_PER_WG;
    // the schedule is a function of the stream-K region only: a workspace that also holds packed wgrad operands splits the same way
    ws_bytes = std::min(ws_bytes, WS_STREAMK);
    p.whole = 0;
    // A tile count that is a whole multiple of the resident slots quantises perfectly: whole tiles per workgroup, no partial
    // tiles through the workspace and no fixup launch (measured: the fixups of the five such layers of the U-Net cost 0.5 ms
    // per step).  Not when the chip is shared (data-parallel backward beside RCCL): there the finer split bounds the tail.
    if (kn.force_mode == 0 && !kn.contended && tiles % slots == 0) {
        if (tiles <= slots * kn.oversub) return (int)tiles;
        for (long mult = kn.oversub; mult >= 1; --mult)
            if (tiles % (slots * mult) == 0) return (int)(slots * mult);       // several whole tiles per workgroup
    }
    long mult = total / (256 * slots);               // whole multiples of the slot count only (a ragged second wave is
    if (mult > kn.oversub) mult = kn.oversub;        // worse than none), and >= 256 slabs per workgroup so that partial-
    if (mult < 1) mult = 1;                          // tile traffic stays negligible
    long G = slots * mult;
    if (G > MAX_STREAMK_WG) G = (MAX_STREAMK_WG / slots) * slots;
    if (G > total) G = total;
    const bool can = p.ws && ws_bytes >= G * ws_per_wg && total < 0x7fffffffL;
    if (kn.force_mode == 1 || !can) return (int)tiles;
    if (kn.force_mode == 2) return (int)G;
    // Hybrid: a tile count slightly above a multiple of the slots (1056, 528) runs its full waves as whole tiles and splits only
    // the remainder over one more wave of workgroups: the same balance as the even split with (almost) no partial tiles -- the
    // fixup then touches 32 tiles instead of 1056.  Not when the chip is shared (see above).
    if (!kn.contended && tiles > slots) {
        const long whole = tiles / slots * slots, rem = tiles - whole;
        if (rem * nslab >= slots * 8 && whole + slots <= MAX_STREAMK_WG && ws_bytes >= (whole + slots) * ws_per_wg) {
            p.whole = (int)whole;
            return (int)(whole + slots);
        }
    }
    return total >= slots * 8 ? (int)G : (int)tiles;
}

// raw-window kernels: supported (k, s) pairs and the window-length bound
bool raw_supported(Kind kind, const IgemmParams& p, const Knobs& kn, int tn = RBN) {
    // (k = 5 forward: a slab is two whole channels; an odd channel count stays on im2col)
    if (kn.no_raw || !unet_ks(p.k, p.s) || (kind == KIND_F && p.k == 5 && p.Q % 2)) return false;
    // a 16-element slab of (b, i) may run over at most ONE sample boundary in the raw-window wgrad kernel
    if (kind == KIND_G) return p.LP >= 16;
    // k = 5 runs the raw-window kernels as a virtual k = 8 (conv_raw_impl.h): taps of the weight image per (row, channel)
    const bool t = kind == KIND_T;
    const int kv = p.k == 5 ? 8 : p.k, kwp = t ? kv / p.s : kv, sc = t ? 1 : p.s, lcol = t ? p.U : p.Ly;
    const int tj = kwp < 16 ? kwp : 16;
    const int nseg_max = (lcol - 1 + tn - 1) / lcol + 1;
    return sc * (tn - 1) + tj + raw_gap(tj) * (nseg_max - 1) + (t ? tj : 0) <= (sc == 1 ? RS1 : RS2);
}

// fp32 raw-window wgrad: layout of the packed operands (IgemmParams.qk / .pk, conv_raw_wgrad.hip), which live in the workspace
// behind its stream-K region.  Q rows reach S * (last gathered frame) + WLP floats (the window slot of the last slab), at least
// p + Lx; P has Kp = nslab * 16 frames per row (flat K) or 16 ceil(LP / 16) per sample (per-sample slabs).  Returns the bytes, or
// -1 where an operand would not fit 31-bit buffer offsets.
long g_pack_layout(IgemmParams& p) {
    const int cps = (p.LP + 15) / 16;
    const long gimax = p.g_ps ? 16L * (cps - 1) : (long)p.LP - 1;
    long lq = (long)p.s * gimax + g_wlp(p.k, p.s);
    if (lq < (long)p.p + p.Lx) lq = (long)p.p + p.Lx;
    lq = (lq + 3) / 4 * 4;
    const long kp = p.g_ps ? 16L * cps : 16L * p.nslab;
    const long qbytes = (long)p.B * p.Q * lq * 4, pbytes = (p.g_ps ? (long)p.B : 1L) * p.M * kp * 4;
    if (qbytes >= 0x7ffffff0L || pbytes >= 0x7ffffff0L) return -1;
    p.Lq = (int)lq; p.qk_bs = (int)((long)p.Q * lq); p.qk_bytes = (unsigned)qbytes;
    p.Kp = (int)kp; p.pk_bytes = (unsigned)pbytes;
    return (qbytes + 255) / 256 * 256 + pbytes;
}

// ---- launch plan: everything a call enqueues, decided before anything is --------------------------------------------------
// pg_conv_describe formats a plan, pg_workspace_bytes_wgrad sizes it, the entry points execute it.  Kernel families (GEMM tile):
// im2col 256 x 128, raw 128 x 256, raw tall 256 x 128, raw3 (fp32 F / T) 256 x 256, g_raw / g_ps (wgrad) 128 x 256, h3 256 x 256.
enum Family { FAM_IM2COL, FAM_RAW, FAM_RAW_TALL, FAM_RAW3, FAM_G_RAW, FAM_G_PS, FAM_H3 };
enum Fixup { FIXUP_NONE, FIXUP_PLAIN, FIXUP_WIDE };
struct ConvPart {           // one GEMM launch, and the fixup of the tiles its grid splits (FIXUP_NONE: none is split)
    Family fam; int grid; long tiles; Fixup fixup;
    IgemmParams p;          // with tiles, slabs, tn_stride, whole, sr, g_ps, n_lo (and the packed layout) filled in
};
struct ConvPlan {
    Kind kind; int prec;
    ConvPart main, tail;    // tail (has_tail): a column split's tall-tile launch over the columns from tail.p.n_lo on
    bool has_tail;
    long pack;              // fp32 raw-window wgrad: bytes of packed operands behind the workspace's stream-K region (else 0)
};

// fp32 F / T problems the one-wave-per-SIMD kernels (conv_raw3.hip: 256 x 256 tile) cover, unless 256-row tiles would compute
// over 3 % more rows than 128-row ones
bool r3_ok(Kind kind, const IgemmParams& p, const Knobs& kn, long rows) {
    return kind != KIND_G && kn.prec == 0 && !kn.no_raw3 && raw_supported(kind, p, kn) && pgconv::raw3_covers(kind, p) &&
           (rows + 255) / 256 * 256 * 100 <= (rows + RBM - 1) / RBM * RBM * 103;
}

Family pick_family(Kind kind, const IgemmParams& p, const Knobs& kn, long rows, long cols) {
    const bool raw = raw_supported(kind, p, kn);
    if (kind == KIND_G) {
        if (!raw) return FAM_IM2COL;
        // short samples: slabs of 16 frames of ONE sample (conv_g_ps_kernel) where padding every sample to whole slabs costs <= 7 %
        // of MFMA work (30 frames: 6.7 %, 61: 4.9 %, 126: 1.6 %, 256: none; 129 would cost 11.6 % and keeps the flat K axis)
        const long cps = (p.LP + 15) / 16;
        return p.k != 32 && (cps * 16 - p.LP) * 100 <= 7L * p.LP && !kn.no_ps ? FAM_G_PS : FAM_G_RAW;
    }
    // F / T problems whose columns the tall 256 x 128 tile covers with at least 3 % fewer computed ones take it (and those whose
    // windows only fit the narrower tile: many short samples per tile): small-batch
    // inference above all (a 128 x 256 tile over 65 columns is 3/4 idle MFMA work per weight byte), and training shapes such as
    // N = 16 x 65 (5 wide tiles = 1280 columns vs 9 tall = 1152: +15 % measured) or 64 x 30.  On ties the wide tile wins (it
    // runs two slabs per barrier; measured 1-7 % faster at equal column counts).
    const long cols_wide = (cols + RBN - 1) / RBN * RBN, cols_tall = (cols + RBN / 2 - 1) / (RBN / 2) * (RBN / 2);
    const bool tall = !kn.no_tall && (cols_tall * 100 <= cols_wide * 97 || !raw) && raw_supported(kind, p, kn, RBN / 2);
    // conv_raw3 also over the tall tile where 256-wide tiles compute at most 8 % more columns (D2 forward / U2 dgrad / D3 forward at
    // batch 64: -6 / -2 / -6 %, and 2.2 instead of 6.95 GB of L2 fills; batch-1 inference and N = 16 x 65 keep the tall tile).
    if (r3_ok(kind, p, kn, rows) && (!tall || kn.all_raw3 || cols_wide * 100 <= cols_tall * 108)) return FAM_RAW3;
    return tall ? FAM_RAW_TALL : (raw ? FAM_RAW : FAM_IM2COL);
}

// K of the GEMM a family runs: the raw-window F / T kernels take k = 5 as virtual taps, the per-sample-slab wgrad pads every sample
// to whole slabs
long family_k(Family fam, Kind kind, const IgemmParams& p, long K) {
    if (fam == FAM_G_PS) return (long)p.B * ((p.LP + 15) / 16) * 16;
    return fam != FAM_IM2COL && kind != KIND_G && p.k == 5 ? (long)p.Q * (kind == KIND_T ? 4 : 8) : K;
}

// grid and fixup form of a part whose tiles and slabs are set
void set_grid(ConvPart& c, const Knobs& kn, long ws_bytes) {
    c.grid = pick_grid(c.tiles, c.p.nslab, c.p, ws_bytes, kn, c.fam == FAM_RAW3 || c.fam == FAM_H3);
    // ranges made of whole tiles (grid == tiles, or a grid that divides the tile count) leave nothing for the fixup.  Many segments
    // per split tile (small-batch inference) -> the wide fixup (conv_raw3 has none): the order in which a tile's segments are added
    // is a function of (grid, tiles) only, so a geometry always takes the same one
    if (c.tiles % c.grid == 0) c.fixup = FIXUP_NONE;
    else c.fixup = c.fam != FAM_RAW3 && fixup_wide(c.grid, c.tiles - c.p.whole) ? FIXUP_WIDE : FIXUP_PLAIN;
}

// one fp32 launch of family `fam` over the columns [n_lo, n_hi): tiles, slabs and grid
int plan_part(Family fam, Kind kind, const Knobs& kn, const IgemmParams& p0, long rows, long n_lo, long n_hi, long K, long ws_bytes, ConvPart& c) {
    const long cols = n_hi - n_lo;
    c.fam = fam;
    c.p = p0;
    IgemmParams& p = c.p;
    p.n_lo = (int)n_lo;
    const int bm = c.fam == FAM_IM2COL ? BM : (c.fam == FAM_RAW_TALL || c.fam == FAM_RAW3 ? 2 * RBM : RBM);
    int bn = c.fam == FAM_IM2COL ? BN : (c.fam == FAM_RAW_TALL ? RBN / 2 : RBN);
    if (kind == KIND_G && p.k == 5 && c.fam != FAM_IM2COL) bn = (RBN / 5) * 5;   // wgrad: a column tile is 51 whole channels x 5 taps = 255 columns (+ 1 idle)
    p.g_ps = c.fam == FAM_G_PS;
    p.tn_stride = bn;
    // conv_raw3's tile order: the 32 workgroups of an XCD (256 CUs / 8) run consecutive tiles.  Row-major (R = 1) they are one tile
    // row: they share the weight panel but each reads its own activation panel.  In super-rows of R tile rows an XCD covers R x 32/R
    // tiles and an activation panel serves R rows at once.  Measured (tools/dbg/sr_ab.py, FETCH_SIZE per launch at the bench shape,
    // R = 1 / 2 / 4): k = 8 layers 1.85 / 1.57 / 1.77, 1.49 / 1.22 / 1.51, 0.68 / 0.54 / 0.68 GB -- R = 2 saves 15-20 % of the L2
    // fills; k = 32: 5.41 / 5.47 / 7.41 and 3.24 / 3.23 / 4.84 GB -- nothing at R = 2, + 40 % at R = 4: those fills are weight-panel
    // re-reads of workgroups that drift apart over 4096 slabs, and fewer sharers per panel make it worse.  Time: equal to 0.3 %.
    // Hence R = 2 for k = 8, row-major otherwise (schedule bits 15-16 force R = 1 / 2 / 4 for the A/B).
    p.sr = c.fam == FAM_RAW3 ? (kn.sr ? kn.sr : (p.k == 8 ? 2 : 1)) : 0;
    p.tilesM = (int)((rows + bm - 1) / bm);
    p.tilesN = (int)((cols + bn - 1) / bn);
    p.nslab = (int)((family_k(c.fam, kind, p, K) + BK - 1) / BK);
    c.tiles = (long)p.tilesM * p.tilesN;
    if (c.tiles <= 0 || c.tiles > 0x0fffffffL || p.nslab <= 0 || cols + bn >= 0x7fffffffL) return pg_fail(PG_ERR_SHAPE, "conv: empty or oversize grid");   // the fixup launches 8 workgroups per tile
    set_grid(c, kn, ws_bytes);
    return PG_OK;
}

// Column split (round 4).  conv_raw3's tiles are 256 columns wide: 64 x 129 frames are 32.25 of them, and the 33rd tile column
// costs what the other 32 cost each (2.3 % of D0 forward / U0 dgrad; at the reference's own batch of 16 x 65 = 1040 columns a
// FIFTH of five).  Where the columns past the last full tile are few (<= 128), the launch covers full tiles only and a second
// launch of the tall two-waves-per-SIMD kernel (256 x 128, column blocks without columns skipped) takes the tail from column
// n_lo on: a weight-streaming pass like demo.py's single clip (the weights once at ~3 TB/s, or its own MFMA work), taken when
// the model below says it costs under 1 / 1.3 of the tile column it replaces.  A pure function of the geometry.
bool split_columns(Kind kind, const IgemmParams& p, const Knobs& kn, long rows, long cols, long K, long ws_bytes) {
    // (r3_ok: also where the whole problem would take the tall tile)
    if (!r3_ok(kind, p, kn, rows) || kn.force_mode == 1 || kn.no_colsplit || kn.no_tall) return false;
    const long full = cols / RBN * RBN, rem = cols - full;
    if (!(full > 0 && rem > 0 && rem <= RBN / 2 && raw_supported(kind, p, kn, RBN / 2))) return false;
    const long Kr = family_k(FAM_RAW3, kind, p, K);
    const double rows_p = (double)((rows + 255) / 256 * 256), rem32 = (double)((rem + 31) / 32 * 32), Kd = (double)Kr;
    const double t_col = 2.0 * rows_p * 256.0 * Kd / 140e6;                                              // us at 140 TFLOP/s
    const double t_tail = fmax(4.0 * (double)rows * Kd / 3e6, 2.0 * rows_p * rem32 * Kd / 100e6) + 25.0;  // us: 3 TB/s | 100 TFLOP/s, + launches
    // ... and only where the full tiles then split into ALIGNED ranges (whole tiles per workgroup, or a whole number of
    // workgroups per tile): those walk K in lockstep and share weight / activation panels in L2.  120 or 240 full tiles
    // (64 x 61 frames) over 256 CUs split unaligned: measured 3 % faster than with the tail kept, but 3.9 instead of
    // 1.4 GB of L2 fills per launch -- not taken.
    IgemmParams pa = p;
    const long tiles_a = (rows + 255) / 256 * (full / RBN);
    const long grid_a = pick_grid(tiles_a, (int)((Kr + BK - 1) / BK), pa, ws_bytes, kn, true);
    const bool aligned = pa.whole == 0 && (grid_a % tiles_a == 0 || tiles_a % grid_a == 0);
    return (t_col > 1.3 * t_tail && aligned) || kn.force_colsplit;
}

// bytes spanned by a (B, C, L) view with batch stride bs; 0 if it does not fit 31-bit buffer offsets
unsigned extent_bytes(long B, long bs, long C, long L) {
    const long e = ((B - 1) * bs + C * L) * 4;
    return (e > 0 && e < 0x7ffffff0L) ? (unsigned)e : 0u;
}

int check_geom(const pg_conv_args* a, bool transposed) {
    if (!a) return pg_fail(PG_ERR_NULL, "conv: null args");
    if (a->B <= 0 || a->Cin <= 0 || a->Cout <= 0 || a->Lin <= 0 || a->Lout <= 0 || a->k <= 0 || a->stride <= 0 || a->pad < 0)
        return pg_fail(PG_ERR_SHAPE, "conv: non-positive dimension");
    const long lo = transposed ? (long)(a->Lin - 1) * a->stride - 2L * a->pad + a->k
                               : ((long)a->Lin + 2L * a->pad - a->k) / a->stride + 1;
    if (lo != a->Lout) return pg_fail(PG_ERR_SHAPE, "conv: Lout inconsistent with Lin/k/stride/pad");
    if ((long)a->Cin * a->Cout * a->k * 4 >= 0x7ffffff0L) return pg_fail(PG_ERR_SHAPE, "conv: weight tensor exceeds 2 GiB");
    return PG_OK;
}

// fills the descriptor extents of the tensors a kernel gathers from (x: (B, Q, Lx), P: (B, M, LP)); fails if one exceeds 31-bit
// byte offsets
int set_extents(IgemmParams& p) {
    p.x_bytes = extent_bytes(p.B, p.x_bs, p.Q, p.Lx);
    if (!p.x_bytes) return pg_fail(PG_ERR_SHAPE, "conv: activation tensor exceeds 2 GiB (31-bit buffer offsets)");
    if (p.w) p.w_bytes = (unsigned)((long)p.M * p.Q * p.k * 4);
    if (p.pt) {
        p.pt_bytes = extent_bytes(p.B, p.pt_bs, p.M, p.LP);
        if (!p.pt_bytes) return pg_fail(PG_ERR_SHAPE, "conv: activation tensor exceeds 2 GiB (31-bit buffer offsets)");
        if ((long)p.B * p.LP >= (1L << 24) - 64) return pg_fail(PG_ERR_UNSUPPORTED, "wgrad: B*L must stay below 2^24");
        p.inv_LP = 1.0f / (float)p.LP;
    }
    // the dgrad epilogue reads the addend and the mask source through descriptors too, at 32-bit offsets b * bs + m * Ly + t
    // (conv_common.h, Epi): both are (B, M, Ly) views like dx, and a load past a truncated extent would return 0 without a word
    if ((p.add && !extent_bytes(p.B, p.add_bs, p.M, p.Ly)) || (p.ref && p.mask_mode && !extent_bytes(p.B, p.ref_bs, p.M, p.Ly)))
        return pg_fail(PG_ERR_SHAPE, "conv: dx_add / dx_ref exceeds 2 GiB (31-bit buffer offsets)");
    p.a_vec = p.w && (((long)p.Q * p.k) & 3) == 0 && ((uintptr_t)p.w & 15) == 0;
    return PG_OK;
}

// pg_conv_args.adam: the optimiser step of this weight in the wgrad epilogue (whole tiles: the GEMM kernel's; split tiles: the
// fixup kernel's -- every element of dW passes through exactly one epilogue_g)
int set_fused_adam(IgemmParams& p, const pg_conv_args* a) {
    const pg_adam_args* ad = a->adam;
    if (!ad) return PG_OK;
    if (!ad->p || !ad->m || !ad->v) return pg_fail(PG_ERR_NULL, "wgrad: fused adam needs p, m and v");
    if (ad->step < 1) return pg_fail(PG_ERR_SHAPE, "wgrad: fused adam: step is 1-based");
    if (ad->n != (int64_t)a->Cin * a->Cout * a->k) return pg_fail(PG_ERR_SHAPE, "wgrad: fused adam: n must equal Cin * Cout * k (p / m / v shaped like dw)");
    if (((uintptr_t)ad->p | (uintptr_t)ad->m | (uintptr_t)ad->v) & 3) return pg_fail(PG_ERR_ALIGN, "wgrad: fused adam: misaligned pointer");
    if ((const float*)ad->p == a->dw || ad->m == a->dw || ad->v == a->dw) return pg_fail(PG_ERR_SHAPE, "wgrad: fused adam: p / m / v alias dw");
    p.ad_p = ad->p; p.ad_m = ad->m; p.ad_v = ad->v;
    p.ad = pg_adam_scalars(ad);
    return PG_OK;
}

// The six fp32 entry points as GEMMs, indexed by PG_OP_*.  Geometry is always the forward op's (tr: nn.ConvTranspose1d).
// swap: M = Cin, Q = Cout and the B operand is dy; else M = Cout, Q = Cin and the B operand is x.
struct ConvOp { Kind kind; bool tr, swap; const char* null_msg; };
const ConvOp CONV_OPS[6] = {
    {KIND_F, false, false, "conv1d_fwd: x, w, y required"},      // nn.Conv1d forward
    {KIND_T, false, true, "conv1d_dgrad: dy, w, dx required"},   // dx[b,c,u] = sum_{o,j,t: s*t+j-p=u} w[o][c][j] dy[b,o,t]
    {KIND_G, false, false, "conv1d_wgrad: dy, x, dw required"},  // dw[o][c][j] = sum_{b,t} dy[b,o,t] act(x)[b,c,s*t+j-p]: P = dy
    {KIND_T, true, false, "convt1d_fwd: x, w, y required"},      // nn.ConvTranspose1d forward
    {KIND_F, true, true, "convt1d_dgrad: dy, w, dx required"},   // dx[b,c,i] = sum_{o,j} w[c][o][j] dy[b,o,s*i+j-p]
    {KIND_G, true, true, "convt1d_wgrad: dy, x, dw required"}};  // dw[c][o][j] = sum_{b,i} act(x)[b,c,i] dy[b,o,s*i+j-p]: P = x

// The plan of fp32 call `op`, after the entry point's checks in their order (ptrs: the tensors must be given).
int plan_conv(int op, const pg_conv_args* a, bool ptrs, ConvPlan& pl) {
    const ConvOp& o = CONV_OPS[op];
    if (int e = check_geom(a, o.tr)) return e;
    Knobs kn; if (int e = decode_knobs(a, kn)) return e;
    IgemmParams p = {};
    p.B = a->B; p.k = a->k; p.s = a->stride; p.p = a->pad;
    p.M = o.swap ? a->Cin : a->Cout; p.Q = o.swap ? a->Cout : a->Cin; p.Lx = o.swap ? a->Lout : a->Lin;
    const int lo = o.swap ? a->Lin : a->Lout;      // frames of the result (F / T) or of P (G)
    p.x = o.swap ? a->dy : a->x; p.x_bs = o.swap ? a->dy_bs : a->x_bs; p.act_x = o.swap ? PG_ACT_NONE : a->x_act;
    if (o.kind == KIND_G) {         // P: the other activation; the result is dW
        p.pt = o.swap ? a->x : a->dy; p.pt_bs = o.swap ? a->x_bs : a->dy_bs; p.act_p = o.swap ? a->x_act : PG_ACT_NONE;
        p.LP = lo; p.y = a->dw;
    } else if (o.swap) {            // dgrad: dx, plus the skip gradient, masked by the activation's derivative
        p.w = a->w; p.Ly = lo; p.y = a->dx; p.y_bs = a->dx_bs; p.y_slope = 1.0f; p.y2_slope = 1.0f;
        p.add = a->dx_add; p.add_bs = a->dx_add_bs; p.ref = a->dx_ref; p.ref_bs = a->dx_ref_bs;
        p.mask_mode = a->dx_ref ? a->dx_mask : 0;
    } else {                        // forward: y (and y2) stored through their activations
        p.w = a->w; p.Ly = lo; p.y = a->y; p.y_bs = a->y_bs; p.y_slope = pg_act_slope(a->y_act);
        p.y2 = a->y2; p.y2_bs = a->y2_bs; p.y2_slope = pg_act_slope(a->y2_act);
    }
    if (ptrs && (!p.x || !p.y || !(o.kind == KIND_G ? p.pt : p.w))) return pg_fail(PG_ERR_NULL, o.null_msg);
    long rows = p.M, cols = (long)p.B * p.Ly, K = (long)p.Q * p.k;
    if (o.kind == KIND_T) {
        // tau = s*u + phi - p >= 0 for some phi  <=>  u >= floor(p/s) at the latest; tau <= Ly-1 => u <= (Ly-1+p)/s
        p.u_off = p.p / p.s;
        p.U = (p.Ly - 1 + p.p) / p.s - p.u_off + 1;
        if (p.U <= 0) return pg_fail(PG_ERR_SHAPE, "convT: empty output");
        rows = (long)p.M * p.s; cols = (long)p.B * p.U; K = (long)p.Q * ((p.k + p.s - 1) / p.s);
    } else if (o.kind == KIND_G) {
        cols = (long)p.Q * p.k; K = (long)p.B * p.LP;
    }
    if (int e = set_extents(p)) return e;
    if (int e = o.kind == KIND_G ? set_fused_adam(p, a) : PG_OK) return e;
    p.ws = (float*)a->workspace;
    pl.kind = o.kind; pl.prec = kn.prec; pl.pack = 0;
    pl.has_tail = split_columns(o.kind, p, kn, rows, cols, K, a->workspace_bytes);
    if (pl.has_tail) {              // conv_raw3 over the full 256-wide tiles, the tall tile over the rest
        const long full = cols / RBN * RBN;
        if (int e = plan_part(FAM_RAW3, o.kind, kn, p, rows, 0, full, K, a->workspace_bytes, pl.main)) return e;
        return plan_part(FAM_RAW_TALL, o.kind, kn, p, rows, full, cols, K, a->workspace_bytes, pl.tail);
    }
    const Family fam = pick_family(o.kind, p, kn, rows, cols);
    if (int e = plan_part(fam, o.kind, kn, p, rows, 0, cols, K, a->workspace_bytes, pl.main)) return e;
    // fp32 raw-window wgrad: operands packed into the workspace first
    if ((pl.main.fam == FAM_G_RAW || pl.main.fam == FAM_G_PS) && kn.prec == 0 && (pl.pack = g_pack_layout(pl.main.p)) < 0)
        return pg_fail(PG_ERR_SHAPE, "wgrad: packed operand exceeds 2 GiB (31-bit buffer offsets)");
    return PG_OK;
}

// pg_conv_fwd_h's checks and descriptor up to the tiling: all of pg_conv_fwd_h_supported (ptrs: the tensors must be given)
int h3_params(const pg_convh_args* a, bool ptrs, IgemmParams& p, Knobs& kn) {
    if (!a) return pg_fail(PG_ERR_NULL, "conv_fwd_h: null args");
    if (a->B <= 0 || a->Cin <= 0 || a->Cout <= 0 || a->Lin <= 0 || a->Lout <= 0 || a->k <= 0 || a->stride <= 0 || a->pad < 0)
        return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: non-positive dimension");
    const bool tr = a->transposed != 0;
    const long lo = tr ? (long)(a->Lin - 1) * a->stride - 2L * a->pad + a->k : ((long)a->Lin + 2L * a->pad - a->k) / a->stride + 1;
    if (lo != a->Lout) return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: Lout inconsistent with Lin/k/stride/pad");
    if (ptrs && (!a->x || !a->w || (!a->y && !a->yh && !a->yh2))) return pg_fail(PG_ERR_NULL, "conv_fwd_h: x, w and at least one output required");
    if (((uintptr_t)a->x & 3) || ((uintptr_t)a->w & 15) || (a->x_bs & 1) || (a->x_pitch & 1))
        return pg_fail(PG_ERR_ALIGN, "conv_fwd_h: x must be 4-byte aligned with even pitch / batch stride, w 16-byte aligned");
    if (a->x_pitch <= a->Lin) return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: x_pitch must exceed Lin (zero tail of at least one element)");
    if ((a->yh && a->yh_pitch < a->Lout) || (a->yh2 && a->yh2_pitch < a->Lout)) return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: output pitch below Lout");
    pg_conv_args kb = {};
    kb.schedule = a->schedule;
    if (int e = decode_knobs(&kb, kn)) return e;
    p = {};
    p.x = reinterpret_cast<const float*>(a->x); p.x_bs = a->x_bs; p.x_pitch = a->x_pitch;
    p.w = reinterpret_cast<const float*>(a->w);
    p.y = a->y; p.y_bs = a->y_bs; p.y_slope = 1.0f; p.y2_slope = 1.0f;
    p.yh = a->yh; p.yh_bs = a->yh_bs; p.yh_pitch = a->yh_pitch; p.yh_slope = pg_act_slope(a->yh_act);
    p.yh2 = a->yh2; p.yh2_bs = a->yh2_bs; p.yh2_pitch = a->yh2_pitch; p.yh2_slope = pg_act_slope(a->yh2_act);
    p.B = a->B; p.Q = a->Cin; p.M = a->Cout; p.Lx = a->Lin; p.Ly = a->Lout; p.k = a->k; p.s = a->stride; p.p = a->pad;
    p.ws = (float*)a->workspace;
    const long xe = ((long)(p.B - 1) * p.x_bs + (long)p.Q * p.x_pitch) * 2;
    if (xe <= 0 || xe >= 0x7ffffff0L) return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: activation tensor exceeds 2 GiB (31-bit buffer offsets)");
    p.x_bytes = (unsigned)xe;
    const int kwp = tr ? pg_shadow_taps(p.k, p.s) : p.k;            // taps per (row, channel) of the weight shadow
    const long wbytes = (long)p.M * (tr ? p.s : 1) * p.Q * kwp * 2;
    if (wbytes >= 0x7ffffff0L) return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: weight shadow exceeds 2 GiB");
    p.w_bytes = (unsigned)wbytes;
    if (tr) {
        p.u_off = p.p / p.s;
        p.U = (p.Ly - 1 + p.p) / p.s - p.u_off + 1;
        if (p.U <= 0) return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: empty output");
    }
    // ONE tile family since 0.4: 256 x 256 on 4 waves, one workgroup per CU and one wave per SIMD (conv_h3.hip).  Round 3 measured it
    // level with or ahead of the 128 x 256 (conv_h.hip) and the eight-wave 128 x 512 / 256 x 256 tiles (conv_h2.hip) on all eight layers
    // inside the forward (6.44 ms against 6.55 / 6.73 / 6.88), so those were never reached automatically and have been removed.
    if (!pgconv::h_supported(tr ? KIND_T : KIND_F, p)) return pg_fail(PG_ERR_UNSUPPORTED, "conv_fwd_h: geometry not covered by the bf16-resident kernels (use the fp32-tensor entry points)");
    return PG_OK;
}

// the plan of a pg_conv_fwd_h call: one conv_h3 launch, K in slabs of 32
int plan_h3(const pg_convh_args* a, ConvPlan& pl) {
    Knobs kn;
    ConvPart& c = pl.main;
    IgemmParams& p = c.p;
    if (int e = h3_params(a, true, p, kn)) return e;
    const bool tr = a->transposed != 0;
    pl.kind = tr ? KIND_T : KIND_F; pl.prec = 0; pl.has_tail = false; pl.pack = 0; c.fam = FAM_H3;
    const long rows = tr ? (long)p.M * p.s : p.M, cols = (long)p.B * (tr ? p.U : p.Ly);
    p.tilesM = (int)((rows + 255) / 256);
    p.tilesN = (int)((cols + 255) / 256);
    p.tn_stride = 256;
    p.nslab = (int)((long)p.Q * (tr ? pg_shadow_taps(p.k, p.s) : p.k) / 32);
    c.tiles = (long)p.tilesM * p.tilesN;
    if (c.tiles <= 0 || c.tiles > 0x0fffffffL || p.nslab <= 0) return pg_fail(PG_ERR_SHAPE, "conv_fwd_h: empty or oversize grid");
    set_grid(c, kn, a->workspace_bytes);
    return PG_OK;
}

// The fixup of a part's split tiles: one instantiation per (wave tile and wave grid of the family's GEMM kernel, epilogue, form).
hipError_t launch_fixup(const ConvPlan& pl, const ConvPart& c, hipStream_t st) {
    typedef void (*Fn)(const IgemmParams, int);
#define FIX2(KIND, MB, NB, WN) {conv_fixup_kernel<KIND, MB, NB, WN, false>, conv_fixup_kernel<KIND, MB, NB, WN, true>}
    static const Fn table[4][4][2] = {      // [geometry][FixupKind][wide]
        {FIX2(FIX_F, WMB, 2, 2), FIX2(FIX_T, WMB, 2, 2), FIX2(FIX_G, WMB, 2, 2), {}},                       // im2col: 4 x 2 blocks, 2 x 2 waves
        {FIX2(FIX_F, 2, 4, 2), FIX2(FIX_T, 2, 4, 2), FIX2(FIX_G, 2, 4, 2), FIX2(FIX_T_PM, 2, 4, 2)},        // raw 128 x 256 (F / T / G): 2 x 4, 2 x 2
        {FIX2(FIX_F, 2, 4, 1), FIX2(FIX_T, 2, 4, 1), {}, FIX2(FIX_T_PM, 2, 4, 1)},                          // raw tall: 2 x 4, 4 x 1
        // one wave per SIMD: 8 x 2, 1 x 4 (conv_raw3 takes the plain form only, set_grid; conv_h3 has no phase-major rows)
        {FIX2(FIX_F, 8, 2, 4), FIX2(FIX_T, 8, 2, 4), {}, {conv_fixup_kernel<FIX_T_PM, 8, 2, 4, false>, nullptr}}};
#undef FIX2
    const int geom = c.fam == FAM_IM2COL ? 0 : (c.fam == FAM_RAW_TALL ? 2 : (c.fam == FAM_RAW3 || c.fam == FAM_H3 ? 3 : 1));
    // the stride-2 raw-window T kernels (conv_raw_impl.h, conv_raw3.hip) store phase-major rows
    const bool pm = pl.kind == KIND_T && c.p.s == 2 && (c.fam == FAM_RAW || c.fam == FAM_RAW_TALL || c.fam == FAM_RAW3);
    const bool wide = c.fixup == FIXUP_WIDE;
    const Fn fn = table[geom][pm ? FIX_T_PM : (int)pl.kind][wide];
    if (!fn) return hipErrorInvalidDeviceFunction;
    const long blocks = (c.tiles - c.p.whole) * (geom == 3 ? 16 : 8) * (wide ? 4 : 1);      // (tile, block of the wave tile [, GEMM wave])
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(NT), 0, st, c.p, c.grid);
    return hipGetLastError();
}

// The kernel of one part: named as rocprofv3 names it (profiles/*_kernel_stats.csv) into `name`, or, with name == NULL, launched
// and followed by the fixup of its split tiles.  One switch, so that a described plan names what runs.
hipError_t part_kernel(const ConvPlan& pl, const ConvPart& c, hipStream_t st, char* name = nullptr) {
    const IgemmParams& p = c.p;
    const Kind kind = pl.kind;
    const char* tk = kind == KIND_T ? "true" : "false";
    hipError_t e = hipSuccess;
    switch (c.fam) {
        case FAM_RAW_TALL:
            if (name) snprintf(name, 96, "conv_raw_kernel<%d, %d, %s, %d, 1>", p.k, p.s, tk, pl.prec);
            else e = pgconv::launch_raw_ft_tall(kind, p, c.grid, st, pl.prec);
            break;
        case FAM_RAW:
            if (name) snprintf(name, 96, "conv_raw_kernel<%d, %d, %s, %d, 2>", p.k, p.s, tk, pl.prec);
            else e = pgconv::launch_raw_ft(kind, p, c.grid, st, pl.prec);
            break;
        case FAM_G_RAW:
        case FAM_G_PS:          // (fp32: the launcher packs the operands first)
            if (name) snprintf(name, 96, "conv_g_%s_kernel<%d, %d, %d>", c.fam == FAM_G_PS ? "ps" : "raw", p.k, p.s, pl.prec);
            else e = pgconv::launch_raw_g(p, c.grid, st, pl.prec);
            break;
        case FAM_IM2COL:
            if (name) snprintf(name, 96, "conv_%c_kernel<0, 0, %d>", "ftg"[kind], pl.prec);
            else e = pgconv::launch_im2col(kind, p, c.grid, st, pl.prec);
            break;
        case FAM_RAW3:
            if (name) snprintf(name, 96, "conv_raw3_kernel<%d, %d, %s, %s>", p.k, p.s, tk, p.act_x == PG_ACT_NONE ? "false" : "true");
            else e = pgconv::launch_raw3(kind, p, c.grid, st);
            break;
        case FAM_H3:
            if (name) snprintf(name, 96, "conv_h3_kernel<%d, %d, %s>", kind == KIND_T && p.k == 5 ? 8 : p.k, p.s, tk);
            else e = pgconv::launch_h3(kind, p, c.grid, st);
            break;
    }
    if (!name && e == hipSuccess && c.fixup != FIXUP_NONE) e = launch_fixup(pl, c, st);
    return e;
}

// "kernel<template args>|grid=G|tiles=T|slabs=S|split=0/1|whole=W|fixup=none/plain/wide", and "|tail=kernel<...>,grid=G" after a
// column split
void describe(const ConvPlan& pl, char* buf, int buflen) {
    static const char* const fixup_name[] = {"none", "plain", "wide"};
    const ConvPart& c = pl.main;
    char name[96];
    (void)part_kernel(pl, c, nullptr, name);
    snprintf(buf, (size_t)buflen, "%s|grid=%d|tiles=%ld|slabs=%d|split=%d|whole=%d|fixup=%s", name, c.grid, c.tiles, c.p.nslab,
             (int)(c.fixup != FIXUP_NONE), c.p.whole, fixup_name[c.fixup]);
    if (!pl.has_tail) return;
    (void)part_kernel(pl, pl.tail, nullptr, name);
    const size_t n = strlen(buf);
    if (n + 7 < (size_t)buflen) snprintf(buf + n, (size_t)buflen - n, "|tail=%s,grid=%d", name, pl.tail.grid);
}

// Enqueues a plan: the packed wgrad operands (behind the workspace's stream-K region), the launch and its fixup, the tail launch.
int execute(ConvPlan& pl, long ws_bytes, hipStream_t st) {
    IgemmParams& p = pl.main.p;
    if (pl.pack) {
        if (!p.ws || ws_bytes < WS_STREAMK + pl.pack)
            return pg_fail(PG_ERR_WORKSPACE, "wgrad: the fp32 kernels need pg_workspace_bytes_wgrad() bytes of workspace (packed operands)");
        p.qk = reinterpret_cast<const float*>(reinterpret_cast<char*>(p.ws) + WS_STREAMK);
        p.pk = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.qk) + ((long)p.qk_bytes + 255) / 256 * 256);
    }
    hipError_t e = part_kernel(pl, pl.main, st);
    if (e == hipSuccess && pl.has_tail) e = part_kernel(pl, pl.tail, st);
    return e == hipSuccess ? PG_OK : pg_fail((int)e, hipGetErrorString(e));
}

int run_conv(int op, const pg_conv_args* a, void* stream) {
    ConvPlan pl;
    if (int e = plan_conv(op, a, true, pl)) return e;
    return execute(pl, a->workspace_bytes, (hipStream_t)stream);
}

}  // namespace

extern "C" int pg_conv1d_fwd(const pg_conv_args* a, void* stream) { return run_conv(PG_OP_CONV1D_FWD, a, stream); }
extern "C" int pg_conv1d_dgrad(const pg_conv_args* a, void* stream) { return run_conv(PG_OP_CONV1D_DGRAD, a, stream); }
extern "C" int pg_conv1d_wgrad(const pg_conv_args* a, void* stream) { return run_conv(PG_OP_CONV1D_WGRAD, a, stream); }
extern "C" int pg_convt1d_fwd(const pg_conv_args* a, void* stream) { return run_conv(PG_OP_CONVT1D_FWD, a, stream); }
extern "C" int pg_convt1d_dgrad(const pg_conv_args* a, void* stream) { return run_conv(PG_OP_CONVT1D_DGRAD, a, stream); }
extern "C" int pg_convt1d_wgrad(const pg_conv_args* a, void* stream) { return run_conv(PG_OP_CONVT1D_WGRAD, a, stream); }

// The launch plan of a conv call without launching it: "kernel<template args>|grid=..|tiles=..|slabs=..|split=0/1", the kernel
// named as rocprofv3 reports it.  Pure function of the arguments (same checks as the real call); bench.py uses it to group
// its per-launch timings by kernel so that its roofline numbers can be recomputed from profiles/*_kernel_stats.csv.
extern "C" int pg_conv_describe(const pg_conv_args* a, int32_t op, char* buf, int32_t buflen) {
    if (!buf || buflen < 128) return pg_fail(PG_ERR_NULL, "conv_describe: buf of >= 128 bytes required");
    buf[0] = 0;
    if (op < PG_OP_CONV1D_FWD || op > PG_OP_CONVT1D_WGRAD) return pg_fail(PG_ERR_UNSUPPORTED, "conv_describe: op must be a PG_OP_* value");
    ConvPlan pl;
    const int e = plan_conv(op, a, true, pl);
    if (e == PG_OK) describe(pl, buf, buflen);
    return e;
}

// ---- bf16-resident forward (conv_h3.hip) ----------------------------------------------------------------------------------
extern "C" int pg_conv_fwd_h(const pg_convh_args* a, void* stream) {
    ConvPlan pl;
    if (int e = plan_h3(a, pl)) return e;
    return execute(pl, a->workspace_bytes, (hipStream_t)stream);
}
// 1 if pg_conv_fwd_h covers this geometry (sizes, strides and pitches of `a`; pointers may be NULL), else 0: pure host check
extern "C" int pg_conv_fwd_h_supported(const pg_convh_args* a) {
    IgemmParams p; Knobs kn;
    return h3_params(a, false, p, kn) == PG_OK ? 1 : 0;
}
// launch plan of a pg_conv_fwd_h call without launching it (as pg_conv_describe; pointers must be non-NULL, they are not read)
extern "C" int pg_conv_fwd_h_describe(const pg_convh_args* a, char* buf, int32_t buflen) {
    if (!buf || buflen < 128) return pg_fail(PG_ERR_NULL, "conv_fwd_h_describe: buf of >= 128 bytes required");
    buf[0] = 0;
    ConvPlan pl;
    const int e = plan_h3(a, pl);
    if (e == PG_OK) describe(pl, buf, buflen);
    return e;
}

// Workspace a caller should hand to the conv entry points (pg_conv_args.workspace) so that badly quantised tile counts
// can be balanced over all CUs (stream-K).  Without it every call falls back to one-tile-per-workgroup scheduling.
extern "C" int64_t pg_workspace_bytes_conv(void) { return (int64_t)WS_STREAMK; }
// Workspace of one wgrad call: the stream-K region plus, behind it, the operands the fp32 raw-window kernels pack (pure host function
// of the geometry, precision and schedule; pointers are not read).  Negative: the call's error code.
extern "C" int64_t pg_workspace_bytes_wgrad(const pg_conv_args* a, int32_t op) {
    if (op != PG_OP_CONV1D_WGRAD && op != PG_OP_CONVT1D_WGRAD)
        return pg_fail(PG_ERR_UNSUPPORTED, "workspace_bytes_wgrad: op must be PG_OP_CONV1D_WGRAD or PG_OP_CONVT1D_WGRAD");
    ConvPlan pl;
    const int e = plan_conv(op, a, false, pl);
    return e != PG_OK ? (int64_t)e : (int64_t)(WS_STREAMK + pl.pack);
}
