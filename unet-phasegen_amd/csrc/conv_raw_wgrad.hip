// conv_raw_wgrad.hip -- raw-window variant of the G (wgrad) kernel.
#include "conv_common.h"

namespace {

// ----------------------------------------------------------------------------------------------------------------
// dW[m][(q,j)] = sum_{k=(b,i)} P[b,m,i] * Q[b,q,s*i+j-p], tile 128 (m) x 256
// ((q,j) columns = 256/k whole channels; k = 5: 51 channels = 255 columns, the 256th is idle and column tiles are 255 apart).  Per slab of 16 consecutive (b,i) the columns of one channel are k shifted
// views of the SAME piece of Q's row: positions s*i0 - p + [0, 15 s + k).  That window is staged once per channel
// (LDS image [sub][channel][WLP], sub 1 only filled when the slab runs over the end of sample b into b+1) and the
// B fragment of column (q,j), slab element kl is read at  q*WLP + j + s*kl  (+ a wave-uniform shift for kl past the
// sample boundary).  For k = 32 that is 6.4x fewer bytes than the im2col tile.
//
// Four slab loops -- the K axis flat (g_raw_*) or in per-sample slabs (g_ps_*), on the caller's tensors (*_bf: the bf16 / bf16x3
// modes) or on packed copies (*_f32) -- built from ONE set of parts.  A loop states what is its own: its constants, its per-tile
// gather offsets, how a slab is gathered (ISSUE) and which fix-ups its fragments need (FRAGS).  Tile decode, fragment reads,
// activation, MFMA block, double-buffer skeleton and finish exist once, below.  The parts are macros, as the body of conv_im2col.hip:
// as __forceinline__ functions (fragment read, MFMA block, or a slab-source policy class around one loop template) hipcc schedules
// the slab loop of most instantiations differently; as macros all of them keep their instruction stream.
// ----------------------------------------------------------------------------------------------------------------
template <int KW, int S> struct GRaw {
    static constexpr int WL = 15 * S + KW;                                   // window floats actually read
    static constexpr int WLP = g_wlp(KW, S);                                 // padded; keeps reads conflict-free
    static constexpr int NQT = RBN / KW;                                      // whole channels per tile (k = 5: 51, one idle column)
    static constexpr int TNV = NQT * KW;                                      // columns of a tile that exist; also the tile pitch in N
    static constexpr int SUB = NQT * WLP;                                     // floats per sub-window set
    static constexpr int SUBS = (SUB + 63) / 64 * 64;                         // its slot: a dword gather instruction writes 64 floats,
                                                                              //   also from lanes past SUB (k = 5: 1836 -> 1856)
    static constexpr int NE = (SUB + NT - 1) / NT;                            // gather pieces per thread and sub-window
    static constexpr int SUBP = (SUB + 255) / 256 * 256;                      // its slot in whole 16-byte wave instructions
    // window inside the row (the common case): the whole window set of the tile loads as 16-byte pieces -- piece pc =
    // floats [4 pc, 4 pc + 4) of the [channel][WLP] image (WLP is a multiple of 4, so a piece never straddles channels;
    // the source only needs dword alignment): SUB / 4 pieces = 2 wave instructions for k = 32 instead of 8
    static constexpr int NE16 = (SUB / 4 + NT - 1) / NT;
    // floats per LDS stage: the flat-K loops keep two sub-window slots (dword gathers: SUBS; packed: SUBP), per-sample slabs one
    static constexpr int STG_FLAT_BF = RTILE_A + 2 * SUBS, STG_FLAT_F32 = RTILE_A + 2 * SUBP, STG_PS = RTILE_A + SUBP;
    static_assert(WL <= WLP, "window does not fit its slot");
    static_assert(WLP % 4 == 0 && WLP <= 64, "16-byte window pieces; channel 0 inside the first 64 floats");
    static_assert(2 * STG_FLAT_F32 * 4 <= 64 * 1024, "LDS budget");
};

// ---- the shared parts --------------------------------------------------------------------------------------------------------------
// workgroup: its LDS stages and thread coordinates
#define G_HEAD(STG)                                                                                       \
    __shared__ __attribute__((aligned(16))) float lds[2 * (STG)];                                         \
    const int tid = threadIdx.x, lane = tid & 63;                                                         \
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wv >> 1, wn = wv & 1;

// tile: its first row, first column and first window channel
#define G_TILE                                                                                            \
    const int m0 = (tile / p.tilesN) * RBM, n0 = (tile % p.tilesN) * C::TNV;                              \
    const int qbase = (tile % p.tilesN) * C::NQT;

// A thread's two 16-byte pieces of the P tile, rows of PITCH floats: 16 consecutive frames of a row are contiguous (16-byte LDS-DMA
// only needs dword alignment, tools/probe/ldsdma16.hip), the (sample, frame) of the slab is wave-uniform and rides in the SGPR offset.
#define G_A_PIECES(PITCH)                                                                                 \
    _Pragma("unroll") for (int e = 0; e < 2; ++e) {                                                       \
        const int m = m0 + dma16_row(lane, wv, e);                                                        \
        pv[e] = m < p.M ? (m * (PITCH) + dma16_kc(lane)) * 4 : FAR;                                       \
    }

// fragment base of this lane's 4 columns (MORE: what else a loop keeps per column), accumulators
#define G_FRAG_BASE_ACC(MORE)                                                                             \
    int bbase[4];                                                                                         \
    _Pragma("unroll") for (int jb = 0; jb < 4; ++jb) {                                                    \
        const int c = wn * 128 + jb * 32 + (lane & 31), qc = c / KW;                                      \
        bbase[jb] = qc * C::WLP + (c - qc * KW) + S * 8 * (lane >> 5);                                    \
        MORE                                                                                              \
    }                                                                                                     \
    AccR acc;                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j)           \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) acc.c[i][j][r] = 0.f;

// Fragments of an interior slab, read order = use order (the MFMAs run kk-major): with the operands of kk = 0, 1 first the first
// MFMA waits for 6 of the 20 fragment reads instead of 17 (hipcc keeps source order; it had sorted them operand by operand).  + 0.4 %
// on the k = 32 layers, + 0.8-1.3 % on the k = 8 ones.  (Round 4 also tried, on the flat-K loop: the CU's second workgroup
// started ~2000 cycles late, or at a higher wave priority, to break the lockstep of the two; the next slab's gathers
// issued one per 8 MFMAs instead of at the slab's start -- all neutral.  What the in-loop gathers cost as a whole:
// without them (-DPG_G_ABL=1, wrong results) 94 % of the pipe against 88 %; a sample end inside a slab, 1 slab in 8
// at 129 frames, costs under 2 of those points (warm: 128 frames 88.2 %, 129 frames 86.5 %), and a K order without such
// slabs -- whole slabs per sample, then "leftover" slabs of one frame of 16 samples -- measured equal: tools/dbg/wgrad_frames.py.)
#define G_READ_INTERIOR                                                                                   \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) a[i][0] = *reinterpret_cast<const f32x4*>(ap + i * 32 * BK + (((2 * h) ^ sw) << 2)); \
    _Pragma("unroll") for (int ip = 0; ip < 4; ++ip) {                                                    \
        if (ip == 2) {                                                                                    \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) a[i][1] = *reinterpret_cast<const f32x4*>(ap + i * 32 * BK + (((2 * h + 1) ^ sw) << 2)); \
        }                                                                                                 \
        _Pragma("unroll") for (int jb = 0; jb < 4; ++jb) { b[jb][2 * ip] = Bw[bbase[jb] + S * 2 * ip]; b[jb][2 * ip + 1] = Bw[bbase[jb] + S * (2 * ip + 1)]; } \
    }

// Fragments of a flat-K slab: interior, or running over a sample end at element kc_cur -- elements kl >= kc_cur live in the second
// sub-window (SLOT floats behind the first), which starts at frame 0 of the next sample.  (Volatile reads: otherwise hipcc sinks the
// loads of both paths into one tail with per-element selected addresses, which cost the common path 60 VALU and left its 32 reads
// unpaired.)
#define G_READ_FLAT(SLOT)                                                                                 \
    if (kc_cur >= 16) {                                                                                   \
        G_READ_INTERIOR                                                                                   \
    } else {                                                                                              \
        _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                     \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) a[i][c] = *reinterpret_cast<const f32x4*>(ap + i * 32 * BK + (((2 * h + c) ^ sw) << 2)); \
        typedef const volatile __attribute__((address_space(3))) float* lds_vptr;                         \
        const lds_vptr Bv = (lds_vptr)Bw;                                                                 \
        const int shift = (SLOT) - S * kc_cur;                                                            \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                   \
            const int d = (8 * h + i >= kc_cur) ? shift : 0;                                              \
            _Pragma("unroll") for (int jb = 0; jb < 4; ++jb) b[jb][i] = Bv[bbase[jb] + S * i + d];        \
        }                                                                                                 \
    }

// the operands' activations on the fragments (the loops on the caller's tensors; the packed copies hold activated values)
#define G_ACT                                                                                             \
    if (slopeA != 1.0f) {                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int c = 0; c < 2; ++c)       \
            _Pragma("unroll") for (int v = 0; v < 4; ++v) a[i][c][v] = pg_act_apply(a[i][c][v], slopeA);  \
    }                                                                                                     \
    if (slopeB != 1.0f) {                                                                                 \
        _Pragma("unroll") for (int jb = 0; jb < 4; ++jb)                                                  \
            _Pragma("unroll") for (int i = 0; i < 8; ++i) b[jb][i] = pg_act_apply(b[jb][i], slopeB);      \
    }

// 64 fp32 MFMAs, kk-major (k pair kk of all eight blocks before pair kk + 1), or the bf16 / bf16x3 block
#define G_MFMA(BF)                                                                                        \
    if (BF) mfma_low_2x4<BF>(a, b, acc);                                                                  \
    else {                                                                                                \
        _Pragma("unroll") for (int kk = 0; kk < 8; ++kk)                                                  \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j)   \
                acc.c[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][kk >> 2][kk & 3], b[j][kk], acc.c[i][j], 0, 0, 0); \
    }

#if defined(PG_G_ABL) && PG_G_ABL == 1      /* dev ablation (wrong results): no gathers inside the loop */
#define G_ISSUE_NEXT(STG, ISSUE, SKIP) SKIP
#else
#define G_ISSUE_NEXT(STG, ISSUE, SKIP) ISSUE(lds + (cur ^ 1) * (STG), (sl + 1) * BK)
#endif
#if defined(PG_G_ABL) && PG_G_ABL == 2      /* dev ablation (wrong results): the barrier does not wait for the gathers */
#define G_BARRIER asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#else
#define G_BARRIER __syncthreads();
#endif

// Slabs [sb, se) of a tile, double-buffered: issue the gathers of slab sl + 1 (one slab ahead), fence, read the fragments of slab
// sl and multiply, fence, barrier.  The only wait is the one the barrier carries, behind the slab's MFMAs.  A loop gives:
//   ISSUE(stage, k0)  gathers a slab into a stage and moves the loop's gather position on; SKIP stands in for it under PG_G_ABL=1
//   PRIMED            after the first slab is in flight; ADVANCE: after a slab is multiplied
//   FRAGS             fills a[2][2] / b[4][8] from As / Bw (ap, r, h, sw: this lane's row pointer and swizzle)
#define G_SLAB_LOOP(STG, BF, ISSUE, SKIP, PRIMED, FRAGS, ADVANCE)                                         \
    PG_STAMP_DECL                                                                                         \
    ISSUE(lds, sb * BK)                                                                                   \
    PRIMED                                                                                                \
    __syncthreads();                                                                                      \
    for (int sl = sb; sl < se; ++sl) {                                                                    \
        const int cur = (sl - sb) & 1;                                                                    \
        PG_STAMP(0)                                                                                       \
        G_ISSUE_NEXT(STG, ISSUE, SKIP)                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        PG_STAMP(1)                                                                                       \
        {   const float* As = lds + cur * (STG);                                                          \
            const float* Bw = As + RTILE_A;                                                               \
            const int r = lane & 31, h = lane >> 5, sw = (r >> 2) & 3;                                    \
            const float* ap = As + (wm * 64 + r) * BK;                                                    \
            f32x4 a[2][2];                                                                                \
            float b[4][8];                                                                                \
            FRAGS                                                                                         \
            G_MFMA(BF)                                                                                    \
        }                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        PG_STAMP(2)                                                                                       \
        ADVANCE                                                                                           \
        G_BARRIER                                                                                         \
        PG_STAMP(3)                                                                                       \
    }                                                                                                     \
    PG_STAMP_FLUSH

// a whole tile goes through the epilogue, a segment of one into slot (G, SLOT) of the workspace
#define G_FINISH(G, SLOT)                                                                                 \
    if (sb == 0 && se == p.nslab) epilogue_g<S, 2, 4>(p, acc, m0, n0, lane, wm, wn, n0 + C::TNV);         \
    else store_partial(p.ws, G, SLOT, acc, tid);

// flat K: wave-uniform (sample, frame) of the slab being GATHERED, and the first slab element that belongs to the next sample
// (16 = none) of the slab being multiplied / gathered
#define G_FLAT_START                                                                                      \
    int gb, gi;                                                                                           \
    { const int k0 = sb * BK; gb = k0 / p.LP; gi = k0 - gb * p.LP; }                                      \
    int kc_cur = 16, kc_next;
#define G_FLAT_ISSUED      kc_next = kc < 16 ? kc : 16; gi += BK; if (gi >= p.LP) { gi -= p.LP; ++gb; }
#define G_FLAT_SKIP        kc_next = 16;
#define G_FLAT_ADVANCE     kc_cur = kc_next;
// per-sample slabs: a slab's (sample, chunk of 16 frames) moves on
#define G_PS_NEXT(B_, C_)  if (++C_ == cps) { C_ = 0; ++B_; }
#define G_NOTHING

// ---- flat K, the caller's tensors ----------------------------------------------------------------------------------------------
// bf16 / bf16x3 modes (BF = 1, 2), with the per-slab fix-ups (sample ends, windows that leave the row, activations) in the loop.
template <int KW, int S, int BF>
__device__ __forceinline__ void g_raw_bf(const IgemmParams& p) {
    using C = GRaw<KW, S>;
    G_HEAD(C::STG_FLAT_BF)
    const int kt = dma_kt(lane, wv);
    const rsrc_t rp = make_rsrc(p.pt, p.pt_bytes), rx = make_rsrc(p.x, p.x_bytes);
    const float slopeA = pg_act_slope(p.act_p), slopeB = pg_act_slope(p.act_x);
    const int pbs4 = (int)p.pt_bs * 4, xbs4 = (int)p.x_bs * 4;
    Walk wk(p);
    while (wk.more()) {
        int tile, sb, se;
        wk.segment(p, tile, sb, se);
        G_TILE

        int aoff[8];                                   // P[b][m][i]: byte offset of row m (this thread's k column added per slab)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int m = m0 + dma_row(lane, wv, e);
            aoff[e] = m < p.M ? m * p.LP * 4 : FAR;
        }
        // window element idx = tid + NT e owned by this thread on the general (per-element) path: channel byte offset and v - pad,
        // held in registers -- short samples (30 frames: every other slab runs over a sample boundary) take that path often.  Only
        // the bf16-mode k = 4 / k = 5 kernels, which would spill, recompute them where used (RECOMP; the opaque copy of tid keeps the
        // compiler from hoisting the values out of the slab loop again).
        constexpr bool RECOMP = KW <= 5 && BF != 0;
        int choff[RECOMP ? 1 : C::NE], vv[RECOMP ? 1 : C::NE];
        if (!RECOMP) {
#pragma unroll
            for (int e = 0; e < C::NE; ++e) {
                const int idx = tid + NT * e, ql = idx / C::WLP, v = idx - ql * C::WLP;
                choff[e] = (idx < C::SUB && qbase + ql < p.Q) ? (qbase + ql) * p.Lx * 4 : FAR;
                vv[e] = v - p.p;
            }
        }
#define GRAW_CHOFF(e) (RECOMP ? ({ int t_ = tid; asm volatile("" : "+v"(t_)); const int idx_ = t_ + NT * (e), ql_ = idx_ / C::WLP; \
                                  (idx_ < C::SUB && qbase + ql_ < p.Q) ? (qbase + ql_) * p.Lx * 4 : FAR; }) : choff[RECOMP ? 0 : (e)])
#define GRAW_VV(e) (RECOMP ? ({ int t_ = tid; asm volatile("" : "+v"(t_)); const int idx_ = t_ + NT * (e); idx_ - (idx_ / C::WLP) * C::WLP - p.p; }) \
                           : vv[RECOMP ? 0 : (e)])
        // Slabs that lie inside one sample (all but one in LP/16) read the P tile as 16-byte pieces (G_A_PIECES) and, where the
        // window lies inside the row, the windows too (GRaw::NE16).  Enabled where registers allow.
        constexpr bool FASTP = BF != 2 && !(KW <= 5 && BF != 0);   // (the bf16-mode k = 4 / k = 5 kernels are at the register limit)
        constexpr bool FASTW = FASTP && KW != 4;          // SGPR-offset window gathers: k = 4 has 9 pieces per thread, their offsets spill
        int pv[FASTP ? 2 : 1], woff[FASTW ? C::NE16 : 1];
        if (FASTW) {
#pragma unroll
            for (int e = 0; e < C::NE16; ++e) {
                const int f = 4 * (tid + NT * e), ql = f / C::WLP, v0 = f - ql * C::WLP;
                woff[e] = (f < C::SUB && qbase + ql < p.Q) ? ((qbase + ql) * p.Lx + v0) * 4 : FAR;
            }
        }
        if (FASTP) { G_A_PIECES(p.LP) }
        G_FRAG_BASE_ACC(G_NOTHING)
        G_FLAT_START

#define GRAW_ISSUE(STAGE_PTR, K0)                                                                         \
    {   float* const As = (STAGE_PTR) + wv * 64; float* const Bw = (STAGE_PTR) + RTILE_A + wv * 64;       \
        const int k0 = (K0);                                                                              \
        const int kc = p.LP - gi;                      /* elements of this slab left in sample gb */      \
        if (FASTP && kc >= 16 && gb < p.B) {                                                              \
            const int sa = gb * pbs4 + gi * 4;                                                            \
            _Pragma("unroll") for (int e = 0; e < 2; ++e) dma16s(rp, As + wv * 192 + e * 1024, pv[FASTP ? e : 0], sa); \
        } else {                                                                                          \
          int bb, ii; divmod24(k0 + kt, p.LP, p.inv_LP, bb, ii);                                          \
          const int po = bb < p.B ? bb * pbs4 + ii * 4 : OOB;                                             \
          _Pragma("unroll") for (int e = 0; e < 8; ++e) dma4(rp, As + e * 256, aoff[e] + po); }           \
        const int w0 = S * gi - p.p;                   /* memory position of window element 0 */          \
        if (FASTW && kc >= 16 && gb < p.B && w0 >= 0 && w0 + C::WLP <= p.Lx) {   /* window inside the row: no per-lane checks */ \
            const int sw_ = gb * xbs4 + w0 * 4;                                                           \
            _Pragma("unroll") for (int e = 0; e < C::NE16; ++e)                                           \
                if (4 * (e * NT + wv * 64) < C::SUB) dma16s(rx, (STAGE_PTR) + RTILE_A + 4 * (e * NT + wv * 64), woff[FASTW ? e : 0], sw_); \
        } else {                                                                                          \
        const int sb0 = gb < p.B ? gb * xbs4 : -NEVER, sb1 = (kc < 16 && gb + 1 < p.B) ? (gb + 1) * xbs4 : -NEVER; \
        _Pragma("unroll") for (int e = 0; e < C::NE; ++e) {                                               \
            if ((e + 1) * NT <= C::SUB || e * NT + wv * 64 < C::SUB) {                                    \
                const int ps = S * gi + GRAW_VV(e);                                                       \
                dma4(rx, Bw + e * NT, ((unsigned)ps < (unsigned)p.Lx && sb0 >= 0) ? sb0 + GRAW_CHOFF(e) + ps * 4 : FAR); \
            }                                                                                             \
        }                                                                                                 \
        if (kc < 16) {                                 /* slab runs into the next sample: second sub-window */ \
            _Pragma("unroll") for (int e = 0; e < C::NE; ++e) {                                           \
                if ((e + 1) * NT <= C::SUB || e * NT + wv * 64 < C::SUB) {                                                          \
                    const int ps = GRAW_VV(e);                                                            \
                    dma4(rx, Bw + C::SUBS + e * NT, ((unsigned)ps < (unsigned)p.Lx && sb1 >= 0) ? sb1 + GRAW_CHOFF(e) + ps * 4 : FAR); \
                }                                                                                         \
            }                                                                                             \
        }                                                                                                 \
        }                                                                                                 \
        G_FLAT_ISSUED                                                                                     \
    }
#define GRAW_FRAGS G_READ_FLAT(C::SUBS) G_ACT
        G_SLAB_LOOP(C::STG_FLAT_BF, BF, GRAW_ISSUE, G_FLAT_SKIP, G_FLAT_ADVANCE, GRAW_FRAGS, G_FLAT_ADVANCE)
#undef GRAW_FRAGS
#undef GRAW_ISSUE
#undef GRAW_CHOFF
#undef GRAW_VV
        G_FINISH(wk.g, wk.slot)
        wk.next(se - sb);
    }
}

// ----------------------------------------------------------------------------------------------------------------
// Per-sample slabs (round 3): the variant for SHORT samples (the loop below serves the bf16 modes; fp32: g_ps_f32 further down).  On the flat K axis,
// with 30 frames per sample every other slab runs over a sample boundary, and almost every remaining one has its window partly
// outside the row, so the 2 + 2 wide gathers of the fast path are the exception and 8 + 2 x 8 dword gathers (~2400 issue cycles
// beside 4096 of MFMA) the rule: 62-69 % of the fp32 pipe at the U-Net's bottleneck.  Here a slab is 16 consecutive frames of ONE
// sample, the last slab of a sample padded (K = B * ceil(LP / 16) * 16: + 6.7 % MFMA work at 30 frames, + 4.9 % at 61, + 1.6 % at
// 126; the host only takes this kernel where that is <= 7 %).  Then EVERY slab gathers with the wide pieces and no range checks:
//   P tile:   frames gi .. gi + 15 of the rows, 16-byte pieces (frames past LP are the next row's: the A fragments of k >= LP - gi
//             are zeroed in registers, one wave-uniform branch per slab);
//   windows:  positions s gi - p + [0, WLP) of every channel as 16-byte pieces; positions outside [0, Lx) hold a neighbouring
//             row's values (or zeros past the tensor): on slabs whose window leaves the row -- wave-uniform -- the B fragment
//             elements are range-checked and zeroed in registers (64 VALU beside 64 MFMAs).
// Zeroing is a select, not a product: every operand that reaches the matrix pipe is real data or 0.  The only gather whose
// offset could become negative -- channel 0's first pieces, p positions in front of the tensor's first row -- is dropped from
// the wide gathers and re-loaded element-wise by ONE extra dword instruction of wave 0 (tiles with qbase == 0 only).
// ----------------------------------------------------------------------------------------------------------------
template <int KW, int S, int BF>
__device__ __forceinline__ void g_ps_bf(const IgemmParams& p) {
    using C = GRaw<KW, S>;
    G_HEAD(C::STG_PS)
    const rsrc_t rp = make_rsrc(p.pt, p.pt_bytes), rx = make_rsrc(p.x, p.x_bytes);
    const float slopeA = pg_act_slope(p.act_p), slopeB = pg_act_slope(p.act_x);
    const int pbs4 = (int)p.pt_bs * 4, xbs4 = (int)p.x_bs * 4;
    const int cps = (p.LP + 15) >> 4;                                  // slabs (chunks of 16 frames) per sample
    Walk wk(p);
    while (wk.more()) {
        int tile, sb, se;
        wk.segment(p, tile, sb, se);
        G_TILE

        int pv[2], woff[C::NE16];
        G_A_PIECES(p.LP)
#pragma unroll
        for (int e = 0; e < C::NE16; ++e) {
            const int f = 4 * (tid + NT * e), ql = f / C::WLP, v0 = f - ql * C::WLP;
            const int off = ((qbase + ql) * p.Lx + v0 - p.p) * 4;         // >= 0 except for channel 0's pieces in front of the tensor
            woff[e] = (f < C::SUB && qbase + ql < p.Q && off >= 0) ? off : FAR;
        }
        // wave 0's element-wise reload of the first 64 floats of the image (channel 0 and the start of channel 1) on tiles that hold channel 0
        const bool fix0 = qbase == 0 && wv == 0;
        int f0_off, f0_v;
        { const int ql = lane / C::WLP, v = lane - ql * C::WLP; f0_off = ql < p.Q ? ql * p.Lx * 4 : FAR; f0_v = v - p.p; }
        int pj[4];                                     // window position of this lane's 4 columns at slab element 0
#define GPS_PJ pj[jb] = (c - qc * KW) + S * 8 * (lane >> 5) - p.p;
        G_FRAG_BASE_ACC(GPS_PJ)
#undef GPS_PJ

        int gb = sb / cps, gc = sb - gb * cps;          // (sample, chunk) of the slab being GATHERED (one ahead of the multiplied one)
        int mc = gc;                                    // chunk of the slab being MULTIPLIED
#define GPS_ISSUE(STAGE_PTR, K0)                                                                          \
    {   float* const As = (STAGE_PTR) + wv * 64;                                                          \
        if (gb < p.B) {                                                                                   \
            const int gi = gc << 4;                                                                       \
            const int sa = gb * pbs4 + gi * 4;                                                            \
            _Pragma("unroll") for (int e = 0; e < 2; ++e) dma16s(rp, As + wv * 192 + e * 1024, pv[e], sa); \
            const int sw_ = gb * xbs4 + S * gi * 4;                                                       \
            _Pragma("unroll") for (int e = 0; e < C::NE16; ++e)                                           \
                if (4 * (e * NT + wv * 64) < C::SUB) dma16s(rx, (STAGE_PTR) + RTILE_A + 4 * (e * NT + wv * 64), woff[e], sw_); \
            if (fix0) {                                                                                   \
                const int ps = S * gi + f0_v;                                                             \
                dma4(rx, (STAGE_PTR) + RTILE_A, (unsigned)ps < (unsigned)p.Lx ? gb * xbs4 + f0_off + ps * 4 : FAR); \
            }                                                                                             \
        }                                                                                                 \
        G_PS_NEXT(gb, gc)                                                                                 \
    }
#define GPS_FRAGS                                                                                         \
    const int gi = mc << 4, kc = p.LP - gi;              /* valid frames of this slab (>= 16: all) */     \
    const int w0 = S * gi;                               /* window element v sits at row position w0 + v - p */ \
    G_READ_INTERIOR                                                                                       \
    if (kc < 16) {                          /* the sample's last, padded slab: frames past LP are not this row's */ \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int c = 0; c < 2; ++c)       \
            _Pragma("unroll") for (int v = 0; v < 4; ++v) a[i][c][v] = (8 * h + 4 * c + v < kc) ? a[i][c][v] : 0.f; \
    }                                                                                                     \
    if (w0 < p.p || w0 - p.p + C::WLP > p.Lx) {   /* the window leaves the row: zero what lies outside [0, Lx) */ \
        _Pragma("unroll") for (int jb = 0; jb < 4; ++jb)                                                  \
            _Pragma("unroll") for (int i = 0; i < 8; ++i) b[jb][i] = (unsigned)(w0 + pj[jb] + S * i) < (unsigned)p.Lx ? b[jb][i] : 0.f; \
    }                                                                                                     \
    G_ACT
#define GPS_ADVANCE if (++mc == cps) mc = 0;
        G_SLAB_LOOP(C::STG_PS, BF, GPS_ISSUE, G_NOTHING, G_NOTHING, GPS_FRAGS, GPS_ADVANCE)
#undef GPS_ADVANCE
#undef GPS_FRAGS
#undef GPS_ISSUE
        G_FINISH(wk.g, wk.slot)
        wk.next(se - sb);
    }
}

// ----------------------------------------------------------------------------------------------------------------
// fp32 slab loops on PACKED operands (round 5).  The launcher first copies both operands into the caller's workspace (pack_g
// below; IgemmParams.qk / .pk) in layouts where every slab is gathered and read by one fixed instruction sequence:
//   Q rows [b][q][Lq] with zero halos: position t of a row at index p + t, zeros in front and behind as far as any slab's window
//     reaches -- a window is always whole 16-byte pieces of ONE row: no range check, no neighbouring row's values, no channel-0
//     special case, no branch on where it lies;
//   P flat-K [m][(b, i)] (conv_g_raw: the A tile of a slab is the same two 16-byte pieces per thread also where the slab runs over a
//     sample end) or per sample [b][m][16 ceil(LP / 16)] (conv_g_ps: frames past LP are zeros in memory, not in registers);
//   the activations (act_x, act_p) applied once there, not on every fragment.
// What is left per slab: 2 A pieces and the window pieces, their slab advance in the SGPR offset; the fragment reads in use order;
// 64 MFMAs; one barrier.  The flat-K loop keeps ONE wave-uniform branch, between interior slabs and the slab that runs into the next
// sample (1 in 8 at 129 frames), whose elements past the sample end read the second sub-window (frame 0 of sample b + 1).  Both
// sub-windows are gathered on every slab (on interior ones the second is a copy of the first, L2 hits): waves 0-1 carry the first,
// waves 2-3 the second at k = 32, so every wave issues 3 pieces per slab.  Same k pairs per MFMA and the same MFMA order along K as
// the loop with in-loop fix-ups, and the packed zeros are the values that loop selected: results are bit-identical.
// ----------------------------------------------------------------------------------------------------------------
template <int KW, int S>
__device__ __forceinline__ void g_raw_f32(const IgemmParams& p) {
    using C = GRaw<KW, S>;
    constexpr int NP = 2 * C::SUBP / 4;                 // 16-byte pieces of both sub-window slots (a multiple of 64: wave-uniform sub)
    constexpr int NE2 = (NP + NT - 1) / NT;
    G_HEAD(C::STG_FLAT_F32)
    const rsrc_t rp = make_rsrc(p.pk, p.pk_bytes), rx = make_rsrc(p.qk, p.qk_bytes);
    const int qbs4 = p.qk_bs * 4, klast4 = (p.nslab - 1) * BK * 4;
    Walk wk(p);
    while (wk.more()) {
        int tile, sb, se;
        wk.segment(p, tile, sb, se);
        G_TILE
        int pv[2], woff[NE2];
        G_A_PIECES(p.Kp)
#pragma unroll
        for (int e = 0; e < NE2; ++e) {     // piece pc: sub-window pc / (SUBP / 4), floats [f, f + 4) of its [channel][WLP] image
            const int pc = tid + NT * e, sub = pc >= C::SUBP / 4 ? 1 : 0, f = 4 * pc - sub * C::SUBP, ql = f / C::WLP, v0 = f - ql * C::WLP;
            woff[e] = (f < C::SUB && qbase + ql < p.Q) ? ((qbase + ql) * p.Lq + v0) * 4 : FAR;
        }
        G_FRAG_BASE_ACC(G_NOTHING)
        // The prefetch behind the range's last slab may lie past K: its offsets are clamped into the operands (that stage is never multiplied).
        G_FLAT_START
#define GRF_ISSUE(STAGE_PTR, K0)                                                                          \
    {   const int sa = min((K0) * 4, klast4);                                                             \
        _Pragma("unroll") for (int e = 0; e < 2; ++e) dma16s(rp, (STAGE_PTR) + wv * 256 + e * 1024, pv[e], sa); \
        const int kc = p.LP - gi;                                                                         \
        const int sw0 = min(gb, p.B - 1) * qbs4 + S * gi * 4;                                             \
        const int sw1 = (kc < 16 && gb + 1 < p.B) ? (gb + 1) * qbs4 : sw0;                                \
        _Pragma("unroll") for (int e = 0; e < NE2; ++e) {                                                 \
            const int pc0 = e * NT + wv * 64;          /* the wave's first piece */                       \
            if ((e + 1) * NT <= NP || pc0 < NP)                                                           \
                dma16s(rx, (STAGE_PTR) + RTILE_A + 4 * pc0, woff[e], pc0 >= C::SUBP / 4 ? sw1 : sw0);     \
        }                                                                                                 \
        G_FLAT_ISSUED                                                                                     \
    }
#define GRF_FRAGS G_READ_FLAT(C::SUBP)
        G_SLAB_LOOP(C::STG_FLAT_F32, 0, GRF_ISSUE, G_FLAT_SKIP, G_FLAT_ADVANCE, GRF_FRAGS, G_FLAT_ADVANCE)
#undef GRF_FRAGS
#undef GRF_ISSUE
        G_FINISH(wk.g, wk.slot)
        wk.next(se - sb);
    }
}

// per-sample slabs on packed operands: every slab is the interior case (no branch in the loop but its back edge)
template <int KW, int S>
__device__ __forceinline__ void g_ps_f32(const IgemmParams& p) {
    using C = GRaw<KW, S>;
    G_HEAD(C::STG_PS)
    const rsrc_t rp = make_rsrc(p.pk, p.pk_bytes), rx = make_rsrc(p.qk, p.qk_bytes);
    const int pbs4 = p.M * p.Kp * 4, qbs4 = p.qk_bs * 4;
    const int cps = p.Kp >> 4;                                         // slabs (chunks of 16 frames) per sample
    // (the walk written out: through Walk hipcc orders a handful of scalar instructions of this kernel differently)
    const int g = logical_wg(blockIdx.x, gridDim.x, p.whole);
    const Split sp = make_split(p.tilesM * p.tilesN, p.nslab, gridDim.x, p.whole);
    int pos = split_lo(sp, g);
    const int pos_end = split_lo(sp, g + 1);
    int slot = 0;
    while (pos < pos_end) {
        const int tile = pos / p.nslab, sb = pos - tile * p.nslab;
        const int se = min(p.nslab, sb + (pos_end - pos));
        G_TILE
        int pv[2], woff[C::NE16];
        G_A_PIECES(p.Kp)
#pragma unroll
        for (int e = 0; e < C::NE16; ++e) {
            const int f = 4 * (tid + NT * e), ql = f / C::WLP, v0 = f - ql * C::WLP;
            woff[e] = (f < C::SUB && qbase + ql < p.Q) ? ((qbase + ql) * p.Lq + v0) * 4 : FAR;
        }
        G_FRAG_BASE_ACC(G_NOTHING)

        int gb = sb / cps, gc = sb - gb * cps;          // (sample, chunk) of the slab being GATHERED; clamped as in g_raw_f32
#define GPF_ISSUE(STAGE_PTR, K0)                                                                          \
    {   const int gbc = min(gb, p.B - 1), gi = gc << 4;                                                   \
        _Pragma("unroll") for (int e = 0; e < 2; ++e) dma16s(rp, (STAGE_PTR) + wv * 256 + e * 1024, pv[e], gbc * pbs4 + gi * 4); \
        const int sw_ = gbc * qbs4 + S * gi * 4;                                                          \
        _Pragma("unroll") for (int e = 0; e < C::NE16; ++e)                                               \
            if (4 * (e * NT + wv * 64) < C::SUB) dma16s(rx, (STAGE_PTR) + RTILE_A + 4 * (e * NT + wv * 64), woff[e], sw_); \
        G_PS_NEXT(gb, gc)                                                                                 \
    }
        G_SLAB_LOOP(C::STG_PS, 0, GPF_ISSUE, G_NOTHING, G_NOTHING, G_READ_INTERIOR, G_NOTHING)
#undef GPF_ISSUE
        G_FINISH(g, slot)
        pos += se - sb;
        slot = 1;
    }
}

template <int KW, int S, int BF>
__global__ __launch_bounds__(NT, 2) void conv_g_raw_kernel(const IgemmParams p) {
    if constexpr (BF == 0) g_raw_f32<KW, S>(p);
    else g_raw_bf<KW, S, BF>(p);
}
template <int KW, int S, int BF>
__global__ __launch_bounds__(NT, 2) void conv_g_ps_kernel(const IgemmParams p) {
    if constexpr (BF == 0) g_ps_f32<KW, S>(p);
    else g_ps_bf<KW, S, BF>(p);
}

// ---- operand packing (HBM-bound, one pass per operand) ----------------------------------------------------------------------
// rows r = (b, c) of W floats: index j holds act(src[b][c][j - F]) for j - F in [0, L), else 0 (Q with halos; P per sample)
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ src, long bs, int C, int L, int F, int W, unsigned n,
                                                       float slope, float* __restrict__ dst) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned r = i / (unsigned)W, b = r / (unsigned)C, c = r - b * (unsigned)C;
        const int t = (int)(i - r * (unsigned)W) - F;
        float v = 0.f;
        if ((unsigned)t < (unsigned)L) {
            v = src[(long)b * bs + (long)c * L + t];
            if (slope != 1.0f) v = pg_act_apply(v, slope);
        }
        dst[i] = v;
    }
}
// flat K: dst[m][k], k = b * LP + i: act(src[b][m][i]) for k < B * LP, zeros up to Kp
__global__ __launch_bounds__(256) void pack_flat_kernel(const float* __restrict__ src, long bs, int B, int LP, int Kp, unsigned n,
                                                       float slope, float* __restrict__ dst) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned m = i / (unsigned)Kp, k = i - m * (unsigned)Kp, b = k / (unsigned)LP, t = k - b * (unsigned)LP;
        float v = 0.f;
        if ((int)b < B) {
            v = src[(long)b * bs + (long)m * LP + t];
            if (slope != 1.0f) v = pg_act_apply(v, slope);
        }
        dst[i] = v;
    }
}
unsigned pack_grid(unsigned n) { return (n + 255u) / 256u < 2048u ? (n + 255u) / 256u : 2048u; }

hipError_t pack_g(const IgemmParams& p, hipStream_t st) {
    float* const qk = const_cast<float*>(p.qk);
    float* const pk = const_cast<float*>(p.pk);
    const unsigned nq = (unsigned)(p.qk_bytes / 4), np = (unsigned)(p.pk_bytes / 4);
    hipLaunchKernelGGL(pack_rows_kernel, dim3(pack_grid(nq)), dim3(256), 0, st, p.x, p.x_bs, p.Q, p.Lx, p.p, p.Lq, nq, pg_act_slope(p.act_x), qk);
    if (p.g_ps) hipLaunchKernelGGL(pack_rows_kernel, dim3(pack_grid(np)), dim3(256), 0, st, p.pt, p.pt_bs, p.M, p.LP, 0, p.Kp, np, pg_act_slope(p.act_p), pk);
    else hipLaunchKernelGGL(pack_flat_kernel, dim3(pack_grid(np)), dim3(256), 0, st, p.pt, p.pt_bs, p.B, p.LP, p.Kp, np, pg_act_slope(p.act_p), pk);
    return hipGetLastError();
}

// the kernel of a (k, s) pair and operand mode: per-sample slabs (host: short samples whose padded K costs <= 7 %) or flat K
typedef void (*g_kernel_t)(const IgemmParams);
template <int KW, int S, int BF> g_kernel_t g_kernel(bool ps) { return ps ? conv_g_ps_kernel<KW, S, BF> : conv_g_raw_kernel<KW, S, BF>; }

template <int KW, int S>
hipError_t launch_g_raw(const IgemmParams& p, int grid, hipStream_t st, int prec) {
    if (prec == 0) {
        if (hipError_t e = pack_g(p, st)) return e;
    }
    const g_kernel_t kernel = prec == 1 ? g_kernel<KW, S, 1>(p.g_ps) : (prec == 2 ? g_kernel<KW, S, 2>(p.g_ps) : g_kernel<KW, S, 0>(p.g_ps));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), 0, st, p);
    return hipGetLastError();
}

}  // namespace

hipError_t pgconv::launch_raw_g(const IgemmParams& p, int grid, hipStream_t st, int prec) {
    if (p.k == 32) return launch_g_raw<32, 2>(p, grid, st, prec);
    if (p.k == 8 && p.s == 1) return launch_g_raw<8, 1>(p, grid, st, prec);
    if (p.k == 8) return launch_g_raw<8, 2>(p, grid, st, prec);
    if (p.k == 5) return launch_g_raw<5, 2>(p, grid, st, prec);
    return launch_g_raw<4, 2>(p, grid, st, prec);
}
