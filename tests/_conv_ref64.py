"""Float64 restatements (numpy, CPU) of the convolution contract of include/phasegen.h -- forward, dgrad and wgrad of Conv1d and
ConvTranspose1d at any (k, s, p), with the fused input activation, the forward's store activations and the dgrad's epilogue -- the
error scale of one output element, and the comparison the value tests make.  Shared by tests/test_conv_bounds_host.py (which shows
that the comparison rejects planted faults and accepts honest fp32 / bf16 / bf16x3 convolutions) and tests/test_z_conv_values_gpu.py
(the kernels).

Every op is one GEMM out = A @ Bm over gathered operands (`gemm`): the forward of a Conv1d and the dgrad of a ConvTranspose1d gather
windows of the zero-padded input; the forward of a ConvTranspose1d and the dgrad of a Conv1d do the same on the input with s - 1
zeros between its frames and the taps reversed; a wgrad sums over (sample, frame).  Terms that multiply a padding zero are exact
zeros in every arithmetic used here, so they change neither a value nor an error.

  value   sum of the products in float64 of the operands AS THE MFMA SEES THEM (`see`): fp32 and bf16x3 take the fp32 values (the
          activation applied in fp32, as the kernels apply it on the fragments), bf16 and the bf16-resident kernels those values
          rounded to bf16 (RNE) after the activation.
  mag     the same sum over the absolute values of the terms; an addend counts with |add|, the dgrad's mask factor scales both.
  r       |got - value| / (u mag) per element, u = 2^-24: the error in unit roundoffs of the element's own terms.  r_max is its
          maximum and r_rms its RMS over the elements with mag > 0; an element with mag = 0 must be exactly 0 (either sign).

A store activation leaves mag as it is (an output just below zero may come out just above: the difference is still an error of the
sum, not of the slope times the sum).

The threshold is MARGIN x the same statistic of an honest stand-in of the same precision on the same input, never anything derived
from the code under test:
  (a) `torch32`  fp32 torch CPU conv / autograd (oneDNN off, as oracle/unet_ref.py arranges);
  (b) `seq32`    numpy float32, products rounded to fp32, strictly sequential accumulation along K: the least accurate honest order
                 and the one the fp32 bound is scaled by;
  (c) `x3`       the bf16x3 split of csrc/conv_common.h: hi = bf16(x), lo = bf16(x - hi), lo hi' + hi lo' + hi hi', sequential fp32;
  (d) `seq32` on bf16-rounded operands.
On the CPU sequential fp32 has r_rms about 0.4 at every K; the split has about 92 / sqrt K (the two dropped residuals are each
<= 2^-18 = 64 u of a product).  So an fp32 call that runs the split is rejected where K is at most about 512 (`gemm_k`)."""
import numpy as np

U = 2.0 ** -24
MARGIN = 4.0
NONE, LEAKY, RELU = 0, 1, 2
SLOPE32 = {NONE: np.float32(1.0), LEAKY: np.float32(0.2), RELU: np.float32(0.0)}
PRECISION_K = 512                   # the longest GEMM K at which the fp32 bound still separates fp32 from the bf16x3 split by 10 x


def out_len(tr, Lin, k, s, p):
    return (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1


def shapes(geom):
    """(x, w, dy) shapes of a (transposed, Cin, Cout, k, s, p, Lin, B) row"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    return (B, Cin, Lin), ((Cin, Cout, k) if tr else (Cout, Cin, k)), (B, Cout, out_len(tr, Lin, k, s, p))


def gemm_k(geom, op):
    """The K of the GEMM a kernel runs: fwd Cin x taps, dgrad Cout x taps (a transposed form: taps per phase), wgrad B x frames."""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    per_phase = -(-k // s)
    if op == "fwd":
        return Cin * (per_phase if tr else k)
    if op == "dgrad":
        return Cout * (k if tr else per_phase)
    return B * (Lin if tr else out_len(tr, Lin, k, s, p))


def act32(x, act):
    """pg_act_apply on fp32: fmaxf(v, slope v)"""
    x = np.asarray(x, np.float32)
    return x if act == NONE else np.maximum(x, SLOPE32[act] * x)


def act64(v, act):
    v = np.asarray(v, np.float64)
    return v if act == NONE else np.maximum(v, float(SLOPE32[act]) * v)


def bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32)


def split(x):
    hi = bf16(x)
    return hi, bf16(np.asarray(x, np.float32) - hi)


def see(t, prec):
    """the operand as the MFMA sees it ("bf16" also stands for the bf16-resident kernels)"""
    t = np.asarray(t, np.float32)
    return bf16(t) if prec == "bf16" else t


def hilo(t):
    """what a bf16x3 product with 1.0 returns: float32(hi) + float32(lo), exact in fp32"""
    hi, lo = split(t)
    return hi + lo


# ---- the ops as GEMMs -------------------------------------------------------------------------------------------------------------
def _cols(z, k, s, T, left):
    """cols[b, c k + j, t] = zp[b, c, t s + j], zp = z behind `left` zeros and in front of as many as the windows reach"""
    assert left >= 0
    B, C, L = z.shape
    zp = np.zeros((B, C, max((T - 1) * s + k, left + L)), z.dtype)
    zp[:, :, left:left + L] = z
    st = zp.strides
    v = np.lib.stride_tricks.as_strided(zp, (B, C, k, T), (st[0], st[1], st[2], st[2] * s), writeable=False)
    return np.ascontiguousarray(v).reshape(B, C * k, T)


def _spread(z, s):
    if s == 1:
        return z
    B, C, L = z.shape
    out = np.zeros((B, C, (L - 1) * s + 1), z.dtype)
    out[:, :, ::s] = z
    return out


def _gather(z, W, k, s, p, T):
    """out[b, o, t] = sum_{c, j} zpad[b, c, t s + j] W[o, c, j]"""
    return np.ascontiguousarray(W).reshape(1, W.shape[0], -1), _cols(z, k, s, T, p)


def _scatter(z, W, k, s, p, T):
    """out[b, o, tau] = sum_{c, j} z[b, c, t] W[c, o, j] over tau = t s - p + j"""
    Wf = np.ascontiguousarray(W.transpose(1, 0, 2)[:, :, ::-1])
    return Wf.reshape(1, Wf.shape[0], -1), _cols(_spread(z, s), k, 1, T, k - 1 - p)


def gemm(op, geom, x, w, dy, x_act=NONE, prec="fp32"):
    """(A, Bm, shape): the op is (A @ Bm).reshape(shape) on the fp32 operands as the MFMA sees them; A (1 | -, M, K), Bm (B | -, K, N).
    fwd reads (x, w), dgrad (dy, w), wgrad (x, dy); the other argument may be None."""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    Lout = out_len(tr, Lin, k, s, p)
    if op == "fwd":
        z, W = see(act32(x, x_act), prec), see(w, prec)
        A, Bm = (_scatter if tr else _gather)(z, W, k, s, p, Lout)
        return A, Bm, (B, Cout, Lout)
    if op == "dgrad":
        z, W = see(dy, prec), see(w, prec)
        A, Bm = (_gather if tr else _scatter)(z, W, k, s, p, Lin)
        return A, Bm, (B, Cin, Lin)
    assert op == "wgrad"
    xa, g = see(act32(x, x_act), prec), see(dy, prec)
    rows, win, T = (xa, g, Lin) if tr else (g, xa, Lout)        # dw[a, c, j] = sum_{b, t} rows[b, a, t] winpad[b, c, t s + j]
    cols = _cols(win, k, s, T, p)
    A = np.ascontiguousarray(rows.transpose(1, 0, 2)).reshape(rows.shape[1], B * T)
    Bm = np.ascontiguousarray(cols.transpose(0, 2, 1)).reshape(B * T, cols.shape[1])
    return A, Bm, ((Cin, Cout, k) if tr else (Cout, Cin, k))


def mm64(A, Bm):
    """(value, mag) of A @ Bm in float64"""
    A, Bm = A.astype(np.float64), Bm.astype(np.float64)
    return A @ Bm, np.abs(A) @ np.abs(Bm)


def _live_k(A, Bm):
    """the K indices at which some product is not an exact zero"""
    return np.flatnonzero(np.any(A != 0, axis=tuple(range(A.ndim - 1))) & np.any(np.moveaxis(Bm, -2, -1) != 0, axis=tuple(range(Bm.ndim - 1))))


def seq32(A, Bm, reverse=False):
    """A @ Bm in float32: each product rounded, added in the order of K (a K index whose terms are all zero adds exact zeros: skipped)"""
    assert A.dtype == np.float32 and Bm.dtype == np.float32
    acc = np.zeros(np.broadcast_shapes(A.shape[:-2], Bm.shape[:-2]) + (A.shape[-2], Bm.shape[-1]), np.float32)
    ks = _live_k(A, Bm)
    for kk in (ks[::-1] if reverse else ks):
        acc += A[..., :, kk, None] * Bm[..., kk, None, :]
    return acc


def x3(A, Bm, reverse=False):
    """the bf16x3 split: products of bf16 values are exact in fp32; per K index lo hi', hi lo', hi hi' as the kernels order them"""
    (Ah, Al), (Bh, Bl) = split(A), split(Bm)
    acc = np.zeros(np.broadcast_shapes(A.shape[:-2], Bm.shape[:-2]) + (A.shape[-2], Bm.shape[-1]), np.float32)
    ks = _live_k(A, Bm)
    for kk in (ks[::-1] if reverse else ks):
        a_h, a_l, b_h, b_l = Ah[..., :, kk, None], Al[..., :, kk, None], Bh[..., kk, None, :], Bl[..., kk, None, :]
        acc += a_l * b_h
        acc += a_h * b_l
        acc += a_h * b_h
    return acc


def conv64(op, geom, x, w, dy, x_act=NONE, prec="fp32"):
    """(value, mag), float64, in the op's output shape"""
    A, Bm, shape = gemm(op, geom, x, w, dy, x_act, prec)
    v, m = mm64(A, Bm)
    return v.reshape(shape), m.reshape(shape)


def standin(op, geom, x, w, dy, x_act=NONE, prec="fp32", reverse=False):
    """the honest fp32-accumulating stand-in of a precision: (b) for fp32, (d) for bf16, (c) for bf16x3"""
    A, Bm, shape = gemm(op, geom, x, w, dy, x_act, prec)
    return (x3 if prec == "bf16x3" else seq32)(A, Bm, reverse).reshape(shape)


def torch32(op, geom, x, w, dy, x_act=NONE):
    """stand-in (a): fp32 torch CPU"""
    import torch
    import torch.nn.functional as F
    from oracle import unet_ref  # noqa: F401  (disables oneDNN)
    tr, Cin, Cout, k, s, p, Lin, B = geom
    conv = (lambda a, b: F.conv_transpose1d(a, b, stride=s, padding=p)) if tr else (lambda a, b: F.conv1d(a, b, stride=s, padding=p))
    xs, ws, dys = shapes(geom)
    xa = torch.from_numpy(act32(x, x_act) if x is not None else np.zeros(xs, np.float32)).clone().requires_grad_(True)
    wt = torch.from_numpy(np.asarray(w if w is not None else np.zeros(ws, np.float32))).clone().requires_grad_(True)
    y = conv(xa, wt)
    if op == "fwd":
        return y.detach().numpy()
    y.backward(torch.from_numpy(np.asarray(dy)))
    return (xa.grad if op == "dgrad" else wt.grad).numpy()


# ---- epilogues --------------------------------------------------------------------------------------------------------------------
def mask64(ref, mask):
    """act'(ref) with act'(0) = act'(-0) = slope"""
    return np.where(np.asarray(ref) > 0, 1.0, float(SLOPE32[mask]))


def dgrad_epilogue64(value, mag, add, ref, mask):
    m = mask64(ref, mask)
    return (value + add.astype(np.float64)) * m, (mag + np.abs(add.astype(np.float64))) * m


def dgrad_epilogue32(g, add, ref, mask, at_zero=None):
    """(g + add) * (ref > 0 ? 1 : slope) in fp32, as csrc/conv_common.h writes it; `at_zero` plants another factor where ref == 0"""
    m = np.where(ref > 0, np.float32(1.0), SLOPE32[mask]).astype(np.float32)
    if at_zero is not None:
        m = np.where(ref == 0, np.float32(at_zero), m)
    return (np.asarray(g, np.float32) + add) * m


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def errors(got, value, mag):
    """{"r_max", "r_rms", "zeros"}: zeros = every element with mag == 0 is exactly 0.  A NaN in `got` makes both ratios NaN."""
    got = np.asarray(got, np.float64)
    assert got.shape == value.shape == mag.shape, (got.shape, value.shape, mag.shape)
    live = mag > 0
    r = np.abs(got - value)[live] / (U * mag[live])
    zeros = bool(np.all(got[~live] == 0.0))
    if r.size == 0:
        return {"r_max": 0.0, "r_rms": 0.0, "zeros": zeros}
    return {"r_max": float(r.max()), "r_rms": float(np.sqrt(np.mean(r * r))), "zeros": zeros}


def accept(err, base, margin=MARGIN):
    """err within margin x the stand-in's statistics (a NaN is rejected) and exact zeros where nothing was summed"""
    return bool(err["zeros"] and err["r_max"] <= margin * base["r_max"] and err["r_rms"] <= margin * base["r_rms"])


def bound_text(base, margin=MARGIN):
    return f"{margin * base['r_max']:.2f} {margin * base['r_rms']:.3f}"


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
SEEDS = {"x": 61, "w": 62, "dy": 63, "add": 64, "ref": 65}
GRADE_SPAN = 12


def _noise(seed, shape):
    from phasegen import detgen
    return detgen.uniform(seed, tuple(shape), -1.0, 1.0)


def grade_exponents(seed, n):
    """n integers from -12 .. 12"""
    from phasegen import detgen
    e = np.floor(detgen.uniform(seed, (n,), -GRADE_SPAN, GRADE_SPAN + 1)).astype(np.int64)
    return np.clip(e, -GRADE_SPAN, GRADE_SPAN)


def grades(geom):
    """{"x": exponents per channel of x, "w": per output row of w, "dy": per channel of dy} of the graded input of a row"""
    Cin, Cout = geom[1], geom[2]
    return {"x": grade_exponents(71, Cin), "w": grade_exponents(72, Cout), "dy": grade_exponents(73, Cout)}


def make_inputs(geom, kind):
    """{"x", "w", "dy", "add", "ref"} float32: "white" is the suite's dense noise (w x 0.1); "graded" multiplies it by a power of two
    per channel of x, per output row of w and per channel of dy (exact).  add / ref have dx's shape; ref is plain noise (no zeros)."""
    tr = geom[0]
    xs, ws, dys = shapes(geom)
    t = {"x": _noise(SEEDS["x"], xs), "w": _noise(SEEDS["w"], ws) * np.float32(0.1), "dy": _noise(SEEDS["dy"], dys),
         "add": _noise(SEEDS["add"], xs), "ref": _noise(SEEDS["ref"], xs)}
    if kind == "graded":
        g = grades(geom)
        two = lambda e: np.exp2(e.astype(np.float64)).astype(np.float32)
        t["x"] = t["x"] * two(g["x"])[None, :, None]
        t["w"] = t["w"] * (two(g["w"])[None, :, None] if tr else two(g["w"])[:, None, None])
        t["dy"] = t["dy"] * two(g["dy"])[None, :, None]
        t["add"] = t["add"] * two(g["x"])[None, :, None]
    else:
        assert kind == "white"
    assert all(v.dtype == np.float32 for v in t.values())
    return t


def with_zeros(ref, seed=66):
    """ref with an exact 0.0 or -0.0 (alternating) at about one element in eight"""
    pick = _noise(seed, ref.shape) < -0.75
    out = ref.copy()
    flat, idx = out.reshape(-1), np.flatnonzero(pick.reshape(-1))
    flat[idx[0::2]] = np.float32(0.0)
    flat[idx[1::2]] = np.float32(-0.0)
    return out


def impulse_sites(C, L, k):
    """(channel, frame) of the one-hot samples: first and last frame with first and last channel in the four combinations (the last
    channel is also the last of a partial 16-deep K slab), the first channel of the last K slab, and frames 127 and 256 modulo the
    frame count: with several samples per tile, the columns beside which a 128- or 256-wide tile changes sample"""
    c_tail = ((C - 1) // 16) * 16 if k >= 16 else max(0, ((C * k - 1) // 16) * 16 // k)
    return [(0, 0), (C - 1, L - 1), (C - 1, 0), (0, L - 1), (min(c_tail, C - 1), L // 2), (C // 2, 127 % L), (C // 3, 256 % L)]


def impulses(B, C, L, k, variant, only_first_sample=False):
    """(B, C, L) of zeros with one 1.0 per sample: sample b of variant v sits at site (v B + b) mod 7"""
    sites = impulse_sites(C, L, k)
    out = np.zeros((B, C, L), np.float32)
    for b in range(1 if only_first_sample else B):
        c, t = sites[(variant * (1 if only_first_sample else B) + b) % len(sites)]
        out[b, c, t] = 1.0
    return out


def impulse_variants(B, only_first_sample=False):
    return -(-7 // (1 if only_first_sample else B))
