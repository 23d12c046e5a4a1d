"""What a NaN or an infinity that enters an entry point must do to its outputs (include/phasegen.h, "Non-finite values"), as a
comparison of four arrays -- the device's output on the poisoned and on the clean input, the float64 restatement on both -- and
the small float64 restatements that no other test module holds as a function.  numpy only.

  R1  nothing is swallowed: an element that is non-finite in the reference of the poisoned input is non-finite on the device.
  R2  nothing spreads: an element that is finite in the reference of the poisoned input and equal there to the reference of the clean
      input has, on the device, the BITS of the clean call.  `allow` names the elements the header excepts.

One element is poisoned per call: every sum then holds at most one non-finite term, so whether it comes out finite is a fact about
the operation and not about the order the reference or the kernel adds in.  Zero padding (and the zeros a transposed convolution
puts between its frames) is "no term", not a product with zero: `conv_cone` says which outputs a poisoned operand element reaches by
index arithmetic alone.  Shared by tests/test_nonfinite_host.py (the checker is honest: stand-ins pass, planted faults fail, every
case's cone is neither empty nor everything) and tests/test_z_nonfinite_gpu.py (the kernels)."""
import math

import numpy as np

NAN, PINF, NINF = np.float32("nan"), np.float32("inf"), np.float32("-inf")
VALUES = (("nan", NAN), ("+inf", PINF), ("-inf", NINF))


def poison(a, index, value):
    """a copy of `a` with a[index] = value (index: a tuple, or an int into the flattened array)"""
    out = np.array(a, copy=True)
    if isinstance(index, (int, np.integer)):
        out.reshape(-1)[index] = value
    else:
        out[tuple(index)] = value
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(_bits(a), _bits(b)))


def check(got_poisoned, got_clean, ref_poisoned, ref_clean, allow=None, tag=""):
    """R1 and R2 (module docstring).  Prints one NONFINITE line and returns its counts: "cone" elements the reference makes
    non-finite, "outside" elements it leaves exactly as they were, "changed" finite ones it moves (held to neither rule), "swallowed"
    violations of R1, "spread" violations of R2 outside `allow`, "allowed" inside it.  Raises AssertionError on a violation."""
    gp, gc = np.asarray(got_poisoned), np.asarray(got_clean)
    rp, rc = np.asarray(ref_poisoned, np.float64), np.asarray(ref_clean, np.float64)
    assert gp.shape == gc.shape == rp.shape == rc.shape, (tag, gp.shape, gc.shape, rp.shape, rc.shape)
    assert gp.dtype == gc.dtype and gp.dtype.kind == "f", (tag, gp.dtype, gc.dtype)
    assert np.isfinite(rc).all() and np.isfinite(gc).all(), f"{tag}: the clean call is not finite"
    cone = ~np.isfinite(rp)
    outside = ~cone & (rp == rc)
    differs = _bits(gp) != _bits(gc)
    swallowed = cone & np.isfinite(gp)
    spread = outside & differs
    allowed = spread & (np.zeros(gp.shape, bool) if allow is None else np.broadcast_to(np.asarray(allow, bool), gp.shape))
    spread = spread & ~allowed
    n = {"cone": int(cone.sum()), "outside": int(outside.sum()), "changed": int((~cone & ~outside).sum()),
         "swallowed": int(swallowed.sum()), "spread": int(spread.sum()), "allowed": int(allowed.sum())}
    print(f"NONFINITE {tag}: cone {n['cone']} outside {n['outside']} changed {n['changed']} of {gp.size}; swallowed {n['swallowed']}, "
          f"spread {n['spread']}, excepted spread {n['allowed']}")
    assert n["swallowed"] == 0, f"{tag}: R1, {n['swallowed']} of {n['cone']} non-finite elements came out finite, first at {tuple(np.argwhere(swallowed)[0])}"
    assert n["spread"] == 0, f"{tag}: R2, {n['spread']} of {n['outside']} untouched elements changed, first at {tuple(np.argwhere(spread)[0])}"
    return n


def cone_is_a_proper_part(ref_poisoned, ref_clean, whole=False):
    """the condition of the issue on a case: the cone holds at least one element and at most half (whole=True: any number: the
    entry points whose cone is a scalar or a channel by definition)"""
    cone = ~np.isfinite(np.asarray(ref_poisoned, np.float64))
    n = int(cone.sum())
    return n >= 1 and (whole or 2 * n <= cone.size)


# ---- convolutions -------------------------------------------------------------------------------------------------------------------
def conv_operands(op):
    return {"fwd": ("x", "w"), "dgrad": ("dy", "w", "add", "ref"), "wgrad": ("x", "dy")}[op]


def _conv_shapes(geom):
    tr, Cin, Cout, k, s, p, Lin, B = geom
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    return {"x": (B, Cin, Lin), "add": (B, Cin, Lin), "ref": (B, Cin, Lin), "w": (Cin, Cout, k) if tr else (Cout, Cin, k), "dy": (B, Cout, Lout)}


def conv_sites(geom, operand):
    """{"edge", "interior", "last"}: an element only edge windows reach (the first frame, or tap 0, which the first windows lay on the
    padding), one in the middle, and the last element of the last sample (the partial tile, the column tail)"""
    shape = _conv_shapes(geom)[operand]
    J = _pairs(geom)
    if operand == "w":
        live = np.isin(np.arange(shape[2]), J[J >= 0])              # taps some window uses at all (a one-frame layer leaves some out)
    elif operand == "dy":
        live = (J >= 0).any(axis=0)
    else:
        live = (J >= 0).any(axis=1) if operand == "x" else np.ones(shape[2], bool)
    near = lambda i: int(np.flatnonzero(live)[np.argmin(np.abs(np.flatnonzero(live) - i))])
    return {"edge": (0, 0, near(0)), "interior": (shape[0] // 2, shape[1] // 2, near(shape[2] // 2)),
            "last": (shape[0] - 1, shape[1] - 1, near(shape[2] - 1))}


def _pairs(geom):
    """pairs[xi, yi] = the tap j that joins frame xi of x with frame yi of y, or -1"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    Lout = _conv_shapes(geom)["dy"][2]
    xi, yi = np.arange(Lin)[:, None], np.arange(Lout)[None, :]
    j = (yi - xi * s + p) if tr else (xi - yi * s + p)
    return np.where((j >= 0) & (j < k), j, -1)


def conv_cone(op, geom, operand, index):
    """bool array of the op's output shape: the elements with a term that holds operand[index].  fwd y[b, o, yi] = sum x[b, c, xi]
    w[o | c, c | o, j], dgrad dx[b, c, xi] = sum dy[b, o, yi] w[.., j] (+ add[b, c, xi]), wgrad dw[.., j] = sum x[b, c, xi] dy[b, o, yi],
    each over the (xi, yi, j) that `_pairs` joins.  `ref` (the mask source) enters no sum."""
    tr = geom[0]
    sh = _conv_shapes(geom)
    J = _pairs(geom)
    out = np.zeros(sh[{"fwd": "dy", "dgrad": "x", "wgrad": "w"}[op]], bool)
    i0, i1, i2 = index
    if operand == "w":
        c, o = (i0, i1) if tr else (i1, i0)
        hit = J == i2
        if op == "fwd":
            out[:, o, hit.any(axis=0)] = True
        else:
            assert op == "dgrad"
            out[:, c, hit.any(axis=1)] = True
    elif operand == "x":
        if op == "fwd":
            out[i0, :, J[i2] >= 0] = True
        else:
            assert op == "wgrad"
            taps = np.unique(J[i2][J[i2] >= 0])
            if tr:
                out[i1, :, taps] = True
            else:
                out[:, i1, taps] = True
    elif operand == "dy":
        if op == "dgrad":
            out[i0, :, J[:, i2] >= 0] = True
        else:
            assert op == "wgrad"
            taps = np.unique(J[:, i2][J[:, i2] >= 0])
            if tr:
                out[:, i1, taps] = True
            else:
                out[i1, :, taps] = True
    elif operand == "add":
        assert op == "dgrad"
        out[index] = True
    else:
        assert operand == "ref" and op == "dgrad"
    return out


def conv_row_mates(op, geom, operand, index):
    """Exception C1 of the header: the outputs in which the poisoned element meets a ZERO the kernel multiplies in -- the padding, the
    zeros a transposed form puts between its frames, the frames past the end of the partner operand.  Every frame of a weight's output
    channel (fwd) or input channel (dgrad) has tap j on a real sample (the cone) or on such a zero, and every tap of a wgrad's channel
    pairs the poisoned frame with a real partner frame or with none: so the exception is the whole row -- a weight's channel in every
    sample; for a wgrad, every tap of the poisoned x's input channel or of the poisoned dy's output channel.  Nothing for the others."""
    tr = geom[0]
    sh = _conv_shapes(geom)
    out = np.zeros(sh[{"fwd": "dy", "dgrad": "x", "wgrad": "w"}[op]], bool)
    if operand == "w":
        c, o = (index[0], index[1]) if tr else (index[1], index[0])
        out[:, o if op == "fwd" else c, :] = True
    elif op == "wgrad":
        in_channel = operand == "x"
        if in_channel == tr:
            out[index[1], :, :] = True
        else:
            out[:, index[1], :] = True
    return out


def conv_phantom_taps(op, geom, operand, index):
    """Exception C2 of the header: a transposed form that runs its taps phase by phase rounds k up to s ceil(k / s) taps of zero weight;
    a poisoned input frame (x of a ConvTranspose1d forward, dy of a Conv1d dgrad) meets them in the frames just behind its window:
    every channel of that sample at frames xi s - p + j, j = k .. s ceil(k / s) - 1"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    sh = _conv_shapes(geom)
    out = np.zeros(sh["dy" if op == "fwd" else "x"], bool)
    assert (op, operand, tr) in (("fwd", "x", True), ("dgrad", "dy", False))
    for j in range(k, s * -(-k // s)):
        t = index[2] * s - p + j
        if 0 <= t < out.shape[2]:
            out[index[0], :, t] = True
    return out


def conv_direct(op, geom, x, w, dy):
    """the op as a loop over the terms that exist (float64, IEEE): the independent statement `conv_cone` is checked against"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    sh = _conv_shapes(geom)
    J = _pairs(geom)
    out = np.zeros(sh[{"fwd": "dy", "dgrad": "x", "wgrad": "w"}[op]])
    with np.errstate(invalid="ignore", over="ignore"):
        for xi, yi in np.argwhere(J >= 0):
            j = J[xi, yi]
            wj = np.asarray(w[:, :, j], np.float64) if w is not None else None         # (Cin, Cout) transposed, else (Cout, Cin)
            if op == "fwd":
                out[:, :, yi] += x[:, :, xi].astype(np.float64) @ (wj if tr else wj.T)
            elif op == "dgrad":
                out[:, :, xi] += dy[:, :, yi].astype(np.float64) @ (wj.T if tr else wj)
            else:
                g = np.einsum("bc,bo->co", x[:, :, xi].astype(np.float64), dy[:, :, yi].astype(np.float64))
                out[:, :, j] += g if tr else g.T
    return out


# ---- BatchNorm, per-clip BatchNorm ------------------------------------------------------------------------------------------------------
def bn_fwd64(x, gamma, beta, rm0, rv0, eps=1e-5, momentum=0.1, per_clip=False):
    """train-mode BatchNorm of x (B, C, L) in float64: {"y", "save_mean", "save_invstd", "running_mean", "running_var"}; per_clip:
    statistics per row (b, c), save_* (B, C), the running buffers one momentum step per clip in clip order (pg_clipnorm_fwd)"""
    x = np.asarray(x, np.float64)
    B, C, L = x.shape
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    rm, rv = np.array(rm0, np.float64), np.array(rv0, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if per_clip:
            mean = x.mean(axis=2)
            var = ((x - mean[:, :, None]) ** 2).mean(axis=2)
            inv = 1.0 / np.sqrt(var + eps)
            y = (x - mean[:, :, None]) * inv[:, :, None] * g[None, :, None] + b[None, :, None]
            for i in range(B):
                rm = (1 - momentum) * rm + momentum * mean[i]
                rv = (1 - momentum) * rv + momentum * var[i] * (L / max(L - 1, 1))
        else:
            n = B * L
            mean = x.mean(axis=(0, 2))
            var = ((x - mean[None, :, None]) ** 2).mean(axis=(0, 2))
            inv = 1.0 / np.sqrt(var + eps)
            y = (x - mean[None, :, None]) * inv[None, :, None] * g[None, :, None] + b[None, :, None]
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * var * (n / max(n - 1, 1))
    return {"y": y, "save_mean": mean, "save_invstd": inv, "running_mean": rm, "running_var": rv}


def bn_bwd64(x, dy, gamma, save_mean, save_invstd):
    """pg_bn_bwd from the forward's saved statistics: {"dx", "dgamma", "dbeta"}"""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = x.shape[0] * x.shape[2]
    sm, si, g = (np.asarray(a, np.float64) for a in (save_mean, save_invstd, gamma))
    with np.errstate(invalid="ignore", over="ignore"):
        xh = (x - sm[None, :, None]) * si[None, :, None]
        dg, db = (dy * xh).sum(axis=(0, 2)), dy.sum(axis=(0, 2))
        dx = (g * si)[None, :, None] * (dy - (db / n)[None, :, None] - xh * (dg / n)[None, :, None])
    return {"dx": dx, "dgamma": dg, "dbeta": db}


def act64(v, act):
    """the select x >= 0 ? x : slope * x (0 none, 1 leaky 0.2, 2 relu)"""
    v = np.asarray(v, np.float64)
    if act == 0:
        return v
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0, v, (0.2 if act == 1 else 0.0) * v)


# ---- loss, Adam ---------------------------------------------------------------------------------------------------------------------
def loss64(pred, batch, mag_weight=0.2):
    """include/phasegen.h: loss = MSE(cos p, cos th) + MSE(sin p, sin th) + mag_weight MSE(m^, m) and its gradient: (losses (3,), dpred)"""
    pred, batch = np.asarray(pred, np.float64), np.asarray(batch, np.float64)
    B, C2, L = pred.shape
    C = C2 // 2
    p, mh, m, th = pred[:, :C], pred[:, C:], batch[:, 0], batch[:, 1]
    N = B * C * L
    with np.errstate(invalid="ignore", over="ignore"):
        dc, ds, dm = np.cos(p) - np.cos(th), np.sin(p) - np.sin(th), mh - m
        cos_l, sin_l, mag_l = (dc * dc).sum() / N, (ds * ds).sum() / N, (dm * dm).sum() / N
        s = 2.0 / N
        dpred = np.concatenate([s * (ds * np.cos(p) - dc * np.sin(p)), mag_weight * s * dm], axis=1)
        return np.array([cos_l + sin_l + mag_weight * mag_l, cos_l + sin_l, mag_l]), dpred


def adam64(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, dtype=np.float64):
    """pg_adam_step's update (p, m, v) in `dtype` arithmetic"""
    f = dtype
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = g * f(grad_scale)
        m = m + f(1.0 - beta1) * (g - m)
        v = v * f(beta2) + f(1.0 - beta2) * (g * g)
        denom = np.sqrt(v) / f(math.sqrt(1.0 - beta2 ** step)) + f(eps)
        p = p - f(lr / (1.0 - beta1 ** step)) * (m / denom)
    return p, m, v


# ---- polar --------------------------------------------------------------------------------------------------------------------------
POLAR_CELLS = [(NAN, 1.0), (1.0, NAN), (PINF, 1.0), (NINF, 1.0), (1.0, PINF), (1.0, NINF), (PINF, PINF)]


def polar64(re, im, use_exp=True):
    """data.py:39-47 in float64: (log1p|z| or |z|, angle z)"""
    with np.errstate(invalid="ignore", over="ignore"):
        # z = re + 1j * im AS data.py:40 FORMS IT: 1j * im = (0 * im - 0) + j im, so an infinite imaginary part makes the real part NaN
        # (csrc/pg_common.h, pg_complex_from_parts, restates that arithmetic for the signed zeros; the infinities follow from it)
        z = np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
        m = np.abs(z)
        return (np.log1p(m) if use_exp else m), np.angle(z)


def atan2_minmax32(y, x):
    """csrc/pg_fastmath.h's pg_atan2 as it stood before its NaN rule, in numpy float32: np.fmax / np.fmin drop a NaN as fmaxf / fminf
    do, so the ratio is that of the other argument with itself and the angle comes out finite (the planted fault of the host test)"""
    y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx, mn = np.fmax(ax, ay), np.fmin(ax, ay)
        a = np.where(mx > 0, mn / mx, np.float32(0))
        r = np.arctan(a).astype(np.float32)
        r = np.where(ay > ax, np.float32(np.pi / 2) - r, r)
        r = np.where(np.signbit(x), np.float32(np.pi) - r, r)
    return np.copysign(r, y).astype(np.float32)


# ---- STFT / ISTFT cones ---------------------------------------------------------------------------------------------------------------
# A transform is a sum of products sample x coefficient, and some coefficients are EXACTLY zero: cos(2 pi k m / N) where k m / N is
# an odd multiple of 1/4, sin(2 pi k m / N) where it is a multiple of 1/2 (every bin at taps 0 and N / 2).  The sum as written
# gives 0 * NaN = NaN there; a fast transform never forms that product (numpy's and torch's do not) and stays finite.  The contract
# takes either: such an output is marked UNHELD (a finite value far from the clean one), which `check` holds to neither rule.
UNHELD = 1e9


def cos_is_zero(k, m, N):
    q, r = np.divmod(4 * np.asarray(k, np.int64) * np.asarray(m, np.int64), N)
    return (r == 0) & (q % 2 == 1)


def sin_is_zero(k, m, N):
    return (2 * np.asarray(k, np.int64) * np.asarray(m, np.int64)) % N == 0


def stft_sites(n_samples, n_fft, hop):
    """{"first", "two-frames", "last"}: sample indices; "two-frames" is the first sample that exactly two frames cover (centred
    frames, reflect padding: tests/_signal_ref64.frame_index), or the one nearest the middle that the fewest cover"""
    import _signal_ref64 as sig
    idx = sig.frame_index(n_samples, n_fft, hop)
    covers = np.array([(idx == i).any(axis=1).sum() for i in range(n_samples)])
    two = np.flatnonzero(covers == 2)
    mid = int(two[0]) if two.size else int(np.argmin(covers + np.abs(np.arange(n_samples) - n_samples // 2) / (4.0 * n_samples)))
    return {"first": 0, "two-frames": mid, "last": n_samples - 1}


def stft_cone(n_samples, n_fft, hop, sample):
    """bool (frames,): the frames that hold the sample"""
    import _signal_ref64 as sig
    return (sig.frame_index(n_samples, n_fft, hop) == sample).any(axis=1)


def stft_poisoned(ref_clean, n_samples, n_fft, hop, sample, nan=True, polar=False):
    """ref_clean (2, n_fft / 2, frames) of one signal -> the reference with `sample` poisoned: in the frames that hold it every part
    whose coefficient is not exactly zero at (one of) its taps is NaN, the others UNHELD.  polar: the magnitude is NaN in every such
    bin (no tap has both coefficients zero), and so is the angle for a NaN; for an infinity the parts may be inf or NaN by the order of
    the butterflies and the angle of (inf, finite) is finite: UNHELD."""
    import _signal_ref64 as sig
    idx = sig.frame_index(n_samples, n_fft, hop)
    out = np.array(ref_clean, np.float64, copy=True)
    k = np.arange(1, n_fft // 2 + 1)[:, None]
    for t in np.flatnonzero((idx == sample).any(axis=1)):
        taps = np.flatnonzero(idx[t] == sample)[None, :]
        re_held, im_held = ~cos_is_zero(k, taps, n_fft).all(axis=1), ~sin_is_zero(k, taps, n_fft).all(axis=1)
        assert (re_held | im_held).all()
        if polar:
            out[0, :, t] = np.nan
            out[1, :, t] = np.nan if nan else UNHELD
        else:
            out[0, :, t] = np.where(re_held, np.nan, UNHELD)
            out[1, :, t] = np.where(im_held, np.nan, UNHELD)
    return out


def istft_cone(n_fft, hop, frames, frame):
    """bool (hop (frames - 1),): the samples frame `frame` overlaps after the n_fft / 2 trim"""
    t = np.arange(hop * (frames - 1)) + n_fft // 2
    return (t >= frame * hop) & (t < frame * hop + n_fft)


def istft_poisoned(ref_clean, n_fft, hop, frame, row, plane, mode):
    """ref_clean (hop (frames - 1),) of one signal -> the reference with the cell (row, frame) of plane `plane` poisoned: NaN on the
    samples the frame overlaps.  Mode 1 (re, im): UNHELD where the coefficient of that part -- cos for re, sin for im, of bin
    row + 1 -- is exactly zero; mode 0 makes both parts non-finite, and no sample has both coefficients zero."""
    out = np.array(ref_clean, np.float64, copy=True)
    frames = len(out) // hop + 1
    s = np.flatnonzero(istft_cone(n_fft, hop, frames, frame))
    m = s + n_fft // 2 - frame * hop
    out[s] = np.nan
    if mode == 1:
        zero = (cos_is_zero if plane == 0 else sin_is_zero)(row + 1, m, n_fft)
        out[s[zero]] = UNHELD
    return out


def normalised(ref_poisoned, nan):
    """y / max|y| per row of a poisoned reference, the maximum as np.max has it: a NaN among the values is the peak and takes the row.
    Poisoned with an infinity the cone holds inf or NaN by the order of the sums, so the peak is inf (the rest of the row becomes 0) or
    NaN (the rest becomes NaN): the rest of such a row is UNHELD"""
    rp = np.asarray(ref_poisoned, np.float64)
    held = np.isnan(rp)
    with np.errstate(invalid="ignore"):
        out = rp / np.abs(np.where(rp == UNHELD, 0.0, rp)).max(axis=1, keepdims=True)
    if not nan:
        out = np.where(held.any(axis=1, keepdims=True) & ~held, UNHELD, out)
    return np.where(rp == UNHELD, UNHELD, out)
