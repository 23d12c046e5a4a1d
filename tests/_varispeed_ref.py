"""numpy restatement of pg_varispeed's contract (include/phasegen.h) word for word, for the pitch-curve tests (no GPU, no phasegen
import; not collected): float64 positions, float32 sums, every operation rounded on its own.

  table(Z, L, beta, r)              the pairs (h_i, d_i) in float64 arithmetic rounded once, as pg_varispeed_table builds them
  positions(pos, scale, n_out, step)   (p, s) of every output
  varispeed(x, pos, scale, n_out, step, Z, L, tab)        the contract: float32 result, and the mask of taps per output on request
  varispeed_exact(x, pos, scale, n_out, step, Z, L, beta, r)   the float64 variant that evaluates h itself instead of the table: the
                                    accuracy yardstick; also returns sum |w x| per output, the scale of the float32 chain's rounding
"""
import numpy as np

FILTERS = {"kaiser_best": (64, 14.769656459379492, 0.9475937167399596), "kaiser_fast": (16, 8.555504641634386, 0.85)}   # resampy's
TINY = (4, 8, 3.0, 0.9)                                           # (Z, L, beta, r) of the small filter of the GPU tests
TILE = 1024                                                       # outputs per workgroup of the kernel (csrc/varispeed.hip, VS_TILE)
WIN_MAX = 12288                                                   # floats of its staged window (VS_WIN_MAX)


def h_exact(t, Z, beta, r):
    """h(t) = r sinc(r t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta) for |t| <= Z, else 0, in float64"""
    t = np.asarray(t, np.float64)
    a = np.pi * r * t
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    c = np.maximum(1.0 - (t / Z) ** 2, 0.0)
    return np.where(np.abs(t) <= Z, r * sinc * np.i0(beta * np.sqrt(c)) / np.i0(beta), 0.0)


def table(Z, L, beta, r):
    """(Z L + 1, 2) float32: h_i = float32(h(i / L)), d_i = fl32(h_{i+1} - h_i) of the rounded values, d_{ZL} = 0"""
    h = h_exact(np.arange(Z * L + 1, dtype=np.float64) / L, Z, beta, r).astype(np.float32)
    d = np.zeros_like(h)
    d[:-1] = h[1:] - h[:-1]
    return np.stack([h, d], axis=1)


def pc(p):
    """the mapped kernels' clamp: a NaN or a negative position counts as 0, anything above 2^52 as 2^52"""
    p = np.asarray(p, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(~(p >= 0.0), 0.0, np.where(p > 2.0 ** 52, 2.0 ** 52, p))


def sc(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(~(v >= np.float32(0.25)), np.float32(0.25), np.where(v > np.float32(1.0), np.float32(1.0), v)).astype(np.float32)


def positions(pos, scale, n_out, step):
    t = np.arange(n_out, dtype=np.int64)
    j = t // step
    q = t - j * step
    P = pc(pos)
    delta = (P[j + 1] - P[j]) * (1.0 / step)
    p = P[j] + q.astype(np.float64) * delta
    return p, sc(scale)[j]


def _taps(p, s, n_in, Z, L):
    """for k = -4Z .. 4Z + 1 around floor(p): (n, u, in the sum), n ascending"""
    n0 = np.floor(p).astype(np.int64)
    sL = s.astype(np.float64) * L
    for k in range(-4 * Z, 4 * Z + 2):
        n = n0 + k
        u = np.abs(p - n.astype(np.float64)) * sL
        yield n, u, (n >= 0) & (n < n_in) & (u < Z * L)


def staged_tiles(pos, n_out, step, n_in, Z):
    """which workgroups of the kernel stage their window in LDS (csrc/varispeed.hip; NOT part of the contract -- the tests use it
    only to make sure that a table exercises the path it is meant to): tile k covers the outputs [k TILE, (k + 1) TILE); its span
    is [floor(min P) - 4 Z - 2, floor(max P) + 4 Z + 3] over the clamped block ends it touches, cut to the row"""
    P = pc(pos)
    out = []
    for t0 in range(0, n_out, TILE):
        j0, j1 = t0 // step, (min(t0 + TILE, n_out) - 1) // step
        lo, hi = P[j0:j1 + 2].min(), P[j0:j1 + 2].max()
        w_lo, w_hi = max(int(np.floor(lo)) - 4 * Z - 2, 0), min(int(np.floor(hi)) + 4 * Z + 3, n_in - 1)
        out.append(w_hi - w_lo + 1 <= WIN_MAX)
    return np.array(out)


def varispeed(x, pos, scale, n_out, step, Z, L, tab, return_support=False):
    """x (n_in,) or (n_sig, n_in) float32 -> (..., n_out) float32 by the contract.  ``return_support``: also the (n_out, n_in) boolean
    matrix of the taps every output adds."""
    x = np.asarray(x, np.float32)
    x2 = x[None] if x.ndim == 1 else x
    n_sig, n_in = x2.shape
    tab = np.asarray(tab, np.float32).reshape(-1, 2)
    p, s = positions(pos, scale, n_out, step)
    acc = np.zeros((n_sig, n_out), np.float32)
    support = np.zeros((n_out, n_in), bool) if return_support else None
    with np.errstate(invalid="ignore", over="ignore"):
        for n, u, ok in _taps(p, s, n_in, Z, L):
            fl = np.floor(u)
            i = np.where(ok, fl, 0.0).astype(np.int64)
            eta = (u - fl).astype(np.float32)
            w = ((tab[i, 0] + eta * tab[i, 1]).astype(np.float32) * s).astype(np.float32)
            xv = x2[:, np.clip(n, 0, n_in - 1)]
            nxt = (acc + (w[None] * xv).astype(np.float32)).astype(np.float32)
            acc = np.where(ok[None], nxt, acc)
            if return_support:
                support[np.nonzero(ok)[0], n[ok]] = True
    y = acc[0] if x.ndim == 1 else acc
    return (y, support) if return_support else y


def varispeed_exact(x, pos, scale, n_out, step, Z, L, beta, r):
    """the same sum in float64 with w = s h(u / L) evaluated exactly: (y, sum |w x|), each (..., n_out) float64"""
    x = np.asarray(x, np.float64)
    x2 = x[None] if x.ndim == 1 else x
    n_sig, n_in = x2.shape
    p, s = positions(pos, scale, n_out, step)
    acc, mag = np.zeros((n_sig, n_out)), np.zeros((n_sig, n_out))
    for n, u, ok in _taps(p, s, n_in, Z, L):
        w = np.where(ok, s.astype(np.float64) * h_exact(u / L, Z, beta, r), 0.0)
        term = w[None] * x2[:, np.clip(n, 0, n_in - 1)]
        acc += np.where(ok[None], term, 0.0)
        mag += np.where(ok[None], np.abs(term), 0.0)
    return (acc[0], mag[0]) if x.ndim == 1 else (acc, mag)
