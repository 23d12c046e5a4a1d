"""numpy restatements of the five mapped contracts (include/phasegen.h: pg_spec_clips_map, pg_phase_vocoder_map, pg_phase_lock_map,
pg_phase_lock_linked_map, pg_ola_stretch_map) and of phasegen.track.TimeMap, word for word (no GPU, no phasegen import).  The device
must reproduce the first five BIT FOR BIT.  Built from tests/_vocoder_ref.py, _lock_ref.py and _transient_ref.py; changes none of them.

  clamp_pos          pc = !(p >= 0) ? 0 : (p > 2^52 ? 2^52 : p)
  positions          (i0, i1, w) of every entry of a position table
  spec_clips_map, phase_vocoder_map, phase_lock_map, phase_lock_linked_map, ola_stretch_map    the kernels' contracts
  TimeMap            anchors -> src_of_out / out_of_src in samples, piecewise linear with one division per segment
  mapped_plan        the plan of the mapped spectral join: (SpectralPlan fields..., pos, grains)
"""
import math

import numpy as np

import _lock_ref as lref
import _transient_ref as tref
from _vocoder_ref import angle_of, q

TWO52 = 4503599627370496.0


def clamp_pos(pos):
    p = np.asarray(pos, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(~(p >= 0.0), 0.0, np.where(p > TWO52, TWO52, p))


def positions(pos, F_src):
    """pos (n,) float64 -> i0, i1 (int64) and w = (float)(pc - floor(pc)) (float32)"""
    pc = clamp_pos(pos)
    fl = np.floor(pc)
    i0 = np.minimum(fl, F_src - 1).astype(np.int64)
    return i0, np.minimum(i0 + 1, F_src - 1), (pc - fl).astype(np.float32)


def spec_clips_map(P, n_clips, frames, sf, pos):
    """P (n_ch, bins, F_src) float32, pos ((n_clips - 1) sf + frames,) -> (n_clips, n_ch, bins, frames) float32:
    a where w == 0, else fl(a + fl(w fl(b1 - a)))."""
    P = np.asarray(P, np.float32)
    pos = np.asarray(pos, np.float64)
    assert pos.shape == ((n_clips - 1) * sf + frames,)
    i0, i1, w = positions(pos, P.shape[2])
    g = np.arange(n_clips, dtype=np.int64)[:, None] * sf + np.arange(frames, dtype=np.int64)[None, :]
    i0, i1, w = i0[g], i1[g], w[g]
    a, b1 = P[:, :, i0], P[:, :, i1]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (b1 - a).astype(np.float32)
        m = (w * d).astype(np.float32)
        s = (a + m).astype(np.float32)
    return np.ascontiguousarray(np.where(w == 0, a, s).transpose(2, 0, 1, 3))


def phase_vocoder_map(A, pos, M=None, reset_below=0.0):
    """A (..., F_src) float32, pos (F_out,) -> (..., F_out) float32: pg_phase_vocoder's scan over the positions of ``pos``."""
    A = np.asarray(A, np.float32)
    F_out = len(pos)
    i0, i1, _ = positions(pos, A.shape[-1])
    qA = q(A)
    floor = np.float32(reset_below)
    out = np.empty(A.shape[:-1] + (F_out,), np.float32)
    acc = np.zeros(A.shape[:-1], np.uint32)
    delta = np.zeros(A.shape[:-1], np.uint32)
    for g in range(F_out):
        if g == 0:
            reset = np.ones(A.shape[:-1], bool)
        elif M is None:
            reset = np.zeros(A.shape[:-1], bool)
        else:
            with np.errstate(invalid="ignore"):
                reset = np.asarray(M, np.float32)[..., i0[g]] < floor
        acc = np.where(reset, qA[..., i0[g]], acc + delta)
        delta = qA[..., i1[g]] - qA[..., i0[g]]
        out[..., g] = angle_of(acc)
    return out


def phase_lock_map(A, pos, M, reset_below=0.0, return_rotation=False):
    """A, M (..., bins, F_src) float32, pos (F_out,) -> (..., bins, F_out) float32: pg_phase_lock's recurrence, the advance into
    frame g measured between i1(g - 1) and i0(g)."""
    A, M = np.asarray(A, np.float32), np.asarray(M, np.float32)
    assert A.shape == M.shape and A.ndim >= 2
    lead, (bins, F_src) = A.shape[:-2], A.shape[-2:]
    A2, M2 = A.reshape(-1, bins, F_src), M.reshape(-1, bins, F_src)
    F_out = len(pos)
    i0, i1, _ = positions(pos, F_src)
    qA = q(A2)
    floor = np.float32(reset_below)
    out = np.empty((A2.shape[0], bins, F_out), np.float32)
    rot = np.empty((A2.shape[0], bins, F_out), np.uint32)
    for c in range(A2.shape[0]):
        T = np.zeros(bins, np.uint32)
        for g in range(F_out):
            a = qA[c, :, i0[g]]
            if g >= 1:
                m = M2[c, :, i0[g]]
                P = lref.peak_map(m)
                e = qA[c, :, i1[g - 1]] - a
                with np.errstate(invalid="ignore"):
                    reset = m[P] < floor
                T = np.where(reset, np.uint32(0), T[P] + e[P])
            rot[c, :, g] = T
            out[c, :, g] = angle_of(T + a)
    out, rot = out.reshape(lead + (bins, F_out)), rot.reshape(lead + (bins, F_out))
    return (out, rot) if return_rotation else out


def phase_lock_linked_map(A, Aref, Mref, pos, reset_below=0.0):
    A, Aref, Mref = np.asarray(A, np.float32), np.asarray(Aref, np.float32), np.asarray(Mref, np.float32)
    assert A.ndim == 3 and Aref.shape == Mref.shape == A.shape[1:]
    T = phase_lock_map(Aref, pos, Mref, reset_below, return_rotation=True)[1]
    i0, _, _ = positions(pos, A.shape[-1])
    return angle_of(T[None] + q(A)[..., i0])


def n_grains(n_out, win_len, hop):
    return (n_out + win_len // 2) // hop + 1


def ola_stretch_map(x, n_out, c, win, hop, base=None, dtype=np.float32):
    """x (n_sig, n_in), c (n_grains,) float64: one source centre per grain, cd = rint(c[g]); a centre that is NaN or beyond +-2^62 is
    outside every signal (it counts in den, not in num).  Everything else is tests/_transient_ref.py's ola_stretch."""
    x = np.asarray(x, dtype)
    win = np.asarray(win, dtype)
    c = np.asarray(c, np.float64)
    n_sig, n_in = x.shape
    w = win.shape[0]
    half = w // 2
    assert c.shape == (n_grains(n_out, w, hop),)
    t = np.arange(n_out, dtype=np.int64)
    g_lo, g_hi = tref.ola_frames(n_out, w, hop)
    with np.errstate(invalid="ignore"):
        cd = np.rint(c)
        inside_g = np.abs(cd) < 2.0 ** 62                                  # (False for a NaN)
    cg_g = np.where(inside_g, cd, 0.0).astype(np.int64)
    den, num = np.zeros(n_out, dtype), np.zeros((n_sig, n_out), dtype)
    for k in range(int((g_hi - g_lo).max()) + 1):
        g = g_lo + k
        covered = g <= g_hi
        gc = np.where(covered, g, 0)
        j = np.where(covered, t - g * hop + half, 0)
        assert ((j >= 0) & (j < w)).all()
        s = cg_g[gc] + j - half
        wj = win[j]
        den = np.where(covered, den + wj, den)
        term = covered & inside_g[gc] & (s >= 0) & (s < n_in)
        sc = np.where(term, s, 0)
        with np.errstate(invalid="ignore", over="ignore"):
            num = np.where(term, num + wj * x[:, sc], num)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0)).astype(dtype)
        return r if base is None else (np.asarray(base, dtype) + r).astype(dtype)


# ---- TimeMap -----------------------------------------------------------------------------------------------------------------------

class TimeMap:
    """phasegen.track.TimeMap restated: anchors (source_seconds, output_seconds) -> piecewise linear maps in samples at ``sr``; past
    the last anchor the last segment's line continues."""

    def __init__(self, anchors):
        a = np.asarray(anchors, np.float64)
        assert a.ndim == 2 and a.shape[1] == 2 and a.shape[0] >= 2
        self.src, self.out = a[:, 0].copy(), a[:, 1].copy()

    def _eval(self, x, xs, ys, sr):
        x = np.asarray(x, np.float64)
        xs, ys = xs * float(sr), ys * float(sr)
        k = np.clip(np.searchsorted(xs, x, side="right") - 1, 0, len(xs) - 1)     # (from the last anchor on: the last anchor)
        slope = (ys[1:] - ys[:-1]) / (xs[1:] - xs[:-1])                    # one division per segment
        return ys[k] + (x - xs[k]) * slope[np.minimum(k, len(xs) - 2)]

    def src_of_out(self, t, sr=16000):
        return self._eval(t, self.out, self.src, sr)

    def out_of_src(self, s, sr=16000):
        return self._eval(s, self.src, self.out, sr)


def mapped_plan(tm, a_len, frames, hop, overlap_frames, sr=16000, transient_hop=64, transient_window=256):
    """-> dict(sf, Vf, a_out, n_clips, F_out, F_src, n_src, pos, grains), the mapped sibling of phasegen.track.spectral_plan"""
    a_out = int(round(float(tm.out_of_src(a_len, sr))))
    T = hop * (frames - 1)
    step = T - overlap_frames * hop
    n_clips = 1 if a_out <= T else 1 + -(-(a_out - T) // step)
    sf, Vf = frames - 1 - overlap_frames, overlap_frames + 1
    F_out = (n_clips - 1) * sf + frames
    pos = tm.src_of_out(np.arange(F_out, dtype=np.float64) * hop, sr) / hop
    F_src = int(math.floor(pos.max())) + 2
    n_out = hop * (F_out - 1)
    grains = tm.src_of_out(np.arange(n_grains(n_out, transient_window, transient_hop), dtype=np.float64) * transient_hop, sr)
    return dict(sf=sf, Vf=Vf, a_out=a_out, n_clips=n_clips, F_out=F_out, F_src=F_src, n_src=hop * (F_src - 1), pos=pos, grains=grains)
