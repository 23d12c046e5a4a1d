"""Float64 restatements (numpy only) of the two contracts of the spectral track join, include/phasegen.h:

  spec_clips   clip windows of a plane (n_ch, bins, F_src), optionally resampled along time.  The positions and weights are the
               contract's own (double position, fp32 weight); the blend runs in float64 (``spec_clips``) or with fp32 rounding after
               every operation (``spec_clips_f32``: the kernel's bits).
  phase_join   one phase per global frame from overlapped clips (``phase_join``: float64 throughout, the fp32 ramp as given) and the
               complex blend z of every frame (``phase_join_z``), |z| being the conditioning of the angle.

Shared by tests/test_spectral_host.py and tests/test_z_spectral_gpu.py.
"""
import numpy as np


def ramp(Vf):
    """pg_stitch_ramp: float32(sin^2(pi (j + 0.5) / (2 Vf))), evaluated in double."""
    j = np.arange(Vf, dtype=np.float64)
    return (np.sin(np.pi * (j + 0.5) / (2.0 * Vf)) ** 2).astype(np.float32)


def _positions(n_clips, frames, sf, src_per_out, F_src):
    g = (np.arange(n_clips, dtype=np.int64)[:, None] * sf + np.arange(frames, dtype=np.int64)[None, :]).astype(np.float64)
    p = g * np.float64(src_per_out)
    fl = np.floor(p)
    i0 = np.minimum(fl, F_src - 1).astype(np.int64)
    i1 = np.minimum(i0 + 1, F_src - 1)
    w = (p - fl).astype(np.float32)
    return i0, i1, w                                              # each (n_clips, frames)


def spec_clips(P, n_clips, frames, sf, src_per_out=1.0):
    """P (n_ch, bins, F_src) -> (n_clips, n_ch, bins, frames) float64: a + w (b1 - a) without intermediate rounding."""
    P = np.asarray(P)
    i0, i1, w = _positions(n_clips, frames, sf, src_per_out, P.shape[2])
    a = P[:, :, i0].astype(np.float64)                            # (n_ch, bins, n_clips, frames)
    b1 = P[:, :, i1].astype(np.float64)
    out = np.where(w == 0, a, a + w.astype(np.float64) * (b1 - a))
    return np.ascontiguousarray(out.transpose(2, 0, 1, 3))


def spec_clips_f32(P, n_clips, frames, sf, src_per_out=1.0):
    """The same with every operation rounded to fp32, nothing contracted: fl(a + fl(w fl(b1 - a))), a itself where w == 0."""
    P = np.asarray(P, dtype=np.float32)
    i0, i1, w = _positions(n_clips, frames, sf, src_per_out, P.shape[2])
    a = P[:, :, i0]
    b1 = P[:, :, i1]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (b1 - a).astype(np.float32)
        m = (w * d).astype(np.float32)
        s = (a + m).astype(np.float32)
    out = np.where(w == 0, a, s)
    return np.ascontiguousarray(out.transpose(2, 0, 1, 3))


def _join_parts(phi, sf):
    phi = np.asarray(phi)
    n_clips, n_ch, bins, frames = phi.shape
    Vf = frames - sf
    assert 1 <= Vf and 2 * Vf <= frames and sf >= 1
    F_out = (n_clips - 1) * sf + frames
    g = np.arange(F_out)
    k = np.minimum(g // sf, n_clips - 1)
    j = g - k * sf
    shared = (k >= 1) & (j < Vf)
    return phi, Vf, F_out, k, j, shared


def phase_join_z(phi, sf, ramp_=None):
    """(z, shared): z (n_ch, bins, F_out) complex128, a e^{j lo} + b e^{j hi} on the shared frames and e^{j phi} elsewhere."""
    phi, Vf, F_out, k, j, shared = _join_parts(phi, sf)
    r = (ramp(Vf) if ramp_ is None else np.asarray(ramp_)).astype(np.float64)
    own = phi[k, :, :, j].astype(np.float64).transpose(1, 2, 0)   # phi[k][j]: (n_ch, bins, F_out)
    z = np.exp(1j * own)
    ks, js = k[shared], j[shared]
    lo = phi[ks - 1, :, :, js + sf].astype(np.float64).transpose(1, 2, 0)
    hi = own[:, :, shared]
    z[:, :, shared] = r[Vf - 1 - js] * np.exp(1j * lo) + r[js] * np.exp(1j * hi)
    return z, shared


def phase_join(phi, sf, ramp_=None):
    """phi (n_clips, n_ch, bins, frames) -> (n_ch, bins, F_out) float64: atan2 of the blend on the shared frames (the documented
    choice b >= a ? hi : lo where the blend is zero or not finite), the clip's own phase, unwrapped, everywhere else."""
    phi, Vf, F_out, k, j, shared = _join_parts(phi, sf)
    r = (ramp(Vf) if ramp_ is None else np.asarray(ramp_)).astype(np.float64)
    out = phi[k, :, :, j].astype(np.float64).transpose(1, 2, 0).copy()
    with np.errstate(invalid="ignore"):
        z, _ = phase_join_z(phi, sf, ramp_)
    ks, js = k[shared], j[shared]
    lo = phi[ks - 1, :, :, js + sf].astype(np.float64).transpose(1, 2, 0)
    hi = out[:, :, shared]
    zs = z[:, :, shared]
    bad = ~np.isfinite(zs) | (zs == 0)
    pick = np.where((r[js] >= r[Vf - 1 - js])[None, None, :], hi, lo)
    out[:, :, shared] = np.where(bad, pick, np.angle(zs))
    return out
