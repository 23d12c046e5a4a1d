"""Float64 restatements (numpy only) of the STFT / ISTFT contract of include/phasegen.h, the error scales of a frame and of an
output sample, and the two comparisons the value tests make.  Shared by tests/test_signal_bounds_host.py (which shows that the
comparisons reject planted faults and accept honest fp32 transforms) and tests/test_z_signal_values_gpu.py (the kernels).

  stft64     exact periodic Hann in float64 on the fp32 samples, reflect framing by index arithmetic, rfft, bin 0 dropped.
  istft64    zero DC row, Nyquist imaginary part ignored, window, overlap-add, / window-sum-square where > fp32 tiny, n_fft/2 trimmed.

u = 2^-24 (the unit roundoff of fp32) throughout.

Tier A (derived; holds for every input).  A transform is a sum of paths input -> output through unit-modulus coefficients, so
|dX_k| <= sum_n |x_n w_n| ((1 + eta_1) .. (1 + eta_s) - 1) with one eta per operation on the path.  Per operation:
  * a tabulated twiddle: sincospif is within 4 ulp (OpenCL's bound for sinpi / cospi; every argument the kernels pass is an
    integer over a power of two, hence exact), an ulp below 1 is at most u: 4 u per component, G_TW = 4 sqrt 2 u as a complex number;
  * a compile-time twiddle (radix-8 / radix-16 cores): rounded once, G_CONST = sqrt 2 / 2 u;
  * a complex product: sqrt 5 u (Brent, Percival, Zimmermann 2007; 2 u with an fma, the larger figure is used for both);
  * a level of butterfly additions: u.
  c_path = 1 [the product x w] + c_rel [the window, where it is relatively accurate: below] + tw_stages (G_TW + sqrt 5)
           + const_stages (G_CONST + sqrt 5) + log2(points) [additions].
  The half-length kernels end in the split X_k = A (1 - i w^k) / 2 + conj(B) (1 + i w^k) / 2 with A = Z_k, B = Z_{M-k}:
  |1 - i w^k| + |1 + i w^k| <= 2 sqrt 2, so c = sqrt 2 c_path + (G_TW + sqrt 5) [w^k O] + 3 [the additions of E, O and E + T].
      family      points  tw_stages                    const_stages  c_fft
      r2          N       log2 N (fft_lds)             0             18 + log2 N (G_TW + sqrt 5 + 1): 124.7 at 4096, 62.5 at 32
      frames      N / 2   floor(log4 M) - 1 radix-4 passes with twiddles (the first has none) + 1 closing radix-2 pass if log2 M
                          is odd      0                              53.2 at 32, 81.1 at 512
      w16         1024    2 (T1, T2)                   2 (radix16 x 2; the closing radix-4 has none)   57.1
      w8          512     2 (T1, T2)                   3 (radix8 x 3)                                   59.8
  The WINDOW.  r2 and frames multiply by hann_tap = sinpif(k / n)^2: sinpif within 4 ulp <= 8 u of its value, squared and rounded:
  c_rel = 17, relative to x_n w_n.  The wave kernels' hann_pair is accurate absolutely, not relatively (0.5 - 0.5 cos: w_n -> 0 at
  the frame edges while its error stays), so its term is scaled by sum |x_n| and not by sum |x_n w_n|: the base (cos, sin) within
  4 u each, one fma rotation by a rounded constant (<= 4.5 sqrt 2 u + u = 7.4 u on the cosine: w0 within 4.2 u), a second by
  (CD, SD) (8.9 u: w1 within 5.0 u); c_win = 5, c_rel = 0.  Together  |dX_k| <= u (c_fft sum |x_n w_n| + c_win sum |x_n|)
  = c_A u sum |x_n w_n| with c_A = c_fft + c_win kappa, kappa = sum |x_n| / sum |x_n w_n| (2.0 on white noise).

  Inverse: the same transforms run backwards (Hermitian build = the split, then the passes, then (1 / M) w), C - 1 additions of the
  overlap-add over the C covering frames and one division: c_A' = c_fft + 2 + C, scale A_i = sum_t w_t(i) g_t / wss_i with
  g_t = (2 / N) sum_k |X_kt| (>= max_n |irfft|); the window term is c_win u sum_t g_t / wss_i.  The fp32 window-sum-square adds
  eps_wss(i) |y_i|: the angle of tap n0 + j is reached by one sincospif and j <= 3 sample rotations, then one rotation per frame
  (wss_step); a rotation by a (4 sqrt 2 u)-accurate unit vector adds (4 sqrt 2 + sqrt 5) u <= 8 u to the error of (cos, sin), so at
  step s the window is within dw_s = (4 sqrt 2 + 8 (3 + s)) u / 2 + u / 2 and eps_wss = (sum_s 2 w_s dw_s + dw_s^2) / wss + C u.
  (The scalar overlap-add and the fused path's interior constants evaluate hann() = 0.5 - 0.5 cospif afresh, within 2.5 u: covered
  by the same figure.)
  Mode 0 adds per bin |dX| <= e^m (|m| + 2) u + u |e^m - 1| [exp2(m log2 e) - 1: the product's rounding, v_exp_f32, the subtraction]
  + |X| sqrt 2 (2.5e-7 + 6e-8 |phi|) [pg_fastmath.h's sincos bound] + 2 u |X|, carried to the samples like g_t.

Tier B (measured; the tight one).  r = |dX_k| / (u ||x w||_2) per frame (inverse: |dy_i| / (u sigma_i), sigma_i =
sqrt(sum_t (w_t(i) rho_t)^2) / wss_i, rho_t the RMS of frame t before windowing): r_max = the maximum, r_rms = the largest per-frame
RMS over bins (inverse: the RMS over the samples).  The threshold is MARGIN x the same statistic of an honest fp32 transform of
the same input (torch.fft on fp32 frames, built by the host test), never anything derived from the code under test.
"""
import numpy as np

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
MARGIN = 4.0
G_TW, G_CONST, C_MUL = 4.0 * 2.0 ** 0.5, 0.5 * 2.0 ** 0.5, 5.0 ** 0.5
C_WIN = {"r2": 0.0, "frames": 0.0, "w16": 5.0, "w8": 5.0}
C_REL = 17.0


def family_of(n_fft, single_frame=False):
    """The transform family that serves n_fft (tests/test_signal_families.py pins the rule)."""
    if single_frame or n_fft == 4096:
        return "r2"
    return {2048: "w16", 1024: "w8"}.get(n_fft, "frames")


def c_fft(family, n_fft):
    """The derived constant of the module docstring."""
    if family == "r2":
        L = n_fft.bit_length() - 1
        return 1.0 + C_REL + L * (G_TW + C_MUL + 1.0)
    if family == "frames":
        L = (n_fft // 2).bit_length() - 1
        tw, const, rel = L // 2 - 1 + L % 2, 0, C_REL
    else:
        (L, tw, const), rel = {"w16": (10, 2, 2), "w8": (9, 2, 3)}[family], 0.0
        assert n_fft == 2 << L
    path = 1.0 + rel + tw * (G_TW + C_MUL) + const * (G_CONST + C_MUL) + L
    return 2.0 ** 0.5 * path + G_TW + C_MUL + 3.0


def hann64(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def frame_index(n_samples, n_fft, hop):
    """idx[t, k]: the sample behind tap k of frame t (centred frames, numpy 'reflect' padding: the edge sample is not repeated)."""
    pos = np.arange(1 + n_samples // hop)[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    period = 2 * (n_samples - 1)
    m = np.mod(pos, period)
    return np.where(m < n_samples, m, period - m)


def _frames64(y, n_fft, hop):
    y = np.asarray(y)
    assert y.dtype == np.float32
    y2 = np.atleast_2d(y).astype(np.float64)
    return y2[:, frame_index(y2.shape[1], n_fft, hop)]                  # (signals, frames, n_fft)


def stft64(y, n_fft, hop):
    """y (n,) or (signals, n) float32 -> (2, n_fft/2, frames) or (signals, 2, n_fft/2, frames) float64."""
    Z = np.fft.rfft(_frames64(y, n_fft, hop) * hann64(n_fft), axis=2)[:, :, 1:]
    out = np.ascontiguousarray(np.stack([Z.real, Z.imag], axis=1).transpose(0, 1, 3, 2))
    return out[0] if np.ndim(y) == 1 else out


def forward_scales(y, n_fft, hop):
    """Per frame, each (signals, frames): l1w = sum |x_n w_n|, l1x = sum |x_n|, l2 = ||x w||_2."""
    f = np.abs(_frames64(y, n_fft, hop))
    fw = f * hann64(n_fft)
    return {"l1w": fw.sum(2), "l1x": f.sum(2), "l2": np.sqrt((fw * fw).sum(2))}


def forward_bound(scales, family, n_fft):
    """Tier A per frame, (signals, frames)."""
    return U * (c_fft(family, n_fft) * scales["l1w"] + C_WIN[family] * scales["l1x"])


def _cplx(a):
    a = np.asarray(a, np.float64)
    return a[..., 0, :, :] + 1j * a[..., 1, :, :]


def forward_errors(got, want, scales, bound):
    """got, want (signals, 2, bins, frames) -> {"a": largest |dX| / Tier A bound, "r_max", "r_rms"}.  A frame of zeros (a chunk's
    zero tail) has every scale 0: its bins must be exactly zero, and it stays out of the ratios."""
    d = np.abs(_cplx(got) - _cplx(want))                                # (signals, bins, frames)
    live = scales["l2"] > 0
    dead = d[np.broadcast_to(~live[:, None, :], d.shape)]
    assert dead.size == 0 or float(dead.max()) == 0.0, "a frame of zeros did not transform to zeros"
    safe = lambda s: np.where(live, s, 1.0)[:, None, :]
    r = d / (U * safe(scales["l2"]))
    return {"a": float((d / safe(bound)).max()), "r_max": float(r.max()), "r_rms": float(np.sqrt((r * r).mean(axis=1)).max())}


def accept(err, standin, margin=MARGIN):
    """(ok, tiers): tiers names what rejects -- "A" (the derived bound) and / or "B" (r_max or r_rms above margin x the stand-in's)."""
    tiers = ""
    if not err["a"] <= 1.0:
        tiers += "A"
    if not (err["r_max"] <= margin * standin["r_max"] and err["r_rms"] <= margin * standin["r_rms"]):
        tiers += "B"
    return tiers == "", tiers


def polar_check(pol, own, want, bound):
    """Fused polar output `pol` against the kernel's own (re, im) `own` and the float64 spectrum `want`, all (signals, 2, bins, frames);
    bound (signals, frames) is the Tier A bound.  Returns {"mag": largest relative deviation from log1p|own| (<= 6e-7),
    "ang": largest |d theta| / (5e-7 + bound / |X|) over the bins with bound / |X| < 1 (<= 1), "excluded": share of the other bins}."""
    pol = np.asarray(pol, np.float64)
    mag = np.log1p(np.abs(_cplx(own)))
    rel = np.abs(pol[:, 0] - mag) / np.maximum(mag, 1e-300)
    z = _cplx(want)
    live = np.broadcast_to((bound > 0)[:, None, :], z.shape)            # a frame of zeros: log1p 0 = 0 and angle 0 = 0, exactly
    assert float(np.abs(pol[:, 0][~live]).max(initial=0.0)) == 0.0 and float(np.abs(pol[:, 1][~live]).max(initial=0.0)) == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = bound[:, None, :] / np.abs(z)
    keep = live & (cond < 1.0)
    dth = np.abs(np.angle(np.exp(1j * (pol[:, 1] - np.angle(z)))))
    return {"mag": float(rel.max()), "ang": float((dth[keep] / (5e-7 + cond[keep])).max()), "excluded": float(1.0 - keep[live].mean())}


def spectrum64(a, b, mode):
    """The complex spectrum a pg_istft call means, in float64: mode 1 (re, im); mode 0 (log-magnitude, phase) -> (e^m - 1) e^{j phi}."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32
    a, b = a.astype(np.float64), b.astype(np.float64)
    return a + 1j * b if mode == 1 else np.expm1(a) * np.exp(1j * b)


def istft64(re, im, hop, mode=1):
    """re, im (signals, bins, frames) float32 (or the two mode-0 planes) -> (y (signals, hop (frames - 1)) float64, info), info
    holding per sample: "wss" (signals-independent, the trimmed window-sum-square), "A", "B", "mode0" (Tier A scales: see the module
    docstring; "mode0" is already an absolute bound), "sigma" (Tier B), "C" (covering frames), "eps_wss"."""
    X = spectrum64(re, im, mode)
    S, bins, T = X.shape
    N = 2 * bins
    full = np.zeros((S, T, bins + 1), np.complex128)
    full[:, :, 1:] = X.transpose(0, 2, 1)
    full[:, :, bins] = full[:, :, bins].real
    raw = np.fft.irfft(full, n=N, axis=2)                               # (signals, frames, N)
    w = hann64(N)
    g = (2.0 / N) * np.abs(X).sum(1)                                    # (signals, frames)
    rho = np.sqrt((raw * raw).mean(2))
    if mode == 0:
        m, phi = np.asarray(re, np.float64), np.asarray(im, np.float64)
        dX = np.exp(m) * (np.abs(m) + 2.0) * U + U * np.abs(np.expm1(m)) + np.abs(X) * (2.0 ** 0.5 * (2.5e-7 + 6e-8 * np.abs(phi)) + 2 * U)
        g0 = (2.0 / N) * dX.sum(1)
    else:
        g0 = np.zeros_like(g)
    total = N + hop * (T - 1)
    acc, wss, cover = np.zeros((S, total)), np.zeros(total), np.zeros(total)
    A, B, M0, sg, dws = np.zeros((S, total)), np.zeros((S, total)), np.zeros((S, total)), np.zeros((S, total)), np.zeros(total)
    for t in range(T):
        sl = slice(t * hop, t * hop + N)
        acc[:, sl] += raw[:, t] * w
        A[:, sl] += w * g[:, t:t + 1]
        B[:, sl] += g[:, t:t + 1]
        M0[:, sl] += w * g0[:, t:t + 1]
        sg[:, sl] += (w * rho[:, t:t + 1]) ** 2
        # the rotation recurrence: this frame is step number `cover` (frames so far) of each sample it covers
        dw = ((G_TW + 8.0 * (3.0 + cover[sl])) / 2.0 + 0.5) * U
        dws[sl] += 2.0 * w * dw + dw * dw
        wss[sl] += w * w
        cover[sl] += 1
    nz = wss > TINY
    div = np.where(nz, wss, 1.0)
    keep = slice(N // 2, total - N // 2)
    info = {"wss": wss[keep], "A": (A / div)[:, keep], "B": (B / div)[:, keep], "mode0": (M0 / div)[:, keep],
            "sigma": (np.sqrt(sg) / div)[:, keep], "C": cover[keep], "eps_wss": (dws / div + cover * U)[keep]}
    return (acc / div)[:, keep], info


def inverse_bound(y64, info, family, n_fft):
    """Tier A per sample, (signals, samples)."""
    c = c_fft(family, n_fft) + 2.0 + info["C"]
    return U * (c * info["A"] + C_WIN[family] * info["B"]) + info["eps_wss"] * np.abs(y64) + info["mode0"]


def inverse_errors(got, y64, info, bound):
    d = np.abs(np.asarray(got, np.float64) - y64)
    live = info["sigma"] > 0
    assert float(d[~live].max(initial=0.0)) == 0.0, "a sample no frame contributes to is not zero"
    r = d / (U * np.where(live, info["sigma"], 1.0))
    return {"a": float((d / np.where(live, bound, 1.0)).max()), "r_max": float(r.max()), "r_rms": float(np.sqrt((r * r).mean()))}


def dft_direct(frames):
    """O(N^2) DFT in float64 of real frames (.., N) -> bins 0 .. N/2 (the independent check of the rfft / irfft calls above)."""
    N = frames.shape[-1]
    k = np.arange(N // 2 + 1)
    return frames @ np.exp(-2j * np.pi * np.outer(np.arange(N), k) / N)


def white(seed, signals, n):
    from phasegen import detgen
    return detgen.normal(seed, (signals, n))


def on_bin_cosine(signals, n, n_fft, k0):
    """k0 cycles per n_fft, amplitude 0.5, one phase per signal: interior frames hold bins k0 and k0 +- 1 only."""
    t = np.arange(n, dtype=np.float64)
    return np.stack([0.5 * np.cos(2.0 * np.pi * k0 * t / n_fft + 0.7 * s) for s in range(signals)]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# The fp32 stand-ins: honest single-precision transforms whose error sets Tier B's threshold.  Windows, framing and the overlap-add
# are written out here; the transform itself is torch.fft on float32 (`fft=None`) or the radix-2 Stockham emulation below, which
# is the algorithm of fft_lds in numpy float32 with tabulated float32 twiddles.  `win32` and `twiddles` let the host test plant faults.
def window32(n):
    return hann64(n).astype(np.float32)


def stockham_twiddles(N):
    a = -2.0 * np.pi * np.arange(N // 2) / N
    return (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)


def stockham_fft(x, sign=1.0, twiddles=None):
    """Radix-2 Stockham autosort FFT along the last axis of complex64 x (N a power of two), every operation in float32.
    twiddles: {stage number: table} overrides (stage 0 is Ns = 1); sign = -1 conjugates the table (the inverse, unnormalised)."""
    x = np.ascontiguousarray(x, np.complex64)
    N = x.shape[-1]
    half, j = N // 2, np.arange(N // 2)
    base = stockham_twiddles(N)
    Ns, stage = 1, 0
    while Ns < N:
        tw = base if not twiddles or stage not in twiddles else twiddles[stage]
        k = j & (Ns - 1)
        w = tw[k * (half // Ns)]
        if sign < 0:
            w = np.conj(w)
        v = (x[..., half:] * w).astype(np.complex64)
        y = np.empty_like(x)
        j0 = 2 * j - k
        y[..., j0] = x[..., :half] + v
        y[..., j0 + Ns] = x[..., :half] - v
        x, Ns, stage = y, 2 * Ns, stage + 1
    return x


def _rfft32(fr, fft):
    if fft is None:
        import torch
        return torch.fft.rfft(torch.from_numpy(fr), dim=2).numpy()
    return fft(fr.astype(np.complex64))[:, :, :fr.shape[2] // 2 + 1]


def standin_stft(y, n_fft, hop, win32=None, fft=None):
    """(signals, n) float32 -> (signals, 2, n_fft/2, frames) float32."""
    y2 = np.atleast_2d(np.asarray(y))
    assert y2.dtype == np.float32
    w = window32(n_fft) if win32 is None else win32
    fr = y2[:, frame_index(y2.shape[1], n_fft, hop)] * w
    assert fr.dtype == np.float32
    Z = _rfft32(fr, fft)[:, :, 1:]
    assert Z.dtype == np.complex64
    return np.ascontiguousarray(np.stack([Z.real, Z.imag], axis=1).transpose(0, 1, 3, 2))


def standin_frames(re, im, mode=1, fft=None):
    """The unwindowed fp32 time-domain frames (signals, frames, n_fft) of a spectrum given as pg_istft takes it."""
    a, b = np.asarray(re), np.asarray(im)
    assert a.dtype == np.float32 and b.dtype == np.float32
    if mode == 0:
        mag = np.exp(a) - np.float32(1.0)
        a, b = mag * np.cos(b), mag * np.sin(b)
    S, bins, T = a.shape
    N = 2 * bins
    full = np.zeros((S, T, bins + 1), np.complex64)
    full[:, :, 1:] = (a + 1j * b).transpose(0, 2, 1)
    full[:, :, bins] = full[:, :, bins].real
    if fft is None:
        import torch
        raw = torch.fft.irfft(torch.from_numpy(full), n=N, dim=2).numpy()
    else:
        herm = np.concatenate([full, np.conj(full[:, :, bins - 1:0:-1])], axis=2)
        raw = fft(herm).real * np.float32(1.0 / N)
    assert raw.dtype == np.float32
    return raw


def standin_ola(raw, hop, win32=None, wss32=None):
    """Window, overlap-add in frame order, divide by the window-sum-square and trim, all in float32.  raw (signals, frames, n_fft)."""
    S, T, N = raw.shape
    w = window32(N) if win32 is None else win32
    total = N + hop * (T - 1)
    acc, wss = np.zeros((S, total), np.float32), np.zeros(total, np.float32)
    for t in range(T):
        acc[:, t * hop:t * hop + N] += raw[:, t] * w
        wss[t * hop:t * hop + N] += w * w
    if wss32 is not None:
        wss = wss32(wss)
    out = np.where(wss > TINY, acc / np.where(wss > TINY, wss, np.float32(1.0)), acc)
    assert out.dtype == np.float32
    return out[:, N // 2:total - N // 2]


def standin_istft(re, im, hop, mode=1, fft=None):
    return standin_ola(standin_frames(re, im, mode, fft), hop)
