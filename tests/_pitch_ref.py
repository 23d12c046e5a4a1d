"""numpy restatement of pg_pitch_track's contract (include/phasegen.h) word for word, for the pitch-detection tests (no GPU, no
phasegen import; not collected): every operation rounded on its own in ``dtype``.

  pitch_track(x, frames, hop, W, tau_min, tau_max, theta, dtype=np.float32, details=False)
        the contract: (period, ap) of every frame of every row, float32 bit for bit with the kernel; with dtype=np.float64 the same
        steps in double, the accuracy yardstick.  details=True also returns (tau_hat, cm): the picked lag per frame (-1 behind the
        non-finite gate) and the normalised difference (rows, frames, tau_max + 1)
  cone(i, frames, hop, W, tau_max)      the frames whose W + tau_max samples hold sample i
  take(notes, sr, ...)                  a monophonic test take with exactly known f0: harmonic tones, 10 ms attack, 1e-3 noise
  cents(f, f_ref)                       1200 log2(f / f_ref)
"""
import numpy as np

SPECTRUM = (1.0, 0.5, 0.25, 0.1)                                  # the harmonic amplitudes of ``take``
WEAK_FUNDAMENTAL = (0.05, 1.0, 0.7, 0.5)
SINE = (1.0,)


def pitch_track(x, frames, hop, W, tau_min, tau_max, theta, dtype=np.float32, details=False):
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype)
    one = x.ndim == 1
    x2 = x[None] if one else x
    n_sig, n_in = x2.shape
    frames, hop, W, tau_min, tau_max = int(frames), int(hop), int(W), int(tau_min), int(tau_max)
    assert frames >= 1 and hop >= 1 and 2 <= tau_min < tau_max
    need = (frames - 1) * hop + W + tau_max
    xp = np.zeros((n_sig, max(need, n_in)), dtype)                # a sample at or beyond n_in counts as +0.0
    xp[:, :n_in] = x2
    T1 = tau_max + 1
    base = (np.arange(frames) * hop)[:, None] + np.arange(T1)[None, :]            # (frames, T1): f hop + tau
    start = np.arange(frames) * hop
    period = np.empty((n_sig, frames), dtype)
    ap = np.empty((n_sig, frames), dtype)
    tau_hat = np.full((n_sig, frames), -1, np.int64)
    cm_all = np.empty((n_sig, frames, T1), dtype)
    theta = dt(theta)
    with np.errstate(all="ignore"):
        for s in range(n_sig):
            row = xp[s]
            d = np.zeros((frames, T1), dtype)                     # 1. the difference function, the chain over j ascending
            for j in range(W):
                e = row[start + j][:, None] - row[base + j]
                d = d + e * e
            d[:, 0] = 0
            S = np.zeros((frames, T1), dtype)                     # 2. the running sum, ascending
            for t in range(1, T1):
                S[:, t] = S[:, t - 1] + d[:, t]
            tau = np.arange(T1).astype(dtype)[None, :]
            cm = np.where(S > 0, (d * tau) / np.where(S > 0, S, dt(1)), dt(1)).astype(dtype)     # 4.
            cm[:, 0] = 1
            cm_all[s] = cm
            for f in range(frames):
                if not np.isfinite(S[f, tau_max]):                # 3. the non-finite gate
                    period[s, f] = ap[s, f] = np.nan
                    cm_all[s, f] = np.nan
                    continue
                c = cm[f]
                A = np.arange(tau_min, tau_max)                   # 5. A = [tau_min, tau_max - 1]
                below = A[c[A] < theta]
                if below.size:
                    t = int(below[0])
                    while t + 1 <= tau_max - 1 and c[t + 1] < c[t]:
                        t += 1
                else:
                    t = int(A[np.argmin(c[A])])                   # (argmin: the first index that attains the minimum)
                tau_hat[s, f] = t
                a_, b_, c_ = c[t - 1], c[t], c[t + 1]             # 6. the parabola through the three
                den = dt(dt(a_ + c_) - dt(dt(2) * b_))
                if den > 0:
                    q = dt(dt(dt(0.5) * dt(a_ - c_)) / den)
                    delta = dt(-1) if q < -1 else (dt(1) if q > 1 else q)
                else:
                    delta = dt(0)
                period[s, f] = dt(dt(t) + delta)
                ap[s, f] = b_
    if one:
        period, ap, tau_hat, cm_all = period[0], ap[0], tau_hat[0], cm_all[0]
    return (period, ap, tau_hat, cm_all) if details else (period, ap)


def cone(i, frames, hop, W, tau_max):
    """bool (frames,): the frames f with f hop <= i < f hop + W + tau_max"""
    f = np.arange(frames) * hop
    return (f <= i) & (i < f + W + tau_max)


def take(notes, sr=16000, spectrum=SPECTRUM, attack_ms=10.0, noise=1e-3, seed=0, amplitude=0.5):
    """A monophonic take: ``notes`` = [(f0 in Hz, seconds), ...], each a harmonic tone sum_k spectrum[k] sin(2 pi (k + 1) f0 t) from
    phase 0 with a linear attack of ``attack_ms``, scaled to ``amplitude`` / sum(spectrum), plus white noise of standard deviation
    ``noise``.  -> (float32 samples, f0 per sample in float64)"""
    rs = np.random.RandomState(seed)
    parts, f0s = [], []
    for f0, seconds in notes:
        n = int(round(seconds * sr))
        t = np.arange(n, dtype=np.float64) / sr
        y = sum(a * np.sin(2 * np.pi * (k + 1) * f0 * t) for k, a in enumerate(spectrum))
        ramp = np.minimum(1.0, np.arange(n) / max(1.0, attack_ms * 1e-3 * sr))
        parts.append(y * ramp * (amplitude / sum(spectrum)))
        f0s.append(np.full(n, float(f0)))
    y = np.concatenate(parts)
    return (y + noise * rs.standard_normal(y.shape[0])).astype(np.float32), np.concatenate(f0s)


def cents(f, f_ref):
    return 1200.0 * np.log2(np.asarray(f, np.float64) / np.asarray(f_ref, np.float64))
