"""GPU: pg_resample (ops.resample) against a float64 restatement of its definition (include/phasegen.h), and the preprocessing
pipeline built on it (phasegen.preproc: load_audio, resample, get_mix_chunks, build_dataset(osr=...)).

The value bound is derived, not measured: an output is a sum of `taps` products bank * x.  Whatever the order, fp32 summation of
n terms is within n * 2^-24 * sum|terms| of exact (first order); the bank entry and the product carry one rounding each (the
kernel's fused multiply-add spares the second; the bound does not rely on it).  So for every output
    |y - y64| <= (taps + 2) * 2^-24 * max_p sum_k |bank[k, p]| * max|x|
which is 4.9e-5 max|x| at 160 / 441 kaiser_best and 2.0e-5 at 441 / 160."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# ---- float64 restatement of the definition (include/phasegen.h; tied to scipy.signal.upfirdn in test_resample_host.py) -------
FILTERS = {0: (64, 14.769656459379492, 0.9475937167399596), 1: (16, 8.555504641634386, 0.85)}   # quality: Z, beta, roll-off
QUALITY = {0: "kaiser_best", 1: "kaiser_fast"}


def geometry(up, down, quality):
    g = math.gcd(up, down)
    U, D = up // g, down // g
    W = Fraction(FILTERS[quality][0]) / min(Fraction(1), Fraction(U, D))
    return U, D, math.floor(W), math.floor(W) + math.ceil(W) + 1                   # U, D, H, taps


def h64(t, quality):
    Z, beta, r = FILTERS[quality]
    t = np.asarray(t, np.float64)
    win = np.i0(beta * np.sqrt(np.clip(1.0 - (t / Z) ** 2, 0.0, None))) / np.i0(beta)
    return np.where(np.abs(t) <= Z, r * np.sinc(r * t) * win, 0.0)


def bank64(up, down, quality):
    """(taps, U): s h(s (p/U + H - k)), the argument as ONE division of exact integers, (p + U (H - k)) / max(U, D), so that
    |t| <= Z is decided exactly at the edge of the support."""
    U, D, H, taps = geometry(up, down, quality)
    k, p = np.arange(taps)[:, None], np.arange(U)[None, :]
    return min(1.0, U / D) * h64((p + U * (H - k)) / max(U, D), quality)


def out_len(n_in, up, down):
    g = math.gcd(up, down)
    return (n_in * (up // g) + down // g - 1) // (down // g)


def direct64(x, up, down, quality, ts=None, bank=None):
    """y[t] = sum_k bank[k, p] x[n0 - H + k] in float64 for the outputs ``ts`` (default: all), x zero outside its ends."""
    U, D, H, taps = geometry(up, down, quality)
    b = bank64(up, down, quality) if bank is None else bank
    x = np.asarray(x, np.float64)
    ts = np.arange(out_len(len(x), up, down)) if ts is None else np.asarray(ts, np.int64)
    n0, p = np.divmod(ts * D, U)
    n = (n0 - H)[:, None] + np.arange(taps)[None, :]
    xs = np.where((n >= 0) & (n < len(x)), x[np.clip(n, 0, len(x) - 1)], 0.0)
    return np.einsum("tk,kt->t", xs, b[:, p])
# -------------------------------------------------------------------------------------------------------------------------------


def bound(up, down, quality, xmax):
    U, D, H, taps = geometry(up, down, quality)
    return (taps + 2) * 2.0 ** -24 * np.abs(bank64(up, down, quality)).sum(axis=0).max() * xmax


def test_the_bound_is_what_the_docstring_says():
    assert abs(bound(160, 441, 0, 1.0) - 4.9e-5) < 1e-6 and abs(bound(441, 160, 0, 1.0) - 2.0e-5) < 1e-6


# (up, down, quality) -> outputs per workgroup (csrc/resample.hip, rs_plan: 4 S with S the first multiple of U that keeps 90 % of
# 256 lanes busy; the last line is the one-output-per-lane kernel, taken where 4 D + taps input samples do not fit its LDS window)
TILE = {(160, 441): 1920, (441, 160): 7056, (1, 2): 924, (2, 1): 928, (3, 2): 924, (147, 160): 2940,
        (1000, 3101): 1024}


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("up,down", list(TILE))
def test_values_against_the_float64_direct_sum(up, down, quality):
    """3 signals in a buffer with 37 NaNs behind every row; y pre-filled with a sentinel, rows n_out + 5 apart."""
    from phasegen import ops
    U, D, H, taps = geometry(up, down, quality)
    tile, edge = TILE[(up, down)], TILE[(up, down)] * D // U
    b64 = bank64(up, down, quality)
    lens = [1, 100, 2823, 2824, 7001, edge - 1, edge, edge + 1, 2 * edge + 1]
    assert out_len(edge, up, down) <= tile < out_len(edge + 1, up, down)           # one either side of a workgroup's tile
    rng = np.random.default_rng(up * 7 + down + quality)
    for n_in in lens:
        n_out = out_len(n_in, up, down)
        x = rng.standard_normal((3, n_in)).astype(np.float32)
        xb = torch.full((3, n_in + 37), float("nan"), device="cuda")
        xb[:, :n_in] = torch.from_numpy(x).cuda()
        yb = torch.full((3, n_out + 5), -12345.0, device="cuda")
        y = ops.resample(xb[:, :n_in], down, up, res_type=QUALITY[quality], out=yb[:, :n_out])
        assert y.data_ptr() == yb.data_ptr() and tuple(y.shape) == (3, n_out)
        got = yb.cpu().numpy()
        assert (got[:, n_out:] == -12345.0).all(), n_in                             # nothing written past a row
        assert np.isfinite(got[:, :n_out]).all(), n_in                              # the NaN padding was never used
        tol = bound(up, down, quality, np.abs(x).max())
        for s in range(3):
            err = np.abs(got[s, :n_out] - direct64(x[s], up, down, quality, bank=b64)).max()
            assert err <= tol, (n_in, s, err, tol)


@pytest.mark.parametrize("up,down", [(160, 441), (441, 160), (1000, 3101)])
def test_a_signal_alone_equals_the_same_signal_in_a_batch(up, down):
    from phasegen import ops
    n_in = 6001
    x = torch.randn(3, n_in, device="cuda")
    res = "kaiser_fast" if up == 1000 else "kaiser_best"
    batch = ops.resample(x, down, up, res_type=res)
    wide = torch.full((3, n_in + 11), float("nan"), device="cuda")
    wide[:, :n_in] = x
    assert torch.equal(ops.resample(wide[:, :n_in], down, up, res_type=res), batch)
    for s in range(3):
        alone = ops.resample(x[s].clone(), down, up, res_type=res)
        assert alone.dim() == 1 and torch.equal(alone, batch[s]), s
        assert torch.equal(ops.resample(x[s:s + 1], down, up, res_type=res)[0], batch[s])


def test_unreduced_rates_equal_the_reduced_ratio():
    from phasegen import ops
    x = torch.randn(2, 5000, device="cuda")
    for res in ("kaiser_best", "kaiser_fast"):
        assert torch.equal(ops.resample(x, 44100, 16000, res_type=res), ops.resample(x, 441, 160, res_type=res))
        assert torch.equal(ops.resample(x, 16000, 44100, res_type=res), ops.resample(x, 160, 441, res_type=res))
    assert ops.resample(x, 16000, 16000) is x                                       # librosa's pass-through


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("up,down", [(160, 441), (441, 160), (3, 2)])
def test_impulse_reproduces_the_bank_exactly(up, down, quality):
    """x = unit impulse at n = 500 of 1500: y[t] = bank[k U + p] with k = 500 - n0 + H wherever 0 <= k < taps, else 0 -- exactly
    (a multiplication by 1.0 and additions of 0.0 are exact)."""
    from phasegen import ops
    U, D, H, taps = geometry(up, down, quality)
    bank = ops.resample_bank_host(up, down, quality)                                # (taps, U) float32, as the kernel reads it
    x = torch.zeros(1500, device="cuda")
    x[500] = 1.0
    y = ops.resample(x, down, up, res_type=QUALITY[quality]).cpu().numpy()
    t = np.arange(out_len(1500, up, down))
    n0, p = np.divmod(t * D, U)
    k = 500 - n0 + H
    want = np.where((k >= 0) & (k < taps), bank[np.clip(k, 0, taps - 1), p], np.float32(0.0))
    assert len(y) == len(t) and np.count_nonzero(want) > taps * min(U, D) // D - 4
    assert np.array_equal(y, want)


def test_tones_pass_and_stop():
    """44.1 -> 16 kHz, kaiser_best, one second; interior samples (400 dropped at each end).  The float64 filter itself reproduces
    a 1 kHz tone to 7e-9 and leaves 2e-8 of a 10 kHz tone (above the new Nyquist); adding the fp32 rounding bound of this
    module's docstring (4.9e-5 for |x| <= 1, loose by orders of magnitude for a smooth signal) gives the 5e-5 asserted here."""
    from phasegen import ops
    n = np.arange(44100)
    for f, passes in ((1000.0, True), (10000.0, False)):
        x = np.sin(2 * np.pi * f * n / 44100.0)
        y = ops.resample(torch.from_numpy(x.astype(np.float32)).cuda(), 44100, 16000).cpu().numpy().astype(np.float64)
        assert len(y) == 16000
        want = np.sin(2 * np.pi * f * np.arange(16000) / 16000.0) if passes else np.zeros(16000)
        err = np.abs(y - want)[400:-400].max()
        assert err <= 5e-5, (f, err)


@pytest.mark.parametrize("up,down,n_in,cross", [(160, 441, 13_500_000, 4_869_624), (441, 160, 5_000_000, 13_421_773)])
def test_indexing_beyond_2_to_the_31(up, down, n_in, cross):
    """t * D passes 2^31 at t = ceil(2^31 / D) (4 869 578 and 13 421 773): 64 outputs around that, 64 around ``cross`` (the
    positions the feature request names; the first lies 46 outputs behind the exact crossing) and the last 64, each by the
    float64 direct sum."""
    from phasegen import ops
    U, D, H, taps = geometry(up, down, 0)
    exact = -(-2 ** 31 // D)
    assert (exact - 1) * D < 2 ** 31 <= exact * D and 0 <= cross - exact < 64
    n_out = out_len(n_in, up, down)
    assert cross + 32 < n_out
    x = torch.randn(n_in, device="cuda")
    y = ops.resample(x, down, up)
    assert y.numel() == n_out
    xh = x.cpu().numpy()
    tol = bound(up, down, 0, float(np.abs(xh).max()))
    b64 = bank64(up, down, 0)
    for ts in (np.arange(exact - 32, exact + 32), np.arange(cross - 32, cross + 32), np.arange(n_out - 64, n_out)):
        got = y[int(ts[0]):int(ts[-1]) + 1].cpu().numpy()
        want = direct64(xh, up, down, 0, ts=ts, bank=b64)
        assert np.abs(want).max() > 0.05                                             # (real signal there, not a run of zeros)
        err = np.abs(got - want).max()
        assert err <= tol, (ts[0], err, tol)


# ---- pipeline ------------------------------------------------------------------------------------------------------------------
def _wavs(tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(11)
    s16 = (rng.standard_normal((30000, 2)) * 6000).astype(np.int16)                 # int16 stereo at 44.1 kHz
    f32 = (rng.standard_normal(14000) * 0.2).astype(np.float32)                     # float32 mono at 22.05 kHz
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    wavfile.write(a, 44100, s16)
    wavfile.write(b, 22050, f32)
    return a, b, s16, f32


def test_load_audio_and_get_mix_chunks(tmp_path):
    from phasegen import preproc
    a, b, s16, f32 = _wavs(tmp_path)
    xa, sra = preproc.load_audio(a)
    xb, srb = preproc.load_audio(b)
    assert (sra, srb) == (44100, 22050) and xa.dtype == xb.dtype == np.float32
    assert np.array_equal(xa, (s16.astype(np.float32) / np.float32(32768)).mean(axis=1)) and np.array_equal(xb, f32)
    t_slice, n_fft, hop = 4064, 512, 128
    got = preproc.get_mix_chunks((a, b), t_slice, n_fft, hop, 1, 16000, osr=44100, rng=np.random.default_rng(3))
    ra = preproc.resample(xa, 44100, 16000)
    rb = preproc.resample(preproc.resample(xb, 22050, 44100), 44100, 16000)
    assert ra.is_cuda and ra.numel() == out_len(30000, 160, 441) and rb.numel() == out_len(28000, 160, 441)
    n = min(ra.numel(), rb.numel())
    want = preproc.chunk_audio(torch.stack([ra[:n], rb[:n]]), t_slice, n_fft, hop, 1, np.random.default_rng(3))
    assert tuple(got.shape) == (preproc.n_chunks(n, t_slice, 1), 2, 2, n_fft // 2, 1 + t_slice // hop)
    assert torch.equal(got, want)
    # a device tensor is chunked like the same samples given as a host array
    host = preproc.chunk_audio(torch.stack([ra[:n], rb[:n]]).cpu().numpy(), t_slice, n_fft, hop, 1, np.random.default_rng(3))
    assert torch.equal(host, want)
    one = preproc.get_mix_chunks(a, t_slice, n_fft, hop, 0, 16000, rng=np.random.default_rng(0))
    assert torch.equal(one, preproc.chunk_audio(ra, t_slice, n_fft, hop, 0, np.random.default_rng(0)))


def _old_build_dataset(tracks, chunk_seconds, rsr, n_fft, hop_length, n_random, n_val, seed):
    """build_dataset as it was before ``osr`` existed (host arrays at the target rate), restated on the ops it called."""
    from phasegen import ops, preproc
    rng = np.random.default_rng(seed)
    t_slice = int(chunk_seconds * rsr)
    outs = []
    for t in tracks:
        a = np.asarray(t, np.float32)[None]
        starts = preproc.chunk_starts(a.shape[1], t_slice, n_random, rng)
        st = torch.tensor(np.asarray(starts, np.int64), device="cuda")
        outs.append(ops.stft(torch.from_numpy(a).cuda(), n_fft, hop_length, chunk_start=st, chunk_len=t_slice))
    x = torch.cat(outs)
    ops.standardize_(x)
    x = x.cpu().numpy()
    idx = np.linspace(0, len(x) - 1, len(x), dtype=int)
    rng.shuffle(idx)
    return x[idx][n_val:], x[idx][:n_val]


def test_build_dataset_from_44k_tracks(tmp_path):
    from phasegen import preproc
    rng = np.random.default_rng(4)
    tracks44 = [(rng.standard_normal(n) * 0.3).astype(np.float32) for n in (30000, 41234, 25001)]
    kw = dict(chunk_seconds=0.254, rsr=16000, n_fft=512, hop_length=128, n_random=1, n_val=3, seed=9)
    tracks16 = [preproc.resample(t, 44100, 16000).cpu().numpy() for t in tracks44]
    assert [len(t) for t in tracks16] == [out_len(n, 160, 441) for n in (30000, 41234, 25001)]
    tr_a, va_a = preproc.build_dataset(tracks44, osr=44100, out_dir=str(tmp_path), genre="Pop", **kw)
    tr_b, va_b = preproc.build_dataset(tracks16, **kw)
    assert tr_a.dtype == np.float32 and va_a.shape[0] == 3 and tr_a.shape[1:] == (2, 256, 1 + 4064 // 128)
    assert np.array_equal(tr_a, tr_b) and np.array_equal(va_a, va_b)
    assert np.array_equal(np.load(tmp_path / "Pop_audio_train.npy"), tr_a) and np.array_equal(np.load(tmp_path / "Pop_audio_val.npy"), va_a)
    # without osr nothing changed: the old path, restated
    tr_c, va_c = _old_build_dataset(tracks16, **kw)
    assert np.array_equal(tr_b, tr_c) and np.array_equal(va_b, va_c)
    # osr == rsr is no rate change either
    tr_d, va_d = preproc.build_dataset(tracks16, osr=16000, **kw)
    assert np.array_equal(tr_d, tr_b) and np.array_equal(va_d, va_b)
