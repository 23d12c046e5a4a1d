"""GPU: pitch detection.  pg_pitch_track (ops.pitch_track) against the numpy restatement of its contract (tests/_pitch_ref.py) BIT FOR
BIT -- the tiny shape (W = 32, lags 2 .. 24, hop 8, rows of 300 samples: one workgroup takes four frames, the last workgroup fewer,
forty frames run off the row), the real shape (1024, 16 .. 320, hop 256: one wave per frame) and the limits (W = 2048, lags 2 .. 1024:
four waves per frame; hop 1: four frames share a span, hop 4096: one frame per workgroup) -- on strided rows, in any company, with
non-finite samples and across the range; ``track.detect_pitch`` as the chain written out; and the closure: a detuned take through
``track.autotune`` is detected again within half its detune, down to the command line.

Closure figures measured on an MI355X are in DESIGN.md section 4.21 and are printed by the test.

This module counts as the stream case of pg_pitch_track (tests/test_z_streams_gpu.py collects after it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _pitch_ref as pref
from test_z_lock_gpu import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
SENT = -77.0
TINY = dict(hop=8, window=32, tau_min=2, tau_max=24)
REAL = dict(hop=256, window=1024, tau_min=16, tau_max=320)
LIMIT_1 = dict(hop=1, window=2048, tau_min=2, tau_max=1024)
LIMIT_FAR = dict(hop=4096, window=2048, tau_min=2, tau_max=1024)
THETAS = (0.15, 0.0, 2.0, NAN)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope="module")
def data():
    """every input of the kernel tests, made once and left unchanged"""
    rs = np.random.RandomState(21)
    row = rs.standard_normal(300).astype(np.float32) * 0.5        # (tests/test_pitch_track_host.py's tiny row)
    row[100:200] = np.sin(2 * np.pi * np.arange(100, 200) / 11.3).astype(np.float32)
    d = {"tiny": np.stack([row, np.full(300, 0.37, np.float32)])}
    take, _ = pref.take([(196.0, 0.2), (261.6, 0.2)], seed=3)
    d["real"] = np.stack([take[:6000], rs.standard_normal(6000).astype(np.float32) * 0.3])
    long_take, _ = pref.take([(110.0, 0.6)], seed=4)
    d["limit"] = np.stack([long_take[:9000], rs.standard_normal(9000).astype(np.float32) * 0.3])
    return d


_want = {}


def want(data, name, frames, cfg, theta=0.15):
    """the restatement's (period, ap), computed once per case"""
    key = (name, frames, tuple(cfg.values()), repr(theta))
    if key not in _want:
        _want[key] = pref.pitch_track(data[name], frames, cfg["hop"], cfg["window"], cfg["tau_min"], cfg["tau_max"], theta)
    return _want[key]


def run(x, frames, cfg, theta=0.15, pad_in=5, pad_out=3):
    """ops.pitch_track on rows with NaN in their stride padding, into rows with a sentinel in theirs -> (period, ap) as numpy;
    asserts that the output padding is as it was"""
    from phasegen import ops
    n_sig, n_in = x.shape
    xb = torch.full((n_sig, n_in + pad_in), NAN, device="cuda")
    xb[:, :n_in] = dev(x)
    pb = torch.full((n_sig, frames + pad_out), SENT, device="cuda")
    ab = torch.full((n_sig, frames + pad_out), SENT, device="cuda")
    p, a = ops.pitch_track(xb[:, :n_in], frames, threshold=theta, out=(pb[:, :frames], ab[:, :frames]), **cfg)
    assert p.data_ptr() == pb.data_ptr() and a.data_ptr() == ab.data_ptr()
    assert bool((pb[:, frames:] == SENT).all()) and bool((ab[:, frames:] == SENT).all()), "output padding was written"
    return pb[:, :frames].cpu().numpy(), ab[:, :frames].cpu().numpy()


def same(got, ref):
    return bits_equal(got[0], ref[0]) and bits_equal(got[1], ref[1])


# ---- the kernel against the restatement, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [1, 7, 40])
def test_tiny_shape_has_the_bits_of_the_restatement(data, frames):
    for theta in THETAS:
        got, ref = run(data["tiny"], frames, TINY, theta), want(data, "tiny", frames, TINY, theta)
        assert same(got, ref), (frames, theta, got[0][0][:8], ref[0][0][:8])
    ap = want(data, "tiny", frames, TINY)[1]
    if frames == 40:
        assert ap[0].min() < 0.05 and ap[0].max() == 1.0          # both branches of the pick in row 0
        assert (got[0][:, -2:] == TINY["tau_min"]).all() and (got[1][:, -2:] == 1.0).all()   # frames past the row: all zeros


@pytest.mark.parametrize("frames", [19, 26])
def test_real_shape_has_the_bits_of_the_restatement(data, frames):
    """19 complete frames of 6000 samples; 26 run off the row (the last begins at 6400)"""
    from phasegen import ops
    assert ops.pitch_frames(6000) == 19
    got, ref = run(data["real"], frames, REAL), want(data, "real", frames, REAL)
    assert same(got, ref)
    assert (ref[1][0, 2:10] < 0.15).all() and (ref[1][1, :19] > 0.5).all()       # the take is voiced, the noise is not


@pytest.mark.parametrize("cfg", [LIMIT_1, LIMIT_FAR], ids=["hop1", "hop4096"])
def test_limits_have_the_bits_of_the_restatement(data, cfg):
    got, ref = run(data["limit"], 3, cfg), want(data, "limit", 3, cfg)
    assert same(got, ref)
    assert abs(float(ref[0][0, 0]) - 16000 / 110.0) < 0.5


# ---- rows, strides, company -----------------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_their_company_their_layout_or_the_frame_count(data):
    from phasegen import ops
    x = data["tiny"]
    both = run(x, 40, TINY)
    assert same(both, want(data, "tiny", 40, TINY))
    for r in (0, 1):
        p, a = ops.pitch_track(dev(x[r]), 40, **TINY)                                          # 1-D in, 1-D out
        assert tuple(p.shape) == tuple(a.shape) == (40,)
        assert bits_equal(p.cpu().numpy(), both[0][r]) and bits_equal(a.cpu().numpy(), both[1][r])
    p, a = (t.cpu().numpy() for t in ops.pitch_track(dev(np.stack([x[1], x[0], x[1]])), 40, **TINY))
    for got, ref in ((p, both[0]), (a, both[1])):
        assert bits_equal(got[0], ref[1]) and bits_equal(got[1], ref[0]) and bits_equal(got[2], ref[1])
    wide = dev(np.concatenate([x, x[::-1]], axis=1))                                            # every second row of a wider tensor
    view = wide.view(4, 300)[::2]
    assert not view.is_contiguous()
    p, a = ops.pitch_track(view, 40, **TINY)
    assert bits_equal(p.cpu().numpy(), both[0]) and bits_equal(a.cpu().numpy(), both[1])
    for frames in (1, 7):                                                                       # a prefix of the frames is the shorter call
        short = run(x, frames, TINY)
        assert bits_equal(short[0], both[0][:, :frames]) and bits_equal(short[1], both[1][:, :frames])
    real = run(data["real"], 26, REAL)
    assert same((real[0][:, :19], real[1][:, :19]), run(data["real"], 19, REAL))
    p, a = ops.pitch_track(dev(data["real"]))                                                   # the defaults: the complete frames
    assert tuple(p.shape) == (2, 19) and bits_equal(p.cpu().numpy(), real[0][:, :19]) and bits_equal(a.cpu().numpy(), real[1][:, :19])


# ---- non-finite samples -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cfg,frames,places", [
    ("tiny", TINY, 40, ((NAN, 0, 0), (INF, 0, 95), (-INF, 0, 96), (NAN, 1, 299), (INF, 1, 150))),     # 95 = 5 * 8 + 32 + 24 - 1
    ("real", REAL, 26, ((NAN, 0, 1855), (-INF, 1, 3000), (INF, 0, 5999)))])                           # 1855 = 2 * 256 + 1024 + 320 - 1
def test_a_non_finite_sample_reaches_exactly_its_cone(data, name, cfg, frames, places):
    clean, ref_clean = run(data[name], frames, cfg), want(data, name, frames, cfg)
    assert same(clean, ref_clean)
    for value, r, i in places:
        x = data[name].copy()
        x[r, i] = value
        got = run(x, frames, cfg)
        ref = pref.pitch_track(x, frames, cfg["hop"], cfg["window"], cfg["tau_min"], cfg["tau_max"], 0.15)
        hit = np.zeros((2, frames), bool)
        hit[r] = pref.cone(i, frames, cfg["hop"], cfg["window"], cfg["tau_max"])
        assert hit.any() and not hit[r].all(), (value, r, i)
        assert np.array_equal(np.isnan(got[0]), hit) and np.array_equal(np.isnan(got[1]), hit), (value, r, i)
        assert same(got, ref), (value, r, i)
        assert bits_equal(got[0][~hit], clean[0][~hit]) and bits_equal(got[1][~hit], clean[1][~hit])
        assert (got[0][hit].view(np.int32) == 0x7fc00000).all() and (got[1][hit].view(np.int32) == 0x7fc00000).all()
    if name == "tiny":                                            # sample 95 is the last of frame 5: only d(tau_max) sees it
        assert pref.cone(95, 40, 8, 32, 24)[5] and not pref.cone(96, 40, 8, 32, 24)[5]


# ---- the range ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cfg,frames", [("tiny", TINY, 40), ("real", REAL, 19)])
def test_range(data, name, cfg, frames):
    x = data[name]
    clean = run(x, frames, cfg)
    for e in (40, -40):
        assert same(run(x * np.float32(2.0 ** e), frames, cfg), clean), e
    with np.errstate(over="ignore"):
        xb = x * np.float32(1e25)
        big, ref = run(xb, frames, cfg), pref.pitch_track(xb, frames, cfg["hop"], cfg["window"], cfg["tau_min"], cfg["tau_max"], 0.15)
    assert same(big, ref)
    inside = np.arange(frames) * cfg["hop"] < x.shape[1]
    rows = [0] if name == "tiny" else [0, 1]                      # (the tiny shape's row 1 is a constant: its differences are zero)
    assert np.isnan(big[0][rows][:, inside]).all() and np.isnan(big[1][rows][:, inside]).all()
    assert (big[0][:, ~inside] == cfg["tau_min"]).all() and (big[1][:, ~inside] == 1.0).all()
    small = run(x * np.float32(1e-25), frames, cfg)
    assert (small[0] == cfg["tau_min"]).all() and (small[1] == 1.0).all()


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------------

def test_argument_errors(data):
    from phasegen import ops
    x = dev(data["tiny"])
    ops.pitch_track(x, 7, **TINY)
    for kw, word in ((dict(window=3), "window"), (dict(window=2049), "window"), (dict(tau_min=1), "lags"), (dict(tau_max=1025), "lags"),
                     (dict(tau_min=24), "lags"), (dict(hop=0), "hop"), (dict(frames=0), "frames"), (dict(out=3), "out must be"),
                     (dict(out=(torch.empty(2, 7, device="cuda"),)), "out must be"),
                     (dict(out=(torch.empty(2, 6, device="cuda"), torch.empty(2, 7, device="cuda"))), "out must be"),
                     (dict(out=(torch.empty(2, 7, device="cuda"), torch.empty(2, 9, device="cuda")[:, :7])), "same row stride"),
                     (dict(out=(torch.empty(2, 7), torch.empty(2, 7))), "out must be")):
        with pytest.raises(ValueError, match="pitch_track: .*" + word):
            ops.pitch_track(x, **{"frames": 7, **TINY, **kw})
    with pytest.raises(ValueError, match="contiguous"):
        ops.pitch_track(x[:, ::2], 7, **TINY)
    for bad in (x.double(), x.cpu(), x[None]):
        with pytest.raises(ValueError, match="pitch_track: expected"):
            ops.pitch_track(bad, 7, **TINY)


def test_runs_on_the_stream_passed_in_and_writes_nothing_else(data):
    """pg_pitch_track has no workspace (tests/test_z_workspace_gpu.py's helper: the guards of none, the same bits) and runs on the
    stream it is given without waiting (tests/test_z_streams_gpu.py)"""
    import test_z_streams_gpu as S
    import test_z_workspace_gpu as W
    from phasegen import _lib, ops
    assert "workspace" not in dict(_lib.PitchTrackArgs._fields_)
    case = W.Case("pitch_track", {"x": W.cuda(data["real"])}, lambda: {"period": W.sent(2, 19), "ap": W.sent(2, 19)},
                  lambda i, o: list(ops.pitch_track(i["x"], 19, out=(o["period"], o["ap"]))), symbol="pg_pitch_track", needs_ws=False)
    W.check(case)
    S.reach(case)
    assert "pg_pitch_track" in S.REACHED


# ---- track level --------------------------------------------------------------------------------------------------------------------------

NOTES = (("A3", 57, +35.0), ("D4", 62, -30.0), ("E4", 64, +20.0), ("A4", 69, -40.0))   # (name, midi, detune in cents), 0.5 s each


@pytest.fixture(scope="module")
def detuned():
    notes = [(440.0 * 2.0 ** ((m - 69 + c / 100.0) / 12.0), 0.5) for _, m, c in NOTES]
    return pref.take(notes, seed=8)[0]


def test_detect_pitch_is_the_chain_written_out(detuned):
    from phasegen import ops, track
    pt = track.detect_pitch(detuned)
    assert isinstance(pt, track.PitchTrack) and all(isinstance(v, np.ndarray) for v in pt)
    n = ops.pitch_frames(detuned.shape[0])
    assert pt.times.shape == pt.f0.shape == pt.voiced.shape == pt.ap.shape == (n,)
    assert pt.times.dtype == pt.f0.dtype == pt.ap.dtype == np.float64 and pt.voiced.dtype == bool
    period, ap = (t.cpu().numpy() for t in ops.pitch_track(dev(detuned), None, 256, 1024, 16, 320, 0.15))
    assert bits_equal(period, pref.pitch_track(detuned, n, 256, 1024, 16, 320, 0.15)[0])
    assert np.array_equal(pt.ap, ap.astype(np.float64)) and np.array_equal(pt.times, (np.arange(n) * 256 + 512.0) / 16000)
    voiced = np.isfinite(ap) & (ap.astype(np.float64) < 0.15)
    assert np.array_equal(pt.voiced, voiced) and voiced.sum() > 0.8 * n
    raw = np.where(voiced, 16000 / np.where(voiced, period.astype(np.float64), 1.0), 0.0)
    hand = raw.copy()
    logf = np.log(np.where(voiced, raw, 1.0))
    for k in np.flatnonzero(voiced):
        lo, hi = max(0, k - 2), min(n, k + 3)
        hand[k] = np.exp(np.median(logf[lo:hi][voiced[lo:hi]]))
    assert np.array_equal(pt.f0, hand) and (pt.f0[~voiced] == 0.0).all()
    assert np.array_equal(track.detect_pitch(detuned, median=1).f0, raw)
    # every note is found where it was put, the detune included
    for k, (_name, m, c) in enumerate(NOTES):
        inside = voiced & (pt.times >= 0.5 * k + 0.1) & (pt.times <= 0.5 * k + 0.4)
        assert inside.sum() >= 10
        assert np.abs(pref.cents(pt.f0[inside], 440.0 * 2.0 ** ((m - 69) / 12.0)) - c).max() < 3.0
    # stereo is tracked on the channel mean, formed on the device; other lags through fmin / fmax
    stereo = np.stack([detuned, 0.5 * detuned[::-1]])
    mean = dev(stereo).mean(dim=0)
    a, b = track.detect_pitch(stereo), track.detect_pitch(mean)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))
    low = track.detect_pitch(detuned, fmin=100.0, fmax=600.0, hop_length=128, window=512)
    p2, a2 = (t.cpu().numpy() for t in ops.pitch_track(dev(detuned), None, 128, 512, 26, 160, 0.15))
    assert np.array_equal(low.ap, a2.astype(np.float64)) and low.times[0] == 256 / 16000


def _off_semitone(f0):
    m = 69.0 + 12.0 * np.log2(f0 / 440.0)
    return 100.0 * np.abs(m - np.round(m))


def test_autotune_closes_the_loop_at_the_real_framing(detuned):
    """2048 / 512, the locked vocoder, no model: four notes 35, 30, 20 and 40 cents off their semitones.  After
    autotune(strength=1, retune_ms=0) the median distance from the nearest semitone over the frames at least 100 ms inside a note is
    at most HALF the note's detune (a correction of the wrong sign doubles it, none leaves it where it was)."""
    from phasegen import track
    out, pt, curve = track.autotune(None, detuned, strength=1.0, retune_ms=0.0, phase="vocoder_locked", return_curve=True)
    assert tuple(out.shape) == detuned.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert float(out.abs().max()) == 1.0
    assert isinstance(curve, track.PitchCurve) and len(curve.seconds) == len(pt.times) + 1
    again = track.detect_pitch(out)
    failed = []
    for k, (name, _m, c) in enumerate(NOTES):
        lo, hi = 0.5 * k + 0.1, 0.5 * k + 0.4
        before = pt.voiced & (pt.times >= lo) & (pt.times <= hi)
        after = again.voiced & (again.times >= lo) & (again.times <= hi)
        assert before.sum() >= 10 and after.sum() >= 10, (name, before.sum(), after.sum())
        was, now = float(np.median(_off_semitone(pt.f0[before]))), float(np.median(_off_semitone(again.f0[after])))
        print(f"{name} {c:+.0f} cents: the median distance from the nearest semitone is {was:.1f} cents before and {now:.1f} after")
        if not now <= 0.5 * abs(c):
            failed.append((name, c, was, now))
    assert not failed, failed
    # strength 0 is pitch_shift along the zero curve
    zero = track.autotune(None, detuned, strength=0.0, retune_ms=0.0, phase="vocoder_locked")
    assert same_bits(zero, track.pitch_shift(None, detuned, track.PitchCurve([(0, 0), (1, 0)]), phase="vocoder_locked"))


# ---- command line -----------------------------------------------------------------------------------------------------------------

def _cli(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--channels", "16", "--hop", "8",
                           "--frames", "24", "--overlap_frames", "4", *map(str, flags)], capture_output=True, text=True, timeout=300)


def test_reconstruct_cli_with_autotune_and_a_pitch_report(tmp_path, detuned):
    from scipy.io import wavfile
    wav, out, rep, curve, tmap = (tmp_path / n for n in ("in.wav", "out.wav", "rep.json", "curve.txt", "map.txt"))
    x = detuned[:8000]
    wavfile.write(str(wav), 16000, x)
    r = _cli("--input", wav, "--output", out, "--autotune", "--phase", "vocoder_locked", "--pitch_report", rep)      # no --weight
    assert r.returncode == 0, r.stderr[-2000:]
    sr, y = wavfile.read(str(out))
    assert sr == 16000 and y.shape == (8000,) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    d = json.loads(rep.read_text())
    n = len(d["times"])
    assert n > 10 and len(d["f0"]) == len(d["voiced"]) == len(d["ap"]) == n and sum(d["voiced"]) > n // 2
    assert len(d["curve"]) == n + 1 and d["curve"][0][0] == 0.0 and all(len(a) == 2 for a in d["curve"])
    voiced = np.array(d["voiced"])
    assert np.abs(pref.cents(np.array(d["f0"])[voiced][3:20], 220.0) - 35.0).max() < 3.0
    os.remove(str(out))
    rep2 = tmp_path / "alone.json"
    r = _cli("--input", wav, "--output", out, "--phase", "vocoder_locked", "--pitch_report", rep2)                    # the report alone
    assert r.returncode == 0, r.stderr[-2000:]
    d2 = json.loads(rep2.read_text())
    assert "curve" not in d2 and d2["f0"] == d["f0"] and os.path.exists(str(out))
    r = _cli("--input", wav, "--output", out, "--autotune", "0.5", "--scale", "A:min", "--a4", "442", "--retune_ms", "20", "--fmin", "80",
             "--fmax", "800", "--phase", "vocoder_locked", "--pitch_report", rep2)
    assert r.returncode == 0, r.stderr[-2000:]
    curve.write_text("0 0\n0.2 1\n")
    tmap.write_text("0 0\n1 1.5\n")
    for flags, name in ((("--pitch", "3"), "--pitch"), (("--stretch", "1.5"), "--stretch"), (("--tempo_map", tmap), "--tempo_map"),
                        (("--pitch_curve", curve), "--pitch_curve"), (("--formants", "keep"), "--formants"),
                        (("--formant_shift", "2"), "--formant_shift"), (("--report", rep), "--report"), (("--stretch_report", rep), "--stretch_report")):
        r = _cli("--input", wav, "--output", out, "--phase", "vocoder", "--autotune", *flags)
        assert r.returncode == 2 and "--autotune" in r.stderr and name in r.stderr, (flags, r.stderr[-500:])
