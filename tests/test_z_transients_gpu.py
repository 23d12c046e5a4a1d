"""GPU: the transient-preserving stretch at the track level (phasegen.track transients="ola", reconstruct.py --transients ola): the
option off changes nothing, the option on is the documented composition of ops.hpss, the chosen phase source on the harmonic plane,
one more ISTFT and ops.ola_stretch, it is the identity at stretch 1, it keeps the clicks of the synthetic signal of
tests/test_transient_host.py on the device, it works with link_channels, and the command line reaches it.

The crest condition is the host test's (float64: medians 2.91 -> 6.63 at stretch 1.5 and 4.24 -> 6.89 at 0.75 on the dense clicky
melody, tests/test_transient_host.py); the device's figures are printed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _signal_ref64 as sig
import _transient_ref as tref
from phasegen import detgen
from test_z_lock_gpu import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
U = 2.0 ** -24


def small_signal(n=1000, channels=2, seed=3):
    """tones, noise and a few clicks, float32 (channels, n)"""
    t = np.arange(n, dtype=np.float64)
    x = 0.5 * np.sin(2 * np.pi * 0.07 * t)[None] + 0.3 * np.sin(2 * np.pi * 0.19 * t)[None] + 0.05 * detgen.normal(seed, (channels, n)).astype(np.float64)
    x[:, 3 * n // 10:3 * n // 10 + 4] += 2.0
    x[:, 7 * n // 10:7 * n // 10 + 3] -= 1.5
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def clicky():
    return tref.clicky_melody()


def small_model():
    from phasegen.model import UNetModel
    return UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0))


# ---- the option off ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase", ["unet", "original", "zero", "vocoder", "vocoder_locked", "spsi"])
def test_none_gives_the_bits_of_a_call_without_the_keyword(phase):
    from phasegen import track
    x = small_signal()
    model = small_model() if phase == "unet" else None
    kw = dict(phase=phase, join="spectral", stretch=1.0 if phase == "original" else 1.5, **SMALL)
    a, b = track.reconstruct_track(model, x, **kw), track.reconstruct_track(model, x, transients=None, **kw)
    assert same_bits(a, b)
    if phase in track.STRETCH_PHASES:
        ra = track.evaluate_stretch(model, x, 1.5, phases=(phase,), return_audio=True, **SMALL)
        rb = track.evaluate_stretch(model, x, 1.5, phases=(phase,), return_audio=True, transients=None, **SMALL)
        assert list(ra) == list(rb) and "transients" not in rb and ra["metrics"] == rb["metrics"] and same_bits(ra["audio"][phase], rb["audio"][phase])
        on = track.reconstruct_track(model, x, transients="ola", **kw)
        assert on.shape == a.shape and bool(torch.isfinite(on).all()) and not same_bits(on, a)
    if phase == "vocoder_locked":
        assert same_bits(track.pitch_shift(None, x, 3, phase=phase, **SMALL), track.pitch_shift(None, x, 3, phase=phase, transients=None, **SMALL))


# ---- the option on -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stretch", [1.5, 0.8])
@pytest.mark.parametrize("link", [False, True], ids=["unlinked", "linked"])
def test_the_option_is_the_documented_composition(stretch, link):
    from phasegen import ops, track
    x = small_signal()
    out = track.reconstruct_track(None, x, phase="vocoder_locked", join="spectral", stretch=stretch, normalize=False, link_channels=link,
                                  transients="ola", **SMALL)
    assert tuple(out.shape) == (2, round(1000 * stretch)) and bool(torch.isfinite(out).all())
    an = track._analyse_spectral(x, 32, 8, 24, 4, None, None, 16000, "kaiser_best", stretch, link)
    pl, spo, floor = an.plan, 1.0 / stretch, track.VOCODER_RESET_BELOW
    with torch.no_grad():
        harm, perc = ops.hpss(an.pol[:, 0], *track.HPSS_WIN)
        wh, wp = tref.hpss(an.pol[:, 0].cpu().numpy(), 17, 17)
        assert same_bits(harm, wh) and same_bits(perc, wp) and bool((perc != 0).any()) and tuple(harm.shape) == (2 + link, 16, pl.F_src)
        if link:
            ph = ops.phase_lock_linked(an.pol[:2, 1], an.pol[2, 1], harm[2], pl.F_out, spo, reset_below=floor)
        else:
            ph = ops.phase_lock(an.pol[:, 1], pl.F_out, spo, logmag=harm, reset_below=floor)
        mag = ops.spec_clips(harm[:2], 1, pl.F_out, pl.F_out, spo)[0]
        h_audio = ops.istft(mag, ph, 8, mode=0, normalize=False)
        p_audio = ops.istft(perc[:2], an.pol[:2, 1], 8, mode=0, normalize=False)
        assert tuple(p_audio.shape) == (2, 8 * (pl.F_src - 1))
        both = ops.ola_stretch(p_audio, 8 * (pl.F_out - 1), spo, track.TRANSIENT_WINDOW, track.TRANSIENT_HOP, base=h_audio)
        want = track._trim_spectral(an, both, False)
    assert same_bits(out, want)
    assert same_bits(both, tref.ola_stretch(p_audio.cpu().numpy(), 8 * (pl.F_out - 1), spo, tref.ola_window(256), 64, base=h_audio.cpu().numpy()))
    normal = track.reconstruct_track(None, x, phase="vocoder_locked", join="spectral", stretch=stretch, link_channels=link, transients="ola", **SMALL)
    assert same_bits(normal, track.peak_normalize(out))


def test_mono_input_linked_equals_the_unlinked_result():
    from phasegen import track
    x = small_signal()
    for mono, stats in ((x[0], None), (x[:1], (0.1, 2.0))):
        kw = dict(phase="vocoder_locked", join="spectral", stretch=1.5, stats=stats, transients="ola", **SMALL)
        a, b = track.reconstruct_track(None, mono, link_channels=True, **kw), track.reconstruct_track(None, mono, **kw)
        assert a.shape == b.shape and a.dim() == mono.ndim and same_bits(a, b)
    stereo = track.reconstruct_track(None, x, link_channels=True, **{**kw, "stats": None})
    assert tuple(stereo.shape) == (2, 1500) and bool(torch.isfinite(stereo).all())
    assert not same_bits(stereo, track.reconstruct_track(None, x, **{**kw, "stats": None}))


def test_evaluate_stretch_records_the_option_and_measures_against_the_full_plane():
    from phasegen import metrics, ops, track
    x = small_signal()
    rep = track.evaluate_stretch(None, x, 1.5, phases=("vocoder_locked", "zero"), return_audio=True, transients="ola", **SMALL)
    assert list(rep) == ["n_samples", "n_out", "sr", "stretch", "n_clips", "reset_below", "metrics", "transients", "audio"] and rep["transients"] == "ola"
    for p in ("vocoder_locked", "zero"):
        assert same_bits(rep["audio"][p], track.reconstruct_track(None, x, phase=p, join="spectral", stretch=1.5, normalize=False, transients="ola", **SMALL))
    an = track._analyse_spectral(x, 32, 8, 24, 4, None, None, 16000, "kaiser_best", 1.5)
    with torch.no_grad():
        full_mag = ops.spec_clips(an.pol[:, 0], 1, an.plan.F_out, an.plan.F_out, 1 / 1.5)[0]
        _, audio = track._invert_spectral(an, None, "zero", 8, 24, 64, None, "ola")
        assert rep["metrics"]["zero"] == metrics.consistency(full_mag, audio, 32, 8)
    both = track.evaluate_stretch(None, x, 1.5, phases=("vocoder_locked",), link_channels=True, transients="ola", **SMALL)
    assert both["link_channels"] is True and both["transients"] == "ola" and list(both["mid_metrics"]) == ["vocoder_locked"]


def test_pitch_shift_forwards_the_option():
    from phasegen import track
    x = small_signal()
    out = track.pitch_shift(None, x, 5, stats=(0.1, 2.0), phase="vocoder_locked", transients="ola", **SMALL)
    assert tuple(out.shape) == (2, 1000) and bool(torch.isfinite(out).all()) and float(out.abs().max()) == 1.0
    assert not same_bits(out, track.pitch_shift(None, x, 5, stats=(0.1, 2.0), phase="vocoder_locked", **SMALL))


# ---- stretch 1: the identity ---------------------------------------------------------------------------------------------------

def _identity_case(x, n_fft, hop, frames, overlap):
    """At stretch 1 with phase="original" the option must not matter.  Derivation of the tolerance, per output sample, u = 2^-24.
    Write I(.) for the exact ISTFT of a plane under the analysis' phase A.  The masks partition the cells and expm1(0) = 0, so
    I(M) = I(harm) + I(perc) exactly, and the joined phase of "original" at rate 1 is A itself outside the clip overlaps -- the test
    uses ONE clip, so everywhere.  (The analysis holds F_src = F_out + 1 frames, the last one for the interpolation; the harmonic
    side inverts F_out of them and the percussive side, on the source grid, all: the samples from hop F_out - n_fft / 2 on, which
    the extra frame covers, are not compared.  They lie behind the track's end in both cases below.)  On the device
        plain = I(M) + e0,   h = I(harm) + e1,   p = I(perc) + e2,        |e_i| <= B_i, the derived per-sample bound of pg_istft
                                                                           (tests/_signal_ref64.py: inverse_bound, Tier A),
        r = p (1 + d), |d| <= 12 u                                         (the header's identity bound of pg_ola_stretch at 256 / 64:
                                                                           at ratio 1 every covering frame reads p[t], den > 0),
        ola = (h + r)(1 + d'), |d'| <= u                                   (the addition of `base`),
    hence |ola - plain| <= B0 + B1 + B2 + 12 u (|I(perc)| + B2) + u (|I(M)| + B1 + (1 + 12 u) (|I(perc)| + B2) + 12 u ...), which the
    code below evaluates with the float64 chain's |I(.)| (the last bracket rounded up by the factor 1.001).  -> the largest
    |ola - plain| / bound, and the measured distances of both results from the float64 chain in units of u max |I(M)|."""
    from phasegen import ops, track
    kw = dict(n_fft=n_fft, hop_length=hop, frames=frames, overlap_frames=overlap, phase="original", join="spectral", stretch=1.0, normalize=False)
    plain = track.reconstruct_track(None, x, **kw)
    ola = track.reconstruct_track(None, x, transients="ola", **kw)
    an = track._analyse_spectral(x, n_fft, hop, frames, overlap, None, None, 16000, "kaiser_best", 1.0)
    Fo = an.plan.F_out
    assert an.n_clips == 1 and an.plan.F_src >= Fo
    pol = an.pol.cpu().numpy()
    M, A = np.ascontiguousarray(pol[:, 0]), np.ascontiguousarray(pol[:, 1])
    harm, perc = tref.hpss(M, 17, 17)
    assert bool((perc != 0).any()) and bool((harm != 0).any())
    fam = sig.family_of(n_fft)
    y, B = {}, {}
    n = plain.shape[-1]
    assert n <= hop * Fo - n_fft // 2                                                             # the compared samples: the whole track
    for name, plane, F in (("M", M, Fo), ("harm", harm, Fo), ("perc", perc, an.plan.F_src)):
        y[name], info = sig.istft64(np.ascontiguousarray(plane[:, :, :F]), np.ascontiguousarray(A[:, :, :F]), hop, 0)
        y[name], B[name] = y[name][:, :n], sig.inverse_bound(y[name], info, fam, n_fft)[:, :n]
    assert np.abs(y["M"] - y["harm"] - y["perc"]).max() <= 1e-12 * np.abs(y["M"]).max()          # linear, and the masks partition
    p_abs = np.abs(y["perc"]) + B["perc"]
    bound = B["M"] + B["harm"] + B["perc"] + 12 * U * p_abs + 1.001 * U * (np.abs(y["M"]) + B["harm"] + B["perc"] + 12 * U * p_abs)
    d = np.abs(ola.cpu().numpy().astype(np.float64) - plain.cpu().numpy().astype(np.float64)).reshape(1, -1)
    scale = U * np.abs(y["M"]).max()
    far = [float(np.abs(t.cpu().numpy().astype(np.float64).reshape(1, -1) - y["M"]).max() / scale) for t in (plain, ola)]
    return float((d / bound).max()), float(d.max() / scale), far


def test_identity_at_stretch_one_on_the_small_geometry():
    x = small_signal(150, 1)[0]                                                                   # one clip of 24 frames: 184 samples
    ratio, dist, far = _identity_case(x, 32, 8, 24, 4)
    print(f"\n32 / 8: max |ola - plain| = {dist:.2f} u max|y|, {ratio:.4f} of the derived bound; from the float64 chain: plain {far[0]:.2f}, ola {far[1]:.2f} u max|y|")
    assert ratio <= 1.0


def test_identity_at_stretch_one_at_2048_512(clicky):
    x = clicky[0][10000:10000 + 60000]                                                            # 3.75 s, one clip of 128 frames; two clicks
    ratio, dist, far = _identity_case(x, 2048, 512, 128, 32)
    print(f"\n2048 / 512: max |ola - plain| = {dist:.2f} u max|y|, {ratio:.4f} of the derived bound; from the float64 chain: plain {far[0]:.2f}, ola {far[1]:.2f} u max|y|")
    assert ratio <= 1.0


# ---- the clicks stay clicks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stretch", [1.5, 0.75])
def test_the_split_keeps_the_clicks_on_the_device(clicky, stretch):
    from phasegen import track
    x, at = clicky
    kw = dict(phase="vocoder_locked", join="spectral", stretch=stretch, normalize=False)
    plain = tref.crests(track.reconstruct_track(None, x, **kw).cpu().numpy(), at, stretch)
    split = tref.crests(track.reconstruct_track(None, x, transients="ola", **kw).cpu().numpy(), at, stretch)
    print(f"\nclicky melody on the device, 2048 / 512, stretch {stretch}: whole plane {np.round(plain, 2)} (median {np.median(plain):.2f}), "
          f"split {np.round(split, 2)} (median {np.median(split):.2f})")
    assert np.median(split) > np.median(plain), (plain, split)


# ---- command line --------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), *args], capture_output=True, text=True, timeout=300)


def test_reconstruct_cli(tmp_path):
    from scipy.io import wavfile
    wav, out, rep = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "stretch.json"
    wavfile.write(str(wav), 16000, np.ascontiguousarray(small_signal(4000, 1)[0] * np.float32(0.25)))
    base = ["--input", str(wav), "--output", str(out), "--channels", "16", "--hop", "8", "--frames", "24", "--overlap_frames", "4"]
    r = _cli(*base, "--stretch", "1.5", "--phase", "vocoder_locked", "--transients", "ola", "--stretch_report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    sr, y = wavfile.read(str(out))
    assert sr == 16000 and y.shape == (round(4000 * 1.5),) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    report = json.load(open(rep))
    assert report["transients"] == "ola" and (report["n_samples"], report["n_out"]) == (4000, 6000)
    # refused before anything is loaded
    for bad in (["--phase", "vocoder_locked", "--transients", "ola"],                                        # neither --stretch nor --pitch
                ["--phase", "zero", "--stretch", "1.0", "--join", "waveform", "--transients", "ola"],
                ["--weight", "none.pt", "--stretch", "1.0", "--report", str(rep), "--transients", "ola"],
                ["--phase", "vocoder_locked", "--stretch", "1.5", "--transients", "wsola"]):
        r = _cli(*base, *bad)
        assert r.returncode != 0 and ("--transients" in r.stderr), (bad, r.stderr[-500:])
