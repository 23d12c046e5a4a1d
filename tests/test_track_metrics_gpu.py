"""GPU: the quality report -- phasegen.metrics.compare_audio, phasegen.track.evaluate_track, griffin_lim_batch(normalize=False) and
``reconstruct.py --report`` -- on tests/test_track_gpu.py's small geometry (C = 16, n_fft 32, hop 8, 24 frames, overlap 8).

compare_audio is checked against a float64 restatement fed the same fp32 signals and the device STFTs.  The restatement takes the
two gains the call reports (they are checked on their own first), so the bounds are those of the kernels (tests/test_compare_gpu.py):
the waveform sums within 1e-10, the spectral ones within 1e-5, the log-spectral distance within 1e-4 dB; carried to the metrics:
  gain, mag_gain      |g - g64| <= 3e-10 * sqrt(sum x^2 / sum y^2) and |g_m - g_m64| <= 3e-5 g_m64 (a quotient of two sums)
  snr_db, si_sdr_db   q = err / sum x^2 within 2e-10 relative; d(10 log10 q) = 4.35 dq / q and d(10 log10((1 - q) / q)) =
                      4.35 dq / (q (1 - q)): bounds 1e-9 and 1e-9 / (1 - q) dB
  spectral_convergence  a square root of a quotient of two sums within 1e-5 each: 1e-5 relative
  lsd_db              1e-4 dB
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from phasegen import detgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=8)      # C = 16: T = 184, step = 120
STATS = (0.1, 2.0)
FLOOR = 1e-10


def small_model():
    from phasegen.model import UNetModel
    return UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0))


@pytest.fixture(scope="module")
def model():
    return small_model()


def make_signal(a_len, channels=1, seed=71):
    """0.5 sin(2 pi (0.01 + 5e-5 t) t) + 0.3 sin(2 pi 0.13 t) + 0.1 noise (the issue's signal), float32 (a_len,) or (channels, a_len)."""
    t = np.arange(a_len, dtype=np.float64)
    tones = 0.5 * np.sin(2 * np.pi * (0.01 + 5e-5 * t) * t) + 0.3 * np.sin(2 * np.pi * 0.13 * t)
    a = (tones[None] + 0.1 * detgen.normal(seed, (channels, a_len)).astype(np.float64)).astype(np.float32)
    return a[0] if channels == 1 else a


def compare64(x, y, R, E, gain, mag_gain, floor=FLOOR):
    """float64 restatement of compare_audio's arithmetic: x, y (channels, n) float32, R, E their STFTs (channels, 2, bins, frames)
    float32, the two gains as the call reports them -> dict (and the optimal gains this restatement finds)."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    sxx, syy, sxy = (x64 * x64).sum(), (y64 * y64).sum(), (x64 * y64).sum()
    d = x64 - gain * y64
    q = (d * d).sum() / sxx
    mR = np.sqrt(R[:, 0].astype(np.float64) ** 2 + R[:, 1].astype(np.float64) ** 2)
    mE0 = np.sqrt(E[:, 0].astype(np.float64) ** 2 + E[:, 1].astype(np.float64) ** 2)
    mE = float(np.float32(mag_gain)) * mE0
    fl = float(np.float32(floor))
    dl = 10 * np.log10(np.maximum(mR * mR, fl)) - 10 * np.log10(np.maximum(mE * mE, fl))
    return {"si_sdr_db": 10 * math.log10((1 - q) / q), "snr_db": -10 * math.log10(q), "q": q,
            "spectral_convergence": math.sqrt(((mR - mE) ** 2).sum() / (mR * mR).sum()),
            "lsd_db": float(np.sqrt((dl * dl).mean(1)).sum() / (R.shape[0] * R.shape[3])),
            "max_abs_error": float(np.abs(d).max()),
            "gain64": sxy / syy, "gain_scale": math.sqrt(sxx / syy), "mag_gain64": (mR * mE0).sum() / (mE0 * mE0).sum()}


def check_metrics(m, x, y, what):
    from phasegen import ops
    x2, y2 = np.atleast_2d(x), np.atleast_2d(y)
    R = ops.stft(torch.from_numpy(x2).cuda(), 32, 8).cpu().numpy()
    E = ops.stft(torch.from_numpy(y2).cuda(), 32, 8).cpu().numpy()
    w = compare64(x2, y2, R, E, m["gain"], m["mag_gain"])
    print(f"\n{what}: SI-SDR {m['si_sdr_db']:.6f} dB (float64 {w['si_sdr_db']:.6f}), SNR {m['snr_db']:.6f} ({w['snr_db']:.6f}), gain {m['gain']:.9f} "
          f"({w['gain64']:.9f}), SC {m['spectral_convergence']:.7f} ({w['spectral_convergence']:.7f}), LSD {m['lsd_db']:.6f} dB ({w['lsd_db']:.6f}), "
          f"mag gain {m['mag_gain']:.7f} ({w['mag_gain64']:.7f})")
    assert (m["n_samples"], m["channels"], m["n_frames"]) == (x2.shape[1], x2.shape[0], R.shape[3])
    assert abs(m["gain"] - w["gain64"]) <= 3e-10 * w["gain_scale"]
    assert abs(m["mag_gain"] - w["mag_gain64"]) <= 3e-5 * w["mag_gain64"]
    assert abs(m["snr_db"] - w["snr_db"]) <= 1e-9
    assert abs(m["si_sdr_db"] - w["si_sdr_db"]) <= 1e-9 / (1 - w["q"])
    assert abs(m["spectral_convergence"] - w["spectral_convergence"]) <= 1e-5 * w["spectral_convergence"]
    assert abs(m["lsd_db"] - w["lsd_db"]) <= 1e-4
    assert abs(m["max_abs_error"] - w["max_abs_error"]) <= 1e-15 * w["max_abs_error"]


@pytest.mark.parametrize("a_len", [700, 1000])
@pytest.mark.parametrize("channels", [1, 2])
def test_compare_audio_against_float64(channels, a_len):
    from phasegen import metrics
    x = make_signal(a_len, channels)
    y = (0.8 * x + 0.05 * detgen.normal(72, x.shape)).astype(np.float32)
    m = metrics.compare_audio(x, y, 32, 8)
    assert tuple(m) == metrics.KEYS
    check_metrics(m, x, y, f"compare_audio {channels} ch, {a_len} samples")
    assert 1.0 < m["gain"] < 1.3 and 10 < m["si_sdr_db"] < 35                       # est = 0.8 x + noise some 17 dB below
    dev = metrics.compare_audio(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 32, 8, FLOOR)     # device tensors in: same bits
    assert dev == m
    same = metrics.compare_audio(x, x.copy(), 32, 8)
    assert same["si_sdr_db"] == math.inf and same["snr_db"] == math.inf and same["gain"] == 1.0 and same["mag_gain"] == 1.0
    assert same["spectral_convergence"] == 0.0 and same["lsd_db"] == 0.0 and same["max_abs_error"] == 0.0
    silent = metrics.compare_audio(x, np.zeros_like(x), 32, 8)                      # nothing to scale: gain 0, q = 1
    assert silent["gain"] == 0.0 and silent["si_sdr_db"] == -math.inf and silent["snr_db"] == 0.0 and silent["spectral_convergence"] == 1.0


def test_compare_audio_refuses_non_finite_audio_and_unequal_shapes():
    from phasegen import metrics
    x = make_signal(700)
    y = x.copy()
    y[300] = np.inf
    with pytest.raises(ValueError, match="Audio buffer is not finite everywhere"):
        metrics.compare_audio(x, y, 32, 8)
    with pytest.raises(ValueError, match="Audio buffer is not finite everywhere"):
        metrics.compare_audio(y, x, 32, 8)
    with pytest.raises(ValueError, match="shapes differ"):
        metrics.compare_audio(x, x[:699], 32, 8)


def stitch64(clips, step, n_out):
    """float64 restatement of pg_stitch (tests/test_track_gpu.py): clips (n_tracks, n_clips, T) float32 numpy -> (n_tracks, n_out)."""
    from phasegen import ops
    n_tracks, n_clips, T = clips.shape
    V = T - step
    ramp = ops.stitch_ramp_host(V).astype(np.float64)
    c = clips.astype(np.float64)
    t = np.arange(n_out)
    k = np.minimum(t // step, n_clips - 1)
    j = t - k * step
    out = c[:, k, j]
    two = (k >= 1) & (j < V)
    if two.any():
        kk, jj = k[two], j[two]
        a, b = ramp[V - 1 - jj], ramp[jj]
        out[:, two] = (a * c[:, kk - 1, jj + step] + b * c[:, kk, jj]) / (a + b)
    return out


@pytest.mark.parametrize("channels", [1, 2])
def test_evaluate_track_audio_and_metrics(model, channels):
    from phasegen import audio as pg_audio
    from phasegen import metrics, track
    a = make_signal(1000, channels)
    res = track.evaluate_track(model, a, stats=STATS, phases=("unet", "zero", "original", "griffinlim"), gl_iters=3, gl_seed=5,
                               return_audio=True, **SMALL)
    assert (res["n_samples"], res["sr"], res["n_clips"]) == (1000, 16000, 8)
    assert list(res["metrics"]) == ["unet", "zero", "original", "griffinlim"] == list(res["audio"])
    for phase in ("unet", "zero", "original"):                                      # the tracks reconstruct_track gives, bit for bit
        want = track.reconstruct_track(model, a, stats=STATS, phase=phase, normalize=False, **SMALL)
        got = res["audio"][phase]
        assert got.shape == want.shape == a.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), phase
    for phase, got in res["audio"].items():                                         # each phase's metrics are compare_audio of its audio
        assert res["metrics"][phase] == metrics.compare_audio(a, got, 32, 8, FLOOR), phase
        check_metrics(res["metrics"][phase], a, got.cpu().numpy(), f"evaluate_track {channels} ch, phase {phase}")
    plain = track.evaluate_track(model, a, stats=STATS, phases=["zero"], **SMALL)   # no audio unless asked; model unused
    assert "audio" not in plain and plain["metrics"]["zero"] == res["metrics"]["zero"]
    assert track.evaluate_track(None, a, stats=STATS, phases=("zero",), **SMALL)["metrics"] == plain["metrics"]
    # Griffin-Lim: the clips of griffin_lim_batch(exp(logmag) - 1, 3 iterations, seeds 5 + clip index, un-normalised), joined by the
    # float64 stitch; bound of tests/test_track_gpu.py: 8 * 2^-24 * max|clip audio|
    an = track._analyse(a, 32, 8, 24, 8, STATS, None, 16000, "kaiser_best")
    clips = pg_audio.griffin_lim_batch(torch.exp(an.pol[:, 0]) - 1.0, 32, 8, 3, seed=5, normalize=False)[0].cpu().numpy()
    assert clips.shape == (8 * channels, 184)
    want = stitch64(clips.reshape(8, channels, 184).transpose(1, 0, 2), 120, 1000)
    got = np.atleast_2d(res["audio"]["griffinlim"].cpu().numpy()).astype(np.float64)
    err = np.abs(got - want).max()
    print(f"griffinlim track: max error vs the float64 stitch {err:.3e} (bound {8 * U * np.abs(clips).max():.3e})")
    assert err <= 8 * U * np.abs(clips).max()
    with pytest.raises(ValueError):
        track.evaluate_track(None, a, stats=STATS, **SMALL)                         # "unet" needs a model
    with pytest.raises(ValueError):
        track.evaluate_track(model, a, stats=STATS, phases=("unet", "nophase"), **SMALL)


def test_peak_normalize_has_the_bits_of_the_normalised_track(model):
    from phasegen import track
    for channels in (1, 2):
        a = make_signal(1000, channels)
        raw = track.reconstruct_track(model, a, stats=STATS, normalize=False, **SMALL)
        want = track.reconstruct_track(model, a, stats=STATS, **SMALL)
        got = track.peak_normalize(raw)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_griffin_lim_batch_without_normalisation():
    from phasegen import audio as pg_audio
    mag = torch.from_numpy(np.abs(detgen.normal(81, (3, 16, 24))) + 0.1).cuda()
    a1, s1, l1 = pg_audio.griffin_lim_batch(mag, 32, 8, 4, seed=9)
    a0, s0, l0 = pg_audio.griffin_lim_batch(mag, 32, 8, 4, seed=9, normalize=False)
    peak = a0.abs().amax(dim=1, keepdim=True)
    assert float(peak.min()) > 0 and not torch.equal(a0, a1)
    assert torch.equal((a0 / peak).view(torch.int32), a1.view(torch.int32))         # the default output, bit for bit
    assert torch.equal(s0, s1) and torch.equal(l0, l1)


@pytest.mark.parametrize("stats", [STATS, None])
@pytest.mark.parametrize("a_len", [700, 1000])
def test_the_metrics_order_the_phase_sources(a_len, stats):
    """Keeping the analysis' phase must beat dropping the phase by a wide margin on every figure.  A float64 CPU restatement of the
    whole pipeline gives, on this geometry: original SI-SDR 15.1-16.4 dB, SC 0.11-0.13, LSD 0.75 dB; zero SI-SDR -33 .. -37 dB, SC
    0.57-0.64, LSD 9.7-9.8 dB."""
    from phasegen import track
    m = track.evaluate_track(None, make_signal(a_len), stats=stats, phases=("zero", "original"), **SMALL)["metrics"]
    o, z = m["original"], m["zero"]
    print(f"\n{a_len} samples, stats {stats}: original SI-SDR {o['si_sdr_db']:.2f} dB, SC {o['spectral_convergence']:.4f}, LSD {o['lsd_db']:.3f} dB; "
          f"zero SI-SDR {z['si_sdr_db']:.2f} dB, SC {z['spectral_convergence']:.4f}, LSD {z['lsd_db']:.3f} dB")
    assert o["si_sdr_db"] >= z["si_sdr_db"] + 20
    assert o["spectral_convergence"] <= 0.5 * z["spectral_convergence"]
    assert o["lsd_db"] <= 0.5 * z["lsd_db"]


def test_command_line_report(tmp_path, model):
    from scipy.io import wavfile
    from phasegen import preproc, track
    weight, wav_in, wav_out, rep = tmp_path / "unet.pth", tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "report.json"
    model.save(str(weight))
    pcm = np.round(detgen.make_clip(1000, seed=61) * 20000).astype(np.int16)
    wavfile.write(wav_in, 16000, pcm)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--weight", str(weight),
                        "--input", str(wav_in), "--output", str(wav_out), "--channels", "16", "--frames", "24", "--overlap_frames", "8",
                        "--report", str(rep)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("Reconstructed 0.06 s of audio in ") and lines[0].endswith(" s (8 clips).")      # the existing line, first
    assert len(lines) == 2 and lines[1].startswith("Report: unet SI-SDR ") and "; zero SI-SDR " in lines[1] and "LSD" in lines[1]
    sr, out = wavfile.read(wav_out)
    audio, file_sr = preproc.load_audio(str(wav_in))
    want = track.reconstruct_track(model, audio, osr=file_sr, **SMALL).cpu().numpy()                            # what the tool writes without --report
    assert sr == 16000 and out.dtype == np.float32 and np.array_equal(out.view(np.int32), want.view(np.int32))
    report = json.loads(rep.read_text())
    assert list(report["metrics"]) == ["unet", "zero", "original"] and "audio" not in report
    assert (report["n_samples"], report["sr"], report["n_clips"], report["input"]) == (1000, 16000, 8, str(wav_in))
    assert report["seconds"] == 1000 / 16000 and report["flags"]["report_phases"] == "unet,zero,original" and report["flags"]["gl_iters"] == 250
    u = report["metrics"]["unet"]
    assert all(math.isfinite(u[k]) for k in ("si_sdr_db", "snr_db", "gain", "spectral_convergence", "lsd_db", "mag_gain", "max_abs_error"))
    assert (u["n_samples"], u["channels"]) == (1000, 1)
    assert report["metrics"]["original"]["si_sdr_db"] > report["metrics"]["zero"]["si_sdr_db"]
