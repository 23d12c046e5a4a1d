"""GPU: whole-track phase reconstruction (phasegen.track.reconstruct_track), the dataset statistics it needs
(preproc.build_dataset(..., return_stats=True)) and the command-line entry (reconstruct.py).

Nothing in the reference does this, so the expected value is COMPOSED here from pieces that have their own tests -- ops.stft on
host-gathered, zero-padded chunks; (x - mean) / std through ops.standardize_with_ (with float64 numpy moments where the pipeline
takes the track's own); ops.polar; ONE model.forward(..., per_clip=True) over all clips; audio.synthesize(normalize=False) -- plus
the float64 restatement of the stitch contract (include/phasegen.h).  Bound: 8 * 2^-24 * max|clip audio| (the stitch's five
roundings, tests/test_stitch_gpu.py), plus 2 * 2^-24 relative when the result is peak-normalised.
"""
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
TOL_F = 2e-5                      # forward tensors, relative to max-abs (tests/test_clip_stats_gpu.py)
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=8)      # C = 16: T = 184, step = 120


def small_model(params=None):
    from phasegen.model import UNetModel
    return UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0) if params is None else params)


def stitch64(clips, step, n_out):
    """float64 restatement of pg_stitch: clips (n_tracks, n_clips, T) float32 numpy -> (n_tracks, n_out)."""
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


def compose(model, audio, n_fft, hop_length, frames, overlap_frames, stats, phase="unet", normalize=True):
    """The expected track: -> (float64 (channels, a_len), max|clip audio|, peak of the un-normalised result)."""
    from phasegen import audio as pg_audio
    from phasegen import ops
    from phasegen.track import track_plan
    a2 = np.atleast_2d(np.asarray(audio, np.float32))
    n_ch, a_len = a2.shape
    T, step, n_clips = track_plan(a_len, frames, hop_length, overlap_frames)
    padded = np.concatenate([a2, np.zeros((n_ch, n_clips * step + T), np.float32)], axis=1)
    chunks = np.stack([padded[c, k * step:k * step + T] for k in range(n_clips) for c in range(n_ch)])      # (clip, channel) order
    x = ops.stft(torch.from_numpy(chunks).cuda(), n_fft, hop_length)
    if stats is None:
        x64 = x.cpu().numpy().astype(np.float64)
        stats = (x64.mean(), x64.std())
    ops.standardize_with_(x, stats[0], stats[1])
    pol = ops.polar(x)
    if phase == "unet":
        with torch.no_grad():
            ph = model.forward(pol[:, 0], per_clip=True)[:, :n_fft // 2]
    else:
        ph = pol[:, 1]
    clips = pg_audio.synthesize(pol[:, 0], ph, hop_length, normalize=False).cpu().numpy()
    ref = stitch64(clips.reshape(n_clips, n_ch, T).transpose(1, 0, 2), step, a_len)
    peak = np.abs(ref).max()
    return (ref / peak if normalize and peak > np.finfo(np.float32).tiny else ref), float(np.abs(clips).max()), float(peak)


def check(got, want, clip_max, peak, normalize, what):
    got = np.atleast_2d(got.cpu().numpy()).astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    bound = 8 * U * clip_max / peak + 2 * U * np.abs(want) if normalize else np.full_like(want, 8 * U * clip_max)
    print(f"\n{what}: max error {err.max():.3e}, worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.fixture(scope="module")
def model():
    return small_model()


@pytest.mark.parametrize("stats", [(0.1, 2.0), None])
@pytest.mark.parametrize("channels", [1, 2])
def test_small_model_equals_the_composition(model, stats, channels):
    from phasegen.track import reconstruct_track, track_plan
    audio = detgen.normal(11, (1000,)) if channels == 1 else detgen.normal(12, (2, 1000))
    assert track_plan(1000, 24, 8, 8) == (184, 120, 8)
    got = reconstruct_track(model, audio, stats=stats, **SMALL)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == audio.shape
    want, cmax, peak = compose(model, audio, 32, 8, 24, 8, stats)
    check(got, want, cmax, peak, True, f"track C=16 {channels} ch stats={stats}")
    assert float(got.abs().max()) == 1.0                                            # one joint peak over the channels
    raw = reconstruct_track(model, audio, stats=stats, normalize=False, **SMALL)
    want, cmax, peak = compose(model, audio, 32, 8, 24, 8, stats, normalize=False)
    check(raw, want, cmax, peak, False, f"track C=16 {channels} ch stats={stats} un-normalised")
    dev = reconstruct_track(model, torch.from_numpy(audio).cuda(), stats=stats, normalize=False, **SMALL)    # device tensor in
    assert torch.equal(dev, raw)


def test_clip_batching_agrees(model):
    """Convolutions may split their work differently with the batch size, so batches of 3 clips against one batch of 8 agree to
    the forward tolerance, not bit for bit."""
    from phasegen.track import reconstruct_track
    audio = detgen.normal(11, (1000,))
    a = reconstruct_track(model, audio, stats=(0.1, 2.0), clip_batch=64, normalize=False, **SMALL)
    b = reconstruct_track(model, audio, stats=(0.1, 2.0), clip_batch=3, normalize=False, **SMALL)
    worst = float((a - b).abs().max() / a.abs().max())
    print(f"\nclip_batch 3 vs 64: worst difference {worst:.3e} of max-abs (bound {TOL_F:g})")
    assert worst <= TOL_F


def test_full_geometry_round_trip_without_a_model():
    from phasegen.track import reconstruct_track, track_plan
    n = 160000
    noise = detgen.normal(21, (n + 15,)).astype(np.float64)
    audio = (0.2 * np.convolve(noise, np.hanning(16) / np.hanning(16).sum(), mode="valid")).astype(np.float32)    # band-limited noise
    assert audio.shape == (n,) and track_plan(n, 128, 512, 32) == (65024, 48640, 3)
    got = reconstruct_track(None, audio, stats=(0.0, 1.0), phase="original", normalize=False)
    want, cmax, peak = compose(None, audio, 2048, 512, 128, 32, (0.0, 1.0), phase="original", normalize=False)
    check(got, want, cmax, peak, False, "full geometry, original phase")
    d = np.abs(got.cpu().numpy() - audio)
    print(f"distance to the input audio (information only: DC is dropped, clip edges are reflect-padded): max {d.max():.3e}, "
          f"rms {np.sqrt((d ** 2).mean()):.3e} (input rms {np.sqrt((audio.astype(np.float64) ** 2).mean()):.3e})")
    with pytest.raises(ValueError):
        reconstruct_track(None, audio[:1000], phase="unet")


@pytest.mark.parametrize("a_len", [100, 184])
def test_short_tracks_are_one_clip(model, a_len):
    from phasegen.track import reconstruct_track, track_plan
    assert track_plan(a_len, 24, 8, 8)[2] == 1
    audio = detgen.normal(31, (a_len,))
    got = reconstruct_track(model, audio, stats=(0.1, 2.0), **SMALL)
    assert tuple(got.shape) == (a_len,)
    want, cmax, peak = compose(model, audio, 32, 8, 24, 8, (0.1, 2.0))
    check(got, want, cmax, peak, True, f"one-clip track of {a_len} samples")


def test_resampling_inside_equals_resampling_first(model):
    from phasegen import preproc
    from phasegen.track import reconstruct_track
    a44 = detgen.make_clip(8820, seed=41)                                           # 0.2 s at 44.1 kHz
    a16 = preproc.resample(a44, 44100, 16000)
    assert tuple(a16.shape) == (3200,)
    got = reconstruct_track(model, a44, stats=(0.1, 2.0), osr=44100, **SMALL)
    want = reconstruct_track(model, a16, stats=(0.1, 2.0), **SMALL)
    assert tuple(got.shape) == (3200,) and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_non_finite_model_output_raises():
    from phasegen.track import reconstruct_track
    p = detgen.make_params(16, seed=0)
    p[detgen.BN_U0 + ".weight"] = np.full_like(p[detgen.BN_U0 + ".weight"], np.inf)
    with pytest.raises(ValueError, match="Audio buffer is not finite everywhere"):
        reconstruct_track(small_model(p), detgen.normal(11, (1000,)), stats=(0.1, 2.0), **SMALL)


def test_build_dataset_returns_and_writes_its_statistics(tmp_path):
    from phasegen import preproc
    tracks = [detgen.make_clip(1000, seed=51), detgen.make_clip(700, seed=52)]
    kw = dict(chunk_seconds=0.01151, rsr=16000, n_fft=32, hop_length=8, n_random=0, n_val=2, seed=0)
    t_slice = int(0.01151 * 16000)
    assert t_slice == 184
    rng = np.random.default_rng(0)
    x = torch.cat([preproc.chunk_audio(t, t_slice, 32, 8, 0, rng) for t in tracks])[:, 0]       # the unnormalised array
    x64 = x.cpu().numpy().astype(np.float64)
    train, val, (mean, std) = preproc.build_dataset(tracks, out_dir=str(tmp_path), genre="T", return_stats=True, **kw)
    assert isinstance(mean, float) and isinstance(std, float)
    print(f"\ndataset statistics: mean {mean:.17g} (numpy {x64.mean():.17g}), std {std:.17g} (numpy {x64.std():.17g})")
    assert abs(mean - x64.mean()) <= 1e-12 * abs(x64.mean()) and abs(std - x64.std()) <= 1e-12 * x64.std()
    saved = np.load(tmp_path / "T_audio_stats.npy")
    assert saved.dtype == np.float64 and saved.shape == (2,) and saved[0] == mean and saved[1] == std
    assert len(val) == 2 and len(train) + len(val) == len(x64)
    both = preproc.build_dataset(tracks, out_dir=str(tmp_path / "plain"), genre="T", **kw)      # the default call: as before
    assert isinstance(both, tuple) and len(both) == 2
    assert np.array_equal(both[0], train) and np.array_equal(both[1], val)
    assert sorted(os.listdir(tmp_path / "plain")) == ["T_audio_train.npy", "T_audio_val.npy"]


def test_command_line(tmp_path, model):
    from scipy.io import wavfile
    weight, wav_in, wav_out = tmp_path / "unet.pth", tmp_path / "in.wav", tmp_path / "out.wav"
    model.save(str(weight))
    pcm = np.round(detgen.make_clip(1000, seed=61) * 20000).astype(np.int16)
    wavfile.write(wav_in, 16000, pcm)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--weight", str(weight),
                        "--input", str(wav_in), "--output", str(wav_out), "--channels", "16", "--frames", "24", "--overlap_frames", "8"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Reconstructed ")]
    assert len(lines) == 1 and lines[0].startswith("Reconstructed 0.06 s of audio in ") and lines[0].endswith(" s (8 clips).")
    assert "own mean and std" in r.stderr                                           # no --stats: says so
    sr, out = wavfile.read(wav_out)
    assert sr == 16000 and out.dtype == np.float32 and out.shape == (1000,) and float(np.abs(out).max()) == 1.0
