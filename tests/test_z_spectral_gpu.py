"""GPU: the spectral track join -- pg_spec_clips and pg_phase_join against the float64 restatements of tests/_spectral_ref.py, the
track-level path built on them (phasegen.track: join="spectral", stretch, pitch_shift), and pg_istft at whole-track frame counts.

  spec_clips   BITWISE against the restatement with fp32 rounding emulated (the positions are doubles and the weights fp32 in both).
  phase_join   frames covered by one clip are bit-identical copies; a shared frame is held to
                   |z_ref| * |exp(j out) - exp(j ref)| <= JOIN_BOUND,   z_ref the float64 blend,
               which does not depend on the blend's conditioning: two roundings per component of z give about 3e-7, the fp32
               sin / cos and atan2 of csrc/pg_fastmath.h (2.5e-7 + 6e-8 |phi| and 3e-7 absolute, |phi| <= 8) about 1e-6: 1.3e-6
               together.  Measured maximum on an MI355X over the cases of this file: 7.8e-7 (printed by every case); JOIN_BOUND
               is 4 x that, 2.5 x the estimate.
  track level  tolerances of tests/test_signal_gpu.py: 5e-5 of max-abs for an STFT -> ISTFT round trip
               (test_stft_istft_round_trip_full_size, line 209) and 2e-5 for pg_istft against the oracle's (test_istft_vs_oracle,
               line 96); everything the join must not touch is compared bit for bit.
"""
import numpy as np
import pytest
import torch

import _spectral_ref as ref
from oracle import signal_ref
from phasegen import detgen

pytestmark = pytest.mark.gpu
JOIN_BOUND = 3.2e-6
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)       # C = 16: sf = 19, Vf = 5; 1000 samples: 7 clips, ragged tail
A_LEN = 1000


def bits(t):
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def relmax(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def offset_view(t):
    """The same values one element off the allocation's 16-byte grid: the scalar path."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- pg_spec_clips ---------------------------------------------------------------------------------------------------------

def plane(seed, shape):
    return detgen.normal(seed, shape).astype(np.float32)


@pytest.mark.parametrize("rate", [1.0, 0.8, 1.25, 1.0 / 3.0, 1.5])       # 1.5: clips 1 and 2 run past the source (g 1.5 > 18) and clamp
def test_spec_clips_bitwise(rate):
    from phasegen import ops
    P = plane(71, (2, 5, 19))
    got = ops.spec_clips(torch.from_numpy(P).cuda(), 3, 8, 5, rate)
    want = ref.spec_clips_f32(P, 3, 8, 5, rate)
    assert tuple(got.shape) == want.shape == (3, 2, 5, 8)
    assert np.array_equal(bits(got), bits(want))
    if rate == 1.5:
        assert np.array_equal(bits(got[2, :, :, 3:]), bits(np.repeat(P[:, :, 18:19], 5, 2)))      # g >= 13 -> p >= 19.5: the last frame
    assert np.abs(got.cpu().numpy().astype(np.float64) - ref.spec_clips(P, 3, 8, 5, rate)).max() <= 3 * 2.0 ** -24 * 2 * np.abs(P).max()


@pytest.mark.parametrize("n_clips", [3, 5])                             # 5: clips 3 and 4 reach frames 12 .. 23 of 20, units past the end
def test_spec_clips_vector_path_equals_scalar_path(n_clips):
    from phasegen import ops
    P = plane(72, (2, 4, 20))
    Pd = torch.from_numpy(P).cuda()
    assert Pd.data_ptr() % 16 == 0
    wide = ops.spec_clips(Pd, n_clips, 8, 4, 1.0)
    want = ref.spec_clips_f32(P, n_clips, 8, 4, 1.0)
    assert np.array_equal(bits(wide), bits(want))
    narrow_in = ops.spec_clips(offset_view(Pd), n_clips, 8, 4, 1.0)
    out = offset_view(torch.zeros_like(wide))
    narrow_out = ops.spec_clips(Pd, n_clips, 8, 4, 1.0, out=out)
    assert np.array_equal(bits(narrow_in), bits(wide)) and np.array_equal(bits(narrow_out), bits(wide))
    assert np.array_equal(bits(ops.spec_clips(Pd, n_clips, 8, 4, 0.5)), bits(ref.spec_clips_f32(P, n_clips, 8, 4, 0.5)))     # aligned, rate != 1


def test_spec_clips_reads_a_plane_of_a_polar_tensor_in_place():
    from phasegen import ops
    pol = plane(73, (2, 2, 5, 19))
    pd = torch.from_numpy(pol).cuda()
    for which in (0, 1):
        for rate in (1.0, 0.8):
            got = ops.spec_clips(pd[:, which], 3, 8, 5, rate)
            assert np.array_equal(bits(got), bits(ref.spec_clips_f32(pol[:, which], 3, 8, 5, rate)))
    wide = plane(74, (2, 2, 4, 20))                                      # channel stride 160: the 16-byte path on a strided plane
    wd = torch.from_numpy(wide).cuda()
    assert np.array_equal(bits(ops.spec_clips(wd[:, 1], 3, 8, 4, 1.0)), bits(ref.spec_clips_f32(wide[:, 1], 3, 8, 4, 1.0)))


@pytest.mark.parametrize("rate,F_out", [(0.8, 23), (1.0, 19), (1.0, 16), (1.25, 15), (0.25, 73)])
def test_spec_clips_whole_plane_form(rate, F_out):
    from phasegen import ops
    P = plane(75, (2, 5, 19))
    got = ops.spec_clips(torch.from_numpy(P).cuda(), 1, F_out, F_out, rate)
    assert tuple(got.shape) == (1, 2, 5, F_out)
    assert np.array_equal(bits(got), bits(ref.spec_clips_f32(P, 1, F_out, F_out, rate)))
    if rate == 1.0:
        assert np.array_equal(bits(got[0]), bits(P[:, :, :F_out]))


@pytest.mark.parametrize("rate", [1.0, 0.8])
def test_spec_clips_batch_independence(rate):
    from phasegen import ops
    P = plane(76, (2, 5, 19))
    Pd = torch.from_numpy(P).cuda()
    three = ops.spec_clips(Pd, 3, 8, 5, rate)
    alone = ops.spec_clips(Pd, 1, 18, 18, rate)                          # the whole-plane form: frames 10 .. 17 are clip 2
    assert np.array_equal(bits(three[2]), bits(alone[0, :, :, 10:18]))
    five = ops.spec_clips(Pd, 5, 8, 5, rate)
    assert np.array_equal(bits(five[:3]), bits(three))
    one_ch = ops.spec_clips(Pd[1:], 3, 8, 5, rate)                       # channel 1 alone, at position 0
    assert np.array_equal(bits(one_ch[:, 0]), bits(three[:, 1]))


def test_spec_clips_several_workgroups():
    from phasegen import ops
    P = plane(77, (2, 40, 61))
    Pd = torch.from_numpy(P).cuda()
    for rate in (1.0, 0.7):
        got = ops.spec_clips(Pd, 9, 12, 6, rate)                         # 720 rows x 3 units
        assert np.array_equal(bits(got), bits(ref.spec_clips_f32(P, 9, 12, 6, rate)))


# ---- pg_phase_join -----------------------------------------------------------------------------------------------------------

def phases(seed, shape):
    return np.random.RandomState(seed).uniform(-8.0, 8.0, shape).astype(np.float32)


def check_join(got, phi, sf, what, ramp_=None):
    """Copies bit for bit, shared frames under JOIN_BOUND; -> the measured maximum."""
    got = got.cpu().numpy()
    want = ref.phase_join(phi, sf, ramp_)
    z, shared = ref.phase_join_z(phi, sf, ramp_)
    assert got.shape == want.shape
    assert np.array_equal(bits(got[:, :, ~shared]), bits(want[:, :, ~shared].astype(np.float32)))
    g, w = got[:, :, shared].astype(np.float64), want[:, :, shared]
    err = np.abs(z[:, :, shared]) * np.abs(np.exp(1j * g) - np.exp(1j * w))
    assert np.all(np.abs(g) <= np.pi + 1e-6)                             # a joined phase is an atan2
    worst = float(err.max()) if err.size else 0.0
    print(f"\nphase_join {what}: max |z| |e^(j out) - e^(j ref)| = {worst:.3e} (bound {JOIN_BOUND:g})")
    assert worst <= JOIN_BOUND
    return worst


@pytest.mark.parametrize("Vf", [1, 3, 4])
def test_phase_join_against_float64(Vf):
    from phasegen import ops
    sf = 8 - Vf
    phi = phases(80 + Vf, (3, 2, 5, 8))
    got = ops.phase_join(torch.from_numpy(phi).cuda(), sf)
    assert tuple(got.shape) == (2, 5, 2 * sf + 8)
    check_join(got, phi, sf, f"Vf = {Vf}")


def test_phase_join_several_workgroups():
    from phasegen import ops
    phi = phases(85, (9, 2, 40, 12))
    for sf in (6, 8, 11):                                                # sf 8: the 16-byte path; Vf = 6, 4, 1
        got = ops.phase_join(torch.from_numpy(phi).cuda(), sf)
        check_join(got, phi, sf, f"9 clips of 12 frames, sf = {sf}")


def test_phase_join_degenerate_cells_take_the_documented_choice():
    from phasegen import ops
    # equal weights, lo = 0, hi = float32(pi): pg_sincos reduces float32(pi) to k = 1, r = 0 exactly, so zr = 0.5 - 0.5 = 0 and
    # zi = 0 + (-0) = 0: out = hi (b >= a), bit for bit -- not atan2(0, 0) = 0
    phi = phases(86, (2, 1, 3, 8))
    pi32 = np.float32(np.pi)
    phi[0, 0, :, 7], phi[1, 0, :, 0] = 0.0, pi32
    half = torch.tensor([0.5], dtype=torch.float32).cuda()
    got = ops.phase_join(torch.from_numpy(phi).cuda(), 7, ramp=half).cpu().numpy()
    assert tuple(got.shape) == (1, 3, 15) and np.array_equal(bits(got[0, :, 7]), bits(np.full(3, pi32)))
    assert np.array_equal(bits(np.delete(got, 7, 2)), bits(np.delete(np.concatenate([phi[0, 0, :, :7], phi[1, 0]], 1), 7, 1)[None]))
    # a blend that is not finite: b >= a picks hi, b < a picks lo
    phi = phases(87, (2, 1, 3, 8))
    phi[0, 0, :, 6:8] = np.inf                                           # lo of both shared frames (sf = 6, Vf = 2)
    r = torch.tensor([0.75, 0.25], dtype=torch.float32).cuda()            # j = 0: a = 0.25, b = 0.75; j = 1: a = 0.75, b = 0.25
    got = ops.phase_join(torch.from_numpy(phi).cuda(), 6, ramp=r).cpu().numpy()
    assert np.array_equal(bits(got[0, :, 6]), bits(phi[1, 0, :, 0])) and np.array_equal(bits(got[0, :, 7]), bits(phi[0, 0, :, 7]))
    assert np.isinf(got[0, :, 7]).all() and np.isfinite(np.delete(got, 7, 2)).all()


def test_phase_join_nan_reaches_only_the_frames_its_clip_covers():
    from phasegen import ops
    for sf in (5, 4):                                                    # scalar and 16-byte path
        phi = phases(88, (3, 2, 4, 8))
        phi[1, 0] = np.nan                                               # clip 1 of channel 0 covers frames sf .. sf + 7
        got = ops.phase_join(torch.from_numpy(phi).cuda(), sf).cpu().numpy()
        covered = np.zeros(got.shape[2], bool)
        covered[sf:sf + 8] = True
        assert np.isfinite(got[1]).all() and np.isfinite(got[0][:, ~covered]).all()
        clean = phi.copy()
        clean[1, 0] = 0.0
        want = ops.phase_join(torch.from_numpy(clean).cuda(), sf).cpu().numpy()
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[0][:, ~covered]), bits(want[0][:, ~covered]))
        Vf = 8 - sf
        assert np.isnan(got[0][:, sf + Vf:2 * sf]).all()                 # the clip's own frames
        # a shared frame falls back to (b >= a ? hi : lo): while b < a that is the finite lower clip, phi[0][j + sf]
        assert np.array_equal(bits(got[0][:, sf:sf + Vf // 2]), bits(phi[0, 0][:, sf:sf + Vf // 2]))
        assert np.isnan(got[0][:, sf + Vf // 2:sf + Vf]).all()


def test_phase_join_reads_the_phase_half_of_a_model_output_in_place():
    from phasegen import ops
    for bins, frames, sf in ((5, 8, 5), (4, 8, 4)):
        y = phases(89, (6, 2 * bins, frames))                            # (clip, channel) rows of 2 * bins
        yd = torch.from_numpy(y).cuda()
        view = yd.view(3, 2, 2 * bins, frames)[:, :, :bins]
        assert not view.is_contiguous()
        got = ops.phase_join(view, sf)
        phi = np.ascontiguousarray(y.reshape(3, 2, 2 * bins, frames)[:, :, :bins])
        check_join(got, phi, sf, f"phase half in place, bins = {bins}")
        assert np.array_equal(bits(got), bits(ops.phase_join(torch.from_numpy(phi).cuda(), sf)))


def test_phase_join_vector_path_equals_scalar_path():
    from phasegen import ops
    phi = phases(90, (3, 2, 4, 8))
    phi[2, 1, 0, 0] = np.nan
    pd = torch.from_numpy(phi).cuda()
    wide = ops.phase_join(pd, 4)
    check_join(wide[:1], phi[:, :1], 4, "16-byte path")
    narrow_in = ops.phase_join(offset_view(pd), 4)
    narrow_out = ops.phase_join(pd, 4, out=offset_view(torch.zeros_like(wide)))
    narrow_ramp = ops.phase_join(pd, 4, ramp=offset_view(torch.from_numpy(ref.ramp(4)).cuda()))
    for other in (narrow_in, narrow_out, narrow_ramp):
        assert np.array_equal(bits(other), bits(wide))


def test_phase_join_channel_position_independence():
    from phasegen import ops
    for sf in (5, 4):
        phi = phases(91, (3, 2, 4, 8))
        pd = torch.from_numpy(phi).cuda()
        both = ops.phase_join(pd, sf)
        for c in (0, 1):
            alone = ops.phase_join(pd[:, c:c + 1], sf)
            assert np.array_equal(bits(alone[0]), bits(both[c]))


# ---- track level -----------------------------------------------------------------------------------------------------------

def small_model():
    from phasegen.model import UNetModel
    return UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0))


@pytest.fixture(scope="module")
def model():
    return small_model()


@pytest.fixture(scope="module")
def tones():
    """Two channels of three sines at bin centres 3, 5, 9 of 32: under the periodic Hann window each occupies exactly three bins, so
    dropping the DC bin removes nothing wherever a frame sees the signal alone (away from the reflected head and the zero tail)."""
    t = np.arange(A_LEN, dtype=np.float64)
    rs = np.random.RandomState(92)
    x = np.zeros((2, A_LEN))
    for c in range(2):
        for k in (3, 5, 9):
            x[c] += rs.uniform(0.2, 1.0) * np.cos(2 * np.pi * k * t / 32 + rs.uniform(0, 2 * np.pi))
    return x.astype(np.float32)


def pipeline64(x, mean, std, stretch=1.0):
    """float64 pipeline of the spectral join, phase "original": whole-track STFT of the zero-filled track, standardise, polar, clip
    windows of the angle plane, join, ISTFT of (exp(logmag) - 1) e^{j phase} on the first F_out frames."""
    from phasegen.track import spectral_plan
    pl = spectral_plan(x.shape[1], 24, 8, 4, stretch)
    outs = []
    for c in range(x.shape[0]):
        xp = np.zeros(pl.n_src, np.float32)
        n = min(x.shape[1], pl.n_src)
        xp[:n] = x[c, :n]
        S = signal_ref.stft(xp, 32, 8).astype(np.complex128)[1:]                      # (16, F_src), DC dropped
        z = ((S.real - mean) / std) + 1j * ((S.imag - mean) / std)
        logmag, ang = np.log1p(np.abs(z)), np.angle(z)
        ph = ref.phase_join(ref.spec_clips(ang[None], pl.n_clips, 24, pl.sf, 1.0)[:, 0][:, None], pl.sf)[0]
        Z = np.expm1(logmag[:, :pl.F_out]) * np.exp(1j * ph)
        Z = np.concatenate([np.zeros((1, pl.F_out)), Z], 0)
        outs.append(signal_ref.istft(Z, 8).astype(np.float64)[:pl.a_out])
    return np.stack(outs)


def test_original_phase_round_trip(tones):
    from phasegen.track import reconstruct_track, spectral_plan
    assert tuple(spectral_plan(A_LEN, 24, 8, 4)) == (19, 5, 1000, 7, 138, 139, 1104)
    got = reconstruct_track(None, tones, phase="original", join="spectral", stats=(0.0, 2.0), normalize=False, **SMALL)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2, A_LEN)
    back = 2.0 * got.cpu().numpy().astype(np.float64)
    # the project's sense of "equals x" (tests/test_signal_gpu.py:206-209): x without what the dropped DC bin carried
    for c in range(2):
        xp = np.zeros(1104, np.float32)
        xp[:A_LEN] = tones[c]
        S0 = signal_ref.stft(xp, 32, 8)
        S0[0] = 0
        w = signal_ref.istft(S0[:, :138], 8)[:A_LEN]
        e = relmax(back[c], w)
        print(f"\nspectral round trip, channel {c}: {e:.3e} of max-abs against the DC-free input (bound 5e-5)")
        assert e < 5e-5
    # and x itself where every covering frame sees the tones alone: frames 2 .. 123, samples 24 .. 975
    e = relmax(back[:, 24:976], tones[:, 24:976])
    print(f"spectral round trip against the input itself, samples 24 .. 975: {e:.3e} of max-abs (bound 5e-5)")
    assert e < 5e-5
    mono = reconstruct_track(None, tones[0], phase="original", join="spectral", stats=(0.0, 2.0), normalize=False, **SMALL)
    assert tuple(mono.shape) == (A_LEN,) and relmax(2.0 * mono.cpu().numpy().astype(np.float64), back[0]) < 5e-5


def test_original_phase_equals_the_float64_pipeline(tones):
    from phasegen.track import reconstruct_track
    x = (tones + 0.3 * detgen.normal(93, (2, A_LEN))).astype(np.float32)
    got = reconstruct_track(None, x, phase="original", join="spectral", stats=(0.3, 2.0), normalize=False, **SMALL)
    want = pipeline64(x, 0.3, 2.0)
    e = relmax(got, want)
    print(f"\nspectral join against the float64 pipeline: {e:.3e} of max-abs (bound 5e-5)")
    assert tuple(got.shape) == want.shape and e < 5e-5
    own = reconstruct_track(None, x, phase="original", join="spectral", normalize=False, **SMALL)        # the track's own moments
    xp = np.zeros((2, 1104), np.float32)
    xp[:, :A_LEN] = x
    S = np.stack([signal_ref.chunk_and_stft(xp[c], 32, 8) for c in range(2)]).astype(np.float64)
    assert relmax(own, pipeline64(x, S.mean(), S.std())) < 5e-5
    normed = reconstruct_track(None, x, phase="original", join="spectral", stats=(0.3, 2.0), **SMALL)
    assert float(normed.abs().max()) == 1.0


def whole_track_polar(x, n_src, stats):
    from phasegen import ops
    xd = torch.from_numpy(x).cuda()
    begin = torch.arange(x.shape[0], dtype=torch.int64) * x.shape[1]
    return ops.stft_crops(xd.reshape(-1), begin.cuda(), (begin + x.shape[1]).cuda(), n_src, 32, 8, polar=True, stats=stats)


def test_zero_phase_keeps_the_magnitudes_bit_for_bit():
    from phasegen import ops
    from phasegen.track import reconstruct_track
    x = detgen.normal(94, (2, A_LEN))
    got = reconstruct_track(None, x, phase="zero", join="spectral", stats=(0.3, 2.0), normalize=False, **SMALL)
    pol = whole_track_polar(x, 1104, (0.3, 2.0))
    assert tuple(pol.shape) == (2, 2, 16, 139)
    mag = pol[:, 0, :, :138].contiguous()
    want = ops.istft(mag, torch.zeros_like(mag), 8, mode=0, normalize=False)[:, :A_LEN]
    assert np.array_equal(bits(got), bits(want))


def test_waveform_join_is_untouched(model):
    from phasegen.track import evaluate_track, reconstruct_track
    x = detgen.normal(95, (2, A_LEN))
    for phase, m in (("original", None), ("unet", model)):
        a = reconstruct_track(m, x, stats=(0.3, 2.0), phase=phase, **SMALL)
        b = reconstruct_track(m, x, stats=(0.3, 2.0), phase=phase, join="waveform", **SMALL)
        c = reconstruct_track(m, x, stats=(0.3, 2.0), phase=phase, join="waveform", stretch=1.0, **SMALL)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    r = evaluate_track(None, x, stats=(0.3, 2.0), phases=("zero", "original"), **SMALL)
    assert r["join"] == "waveform" and r["n_clips"] == 7


@pytest.mark.parametrize("stretch", [1.5, 0.75])
def test_stretch_with_zero_phase(stretch):
    from phasegen import ops
    from phasegen.track import reconstruct_track, spectral_plan
    x = detgen.normal(96, (2, A_LEN))
    pl = spectral_plan(A_LEN, 24, 8, 4, stretch)
    got = reconstruct_track(None, x, phase="zero", join="spectral", stretch=stretch, stats=(0.3, 2.0), normalize=False, **SMALL)
    assert tuple(got.shape) == (2, round(A_LEN * stretch)) == (2, pl.a_out) and bool(torch.isfinite(got).all())
    logmag = whole_track_polar(x, pl.n_src, (0.3, 2.0))[:, 0].cpu().numpy()
    assert logmag.shape == (2, 16, pl.F_src)
    mag = torch.from_numpy(ref.spec_clips_f32(logmag, 1, pl.F_out, pl.F_out, 1.0 / stretch)[0]).cuda()
    want = ops.istft(mag, torch.zeros_like(mag), 8, mode=0, normalize=False)[:, :pl.a_out]
    assert np.array_equal(bits(got), bits(want))
    mono = reconstruct_track(None, x[0], phase="zero", join="spectral", stretch=stretch, stats=(0.3, 2.0), normalize=False, **SMALL)
    assert np.array_equal(bits(mono), bits(got[0]))


def test_small_model_report_and_reconstruction_agree(model):
    from phasegen.track import evaluate_track, reconstruct_track
    x = detgen.normal(97, (2, A_LEN))
    rep = evaluate_track(model, x, stats=(0.1, 2.0), phases=("unet", "zero", "original"), join="spectral", return_audio=True, **SMALL)
    assert rep["join"] == "spectral" and rep["n_clips"] == 7 and rep["n_samples"] == A_LEN
    for p in ("unet", "zero", "original"):
        m = rep["metrics"][p]
        assert all(np.isfinite(v) for v in m.values() if isinstance(v, float)), (p, m)
        assert tuple(rep["audio"][p].shape) == (2, A_LEN)
    assert rep["metrics"]["original"]["si_sdr_db"] > rep["metrics"]["zero"]["si_sdr_db"]
    raw = reconstruct_track(model, x, stats=(0.1, 2.0), join="spectral", normalize=False, **SMALL)
    assert np.array_equal(bits(rep["audio"]["unet"]), bits(raw))
    chunked = reconstruct_track(model, x, stats=(0.1, 2.0), join="spectral", normalize=False, clip_batch=3, **SMALL)
    # (convolutions may split their work differently with the batch size, and a circular mean of two nearly opposite phases is
    # ill-conditioned: the two runs need not agree to any fixed tolerance -- the chunked path is exercised, the difference printed)
    assert tuple(chunked.shape) == (2, A_LEN) and bool(torch.isfinite(chunked).all())
    print(f"\nclip_batch 3 vs 64 under the spectral join: {relmax(chunked, raw.cpu().numpy()):.3e} of max-abs (information only)")
    stretched = reconstruct_track(model, x[0], stats=(0.1, 2.0), join="spectral", stretch=1.25, **SMALL)
    assert tuple(stretched.shape) == (1250,) and float(stretched.abs().max()) == 1.0


@pytest.mark.parametrize("semitones", [12, -7])
def test_pitch_shift(model, semitones):
    from phasegen.track import pitch_shift
    x = detgen.normal(98, (2, A_LEN))
    out = pitch_shift(model, x, semitones, stats=(0.1, 2.0), **SMALL)
    assert out.is_cuda and tuple(out.shape) == (2, A_LEN) and bool(torch.isfinite(out).all()) and float(out.abs().max()) == 1.0
    mono = pitch_shift(None, x[0], semitones, stats=(0.1, 2.0), phase="zero", normalize=False, **SMALL)
    assert tuple(mono.shape) == (A_LEN,) and bool(torch.isfinite(mono).all())


def test_value_errors(model):
    from phasegen.track import evaluate_track, pitch_shift, reconstruct_track
    x = detgen.normal(99, (A_LEN,))
    for kw in (dict(join="spectral", phase="griffinlim"), dict(join="nope"), dict(stretch=1.5), dict(join="waveform", stretch=0.5),
               dict(join="spectral", stretch=1.5, phase="original"), dict(join="spectral", stretch=5.0, phase="zero"),
               dict(join="spectral", stretch=float("nan"), phase="zero"), dict(join="spectral", phase="unet")):
        with pytest.raises(ValueError):
            reconstruct_track(None, x, stats=(0.1, 2.0), **{**dict(phase="zero"), **kw}, **SMALL)
    with pytest.raises(ValueError):
        evaluate_track(model, x, phases=("unet", "griffinlim"), join="spectral", **SMALL)
    with pytest.raises(ValueError):
        pitch_shift(None, x, 25, phase="zero", **SMALL)
    with pytest.raises(ValueError):
        pitch_shift(None, x, 3, phase="original", **SMALL)


# ---- pg_istft at whole-track frame counts --------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsig,frames", [(1, 1500), (3, 700)])
def test_istft_on_long_tracks_vs_oracle(nsig, frames):
    from phasegen import ops
    bins, hop = 32, 16                                                  # n_fft = 64
    re = detgen.normal(33, (nsig, bins, frames))
    im = detgen.normal(34, (nsig, bins, frames))
    y = ops.istft(torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda(), hop, mode=1, normalize=False).cpu().numpy()
    for i in range(nsig):
        S = np.concatenate([np.zeros((1, frames), np.complex64), (re[i] + 1j * im[i]).astype(np.complex64)], 0)
        w = signal_ref.istft(S, hop)
        assert y[i].shape == w.shape == (hop * (frames - 1),)
        e = relmax(y[i], w)
        print(f"\nistft, {frames} frames, signal {i}: {e:.3e} of max-abs (bound 2e-5)")
        assert e < 2e-5
