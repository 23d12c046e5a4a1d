"""GPU: single-pass spectrogram inversion -- pg_phase_spsi BIT FOR BIT against the numpy restatement of its contract
(tests/_spsi_ref.py) at every chunk boundary of the three-launch scan it shares with pg_phase_lock, its widths, layouts, store paths
and special inputs, the workspace and stream contract of the entry point, and the track level built on it (phasegen.track
phase="spsi", evaluate_stretch, evaluate_track with gl_init, reconstruct.py --phase spsi / --report_phases spsi / --gl_init).

Bounds.  The offset is three fp32 subtractions / additions, one multiplication by 0.5 and one IEEE division, the advance two double
operations and one rint, the scan integer sums modulo 2^32 and the peak rule plain fp32 comparisons: every comparison with the
restatement is exact.  The ordering on the melody: the float64 chain gives SC(spsi) = 0.072 against 0.90 for zero phase and 0.20
for the plain vocoder at stretch 1.5 (tests/test_spsi_host.py, tests/test_lock_host.py), so "below the plain vocoder" and "below a
quarter of zero" hold with room.  The device figure against the float64 chain: 1e-5 relative, the bound of
tests/test_z_lock_gpu.py::test_evaluate_stretch_orders_locked_before_plain_before_zero, between metrics.consistency on the device
and _vocoder_ref.consistency64 of the restatement's phase on the device's magnitudes.  Griffin-Lim: on one clip of the melody eight
iterations from the single-pass inversion reach 0.022 and from noise 0.24 on the CPU, so "lower" holds with room."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lock_ref as lref
import _spsi_ref as sref
import _vocoder_ref as ref
from phasegen import detgen
from test_z_lock_gpu import offset_view, same_bits, sparse_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)


def L():
    from phasegen import ops
    return ops.PHASE_LOCK_CHUNK


def plane(seed, n_ch, bins, F):
    """Magnitudes uniform in [0, 1): a peak every few bins, the regions change from frame to frame."""
    return np.random.RandomState(seed).uniform(0.0, 1.0, (n_ch, bins, F)).astype(np.float32)


def run(M, n_fft=64, hop=16, bin0=1, **kw):
    from phasegen import ops
    return ops.phase_spsi(torch.from_numpy(M).cuda(), n_fft, hop, bin0, **kw)


# ---- bit for bit against the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ch,bins", [(1, 5), (3, 5), (1, 130), (3, 65)])
def test_bitwise_against_the_restatement_at_every_chunk_boundary(n_ch, bins):
    for F in (1, 2, L() - 1, L(), L() + 1, 2 * L(), 2 * L() + 1, 3 * L() + 5):
        M = plane(1000 + F + bins, n_ch, bins, F)
        got = run(M)
        assert tuple(got.shape) == (n_ch, bins, F) and got.dtype == torch.float32
        want = sref.phase_spsi(M, 64, 16)
        assert np.abs(want).max() <= np.float32(np.pi)
        assert same_bits(got, want), (F, n_ch, bins)


@pytest.mark.parametrize("bins", [1, 2, 3, 5, 63, 64, 65, 130])
def test_bitwise_for_every_width(bins):
    M = plane(2000 + bins, 2, bins, 3 * L() + 5)
    assert same_bits(run(M), sref.phase_spsi(M, 64, 16)), bins


def test_an_odd_width_of_several_bins_per_thread():
    """bins = 1025 (two bins per thread, a last word of the peak mask with one bin in it) x 2 L + 1 frames."""
    M = plane(12, 1, 1025, 2 * L() + 1)
    assert same_bits(run(M, 2048, 512), sref.phase_spsi(M, 2048, 512))


def test_two_bins_per_thread_with_a_window():
    """bins = 2048 over L + 8 frames: two bins per thread and a staged window narrower than the chunk (several reloads per chunk)."""
    M = plane(21, 1, 2048, L() + 8)
    assert same_bits(run(M, 4096, 1024), sref.phase_spsi(M, 4096, 1024))


@pytest.mark.parametrize("bins", [4096, 3000])
def test_wide_planes_with_empty_words_in_the_peak_mask(bins):
    """Four (three) bins per thread, the narrowest window or none, over L + 3 frames; tests/test_z_lock_gpu.py's sparse planes: long
    runs of empty 64-bin words in the peak mask, the bins under them follow a peak many words away."""
    F = L() + 3
    _A, M = sparse_planes(13 + bins, bins, F)
    empty = [not lref.peaks(M[0, :, f])[w * 64:(w + 1) * 64].any() for f in range(F) for w in range(-(-bins // 64))]
    assert sum(empty) >= F * {4096: 27, 3000: 19}[bins]
    want, theta = sref.phase_spsi(M, 2 * bins, bins // 2, return_theta=True)
    b, P = bins // 3, lref.peak_map(M[0, :, F - 1])
    assert abs(P[b] - b) >= 64 and theta[0, b, -1] == theta[0, P[b], -1] and theta[0, :, -1].any()
    assert same_bits(run(M, 2 * bins, bins // 2), want)


@pytest.mark.parametrize("hop,n_fft,bin0", [(512, 2048, 1), (256, 1024, 1), (3, 8, 0), (1, 32, 1), (2048, 2048, 1)])
def test_hops_transform_sizes_and_first_bins(hop, n_fft, bin0):
    F = 2 * L() + 3
    for bins in (5, 130):
        M = plane(30 + bins + hop, 2, bins, F)
        want = sref.phase_spsi(M, n_fft, hop, bin0)
        assert same_bits(run(M, n_fft, hop, bin0), want), (bins, hop, n_fft, bin0)
    if bin0 == 1:
        assert not same_bits(run(M, n_fft, hop, 0), want)                   # bin0 enters: the advance and the half turn
    assert same_bits(run(M, n_fft, hop, 65536), sref.phase_spsi(M, n_fft, hop, 65536))       # the largest first bin


def test_constant_columns_advance_by_g_times_adv():
    """Every column the same: Theta_g[b] = g adv[P(b)] exactly over 3 L + 5 frames, whatever the chunking."""
    F, bins = 3 * L() + 5, 97
    m = plane(40, 1, bins, 1)[0, :, 0]
    M = np.ascontiguousarray(np.repeat(m[None, :, None], F, 2))
    for n_fft, hop, bin0 in ((2048, 512, 1), (8, 3, 0)):
        P, adv = lref.peak_map(m), sref.advance(m, n_fft, hop, bin0)
        g = np.arange(F, dtype=np.uint64)
        theta = ((g[None, :] * adv[P].astype(np.uint64)[:, None]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        want = ref.angle_of(theta + sref.parity(bins, bin0)[:, None])[None]
        assert same_bits(sref.phase_spsi(M, n_fft, hop, bin0), want)
        assert same_bits(run(M, n_fft, hop, bin0), want), (n_fft, hop, bin0)


# ---- special inputs ------------------------------------------------------------------------------------------------------

def test_plateaus_ties_infinities_and_nans_in_the_magnitude():
    inf, nan = np.inf, np.nan
    rows = [[1, 3, 3, 3, 1, 0, 0, 2, 0, 0, 0],                              # a plateau: its first bin is the peak, half a bin up
            [5, 0, 0, 0, 5, 0, 0, 0, 5, 0, 0],                              # exact ties between equal peaks: the lower one
            [0, inf, inf, 0, -inf, -inf, 1, 0, inf, 0, 0],                  # +-inf: inf - inf in the offset
            [0, 0, 7, nan, 0, 0, 9, 0, nan, 0, 8],                          # a NaN next to a peak disqualifies it
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],                              # all equal: bin 0 is the only peak
            [nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan],        # no peak at all: every bin on its own, offset 0
            [3, 1, 3, 2, 1e-40, 0, 2, 2, 5, 4, 5]]                          # d >= 0 at bin 1 (not a peak), a denormal, a peak at the end
    F = L() + 5
    M = np.ascontiguousarray(np.array(rows, np.float32)[np.arange(F) % 7].T[None])          # frame f shows row f % 7
    assert M.shape == (1, 11, F) and np.array_equal(M[0, :, 8], np.array(rows[1], np.float32), equal_nan=True)
    want, theta = sref.phase_spsi(M, 32, 8, return_theta=True)
    assert np.isfinite(want).all() and theta[0, :, -1].any()
    assert same_bits(run(M, 32, 8), want)
    assert same_bits(run(M, 32, 8, 0), sref.phase_spsi(M, 32, 8, 0))


# ---- layouts -------------------------------------------------------------------------------------------------------------

def test_a_plane_of_a_polar_tensor_is_read_in_place():
    from phasegen import ops
    rs = np.random.RandomState(16)
    F = 2 * L() + 9
    pol = np.stack([rs.uniform(0, 1, (3, 21, F)), rs.uniform(-np.pi, np.pi, (3, 21, F))], 1).astype(np.float32)     # (n_ch, 2, bins, F)
    pd = torch.from_numpy(pol).cuda()
    assert not pd[:, 0].is_contiguous() and pd[:, 0].stride(0) == 2 * 21 * F
    got = ops.phase_spsi(pd[:, 0], 64, 16)
    assert same_bits(got, sref.phase_spsi(pol[:, 0], 64, 16))
    assert same_bits(got, ops.phase_spsi(pd[:, 0].contiguous(), 64, 16))
    assert same_bits(pd.cpu(), pol)                                         # (and nothing of it was written)


def test_a_channel_alone_has_the_bits_it_has_in_a_batch():
    from phasegen import ops
    Md = torch.from_numpy(plane(17, 3, 21, 2 * L() + 1)).cuda()
    both = ops.phase_spsi(Md, 64, 16)
    for c in range(3):
        assert same_bits(ops.phase_spsi(Md[c:c + 1], 64, 16)[0], both[c]), c
    assert same_bits(ops.phase_spsi(Md[1:], 64, 16), both[1:])


def test_element_wise_store_path_equals_the_16_byte_path():
    from phasegen import ops
    full = plane(18, 2, 21, 2 * L() + 5)
    for F in (L(), 2 * L() + 4):                                            # multiples of 4: the 16-byte path when aligned
        M = np.ascontiguousarray(full[..., :F])
        Md = torch.from_numpy(M).cuda()
        wide = ops.phase_spsi(Md, 64, 16)
        assert wide.data_ptr() % 16 == 0 and same_bits(wide, sref.phase_spsi(M, 64, 16))
        out = offset_view(torch.zeros_like(wide))
        assert ops.phase_spsi(Md, 64, 16, out=out) is out
        assert same_bits(out, wide)
        assert same_bits(ops.phase_spsi(offset_view(Md), 64, 16), wide)
        M1 = np.ascontiguousarray(full[..., :F + 1])                        # F % 4 == 1: element-wise; a causal scan: the same head
        odd = ops.phase_spsi(torch.from_numpy(M1).cuda(), 64, 16)
        assert same_bits(odd[..., :F], wide) and same_bits(odd, sref.phase_spsi(M1, 64, 16))


# ---- the workspace and stream contract of the entry point ----------------------------------------------------------------------

def spsi_case(F, bins, n_ch=2):
    import test_z_workspace_gpu as W
    from phasegen import ops
    M = plane(3000 + F + bins, n_ch, bins, F)
    return W.Case(f"spsi-F{F}-b{bins}", {"M": W.cuda(M)}, lambda: {"out": W.sent(n_ch, bins, F)},
                  lambda i, o: [ops.phase_spsi(i["M"], 64, 16, out=o["out"])], poisons=(0x00,), symbol="pg_phase_spsi", lock=True)


def test_exact_poisoned_and_stale_workspaces_and_the_stream():
    """pg_phase_spsi under the helpers of tests/test_z_workspace_gpu.py and tests/test_z_streams_gpu.py: a workspace of EXACTLY the
    queried size between guards, zeroed or holding the maps of another, larger problem (the workspace holds gather indices, so a
    mistake has to show as wrong values, never as wrong addresses), 4 bytes off its alignment, and a busy side stream: the same
    bits, nothing written outside, no wait for the device.  Both modules count the entry point as reached by these cases."""
    import test_z_streams_gpu as S
    import test_z_workspace_gpu as W
    from _strict import strict_workspaces
    for F, bins in ((1, 1), (33, 5), (65, 64), (33, 1025)):
        case = spsi_case(F, bins, 1 if bins == 1025 else 2)
        W.check(case)
        big = spsi_case(F + 70, min(2 * bins + 3, 4096), 1 if bins == 1025 else 2)
        with strict_workspaces(0x00, keep=True) as s:
            big.run(big.ins, big.make_outs())
        (stale,) = s.contents
        assert bool((stale != 0).any())
        want = case.run(case.ins, case.make_outs())
        with strict_workspaces(0x00, stale=stale) as s:
            got = case.run(case.ins, case.make_outs())
        assert same_bits(got[0], want[0]), (F, bins)
    W.check(spsi_case(33, 5), offset=4)
    S.reach(spsi_case(33, 5))
    assert "pg_phase_spsi" in W.REACHED and "pg_phase_spsi" in S.REACHED


# ---- argument errors -----------------------------------------------------------------------------------------------------

def test_argument_errors():
    from phasegen import _lib, ops
    M = torch.zeros(2, 5, 25, device="cuda")
    for bad in (dict(hop=0), dict(hop=33), dict(n_fft=0), dict(bin0=-1), dict(bin0=65537), dict(out=torch.zeros(2, 5, 24, device="cuda"))):
        with pytest.raises(ValueError):
            ops.phase_spsi(M, **{**dict(n_fft=32, hop=8), **bad})
    for view in (M[:, :, ::2], M.transpose(1, 2), M.double(), M[0], M.cpu()):
        with pytest.raises(ValueError):
            ops.phase_spsi(view, 32, 8)
    wide = torch.zeros(1, 4097, 3, device="cuda")
    with pytest.raises(RuntimeError, match="4096 bins"):
        ops.phase_spsi(wide, 8194, 2048)
    # the workspace one byte short, with real pointers: refused before any launch
    lib = _lib.load()
    out = torch.full((2, 5, 25), 7.0, device="cuda")
    a = _lib.PhaseSpsiArgs()
    a.n_ch, a.bins, a.F, a.n_fft, a.hop, a.bin0 = 2, 5, 25, 32, 8, 1
    a.M, a.out, a.m_stride = M.data_ptr(), out.data_ptr(), 125
    need = lib.pg_workspace_bytes_phase_spsi(ctypes.byref(a))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert lib.pg_phase_spsi(ctypes.byref(a), None) == _lib.ERR_WORKSPACE
    a.workspace, a.workspace_bytes = None, need
    assert lib.pg_phase_spsi(ctypes.byref(a), None) == _lib.ERR_WORKSPACE
    a.workspace, a.hop = ws.data_ptr(), 33
    assert lib.pg_phase_spsi(ctypes.byref(a), None) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    a.hop, a.bins, a.workspace_bytes = 8, 4097, 1 << 40
    assert lib.pg_phase_spsi(ctypes.byref(a), None) == _lib.ERR_SHAPE


# ---- track level ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def melody():
    return ref.melody()


@pytest.mark.parametrize("stretch", [1.0, 1.5, 0.75])
def test_reconstruct_track_from_the_magnitudes_alone(melody, stretch):
    from phasegen.track import reconstruct_track
    out = reconstruct_track(None, melody, phase="spsi", join="spectral", stretch=stretch)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (round(melody.shape[0] * stretch),)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) == 1.0


def test_evaluate_stretch_orders_spsi_before_the_plain_vocoder_and_zero(melody):
    from phasegen import metrics, ops, track
    rep = track.evaluate_stretch(None, melody, 1.5, phases=("spsi", "vocoder", "zero"), return_audio=True)
    assert list(rep["metrics"]) == ["spsi", "vocoder", "zero"]
    sp, v, z = (rep["metrics"][p]["spectral_convergence"] for p in ("spsi", "vocoder", "zero"))
    print(f"\nmelody at stretch 1.5 on the device: SC spsi {sp:.4f}, vocoder {v:.4f}, zero {z:.4f}")
    assert sp < v and sp < 0.25 * z
    assert tuple(rep["audio"]["spsi"].shape) == (144000,)
    raw = track.reconstruct_track(None, melody, phase="spsi", join="spectral", stretch=1.5, normalize=False)
    assert same_bits(rep["audio"]["spsi"], raw)
    # against the float64 chain on the restatement's phase, the restatement run on the device's magnitudes
    an = track._analyse_spectral(melody, 2048, 512, 128, 32, None, None, 16000, "kaiser_best", 1.5)
    with torch.no_grad():
        dmag, full = track._invert_spectral(an, None, "spsi", 512, 128, 64)
        dph = ops.phase_spsi(dmag, 2048, 512)
    ph = sref.phase_spsi(dmag.cpu().numpy(), 2048, 512)
    assert same_bits(dph, ph)
    want = ref.consistency64(dmag.cpu().numpy(), 2048, 512, phase=ph)["spectral_convergence"]
    again = metrics.consistency(dmag, full, 2048, 512)["spectral_convergence"]
    print(f"spsi SC: device {sp:.7f} (again {again:.7f}), float64 chain on the restatement's phase {want:.7f}")
    assert again == sp
    assert abs(sp - want) <= 1e-5 * want


def test_evaluate_track_reports_spsi_under_the_spectral_join(melody):
    from phasegen import track
    rep = track.evaluate_track(None, melody, join="spectral", phases=("spsi",), return_audio=True)
    assert list(rep["metrics"]) == ["spsi"] and rep["join"] == "spectral" and rep["gl_init"] == "noise"
    m = rep["metrics"]["spsi"]
    print(f"\nmelody, spectral join, spsi against the input: SC {m['spectral_convergence']:.4f}, LSD {m['lsd_db']:.3f} dB")
    assert np.isfinite(m["spectral_convergence"]) and np.isfinite(m["lsd_db"])
    raw = track.reconstruct_track(None, melody, phase="spsi", join="spectral", normalize=False)
    assert same_bits(rep["audio"]["spsi"], raw)


def test_griffin_lim_starts_better_from_spsi_than_from_noise(melody):
    from phasegen import track
    reps = {init: track.evaluate_track(None, melody, phases=("griffinlim",), gl_iters=8, gl_init=init) for init in ("noise", "spsi")}
    sc = {init: rep["metrics"]["griffinlim"]["spectral_convergence"] for init, rep in reps.items()}
    print(f"\nmelody, 8 Griffin-Lim iterations per clip: SC from noise {sc['noise']:.4f}, from spsi {sc['spsi']:.4f}")
    assert [rep["gl_init"] for rep in reps.values()] == ["noise", "spsi"]
    assert sc["spsi"] < sc["noise"]
    default = track.evaluate_track(None, melody, phases=("griffinlim",), gl_iters=8)               # the default is the start from noise
    assert default["gl_init"] == "noise" and default["metrics"]["griffinlim"] == reps["noise"]["metrics"]["griffinlim"]


def test_pitch_shift_with_spsi():
    from phasegen.track import pitch_shift
    x = detgen.normal(98, (2, 1000))
    out = pitch_shift(None, x, 5, stats=(0.1, 2.0), phase="spsi", **SMALL)
    assert tuple(out.shape) == (2, 1000) and bool(torch.isfinite(out).all()) and float(out.abs().max()) == 1.0


# ---- command line --------------------------------------------------------------------------------------------------------

def _cli(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--channels", "16", "--hop", "8",
                           "--frames", "24", "--overlap_frames", "4", *map(str, flags)], capture_output=True, text=True, timeout=300)


def test_reconstruct_cli_with_spsi_and_a_stretch_report(tmp_path):
    from scipy.io import wavfile
    wav, out, rep = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "stretch.json"
    wavfile.write(str(wav), 16000, detgen.normal(99, (4000,)).astype(np.float32) * 0.1)
    r = _cli("--input", wav, "--output", out, "--phase", "spsi", "--stretch", "1.5", "--stretch_report", rep)      # no --weight
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Stretch report" in r.stdout and "spsi spectral convergence" in r.stdout
    sr, y = wavfile.read(str(out))
    assert sr == 16000 and y.shape == (6000,) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    report = json.load(open(rep))
    assert list(report["metrics"]) == ["spsi", "vocoder", "zero"] and (report["n_samples"], report["n_out"]) == (4000, 6000)


def test_reconstruct_cli_reports_spsi_and_starts_griffin_lim_from_it(tmp_path):
    from scipy.io import wavfile
    from phasegen.model import UNetModel
    weight, wav, out = tmp_path / "unet.pth", tmp_path / "in.wav", tmp_path / "out.wav"
    UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0)).save(str(weight))
    wavfile.write(str(wav), 16000, detgen.normal(97, (1500,)).astype(np.float32) * 0.1)
    base = ("--weight", weight, "--input", wav, "--output", out)
    rep = tmp_path / "spectral.json"
    r = _cli(*base, "--join", "spectral", "--report", rep, "--report_phases", "unet,spsi")
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.load(open(rep))
    assert list(report["metrics"]) == ["unet", "spsi"] and report["join"] == "spectral" and report["gl_init"] == "noise"
    rep = tmp_path / "gl.json"
    r = _cli(*base, "--report", rep, "--report_phases", "unet,griffinlim", "--gl_iters", "2", "--gl_init", "spsi")
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.load(open(rep))
    assert list(report["metrics"]) == ["unet", "griffinlim"] and report["gl_init"] == "spsi" and report["flags"]["gl_init"] == "spsi"
    r = _cli(*base, "--report", rep, "--report_phases", "unet,spsi")                # the waveform join: refused by the parser
    assert r.returncode == 2 and "spsi needs --join spectral" in r.stderr
