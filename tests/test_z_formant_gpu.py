"""GPU: pg_formant_shift (ops.formant_shift) against the float64 restatement of its contract (tests/_formant_ref.py), the bit-for-bit
promises of the header, the confinement of non-finite cells, one far channel stride, the stream contract of the entry point, the
track-level option (reconstruct_track / pitch_shift) and the command-line flags.

Bounds.  Per frame r = |got - ref64| / (2^-24 max_k h[k]) for the envelope (h: the peak-held frame) and |got - ref64| / (2^-24 max_k
|out|) for `out`; a case passes when its largest r is at most MARGIN = 4 times the largest r of seq32 -- the same steps in numpy
float32 with strictly sequential sums -- ON THE SAME INPUT.  Nothing here is derived from what the kernel gives; each case prints
both figures before it asserts.  A frame whose h is all zero must be exactly zero.

Shapes: bins 5 / 40 / 1024 (below one 32-bin block, two blocks with a partial one, every wave busy), 1056 / 2080 / 4096 bins (the 16-
and 8-frame tiles), F 1 / 33 / 70 (one partial tile, a tile and a frame, three tiles), hold on both sides of every path of the
peak hold (0, 1, 2, 3, 16, and one at least as wide as the plane), orders 1 / 5 / 64.

The stream case goes through tests/test_z_streams_gpu.py's `reach`, which registers pg_formant_shift in that module's REACHED: its
coverage gate (test_zz_every_stream_entry_point_...) therefore passes in a whole-suite run only, as the workspace module's does."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _far
import _formant_ref as fref
from test_z_lock_gpu import same_bits
from test_z_workspace_gpu import off4

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R4 = 2.0 ** (4.0 / 12.0)
EPS = 0.01


def plane(seed, shape, top=6.0):
    """uniform in [0, top] with a tenth of the cells zero and one silent frame per channel where there is room"""
    rs = np.random.RandomState(seed)
    M = rs.uniform(0.0, top, shape).astype(np.float32)
    M[rs.uniform(size=shape) < 0.1] = 0.0
    if shape[2] > 2:
        M[:, :, 2] = 0.0
    return M


def on_device(M, layout):
    """dense, or pol[:, 0] of a (n_ch, 2, bins, F) polar tensor (channels 2 bins rows apart), optionally 4 bytes off 16-byte alignment"""
    t = torch.from_numpy(M).cuda()
    if layout.startswith("polar"):
        pol = torch.full((M.shape[0], 2) + M.shape[1:], float("nan"), device="cuda")
        if layout.endswith("off4"):
            pol = off4(pol)
        pol[:, 0] = t
        v = pol[:, 0]
        assert not v.is_contiguous() or M.shape[0] == 1
        return v
    return off4(t) if layout.endswith("off4") else t


#        bins order hold iters  F  layout        ratio  outputs
CASES = [(5, 1, 0, 0, 1, "dense", 1.0, "both"),
         (5, 5, 1, 2, 33, "polar", 0.5, "both"),
         (5, 5, 16, 2, 70, "dense", 4.0, "out"),
         (40, 1, 16, 0, 70, "polar", R4, "env"),
         (40, 5, 0, 2, 33, "dense_off4", 2.0, "both"),
         (40, 5, 2, 2, 33, "polar_off4", 0.5, "both"),
         (40, 5, 3, 0, 70, "dense", R4, "both"),
         (40, 5, 64, 2, 1, "polar", 4.0, "both"),
         (1024, 64, 16, 2, 70, "polar", R4, "both"),
         (1024, 64, 1, 0, 33, "dense_off4", 0.5, "both"),
         (1024, 5, 0, 2, 33, "dense", 2.0, "out"),
         (1024, 1, 16, 2, 1, "dense", 4.0, "env"),
         (1024, 64, 16, 2, 33, "dense", 1.0, "both"),
         (1056, 64, 16, 2, 33, "dense", R4, "both"),
         (2080, 64, 64, 1, 17, "polar", 0.5, "both"),
         (4096, 64, 2, 1, 9, "dense", 2.0, "both")]


def run(Md, ratio, order, hold, iters, outputs, off=False):
    from phasegen import ops
    n = tuple(Md.shape)
    if outputs == "env":
        o = off4(torch.full(n, -77.0, device="cuda")) if off else None
        return ops.formant_envelope(Md, order, hold, iters, out=o), None
    o = off4(torch.full(n, -77.0, device="cuda")) if off else None
    if outputs == "out":
        return None, ops.formant_shift(Md, ratio, order, hold, iters, EPS, out=o)
    out, env = ops.formant_shift(Md, ratio, order, hold, iters, EPS, return_env=True, out=o)
    return env, out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(round(v, 3)) if isinstance(v, float) else str(v) for v in c))
def test_values_against_float64(case):
    from phasegen import ops
    bins, order, hold, iters, F, layout, ratio, outputs = case
    M = plane(bins * 100 + F, (2, bins, F))
    basis = ops.formant_basis_host(bins, order)
    ref, thr = fref.thresholds(M, basis, order, hold, iters, ratio, EPS)
    env, out = run(on_device(M, layout), ratio, order, hold, iters, outputs, off=layout.endswith("off4"))
    ge = None if env is None else env.cpu().numpy()
    go = None if out is None else out.cpu().numpy()
    ok, (re_, ro) = fref.accepted(ge, go, ref, thr)
    print(f"{case}: env r_max {re_:.3f} (seq32 {thr[2]:.3f}, threshold {thr[0]:.3f}); out r_max {ro:.3f} (seq32 {thr[3]:.3f}, threshold {thr[1]:.3f})")
    assert ok, (case, re_, ro, thr)
    if go is not None:
        assert not go[M == 0.0].any() and not np.signbit(go[M == 0.0]).any()           # zeros stay +0.0
        if ratio == 1.0:
            assert np.array_equal(go.view(np.uint32), M.view(np.uint32))                # ratio 1.0 copies
    if ge is not None and F > 2:
        assert not ge[:, :, 2].any()                                                    # the silent frame


def test_outputs_do_not_depend_on_which_are_asked_for_or_on_alignment():
    from phasegen import ops
    M = plane(7, (2, 40, 33))
    Md = torch.from_numpy(M).cuda()
    out, env = ops.formant_shift(Md, R4, 5, 3, 2, EPS, return_env=True)
    assert same_bits(ops.formant_shift(Md, R4, 5, 3, 2, EPS), out) and same_bits(ops.formant_envelope(Md, 5, 3, 2), env)
    o4, e4 = ops.formant_shift(off4(Md), R4, 5, 3, 2, EPS, return_env=True, out=off4(torch.zeros_like(Md)))
    assert same_bits(o4.contiguous(), out) and same_bits(e4, env)
    M36 = plane(8, (2, 40, 36))                                                         # F % 4 == 0: the 16-byte path against the scalar one
    Md = torch.from_numpy(M36).cuda()
    out, env = ops.formant_shift(Md, 0.5, 5, 16, 1, EPS, return_env=True)
    o4, e4 = ops.formant_shift(off4(Md), 0.5, 5, 16, 1, EPS, return_env=True, out=off4(torch.zeros_like(Md)))
    assert same_bits(o4.contiguous(), out) and same_bits(e4, env)


@pytest.mark.parametrize("bins,order,hold", [(40, 5, 3), (1024, 64, 16)])
def test_a_frame_does_not_depend_on_its_position_its_channel_or_the_plane(bins, order, hold):
    from phasegen import ops
    A = plane(21, (2, bins, 33))
    B = plane(22, (3, bins, 70))
    moves = [((0, 5), (2, 40)), ((1, 32), (0, 0)), ((0, 0), (1, 69)), ((1, 17), (1, 31))]     # (channel, frame) of A -> of B
    for (ca, ga), (cb, gb) in moves:
        B[cb, :, gb] = A[ca, :, ga]
    oa, ea = ops.formant_shift(torch.from_numpy(A).cuda(), R4, order, hold, 2, EPS, return_env=True)
    ob, eb = ops.formant_shift(torch.from_numpy(B).cuda(), R4, order, hold, 2, EPS, return_env=True)
    for (ca, ga), (cb, gb) in moves:
        assert same_bits(oa[ca, :, ga], ob[cb, :, gb]) and same_bits(ea[ca, :, ga], eb[cb, :, gb]), ((ca, ga), (cb, gb))
    one = ops.formant_shift(torch.from_numpy(A[1:, :, 17:18].copy()).cuda(), R4, order, hold, 2, EPS)   # the frame alone: n_ch 1, F 1
    assert same_bits(one[0, :, 0], oa[1, :, 17])


def test_a_plane_constant_along_frequency_is_its_own_envelope():
    from phasegen import ops
    for bins, order in ((40, 5), (1024, 64)):
        M = np.broadcast_to(np.float32([0.0, 0.5, 3.0, 80.0, 1e-3])[None, None, :], (2, bins, 5)).copy()
        out, env = ops.formant_shift(torch.from_numpy(M).cuda(), R4, order, 16, 2, EPS, return_env=True)
        env, out = env.cpu().numpy(), out.cpu().numpy()
        assert np.abs(env.astype(np.float64) - M).max() <= 64 * fref.U24 * 80.0 and not env[:, :, 0].any()
        assert np.isfinite(out).all() and np.abs(out.astype(np.float64) - M).max() <= 1e-4 * 80.0


@pytest.mark.parametrize("bins,order,F", [(40, 5, 70), (1024, 64, 33)])
def test_a_bad_cell_stays_in_its_own_frame(bins, order, F):
    from phasegen import ops
    M = plane(31, (2, bins, F))
    clean = ops.formant_shift(torch.from_numpy(M).cuda(), R4, order, 16, 2, EPS, return_env=True)
    c, k, g = 1, 7, 5
    keep = np.ones((2, F), bool)
    keep[c, g] = False
    keep = torch.from_numpy(keep).cuda()
    for bad in (float("nan"), float("inf"), 200.0):
        P = M.copy()
        P[c, k, g] = bad
        got = ops.formant_shift(torch.from_numpy(P).cuda(), R4, order, 16, 2, EPS, return_env=True)
        for a, b in zip(got, clean):
            assert same_bits(a.permute(0, 2, 1)[keep], b.permute(0, 2, 1)[keep]), bad
    again = ops.formant_shift(torch.from_numpy(M).cuda(), R4, order, 16, 2, EPS, return_env=True)
    assert same_bits(again[0], clean[0]) and same_bits(again[1], clean[1])


def test_channel_stride_past_2_to_the_32_bytes():
    """m_ch_rows = 2^24 + 1 rows of 64 frames: channel 1 begins 2^32 + 256 bytes behind channel 0.  The arena of tests/_far.py, a
    quarter of the far-offset module's: every word a sentinel NaN, whatever the call writes must land in the output windows, and the
    far call must give the bits of the call on a dense plane."""
    from phasegen import ops
    b, cls, bins, F = 29, "D", 40, 64
    S = _far.strides(b)[cls]
    assert S * 4 > 1 << 32 and S % F == 0 and S // F == (1 << 24) + 1
    free, _total = torch.cuda.mem_get_info()
    if free < _far.arena_words(b) * 4 + (2 << 30):
        pytest.skip(f"{free / 2**30:.1f} GiB free, {(_far.arena_words(b) * 4 + (2 << 30)) / 2**30:.1f} GiB needed")
    M = torch.from_numpy(plane(41, (2, bins, F)))
    want_out, want_env = ops.formant_shift(M.cuda(), R4, 5, 16, 2, EPS, return_env=True)
    words = torch.empty(_far.arena_words(b), dtype=torch.int32, device="cuda")
    try:
        arena = _far.Arena(words)
        arena.fill()
        L = _far.Lanes(arena, S, far=True)
        Mv = L.view("M", (2, bins, F), data=M)
        assert Mv.stride() == (S, F, 1) and Mv.data_ptr() % 16 == 0
        out = L.dense("out", (2, bins, F), out=True)
        got_out, got_env = ops.formant_shift(Mv, R4, 5, 16, 2, EPS, return_env=True, out=out)
        torch.cuda.synchronize()
        _far.check_rows(arena, L.results(), [want_out.reshape(-1).view(torch.int32)], "formant_shift, channel stride past 2^32 bytes")
        assert same_bits(got_env, want_env) and same_bits(got_out, want_out)
    finally:
        del words
        torch.cuda.empty_cache()


def formant_case():
    import test_z_workspace_gpu as W
    from phasegen import ops
    made = {}

    def run_case(i, o):
        out, env = ops.formant_shift(i["M"], R4, 5, 16, 2, EPS, return_env=True, out=o["out"])
        made["env"] = env
        return [out, env]

    return W.Case("formant_shift", {"M": W.cuda(plane(51, (2, 40, 70)))}, lambda: {"out": W.sent(2, 40, 70)}, run_case,
                  symbol="pg_formant_shift", needs_ws=False)


def test_the_stream_contract():
    """pg_formant_shift on a busy side stream: the same bits, no wait for the device, nothing on another stream, no workspace asked for."""
    import test_z_streams_gpu as S
    from _strict import strict_workspaces
    case = formant_case()
    with strict_workspaces(0xFF) as s:
        got = case.run(case.ins, case.make_outs())
    assert s.requests == [] and "pg_formant_shift" in s.symbols()
    M = case.ins["M"].cpu().numpy()
    from phasegen import ops
    basis = ops.formant_basis_host(40, 5)
    ref, thr = fref.thresholds(M, basis, 5, 16, 2, R4, EPS)
    assert fref.accepted(got[1].cpu().numpy(), got[0].cpu().numpy(), ref, thr)[0]
    S.reach(case)
    assert "pg_formant_shift" in S.REACHED


def test_argument_errors():
    from phasegen import ops
    M = torch.zeros(2, 40, 19, device="cuda")
    for bad in (dict(ratio=0.2), dict(ratio=4.5), dict(ratio=float("nan")), dict(order=0), dict(order=41), dict(order=65), dict(hold=-1),
                dict(hold=65), dict(iters=-1), dict(iters=17), dict(eps=0.0), dict(eps=float("inf")), dict(out=torch.zeros(2, 40, 18, device="cuda"))):
        with pytest.raises(ValueError):
            ops.formant_shift(**{**dict(logmag=M, ratio=1.5, order=5), **bad})
    wide = torch.zeros(2, 81, 19, device="cuda").view(-1)[:2 * 80 * 19 + 19]
    odd = torch.as_strided(wide, (2, 40, 19), (40 * 19 + 7, 19, 1))                    # channels not a whole number of rows apart
    for view in (M[:, :, ::2], M.transpose(1, 2), M.double(), M[0], M.cpu(), odd, torch.zeros(1, 4097, 2, device="cuda")):
        with pytest.raises(ValueError):
            ops.formant_shift(view, 1.5, 5)


# ---- the track ------------------------------------------------------------------------------------------------------------------------
F0, SEMITONES = 180.0, 4.0
SMALL = dict(n_fft=2048, hop_length=512, frames=32, overlap_frames=8)


def test_pitch_shift_keeps_the_formants():
    """2 s of a 180 Hz vowel, up four semitones with the locked vocoder (no weights): the partials of the result against the INPUT's
    true envelope at their new frequencies, with and without formants="keep"."""
    from phasegen import track
    x = fref.vowel_audio(F0, 2.0)
    assert fref.played_error_db(x, F0) < 1.0                                                 # the measure reads the input's own envelope back
    plain = track.pitch_shift(None, x, SEMITONES, phase="vocoder_locked", **SMALL).cpu().numpy()
    kept = track.pitch_shift(None, x, SEMITONES, phase="vocoder_locked", formants="keep", **SMALL).cpu().numpy()
    assert plain.shape == kept.shape == x.shape and np.isfinite(kept).all()
    f0 = F0 * 2.0 ** (SEMITONES / 12.0)
    e_plain, e_kept = fref.played_error_db(plain, f0), fref.played_error_db(kept, f0)
    print(f"pitch_shift(+{SEMITONES:g} st) of a {F0:g} Hz vowel: harmonic-amplitude error {e_plain:.2f} dB without, {e_kept:.2f} dB with formants='keep'")
    assert e_kept < e_plain


def test_formant_semitones_zero_changes_no_bit_and_the_option_reaches_every_path():
    from phasegen import track
    x = np.stack([fref.vowel_audio(F0, 1.0), fref.vowel_audio(260.0, 1.0)])
    kw = dict(phase="vocoder_locked", join="spectral", stretch=1.25, normalize=False, **SMALL)
    base = track.reconstruct_track(None, x, **kw)
    assert same_bits(track.reconstruct_track(None, x, formant_semitones=0.0, **kw), base)
    moved = track.reconstruct_track(None, x, formant_semitones=-4.0, **kw)
    assert moved.shape == base.shape and bool(torch.isfinite(moved).all()) and not same_bits(moved, base)
    both = track.reconstruct_track(None, x, formant_semitones=-4.0, link_channels=True, transients="ola", **kw)
    assert both.shape == base.shape and bool(torch.isfinite(both).all())
    rep = track.evaluate_stretch(None, x, 1.25, phases=("vocoder_locked", "spsi", "zero"), formant_semitones=3.0, **SMALL)
    assert rep["formant_semitones"] == 3.0 and set(rep["metrics"]) == {"vocoder_locked", "spsi", "zero"}
    assert "formant_semitones" not in track.evaluate_stretch(None, x, 1.25, phases=("zero",), **SMALL)


def _reconstruct(args, timeout=180):
    return subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py")] + args, capture_output=True, text=True, timeout=timeout)


def test_reconstruct_flags(tmp_path):
    from scipy.io import wavfile
    wav_in, wav_out = tmp_path / "in.wav", tmp_path / "out.wav"
    wavfile.write(wav_in, 16000, np.round(fref.vowel_audio(F0, 1.0) * 20000).astype(np.int16))
    io = ["--input", str(wav_in), "--output", str(wav_out), "--phase", "vocoder_locked", "--frames", "32", "--overlap_frames", "8"]
    for bad, word in ((["--formants", "keep"], "--formants needs --pitch"),
                      (["--formants", "keep", "--stretch", "1.5"], "--formants needs --pitch"),
                      (["--formants", "drop", "--pitch", "4"], "invalid choice"),
                      (["--formant_shift", "3", "--pitch", "4"], "excludes --pitch"),
                      (["--formant_shift", "3", "--join", "waveform"], "--formant_shift needs --join spectral"),
                      (["--formant_shift", "30"], "within +-24"),
                      (["--pitch", "4", "--formants", "keep", "--join", "waveform"], "need --join spectral")):
        r = _reconstruct(io + bad)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
        assert not wav_out.exists()
    for good in (["--pitch", "4", "--formants", "keep"], ["--formant_shift", "-3", "--join", "spectral"]):
        r = _reconstruct(io + good)
        assert r.returncode == 0, (good, r.stderr[-2000:])
        sr, out = wavfile.read(wav_out)
        assert sr == 16000 and out.dtype == np.float32 and out.shape == (16000,) and np.isfinite(out).all() and float(np.abs(out).max()) == 1.0
        wav_out.unlink()
