"""GPU: pitch curves.  pg_varispeed (ops.varispeed) against the numpy restatement of its contract (tests/_varispeed_ref.py) BIT FOR BIT
on uniform, bent, frozen, backward, jumping and hostile tables, on both of the kernel's paths (window staged in LDS / taps from global
memory); rows, strides and batches; non-finite inputs; its error against the float64 exact-filter variant; and
``track.pitch_shift`` along a ``PitchCurve`` down to the command line.

The error bound.  Per output |y - y64| <= 4 * 2^-24 * sum |w x| + E s sum |x_n| over the output's taps: the first term is the float32
chain (three roundings per weight, one per product, one per addition, the additions growing as sqrt of the tap count at worst -- 4 ulp
of the absolute sum covers them), the second the table: a linear interpolation between samples 1 / L apart is within max |h''| / (8 L^2)
of h, and |h''| <= r (pi r)^2 (the sinc's curvature is a third of that, (pi r)^2 / 3 at the origin; the window's terms 2 sinc' w' + sinc w''
fit into the rest for Z >= 4), so E = r (pi r)^2 / (8 L^2): 1.4e-2 for the tiny filter (L = 8), 2.9e-6 for kaiser_fast (L = 512), beside
the 3.0e-6 the host test measures for kaiser_best on unit sines.  Measured on an MI355X: at most 0.18 of the bound (tiny filter) and
0.056 (kaiser_fast, 5.0e-6).

Shapes: the issue's -- the tiny filter Z = 4, L = 8, beta = 3, r = 0.9 on rows of 300 samples and kaiser_fast on rows of 3000, two rows,
step 1 / 16 / 1024, n_out = tile - 1, tile + 3, 2 tile - 1 and 7 -- and, because a window cut to a row of 3000 samples always fits the
staged path, rows of 20000 samples for the tables that must reach the global path (a jump of 18000 samples).

This module counts as the stream case of pg_varispeed (tests/test_z_streams_gpu.py collects after it)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _nonfinite as NF
import _varispeed_ref as vref
import _vocoder_ref as ref
import _link_ref as kref
from phasegen import detgen
from test_z_lock_gpu import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
NAN, INF = float("nan"), float("inf")
TILE = vref.TILE
N_OUTS = (TILE - 1, TILE + 3, 2 * TILE - 1, 7)
STEPS = (1, 16, 1024)
SENT = -77.0
FILTERS = {"tiny": vref.TINY, "kaiser_fast": (16, 512) + vref.FILTERS["kaiser_fast"][1:]}
N_IN = {"tiny": 300, "kaiser_fast": 3000}
FAR = 20000                                                       # a row in which a jump can outrun the staged window


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def data():
    """every input of the kernel tests, made once and left unchanged: the rows per filter and the two filter tables"""
    from phasegen import ops
    rs = np.random.RandomState(11)
    d = {("x", n): rs.standard_normal((2, n)).astype(np.float32) for n in (300, 3000, FAR)}
    for name, (Z, L, beta, r) in FILTERS.items():
        d["tab", name] = ops.varispeed_table_host(Z, L, beta, r)   # the library's own table, for the kernel and for the restatement
    return d


# ---- tables: (pos of nb + 1 entries, scale of nb entries) ------------------------------------------------------------------

def blocks(n_out, step):
    return -(-n_out // step)


def uniform(nb, step, rate, start=0.0):
    return start + np.arange(nb + 1, dtype=np.float64) * (step * rate), np.full(nb, min(1.0, 1.0 / rate), np.float32)


def _scale_of(pos, step):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(1.0, step / np.abs(np.diff(pos))).astype(np.float32)


def tables(nb, step, n_in):
    """the real tables of the issue, every one inside (or mostly inside) a row of n_in samples"""
    j = np.arange(nb + 1, dtype=np.float64)
    t = {f"uniform {r:.3g}": uniform(nb, step, r) for r in (0.25, 1 / 1.3, 1.0, 2.0, 4.0)}
    jb = nb // 2
    two = np.where(j <= jb, j * 2.0, jb * 2.0 + (j - jb) * 0.5) * step
    t["two slopes"] = (two, _scale_of(two, step))
    rp = (n_in - 1.5) * (j / max(nb, 1)) ** 1.3
    t["ramp"] = (rp, _scale_of(rp, step))
    t["frozen"] = (np.full(nb + 1, 100.25), np.ones(nb, np.float32))
    back = np.where(j <= jb, j, 2 * jb - j + 0.5 * (j - jb)) * step * 0.75 + 7.5          # forwards, then backwards at half the rate
    t["backward"] = (back, _scale_of(back, step))
    return t


def hostile_pos(nb, step):
    pos, scale = uniform(nb, step, 0.75, 3.0)
    for k, v in enumerate((NAN, INF, -INF, -5.0, 1e9, 1e300, 2.0 ** 52 + 2.0, -0.0, 5e-324)):
        pos[(1 + 2 * k) % (nb + 1)] = v
    return pos, scale


def hostile_scale(nb, step):
    pos, scale = uniform(nb, step, 0.75, 3.0)
    for k, v in enumerate((NAN, 0.0, 1e-9, 2.0, -1.0, INF, -INF, 0.2499999, 1e-45)):
        scale[(2 * k) % nb] = v
    return pos, scale


def run(x, pos, scale, n_out, step, filt, tab, pad_in=5, pad_out=3):
    """ops.varispeed on rows with NaN in their stride padding, into rows with a sentinel in theirs -> the result (numpy); asserts
    that the output padding is as it was"""
    from phasegen import ops
    Z, L = FILTERS[filt][:2]
    n_sig, n_in = x.shape
    xb = torch.full((n_sig, n_in + pad_in), NAN, device="cuda")
    xb[:, :n_in] = dev(x)
    yb = torch.full((n_sig, n_out + pad_out), SENT, device="cuda")
    got = ops.varispeed(xb[:, :n_in], dev(pos), dev(scale), n_out, step=step, table=(dev(tab), Z, L), out=yb[:, :n_out])
    assert got.data_ptr() == yb.data_ptr()
    assert bool((yb[:, n_out:] == SENT).all()), "output padding was written"
    return yb[:, :n_out].cpu().numpy()


def want(x, pos, scale, n_out, step, filt, tab, **kw):
    Z, L = FILTERS[filt][:2]
    return vref.varispeed(x, pos, scale, n_out, step, Z, L, tab, **kw)


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---- the kernel against the restatement, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("filt", list(FILTERS))
def test_every_table_has_the_bits_of_the_restatement(data, filt, step):
    n_in = N_IN[filt]
    x, tab = data["x", n_in], data["tab", filt]
    for n_out in N_OUTS:
        nb = blocks(n_out, step)
        cases = tables(nb, step, n_in)
        cases["hostile pos"], cases["hostile scale"] = hostile_pos(nb, step), hostile_scale(nb, step)
        for name, (pos, scale) in cases.items():
            got = run(x, pos, scale, n_out, step, filt, tab)
            assert bits_equal(got, want(x, pos, scale, n_out, step, filt, tab)), (filt, step, n_out, name)
            assert np.isfinite(got).all(), (filt, step, n_out, name)


@pytest.mark.parametrize("step", STEPS)
def test_a_jump_longer_than_the_window_takes_the_global_path_with_the_same_bits(data, step):
    """rows of 20000 samples, kaiser_fast: a table whose second tile jumps 18000 samples (global path) between staged tiles -- both
    paths in one launch -- and the same table without the jump: the tiles the jump does not touch keep their bits"""
    filt = "kaiser_fast"
    Z = FILTERS[filt][0]
    x, tab = data["x", FAR], data["tab", filt]
    n_out = 3 * TILE + 3
    nb = blocks(n_out, step)
    calm, scale = uniform(nb, step, 1.25, 40.0)
    jump = calm.copy()
    per_tile = max(TILE // step, 1)
    k = per_tile + max(per_tile // 2, 1)                          # a block end inside tile 1 (step 1024: the end tiles 1 and 2 share)
    jump[k] = 19000.5
    staged = vref.staged_tiles(jump, n_out, step, FAR, Z)
    assert vref.staged_tiles(calm, n_out, step, FAR, Z).all() and staged[0] and not staged[1] and staged[-1], staged
    got_calm, got_jump = run(x, calm, scale, n_out, step, filt, tab), run(x, jump, scale, n_out, step, filt, tab)
    assert bits_equal(got_calm, want(x, calm, scale, n_out, step, filt, tab))
    assert bits_equal(got_jump, want(x, jump, scale, n_out, step, filt, tab))
    touched = np.zeros(n_out, bool)
    touched[max(k - 1, 0) * step:(k + 1) * step] = True            # the two blocks that end or begin at the moved entry
    assert bits_equal(got_calm[:, ~touched], got_jump[:, ~touched]) and not bits_equal(got_calm[:, touched], got_jump[:, touched])
    # hostile tables in the long row: 1e300, inf and NaN next to ordinary entries span the whole row
    for pos, sc in (hostile_pos(nb, step), hostile_scale(nb, step)):
        assert bits_equal(run(x, pos, sc, n_out, step, filt, tab), want(x, pos, sc, n_out, step, filt, tab))
    assert not vref.staged_tiles(hostile_pos(nb, step)[0], n_out, step, FAR, Z).all()


# ---- rows, strides, batches --------------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_their_company_or_their_layout(data):
    from phasegen import ops
    filt, step, n_out = "kaiser_fast", 16, TILE + 3
    Z, L = FILTERS[filt][:2]
    x, tab = data["x", 3000], data["tab", filt]
    pos, scale = tables(blocks(n_out, step), step, 3000)["ramp"]
    both = run(x, pos, scale, n_out, step, filt, tab)                                        # (padded rows, NaN in the padding)
    dpos, dscale, dtab = dev(pos), dev(scale), (dev(tab), Z, L)
    alone = ops.varispeed(dev(x[1]), dpos, dscale, n_out, step=step, table=dtab)             # 1-D in, 1-D out
    assert tuple(alone.shape) == (n_out,) and bits_equal(alone.cpu().numpy(), both[1])
    three = ops.varispeed(dev(np.stack([x[1], x[0], x[1]])), dpos, dscale, n_out, step=step, table=dtab).cpu().numpy()
    assert bits_equal(three[0], both[1]) and bits_equal(three[1], both[0]) and bits_equal(three[2], both[1])
    wide = dev(np.concatenate([x, x[::-1]], axis=1))                                          # a strided view: every second row of a wider tensor
    view = wide.view(4, 3000)[::2]
    assert not view.is_contiguous()
    assert bits_equal(ops.varispeed(view, dpos, dscale, n_out, step=step, table=dtab).cpu().numpy(), both)
    # the cached table of a res_type is the explicit one
    assert bits_equal(ops.varispeed(dev(x), dpos, dscale, n_out, step=step, res_type="kaiser_fast").cpu().numpy(), both)


def test_argument_errors(data):
    from phasegen import ops
    x = dev(data["x", 300])
    pos, scale = (dev(v) for v in uniform(4, 16, 1.0))
    ops.varispeed(x, pos, scale, 64, step=16)
    for kw, word in ((dict(step=48), "power of two"), (dict(step=8192), "power of two"), (dict(per_zero=100), "per_zero"), (dict(res_type="sinc"), "res_type"),
                     (dict(table=(pos, 4, 8)), "table must be a float32"), (dict(table=(x, 4, 8)), "table must be a float32"), (dict(table=3), "table must be"),
                     (dict(out=torch.empty(2, 63, device="cuda")), "out must be")):
        with pytest.raises(ValueError, match="varispeed: .*" + word):
            ops.varispeed(x, pos, scale, 64, **{"step": 16, **kw})
    for bad_pos, bad_scale, word in ((pos[:-1], scale, "pos must hold 5"), (pos.float(), scale, "pos must be a 1-D float64"), (pos, scale[:-1], "scale must hold 4"),
                                     (pos, scale.double(), "scale must be a 1-D float32"), (pos.cpu(), scale, "pos must be")):
        with pytest.raises(ValueError, match="varispeed: " + word):
            ops.varispeed(x, bad_pos, bad_scale, 64, step=16)
    with pytest.raises(ValueError, match="contiguous"):
        ops.varispeed(x[:, ::2], pos, scale, 64, step=16)
    with pytest.raises(ValueError, match="n_out"):
        ops.varispeed(x, pos, scale, 0, step=16)


# ---- non-finite inputs -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", list(FILTERS))
def test_a_nan_and_an_inf_reach_exactly_the_outputs_whose_support_holds_them(data, filt):
    n_in, step, n_out = N_IN[filt], 16, TILE + 3
    x, tab = data["x", n_in], data["tab", filt]
    pos, scale = tables(blocks(n_out, step), step, n_in)["two slopes"]
    clean, ref_clean = run(x, pos, scale, n_out, step, filt, tab), want(x, pos, scale, n_out, step, filt, tab)
    for value, where in ((NAN, (0, n_in // 10)), (INF, (1, n_in // 8)), (-INF, (1, 0)), (NAN, (0, min(n_in - 1, 1200)))):   # (the table reads 0 .. 1288)
        xp = x.copy()
        xp[where] = value
        got, (ref_p, support) = run(xp, pos, scale, n_out, step, filt, tab), want(xp, pos, scale, n_out, step, filt, tab, return_support=True)
        n = NF.check(got, clean, ref_p, ref_clean, tag=f"varispeed {filt} {value} at {where}")
        hit = support[:, where[1]]
        cone = ~np.isfinite(ref_p)
        assert hit.any() and not hit.all() and n["cone"] >= 1
        assert not cone[1 - where[0]].any() and (cone[where[0]] <= hit).all()             # only the poisoned row, only inside the support
        assert bits_equal(got, ref_p)


# ---- the error against the exact filter ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", list(FILTERS))
def test_error_against_the_float64_exact_filter(data, filt):
    Z, L, beta, r = FILTERS[filt]
    n_in, step, n_out = N_IN[filt], 16, TILE + 3
    x, tab = data["x", n_in], data["tab", filt]
    E = r * (np.pi * r) ** 2 / (8 * L * L)
    worst = 0.0
    for name in ("uniform 0.769", "uniform 4", "ramp", "backward"):
        pos, scale = tables(blocks(n_out, step), step, n_in)[name]
        got = run(x, pos, scale, n_out, step, filt, tab).astype(np.float64)
        y64, mag = vref.varispeed_exact(x, pos, scale, n_out, step, Z, L, beta, r)
        _y, support = want(x[0], pos, scale, n_out, step, filt, tab, return_support=True)
        _p, s = vref.positions(pos, scale, n_out, step)
        absx = s.astype(np.float64)[None] * (support.astype(np.float64) @ np.abs(x.astype(np.float64)).T).T     # s sum |x_n| over the taps
        bound = 4 * 2.0 ** -24 * mag + E * absx
        ratio = float((np.abs(got - y64) / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print(f"{filt} {name}: max |y - y64| = {float(np.abs(got - y64).max()):.2e}, at most {ratio:.3f} of the bound (table term E = {E:.2e})")
        assert (np.abs(got - y64) <= bound).all(), (filt, name, ratio)


# ---- workspace-free, on the stream passed in ------------------------------------------------------------------------------------

def test_runs_on_the_stream_passed_in_and_writes_nothing_else(data):
    """pg_varispeed has no workspace (tests/test_z_workspace_gpu.py's helper: the guards of none, the same bits) and runs on the
    stream it is given without waiting (tests/test_z_streams_gpu.py)"""
    import test_z_streams_gpu as S
    import test_z_workspace_gpu as W
    from phasegen import _lib, ops
    assert "workspace" not in dict(_lib.VarispeedArgs._fields_)
    n_out, step = TILE + 3, 16
    pos, scale = tables(blocks(n_out, step), step, 3000)["ramp"]
    case = W.Case("varispeed", {"x": W.cuda(data["x", 3000]), "pos": W.cuda(pos), "scale": W.cuda(scale)}, lambda: {"y": W.sent(2, n_out)},
                  lambda i, o: [ops.varispeed(i["x"], i["pos"], i["scale"], n_out, step=step, res_type="kaiser_fast", out=o["y"])],
                  symbol="pg_varispeed", needs_ws=False)
    W.check(case)
    S.reach(case)
    assert "pg_varispeed" in S.REACHED


# ---- track level ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def melody():
    return ref.melody(seconds=1.0)


@pytest.fixture(scope="module")
def stereo():
    return kref.stereo_melody(seconds=1.0)


CURVE = [(0, -3), (0.4, 5), (0.7, 5), (1.0, -12)]


@pytest.mark.parametrize("phase", ["zero", "vocoder_locked", "spsi"])
def test_pitch_shift_along_a_curve_is_the_chain_written_out(melody, phase):
    from phasegen import ops, track
    curve = track.PitchCurve(CURVE)
    out = track.pitch_shift(None, melody, curve, phase=phase, normalize=False, **SMALL)
    assert tuple(out.shape) == melody.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    pl = curve.plan(melody.shape[0])
    mid = track.reconstruct_track(None, melody, phase=phase, join="spectral", stretch=pl.time_map, normalize=False, **SMALL)
    assert tuple(mid.shape) == (int(round(pl.time_map.out_of_src(melody.shape[0]))),)
    hand = ops.varispeed(mid, dev(pl.pos), dev(pl.scale), melody.shape[0], step=pl.step)
    assert same_bits(out, hand)
    assert bits_equal(hand.cpu().numpy(), vref.varispeed(mid.cpu().numpy(), pl.pos, pl.scale, melody.shape[0], pl.step, 64, 512,
                                                         ops.varispeed_table_host(64, 512, *vref.FILTERS["kaiser_best"][1:])))
    normal = track.pitch_shift(None, melody, curve, phase=phase, **SMALL)
    assert float(normal.abs().max()) == 1.0 and same_bits(normal, track.peak_normalize(out))


def test_stereo_linked_with_transients_and_the_refusals(melody, stereo):
    from phasegen import track
    curve = track.PitchCurve(CURVE)
    plain = track.pitch_shift(None, stereo, curve, phase="vocoder_locked", **SMALL)
    linked = track.pitch_shift(None, stereo, curve, phase="vocoder_locked", link_channels=True, transients="ola", **SMALL)
    assert tuple(plain.shape) == tuple(linked.shape) == stereo.shape and bool(torch.isfinite(linked).all())
    assert not same_bits(plain, linked)
    with pytest.raises(ValueError, match="formants='keep' is not available with a PitchCurve"):
        track.pitch_shift(None, melody, curve, phase="zero", formants="keep", **SMALL)
    with pytest.raises(ValueError, match="TimeMap"):
        track.pitch_shift(None, melody, track.TimeMap([(0, 0), (1, 1.5)]), phase="zero", **SMALL)


def _peak_hz(frame, sr=16000):
    return float(np.argmax(np.abs(np.fft.rfft(frame)))) * sr / len(frame)


def test_pitch_at_the_real_framing():
    """2048 / 512, one second of a 440 Hz sine, the locked vocoder.  A constant +7 curve lands within one 1 Hz bin of the uniform
    pitch_shift(7) on the same input (the parent's path: pg_resample at pitch_ratio's fraction, at most 0.85 cent off); a glide from 0
    to +12 over the second has, in a Hann-windowed frame of 2048 samples around 0.25 s and around 0.75 s, its peak between the lowest
    and the highest frequency the curve takes inside the frame, widened by one 7.8 Hz bin on either side"""
    from phasegen import track
    sr, n = 16000, 16000
    x = np.sin(2 * np.pi * 440.0 * np.arange(n) / sr).astype(np.float32) * 0.5
    uni = track.pitch_shift(None, x, 7, phase="vocoder_locked").cpu().numpy()
    const = track.pitch_shift(None, x, track.PitchCurve([(0, 7), (1, 7)]), phase="vocoder_locked").cpu().numpy()
    assert const.shape == uni.shape == (n,)
    f_uni, f_const = _peak_hz(uni), _peak_hz(const)
    print(f"constant +7: the curve's peak at {f_const:.0f} Hz, the uniform shift's at {f_uni:.0f} Hz (440 * 2^(7/12) = {440 * 2 ** (7 / 12):.1f})")
    assert abs(f_const - f_uni) <= 1.0
    glide = track.pitch_shift(None, x, track.PitchCurve([(0, 0), (1, 12)]), phase="vocoder_locked").cpu().numpy()
    assert glide.shape == (n,) and np.isfinite(glide).all()
    win = np.hanning(2048)
    for centre in (0.25, 0.75):
        c = int(centre * sr)
        f = _peak_hz(glide[c - 1024:c + 1024] * win)
        lo, hi = (440.0 * 2 ** (12 * (c + d) / sr / 12) for d in (-1024, 1024))
        print(f"glide: the frame around {centre} s peaks at {f:.1f} Hz; the curve runs from {lo:.1f} to {hi:.1f} Hz inside it")
        assert lo - sr / 2048 <= f <= hi + sr / 2048, (centre, f, lo, hi)


# ---- command line -----------------------------------------------------------------------------------------------------------------

def _cli(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--channels", "16", "--hop", "8",
                           "--frames", "24", "--overlap_frames", "4", *map(str, flags)], capture_output=True, text=True, timeout=300)


def test_reconstruct_cli_with_a_pitch_curve(tmp_path):
    from scipy.io import wavfile
    wav, out, curve, tmap = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "curve.txt", tmp_path / "map.txt"
    wavfile.write(str(wav), 16000, detgen.normal(98, (4000,)).astype(np.float32) * 0.1)
    curve.write_text("# seconds semitones\n0 0\n0.1 3.5   # up\n0.25, -2\n")
    tmap.write_text("0 0\n1 1.5\n")
    r = _cli("--input", wav, "--output", out, "--phase", "vocoder_locked", "--pitch_curve", curve, "--transients", "ola")      # no --weight
    assert r.returncode == 0, r.stderr[-2000:]
    sr, y = wavfile.read(str(out))
    assert sr == 16000 and y.shape == (4000,) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    rep = tmp_path / "rep.json"
    for flags, name in ((("--pitch", "3"), "--pitch"), (("--stretch", "1.5"), "--stretch"), (("--tempo_map", tmap), "--tempo_map"),
                        (("--formants", "keep"), "--formants"), (("--formant_shift", "2"), "--formant_shift"), (("--report", rep), "--report"),
                        (("--stretch_report", rep), "--stretch_report")):
        r = _cli("--input", wav, "--output", out, "--phase", "vocoder", "--pitch_curve", curve, *flags)
        assert r.returncode == 2 and "--pitch_curve" in r.stderr and name in r.stderr, (flags, r.stderr[-500:])
    r = _cli("--input", wav, "--output", out, "--phase", "vocoder", "--pitch", "3", "--tempo_map", tmap)
    assert r.returncode == 2 and "--tempo_map is a stretch of its own" in r.stderr
