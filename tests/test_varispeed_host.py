"""CPU: the host half of pitch curves -- pg_varispeed's symbols, struct layout and error table in its order (validation runs before
any launch), pg_varispeed_table against float64 numpy, phasegen.track.PitchCurve with its plan, and the accuracy of the contract
itself, measured on its numpy restatement (tests/_varispeed_ref.py) alone.

Accuracy.  Unit sines at f = 0.01, 0.2 and 0.4 cycles per sample times the smallest block scale, read at constant rates 0.25 .. 4 and
along a ramp 0.5 -> 2 (n_in 6000, step 64, kaiser_best, L = 512): |y - sin(2 pi f p_t)| <= 1e-5.  What the bound is made of: the
exact filter reproduces the sine within 6.5e-8; the table's linear interpolation between 512 samples per zero crossing adds up to
3.0e-6 (measured on the restatement, printed below: the maximum over all cases is 3.03e-6, at rate 0.9 and f = 0.4); the bound is
three times the 3.1e-6 of the first prototype.  kaiser_fast (transition band from 0.425) is measured up to f = 0.3 against its own
stop band: see test_kaiser_fast_is_held_to_its_own_stop_band."""
import ctypes
import os
import re

import numpy as np
import pytest

import _varispeed_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pg_varispeed_table_elems", "pg_varispeed_table", "pg_varispeed")
NULL, SHAPE, ALIGN, UNSUPPORTED = -1, -2, -3, -4


def _header_fields(struct):
    h = open(os.path.join(ROOT, "include", "phasegen.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.findall(r"(\w+)\s*$", first)[0])
            names.extend(m.strip() for m in more)
    return names


# ---- the C entry points --------------------------------------------------------------------------------------------------

def test_symbols_and_struct_layout():
    from phasegen import _lib
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.SYMBOLS["pg_varispeed_table_elems"][0] is ctypes.c_int64
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4
    V = _lib.VarispeedArgs
    assert ctypes.sizeof(V) == 72
    h = open(os.path.join(ROOT, "include", "phasegen.h")).read()
    assert re.search(r"\}\s*pg_varispeed_args;\s*/\*\s*72 bytes\s*\*/", h)
    assert [f[0] for f in V._fields_] == _header_fields("pg_varispeed_args")
    assert not any(t in (ctypes.c_int64, ctypes.c_double) for _, t in V._fields_)   # int32 sizes, no rate: the tables are the grid
    assert "workspace" not in dict(V._fields_)
    assert (V.step.offset, V.zeros.offset, V.per_zero.offset, V.x_stride.offset, V.y_stride.offset) == (12, 16, 20, 24, 28)
    assert (V.pos.offset, V.scale.offset, V.table.offset, V.x.offset, V.y.offset) == (32, 40, 48, 56, 64)


def _good(_lib):
    a = _lib.VarispeedArgs()
    a.n_sig, a.n_in, a.n_out, a.step, a.zeros, a.per_zero, a.x_stride, a.y_stride = 2, 300, 100, 16, 4, 8, 300, 100
    a.pos = a.scale = a.table = a.x = a.y = 4096                  # never dereferenced: every case below fails before the launch
    return a


def test_argument_errors_are_reported_before_any_launch_and_in_order():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_varispeed(None, None) == NULL
    # (what is broken, expected code), in the documented order: each case also carries every fault that comes LATER in the order
    later = [({"pos": 4100}, ALIGN), ({"x": 0}, NULL), ({"y_stride": 99}, SHAPE), ({"per_zero": 12}, UNSUPPORTED), ({"n_out": 0}, SHAPE)]
    for k in range(len(later)):
        a = _good(_lib)
        for fields, _code in later[:k + 1]:
            for f, v in fields.items():
                setattr(a, f, v)
        assert lib.pg_varispeed(ctypes.byref(a), None) == later[k][1], later[k]
        assert lib.pg_last_error_string().startswith(b"varispeed: ")
    singles = [({"n_sig": 0}, SHAPE), ({"n_in": -1}, SHAPE), ({"step": 0}, UNSUPPORTED), ({"step": 48}, UNSUPPORTED), ({"step": 8192}, UNSUPPORTED),
               ({"zeros": 0}, UNSUPPORTED), ({"zeros": 65}, UNSUPPORTED), ({"per_zero": 0}, UNSUPPORTED), ({"per_zero": 1024}, UNSUPPORTED),
               ({"x_stride": 299}, SHAPE), ({"pos": 0}, NULL), ({"scale": 0}, NULL), ({"table": 0}, NULL), ({"y": 0}, NULL),
               ({"table": 4100}, ALIGN)]
    for fields, code in singles:
        a = _good(_lib)
        for f, v in fields.items():
            setattr(a, f, v)
        assert lib.pg_varispeed(ctypes.byref(a), None) == code, fields
    for step in (1, 4096):
        a = _good(_lib)
        a.step, a.pos = step, 4100                                # the limits themselves pass on to the next row
        assert lib.pg_varispeed(ctypes.byref(a), None) == ALIGN
    assert lib.pg_varispeed_table_elems(0, 8) == UNSUPPORTED and lib.pg_varispeed_table_elems(4, 6) == UNSUPPORTED
    assert lib.pg_varispeed_table_elems(65, 8) == UNSUPPORTED and lib.pg_varispeed_table_elems(4, 1024) == UNSUPPORTED
    buf = np.empty(2 * 33, np.float32)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.pg_varispeed_table(None, 4, 8, 3.0, 0.9) == NULL
    assert lib.pg_varispeed_table(ptr, 4, 3, 3.0, 0.9) == UNSUPPORTED
    for beta, r in ((float("nan"), 0.9), (-1.0, 0.9), (16.0, 0.9), (3.0, 0.0), (3.0, 1.5), (3.0, float("nan"))):
        assert lib.pg_varispeed_table(ptr, 4, 8, beta, r) == SHAPE, (beta, r)


@pytest.mark.parametrize("Z,L,beta,r", [vref.TINY, (1, 1, 0.0, 1.0), (16, 512) + vref.FILTERS["kaiser_fast"][1:], (64, 512) + vref.FILTERS["kaiser_best"][1:],
                                        (64, 64) + vref.FILTERS["kaiser_best"][1:]])
def test_table_is_the_double_formula_rounded_once(Z, L, beta, r):
    from phasegen import _lib, ops
    tab = ops.varispeed_table_host(Z, L, beta, r)
    assert tab.shape == (Z * L + 1, 2) and tab.dtype == np.float32
    assert _lib.load().pg_varispeed_table_elems(Z, L) == 2 * (Z * L + 1) == tab.size
    h64 = vref.h_exact(np.arange(Z * L + 1, dtype=np.float64) / L, Z, beta, r)
    want = h64.astype(np.float32)
    # within one float32 ulp of numpy's float64 value: libm and numpy may differ in the last bit of sin and of I0
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(tab[:, 0].astype(np.float64) - want.astype(np.float64))
    print(f"Z {Z} L {L}: {int((err > 0).sum())} of {want.size} entries differ from numpy's, the largest by {float((err / ulp).max()):.2f} ulp")
    assert (err <= ulp).all()
    assert tab[0, 0] == np.float32(r)
    d = tab[1:, 0] - tab[:-1, 0]                                  # float32 arithmetic on the table's OWN values
    assert np.array_equal(tab[:-1, 1].view(np.int32), d.view(np.int32))
    assert tab[-1, 1] == 0.0 and not np.signbit(tab[-1, 1])


def test_python_wrapper_checks_its_arguments_without_a_gpu():
    import inspect
    from phasegen import ops
    sig = inspect.signature(ops.varispeed)
    assert list(sig.parameters) == ["x", "pos", "scale", "n_out", "step", "res_type", "per_zero", "table", "out"]
    assert (sig.parameters["step"].default, sig.parameters["res_type"].default, sig.parameters["per_zero"].default) == (64, "kaiser_best", 512)
    assert ops.varispeed_blocks(1, 64) == 1 and ops.varispeed_blocks(64, 64) == 1 and ops.varispeed_blocks(65, 64) == 2
    import torch
    with pytest.raises(ValueError, match="varispeed: expected a 1-D or 2-D float32 device tensor"):
        ops.varispeed(torch.zeros(10), torch.zeros(2, dtype=torch.float64), torch.zeros(1), 10)
    with pytest.raises(RuntimeError, match="zeros"):
        ops.varispeed_table_host(0, 8, 3.0, 0.9)


# ---- PitchCurve ----------------------------------------------------------------------------------------------------------

def test_every_rejection():
    from phasegen import track
    P = track.PitchCurve
    nan, inf = float("nan"), float("inf")
    for bad, word in (([(0, 0)], "at least two"), ([], "at least two"), ([(0, 0, 0), (1, 0, 0)], "at least two"), ([(0, 0), (1, nan)], "finite"),
                      ([(0, 0), (inf, 1)], "finite"), ([(0.5, 0), (1, 0)], "first anchor"), ([(0, 0), (1, 0), (1, 2)], "increase strictly"),
                      ([(0, 0), (2, 0), (1, 2)], "increase strictly"), ([(0, 0), (1, 24.5)], r"within \[-24, 24\]"), ([(0, -25), (1, 0)], r"within \[-24, 24\]"),
                      ([(0, "a"), (1, 0)], "pairs"), (7, "pairs")):
        with pytest.raises(ValueError, match="PitchCurve: .*" + word):
            P(bad)
    c = P([(0, 0), (1, 12)])
    for kw, word in ((dict(a_len=0), "positive"), (dict(a_len=100, sr=0), "positive"), (dict(a_len=100, step=48), "power of two"),
                     (dict(a_len=100, step=8192), "power of two"), (dict(a_len=100, step=64, segment=96), "multiple of step"),
                     (dict(a_len=100, step=64, segment=32), "multiple of step")):
        with pytest.raises(ValueError, match="PitchCurve.plan: .*" + word):
            c.plan(**kw)
    for args in ((0.0, 1, 5), (1.0, 25, 5), (1.0, 1, 0.0), (1.0, 1, inf), (1.0, 1, 5, 3)):
        with pytest.raises(ValueError, match="PitchCurve.vibrato"):
            P.vibrato(*args)


def test_curve_is_piecewise_linear_and_constant_past_its_end():
    from phasegen import track
    c = track.PitchCurve([(0, -2), (1, 2), (3, 12)])
    assert c.anchors == [(0.0, -2.0), (1.0, 2.0), (3.0, 12.0)] and "PitchCurve" in repr(c)
    assert c.semitones_at(0) == -2 and c.semitones_at(0.5) == 0 and c.semitones_at(1) == 2 and c.semitones_at(2) == 7
    assert c.semitones_at(3) == 12 and c.semitones_at(1e6) == 12
    assert np.array_equal(c.semitones_at(np.array([0.25, 2.5])), [-1.0, 9.5])
    with pytest.raises(ValueError):
        c.seconds[0] = 1.0                                        # read-only


def test_load_round_trips(tmp_path):
    from phasegen import track
    c = track.PitchCurve([(0, 0.1), (1 / 3, -7.3), (2.5, 24)])
    c.save(str(tmp_path / "c.txt"))
    d = track.PitchCurve.load(str(tmp_path / "c.txt"))
    assert np.array_equal(c.seconds, d.seconds) and np.array_equal(c.semitones, d.semitones)
    (tmp_path / "h.txt").write_text("# a glide\n0, 0\n\n1.5  12   # an octave\n")
    assert track.PitchCurve.load(str(tmp_path / "h.txt")).anchors == [(0.0, 0.0), (1.5, 12.0)]
    for text, word in (("0 0 0\n1 1\n", "expected two columns"), ("0 0\n1 x\n", "not two numbers")):
        (tmp_path / "bad.txt").write_text(text)
        with pytest.raises(ValueError, match="PitchCurve.load: .*" + word):
            track.PitchCurve.load(str(tmp_path / "bad.txt"))


def test_vibrato():
    from phasegen import track
    v = track.PitchCurve.vibrato(2.0, 0.5, 5.0)
    assert len(v.seconds) == 2 * 5 * 16 + 1 and v.seconds[-1] >= 2.0
    assert np.allclose(np.diff(v.seconds), 1 / 80, rtol=1e-12, atol=0)
    assert np.allclose(v.semitones, 0.5 * np.sin(2 * np.pi * 5.0 * v.seconds), atol=1e-12)
    assert abs(v.semitones).max() == pytest.approx(0.5) and v.semitones_at(0.05) == pytest.approx(0.5)   # a quarter cycle in
    assert len(track.PitchCurve.vibrato(1.0, 1.0, 4.0, per_cycle=8).seconds) == 33


@pytest.mark.parametrize("a_len", [1, 64, 300, 16000, 16000 * 180 + 77])
def test_plan_properties(a_len):
    from phasegen import track
    step = 64
    nb = -(-a_len // step)
    idx = np.arange(nb + 1, dtype=np.float64)
    flat = track.PitchCurve([(0, 0), (1, 0)]).plan(a_len)
    assert isinstance(flat, track.CurvePlan) and flat._fields == ("time_map", "pos", "scale", "step") and flat.step == step
    assert flat.pos.dtype == np.float64 and flat.scale.dtype == np.float32 and flat.pos.shape == (nb + 1,) and flat.scale.shape == (nb,)
    assert np.array_equal(flat.pos, idx * step) and (flat.scale == 1.0).all()
    up = track.PitchCurve([(0, 12), (1, 12)]).plan(a_len)
    assert np.array_equal(up.pos, 2.0 * idx * step) and (up.scale == 0.5).all()
    down = track.PitchCurve([(0, -12), (1, -12)]).plan(a_len)
    assert np.array_equal(down.pos, 0.5 * idx * step) and (down.scale == 1.0).all()
    for st in (24, -24):
        pl = track.PitchCurve([(0, st), (1, st)]).plan(a_len)
        s = pl.time_map.stretches
        assert (s >= 0.25).all() and (s <= 4.0).all()
        assert (pl.scale == (0.25 if st > 0 else 1.0)).all()
    # a real curve: pos is the tempo map's image of the block ends, exactly; every block lies inside one segment of the map
    curve = track.PitchCurve([(0, -24), (a_len / 32000, 24), (a_len / 16000, -5)])
    for kw in (dict(), dict(step=16, segment=64), dict(step=256, segment=256), dict(sr=44100)):
        pl = curve.plan(a_len, **kw)
        st, sr = pl.step, kw.get("sr", 16000)
        n = -(-a_len // st)
        assert np.array_equal(pl.pos, pl.time_map.out_of_src(np.arange(n + 1, dtype=np.float64) * st, sr))
        assert np.array_equal(pl.scale, np.minimum(1.0, st / np.diff(pl.pos)).astype(np.float32))
        s = pl.time_map.stretches
        assert (s >= 0.25).all() and (s <= 4.0).all() and (np.diff(pl.pos) > 0).all()
        seg = kw.get("segment", 256)
        assert np.allclose(pl.time_map.src * sr, np.arange(len(pl.time_map.src)) * seg, rtol=1e-15, atol=0)
        mid = (np.arange(len(s)) + 0.5) * seg / sr
        assert np.allclose(s, 2.0 ** (curve.semitones_at(mid) / 12.0), rtol=1e-9)


def test_pitch_shift_surface_and_refusals():
    import inspect
    from phasegen import track
    names = list(inspect.signature(track.pitch_shift).parameters)
    assert names[:3] == ["model", "audio", "semitones"] and names[-3:] == ["link_channels", "transients", "formants"]
    x = np.zeros(4000, np.float32)
    curve = track.PitchCurve([(0, 0), (1, 12)])
    with pytest.raises(ValueError, match="formants='keep' is not available with a PitchCurve"):
        track.pitch_shift(None, x, curve, phase="zero", formants="keep")
    with pytest.raises(ValueError, match="TimeMap.*PitchCurve"):
        track.pitch_shift(None, x, track.TimeMap([(0, 0), (1, 1.5)]), phase="zero")
    with pytest.raises(ValueError, match="link_channels needs"):
        track.pitch_shift(None, x, curve, phase="zero", link_channels=True)
    with pytest.raises(ValueError, match="transients must be"):
        track.pitch_shift(None, x, curve, phase="zero", transients="wsola")


# ---- the accuracy of the contract, on the restatement alone --------------------------------------------------------------

N_IN, STEP = 6000, 64
RATES = (0.25, 0.5, 0.9, 1.0, 1.3, 2.0, 4.0, "ramp")
WORST = {}


def _tables(rate):
    if rate == "ramp":
        n_out = 3000
        nb = -(-n_out // STEP)
        rates = np.linspace(0.5, 2.0, nb)
        pos = np.concatenate([[100.0], 100.0 + np.cumsum(rates * STEP)])
    else:
        n_out = int(min(3000, (N_IN - 600) / rate))
        nb = -(-n_out // STEP)
        rates = np.full(nb, rate)
        pos = 300.0 + np.arange(nb + 1) * STEP * rate
    return n_out, pos, np.minimum(1.0, 1.0 / rates).astype(np.float32)


@pytest.mark.parametrize("rate", RATES)
def test_a_sine_comes_back_at_its_place(rate):
    Z, beta, r = vref.FILTERS["kaiser_best"]
    L = 512
    tab = vref.table(Z, L, beta, r)
    n_out, pos, scale = _tables(rate)
    for f in (0.01, 0.2, 0.4):
        ff = f * float(scale.min())
        x = np.sin(2 * np.pi * ff * np.arange(N_IN)).astype(np.float32)
        y = vref.varispeed(x, pos, scale, n_out, STEP, Z, L, tab)
        p, _s = vref.positions(pos, scale, n_out, STEP)
        err = float(np.abs(y.astype(np.float64) - np.sin(2 * np.pi * ff * p)).max())
        WORST["best"] = max(WORST.get("best", 0.0), err)
        print(f"kaiser_best rate {rate} f {f}: max |y - sin| = {err:.2e} (largest so far {WORST['best']:.2e})")
        assert err <= 1e-5, (rate, f, err)


@pytest.mark.parametrize("rate", RATES)
def test_kaiser_fast_is_held_to_its_own_stop_band(rate):
    """kaiser_fast up to f = 0.3 (its transition band begins at 0.425).  The EXACT filter is 5.5e-6 .. 5.4e-5 off the sine here
    (measured: 5.4e-5 at the worst, the table chain 1.7e-6 off the exact filter), so the 1e-5 of kaiser_best cannot hold against the sine; that is the window, not the table:
    Kaiser's formula gives beta = 8.5555 a stop band of 8.7 + beta / 0.1102 = 86.3 dB = 4.8e-5 per image.  Held instead: the table
    chain within 1e-5 of the exact filter (the table's term, the same bound as above), and the exact filter within twice the
    stop-band figure, 1e-4, of the sine."""
    Z, beta, r = vref.FILTERS["kaiser_fast"]
    L = 512
    tab = vref.table(Z, L, beta, r)
    n_out, pos, scale = _tables(rate)
    for f in (0.01, 0.2, 0.3):
        ff = f * float(scale.min())
        x = np.sin(2 * np.pi * ff * np.arange(N_IN)).astype(np.float32)
        y = vref.varispeed(x, pos, scale, n_out, STEP, Z, L, tab).astype(np.float64)
        y64, _mag = vref.varispeed_exact(x, pos, scale, n_out, STEP, Z, L, beta, r)
        p, _s = vref.positions(pos, scale, n_out, STEP)
        e_tab, e_win = float(np.abs(y - y64).max()), float(np.abs(y64 - np.sin(2 * np.pi * ff * p)).max())
        print(f"kaiser_fast rate {rate} f {f}: table chain against the exact filter {e_tab:.2e}, exact filter against the sine {e_win:.2e}")
        assert e_tab <= 1e-5 and e_win <= 1e-4, (rate, f, e_tab, e_win)


def test_the_exact_filter_variant_is_the_limit_of_the_table():
    """the float64 variant evaluates h itself: it is within 1e-7 of the sine where the table scheme is within 1e-5, and the float32
    chain lies within 4 * 2^-24 * sum |w x| plus the table's interpolation error of it"""
    Z, beta, r = vref.FILTERS["kaiser_best"]
    L = 512
    tab = vref.table(Z, L, beta, r)
    n_out, pos, scale = _tables(1.3)
    n_out = 400
    nb = -(-n_out // STEP)
    pos, scale = pos[:nb + 1], scale[:nb]
    ff = 0.2 * float(scale.min())
    x = np.sin(2 * np.pi * ff * np.arange(N_IN)).astype(np.float32)
    y64, mag = vref.varispeed_exact(x, pos, scale, n_out, STEP, Z, L, beta, r)
    p, _s = vref.positions(pos, scale, n_out, STEP)
    e64 = float(np.abs(y64 - np.sin(2 * np.pi * ff * p)).max())
    y32 = vref.varispeed(x, pos, scale, n_out, STEP, Z, L, tab).astype(np.float64)
    e32 = float(np.abs(y32 - y64).max())
    print(f"exact filter against the sine {e64:.2e}; float32 table chain against the exact filter {e32:.2e}; largest sum |w x| {float(mag.max()):.2f}")
    assert e64 <= 2e-7                                            # (the input itself is rounded to float32: 6e-8)
    assert (np.abs(y32 - y64) <= 4 * 2.0 ** -24 * mag + 3.1e-6).all()
