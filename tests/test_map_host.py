"""CPU: the host half of tempo maps -- the five mapped entry points (pg_spec_clips_map, pg_phase_vocoder_map, pg_phase_lock_map,
pg_phase_lock_linked_map, pg_ola_stretch_map): exported symbols, struct sizes against the header's "N bytes" comments, no 64-bit
integer field but workspace_bytes, every argument error in the documented order (validation runs before any launch), the workspace
queries against their twins' -- and phasegen.track.TimeMap with its plan, against the restatement of tests/_map_ref.py.

The impulse.  With the restatement of pg_ola_stretch_map alone (win_len 256, hop 64): a unit impulse at source sample s0 under the
map [(0, 0), (0.5, 0.25), (1.5, 2.25)] (stretch 0.5 over the first half second, 2 after it).  Grain g, centred on output sample 64 g,
reads the source around rint(src_of_out(64 g)); the grain whose centre's image lies nearest to s0 is at most half an output hop
times the local slope away from it, so it carries the impulse to within 32 output samples of out_of_src(s0), and every other grain
that carries it puts it at the SAME source offset from its own centre, at most 128 samples from that centre -- weighted by a Hann
window that is largest at the centre.  The largest output sample therefore lies within 32 + 64 < win_len / 2 = 128 samples of
out_of_src(s0) on either segment; s0 is taken once in each (and away from the break, where two slopes meet under one window)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _map_ref as mref
import _transient_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_SYMBOLS = ("pg_spec_clips_map", "pg_phase_vocoder_map", "pg_workspace_bytes_phase_lock_map", "pg_phase_lock_map",
               "pg_workspace_bytes_phase_lock_linked_map", "pg_phase_lock_linked_map", "pg_ola_stretch_map")
STRUCTS = {"pg_spec_clips_map_args": ("SpecClipsMapArgs", 56), "pg_phase_vocoder_map_args": ("PhaseVocoderMapArgs", 64),
           "pg_phase_lock_map_args": ("PhaseLockMapArgs", 80), "pg_phase_lock_linked_map_args": ("PhaseLockLinkedMapArgs", 88),
           "pg_ola_stretch_map_args": ("OlaStretchMapArgs", 72)}


# ---- the C entry points --------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in MAP_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    for name in MAP_SYMBOLS:
        assert _lib.SYMBOLS[name][0] is (ctypes.c_int64 if "workspace_bytes" in name else ctypes.c_int)
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def test_struct_sizes_match_the_header_and_hold_no_64_bit_size():
    from phasegen import _lib
    h = open(os.path.join(ROOT, "include", "phasegen.h")).read()
    for cname, (pyname, size) in STRUCTS.items():
        S = getattr(_lib, pyname)
        assert ctypes.sizeof(S) == size, (cname, ctypes.sizeof(S))
        assert re.search(r"\}\s*" + cname + r";\s*/\*\s*" + str(size) + r" bytes\s*\*/", h), cname
        assert [f for f, t in S._fields_ if t is ctypes.c_int64] == (["workspace_bytes"] if "lock" in cname else []), cname
        assert dict(S._fields_)["pos"] is ctypes.c_void_p
        assert not any(t is ctypes.c_double for _, t in S._fields_), cname       # no rate: the table is the grid
    # the layout the header states, field by field
    V = _lib.PhaseLockMapArgs
    assert (V.n_ch.offset, V.bins.offset, V.F_src.offset, V.F_out.offset, V.reset_below.offset, V.a_ch_rows.offset, V.m_ch_rows.offset) == (0, 4, 8, 12, 16, 20, 24)
    assert (V.pos.offset, V.A.offset, V.M.offset, V.out.offset, V.workspace.offset, V.workspace_bytes.offset) == (32, 40, 48, 56, 64, 72)
    K = _lib.PhaseLockLinkedMapArgs
    assert (K.pos.offset, K.A.offset, K.Aref.offset, K.Mref.offset, K.out.offset, K.workspace.offset, K.workspace_bytes.offset) == (32, 40, 48, 56, 64, 72, 80)
    C = _lib.SpecClipsMapArgs
    assert (C.sf.offset, C.F_src.offset, C.p_ch_rows.offset, C.pos.offset, C.P.offset, C.out.offset) == (16, 20, 24, 32, 40, 48)
    O = _lib.OlaStretchMapArgs
    assert (O.n_in.offset, O.n_out.offset, O.x_stride.offset, O.base_stride.offset, O.y_stride.offset, O.pos.offset, O.y.offset) == (12, 16, 20, 24, 28, 32, 64)


def _clips(_lib):
    a = _lib.SpecClipsMapArgs()
    a.n_clips, a.n_ch, a.bins, a.frames, a.sf, a.F_src, a.p_ch_rows = 3, 2, 5, 8, 5, 23, 5
    a.pos = a.P = a.out = 4096
    return a


def _voc(_lib, cls="PhaseVocoderMapArgs"):
    a = getattr(_lib, cls)()
    a.n_ch, a.bins, a.F_src, a.F_out, a.reset_below, a.a_ch_rows, a.m_ch_rows = 2, 5, 19, 25, 0.05, 5, 5
    a.pos = a.A = a.M = a.out = 4096
    return a


def _lock(_lib):
    a = _voc(_lib, "PhaseLockMapArgs")
    a.workspace, a.workspace_bytes = 4096, 1 << 20
    return a


def _linked(_lib):
    a = _lib.PhaseLockLinkedMapArgs()
    a.n_ch, a.bins, a.F_src, a.F_out, a.reset_below, a.a_ch_rows = 2, 5, 19, 25, 0.05, 5
    a.pos = a.A = a.Aref = a.Mref = a.out = 4096
    a.workspace, a.workspace_bytes = 4096, 1 << 20
    return a


def _ola(_lib):
    a = _lib.OlaStretchMapArgs()
    a.n_sig, a.win_len, a.hop, a.n_in, a.n_out, a.x_stride, a.base_stride, a.y_stride = 2, 256, 64, 1000, 1500, 1000, 1500, 1500
    a.pos = a.x = a.win = a.base = a.y = 4096
    return a


BAD_FLOOR = [dict(reset_below=bad) for bad in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan"))]
# per entry point: (symbol, message prefix, good arguments, classes of bad fields in the order the header lists them)
ERROR_TABLES = {
    "spec_clips_map": ("pg_spec_clips_map", _clips,
                       [[dict(P=None), dict(out=None), dict(pos=None)],
                        [{k: bad} for k in ("n_clips", "n_ch", "bins", "frames", "F_src") for bad in (0, -3)] + [dict(sf=0), dict(sf=-1), dict(p_ch_rows=4)],
                        [{k: 4096 + off} for k in ("P", "out") for off in (1, 2, 3)] + [dict(pos=4096 + off) for off in (1, 2, 4, 7)]]),
    "phase_vocoder_map": ("pg_phase_vocoder_map", _voc,
                          [[dict(A=None), dict(out=None), dict(pos=None)],
                           [{k: bad} for k in ("n_ch", "bins", "F_src", "F_out") for bad in (0, -3)] + BAD_FLOOR + [dict(a_ch_rows=4), dict(m_ch_rows=4)],
                           [{k: 4096 + off} for k in ("A", "M", "out") for off in (1, 2, 3)] + [dict(pos=4096 + off) for off in (1, 2, 4, 7)]]),
    "phase_lock_map": ("pg_phase_lock_map", _lock,
                       [[dict(A=None), dict(M=None), dict(out=None), dict(pos=None)],
                        [{k: bad} for k in ("n_ch", "bins", "F_src", "F_out") for bad in (0, -3)] + [dict(bins=4097, a_ch_rows=4097, m_ch_rows=4097)]
                        + BAD_FLOOR + [dict(a_ch_rows=4), dict(m_ch_rows=4)],
                        [{k: 4096 + off} for k in ("A", "M", "out", "workspace") for off in (1, 2, 3)] + [dict(pos=4096 + off) for off in (1, 2, 4, 7)],
                        [dict(workspace=None), dict(workspace_bytes=12 * 2 * 5 - 1), dict(workspace_bytes=0), dict(workspace_bytes=-1)]]),
    "phase_lock_linked_map": ("pg_phase_lock_linked_map", _linked,
                              [[dict(A=None), dict(Aref=None), dict(Mref=None), dict(out=None), dict(pos=None)],
                               [{k: bad} for k in ("n_ch", "bins", "F_src", "F_out") for bad in (0, -3)] + [dict(bins=4097, a_ch_rows=4097)]
                               + BAD_FLOOR + [dict(a_ch_rows=4)],
                               [{k: 4096 + off} for k in ("A", "Aref", "Mref", "out", "workspace") for off in (1, 2, 3)]
                               + [dict(pos=4096 + off) for off in (1, 2, 4, 7)],
                               [dict(workspace=None), dict(workspace_bytes=12 * 5 - 1), dict(workspace_bytes=0), dict(workspace_bytes=-1)]]),
    "ola_stretch_map": ("pg_ola_stretch_map", _ola,
                        [[dict(x=None), dict(win=None), dict(y=None), dict(pos=None)],
                         [{k: bad} for k in ("n_sig", "n_in", "n_out") for bad in (0, -3)]
                         + [dict(win_len=w) for w in (0, 1, 255, 4098)] + [dict(hop=0), dict(hop=129)]
                         + [dict(x_stride=999), dict(y_stride=1499), dict(base_stride=1499)],
                         [{k: 4096 + off} for k in ("x", "win", "base", "y") for off in (1, 2, 3)] + [dict(pos=4096 + off) for off in (1, 2, 4, 7)]]),
}


@pytest.mark.parametrize("op", sorted(ERROR_TABLES))
def test_argument_errors_are_reported_before_any_launch_and_in_order(op):
    """NULL before shapes before alignment before the workspace: each class alone, then every pair of classes in one call -- the
    earlier class decides.  The pointers are fake and never dereferenced: nothing is launched."""
    from phasegen import _lib
    lib = _lib.load()
    symbol, good, classes = ERROR_TABLES[op]
    f = getattr(lib, symbol)
    codes = (_lib.ERR_NULL, _lib.ERR_SHAPE, _lib.ERR_ALIGN, _lib.ERR_WORKSPACE)[:len(classes)]
    assert f(None, None) == _lib.ERR_NULL

    def code(fields):
        a = good(_lib)
        for k, v in fields.items():
            setattr(a, k, v)
        rc = f(ctypes.byref(a), None)
        msg = lib.pg_last_error_string()
        assert rc != 0 and msg.startswith(op.encode() + b": "), (fields, rc, msg)
        return rc

    for rows, want in zip(classes, codes):
        for fields in rows:
            assert code(fields) == want, (op, fields)
    for i in range(len(classes)):
        for j in range(i + 1, len(classes)):
            for early in classes[i]:
                for late in classes[j]:
                    if set(early) & set(late):
                        continue
                    assert code({**late, **early}) == codes[i], (op, early, late)


def test_optional_planes_and_unused_strides_do_not_decide():
    """M NULL (vocoder) and base NULL (overlap-add) are legal and their strides are then not looked at; one channel / one signal
    never applies a stride, so a short one is not an error -- the twins' rule.  Every call here ends at the launch, which fails
    without a device or, on one, would read the fake pointers: so only the checks in FRONT of the one that fails are observed."""
    from phasegen import _lib
    lib = _lib.load()
    a = _voc(_lib)
    a.M, a.m_ch_rows, a.out = None, 0, 4097                                         # past M's row: the alignment row answers
    assert lib.pg_phase_vocoder_map(ctypes.byref(a), None) == _lib.ERR_ALIGN
    o = _ola(_lib)
    o.base, o.base_stride, o.y = None, 0, 4097
    assert lib.pg_ola_stretch_map(ctypes.byref(o), None) == _lib.ERR_ALIGN


def test_workspace_queries_equal_their_twins():
    from phasegen import _lib, ops
    lib = _lib.load()
    assert lib.pg_workspace_bytes_phase_lock_map(None) == _lib.ERR_NULL
    assert lib.pg_workspace_bytes_phase_lock_linked_map(None) == _lib.ERR_NULL
    L = ops.PHASE_LOCK_CHUNK
    for n_ch in (1, 2, 7):
        for bins in (1, 5, 1024, 4096):
            for F_out in (1, L - 1, L, L + 1, 3 * L + 5, 10 ** 6, 2 ** 31 - 1):
                m, t = _lib.PhaseLockMapArgs(), _lib.PhaseLockArgs()
                m.n_ch, m.bins, m.F_src, m.F_out = n_ch, bins, 19, F_out
                t.n_ch, t.bins, t.F_src, t.F_out = n_ch, bins, 19, F_out
                got = lib.pg_workspace_bytes_phase_lock_map(ctypes.byref(m))
                assert got == lib.pg_workspace_bytes_phase_lock(ctypes.byref(t)) == 12 * n_ch * bins * -(-F_out // L)
                km, kt = _lib.PhaseLockLinkedMapArgs(), _lib.PhaseLockLinkedArgs()
                km.n_ch, km.bins, km.F_src, km.F_out = n_ch, bins, 19, F_out
                kt.n_ch, kt.bins, kt.F_src, kt.F_out = n_ch, bins, 19, F_out
                got = lib.pg_workspace_bytes_phase_lock_linked_map(ctypes.byref(km))
                assert got == lib.pg_workspace_bytes_phase_lock_linked(ctypes.byref(kt)) == 12 * bins * -(-F_out // L)
    for field, bad in (("n_ch", 0), ("bins", 0), ("F_out", 0), ("bins", 4097), ("F_out", -1)):
        for make, q in ((_lock, lib.pg_workspace_bytes_phase_lock_map), (_linked, lib.pg_workspace_bytes_phase_lock_linked_map)):
            a = make(_lib)
            setattr(a, field, bad)
            assert q(ctypes.byref(a)) == _lib.ERR_SHAPE, (field, bad)


def test_python_wrappers_take_pos_by_keyword_only():
    import inspect
    from phasegen import ops
    for fn in (ops.spec_clips, ops.phase_vocoder, ops.phase_lock, ops.phase_lock_linked, ops.ola_stretch):
        assert fn.options == {"pos": None}, fn.__name__
        params = inspect.signature(fn).parameters                                   # the list callers pinned: without the keyword
        assert "pos" not in params and params["src_per_out"].default == 1.0 and list(params)[-1] == "out"
        with pytest.raises(TypeError):
            fn(*range(len(params) + 1))                                             # pos is not positional
    assert ops.ola_grains(1025, 256, 64) == (1025 + 128) // 64 + 1 == mref.n_grains(1025, 256, 64)
    assert ops.ola_grains(7, 8, 2) == 6


# ---- TimeMap -------------------------------------------------------------------------------------------------------------

def test_anchors_are_hit_exactly_and_the_two_directions_invert_each_other():
    from phasegen.track import TimeMap
    anchors = [(0, 0), (0.7, 0.35), (1.3, 2.0), (2.9, 3.1), (4.0, 7.5)]
    tm, rm = TimeMap(anchors), mref.TimeMap(anchors)
    assert tm.anchors == [(float(s), float(o)) for s, o in anchors]
    for sr in (16000, 44100):
        for s, o in anchors:
            assert tm.out_of_src(s * sr, sr) == o * sr and tm.src_of_out(o * sr, sr) == s * sr
        s = np.concatenate([np.linspace(0.0, 6.0 * sr, 4001), np.array([0.0, 1.0, 0.7 * sr, 4.0 * sr, 1e9])])
        back = tm.src_of_out(tm.out_of_src(s, sr), sr)
        assert np.all(np.abs(back - s) <= 1e-9 * np.maximum(np.abs(s), 1.0))
        assert np.array_equal(tm.out_of_src(s, sr), rm.out_of_src(s, sr)) and np.array_equal(tm.src_of_out(s, sr), rm.src_of_out(s, sr))
        assert np.all(np.diff(tm.out_of_src(np.sort(s), sr)) >= 0)
    assert isinstance(tm.src_of_out(5.0), float)
    # past the last anchor the last segment's line continues
    assert tm.out_of_src(5.0 * 16000) == pytest.approx((7.5 + (7.5 - 3.1) / (4.0 - 2.9)) * 16000, rel=1e-12)
    assert np.allclose(tm.stretches, [0.5, 1.65 / 0.6, 1.1 / 1.6, 4.4 / 1.1])


def test_every_rejection():
    from phasegen.track import TimeMap
    nan, inf = float("nan"), float("inf")
    for bad in ([], [(0, 0)], [(0.1, 0), (1, 1)], [(0, 0.1), (1, 1)], [(0, 0), (1, nan)], [(0, 0), (inf, 1)],
                [(0, 0), (1, 1), (1, 2)], [(0, 0), (1, 1), (2, 1)], [(0, 0), (1, 1), (0.5, 2)], [(0, 0), (1, 2), (2, 1.5)],
                [(0, 0), (1, 0.2499)], [(0, 0), (1, 4.001)], [(0, 0), (1, 1), (2, 1.2)], [(0, 0), (1, 1), (1.1, 2)],
                [(0, 0, 0), (1, 1, 1)], [(0, 0), (1,)], [(0, 0), ("a", 1)], 5):
        with pytest.raises(ValueError):
            TimeMap(bad)
    TimeMap([(0, 0), (1, 0.25)]), TimeMap([(0, 0), (1, 4)])                         # the ends of the domain are inside it
    for kw in (dict(duration_s=0), dict(duration_s=inf), dict(n=0), dict(r0=0.2), dict(r1=4.5)):
        with pytest.raises(ValueError):
            TimeMap.ramp(**{**dict(duration_s=3.0, r0=1.0, r1=1.5, n=8), **kw})
    with pytest.raises(ValueError):
        TimeMap([(0, 0), (1, 1)]).plan(0, 24, 8, 4)


@pytest.mark.parametrize("R", [0.25, 0.5, 1.0, 2.0, 4.0])
def test_a_one_segment_map_is_the_uniform_plan(R):
    from phasegen.track import SpectralPlan, TimeMap, spectral_plan
    tm = TimeMap([(0, 0), (1, R)])
    for a_len, frames, hop, ov in ((48000, 128, 512, 32), (4000, 24, 8, 4), (96001, 128, 512, 32), (700, 24, 8, 0), (15999, 24, 8, 4), (16001, 24, 8, 4)):
        want = spectral_plan(a_len, frames, hop, ov, R)
        got = tm.plan(a_len, frames, hop, ov)
        assert SpectralPlan(*got[:7]) == want and got._fields[:7] == want._fields, (R, a_len)
        assert got.pos.dtype == np.float64 and got.pos.shape == (want.F_out,)
        assert np.array_equal(got.pos, np.arange(want.F_out, dtype=np.float64) * (1.0 / R))
        n_out = hop * (want.F_out - 1)
        assert got.grains.shape == (mref.n_grains(n_out, 256, 64),)
        assert np.array_equal(got.grains, (np.arange(got.grains.shape[0], dtype=np.int64) * 64).astype(np.float64) * (1.0 / R))
        ref = mref.mapped_plan(mref.TimeMap(tm.anchors), a_len, frames, hop, ov)
        assert all(ref[k] == getattr(got, k) for k in want._fields)
        assert np.array_equal(ref["pos"], got.pos) and np.array_equal(ref["grains"], got.grains)


def test_the_plan_of_a_real_map_equals_the_restatement():
    from phasegen.track import TimeMap
    anchors = [(0, 0), (1.0, 0.5), (2.0, 2.5), (3.0, 3.25)]
    got = TimeMap(anchors).plan(48000, 128, 512, 32)
    ref = mref.mapped_plan(mref.TimeMap(anchors), 48000, 128, 512, 32)
    assert got.a_out == 52000 and all(ref[k] == getattr(got, k) for k in ("sf", "Vf", "a_out", "n_clips", "F_out", "F_src", "n_src"))
    assert np.array_equal(ref["pos"], got.pos) and np.array_equal(ref["grains"], got.grains)
    assert got.F_src - 1 > got.pos.max() >= got.F_src - 2 and np.all(np.diff(got.pos) > 0)     # the upper neighbour always exists
    assert got.n_src == 512 * (got.F_src - 1)


def test_ramp_has_monotone_slopes_within_its_ends():
    from phasegen.track import TimeMap
    for r0, r1, n in ((1.0, 1.5, 64), (2.0, 0.5, 7), (0.25, 4.0, 64), (1.25, 1.25, 3), (1.0, 1.5, 1)):
        tm = TimeMap.ramp(10.0, r0, r1, n)
        s = tm.stretches
        assert s.shape == (n,) and tm.src[-1] == 10.0 and np.allclose(np.diff(tm.src), 10.0 / n)
        assert np.all(s >= min(r0, r1) - 1e-12) and np.all(s <= max(r0, r1) + 1e-12)
        assert np.all(np.diff(s) >= -1e-12) if r1 >= r0 else np.all(np.diff(s) <= 1e-12)
        assert np.allclose(s, r0 + (r1 - r0) * (np.arange(n) + 0.5) / n, rtol=1e-12)
        assert tm.out[-1] == pytest.approx(10.0 * (r0 + r1) / 2, rel=1e-12)            # midpoint rule: exact for a line


def test_load_round_trips(tmp_path):
    from phasegen.track import TimeMap
    tm = TimeMap([(0, 0), (0.1 + 0.2, 1 / 3), (2.5, 3.0), (1e3 / 7, 400.0)])
    path = tmp_path / "map.txt"
    tm.save(str(path))
    again = TimeMap.load(str(path))
    assert np.array_equal(again.src, tm.src) and np.array_equal(again.out, tm.out)
    path.write_text("# a click track\n\n0 0   # start\n  1.5, 3\n4\t5.5\n")
    assert TimeMap.load(str(path)).anchors == [(0.0, 0.0), (1.5, 3.0), (4.0, 5.5)]
    for text in ("0 0\n1\n", "0 0\n1 2 3\n", "0 0\n1 x\n", "0 0\n", "0 0\n1 9\n"):
        path.write_text(text)
        with pytest.raises(ValueError):
            TimeMap.load(str(path))


def test_a_map_is_refused_where_a_stretch_other_than_one_is():
    """before any device work: the checks run on the arguments alone"""
    from phasegen import track
    tm = track.TimeMap([(0, 0), (1, 1)])                                            # even the identity: a map is a map
    x = np.zeros(4000, np.float32)
    with pytest.raises(ValueError, match="join='spectral'"):
        track.reconstruct_track(None, x, phase="zero", stretch=tm)
    with pytest.raises(ValueError, match="TimeMap needs phase"):
        track.reconstruct_track(None, x, phase="original", join="spectral", stretch=tm)
    with pytest.raises(ValueError, match="TimeMap"):
        track.pitch_shift(None, x, tm, phase="zero")
    with pytest.raises(ValueError):
        track.evaluate_stretch(None, x, tm, phases=("original",))
    assert track.reconstruct_track.options == {"join": "waveform", "stretch": 1.0}   # no new keyword


# ---- the restatement alone -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s0", [3000, 4001, 12000, 20000])
def test_an_impulse_lands_where_the_map_sends_it(s0):
    """module docstring: stretch 0.5 then 2, win_len 256, hop 64; s0 on the first segment (twice) and on the second (twice)"""
    anchors = [(0, 0), (0.5, 0.25), (1.5, 2.25)]
    tm = mref.TimeMap(anchors)
    n_in, win_len, hop = 24000, 256, 64
    n_out = int(round(float(tm.out_of_src(n_in))))
    assert n_out == 36000
    x = np.zeros((1, n_in), np.float32)
    x[0, s0] = 1.0
    c = tm.src_of_out(np.arange(mref.n_grains(n_out, win_len, hop), dtype=np.float64) * hop)
    y = mref.ola_stretch_map(x, n_out, c, tref.ola_window(win_len), hop)
    at, want = int(np.abs(y[0]).argmax()), float(tm.out_of_src(s0))
    assert y[0, at] > 0.0 and abs(at - want) <= win_len / 2, (s0, at, want)
    # a uniform table is the uniform restatement, bit for bit
    noise = np.random.RandomState(s0).standard_normal((2, 2000)).astype(np.float32)
    for spo in (1.0, 0.5, 1 / 1.3, 4.0):
        cu = (np.arange(mref.n_grains(1025, win_len, hop), dtype=np.int64) * hop).astype(np.float64) * spo
        want = tref.ola_stretch(noise, 1025, spo, tref.ola_window(win_len), hop)
        assert np.abs(want).max() > 0 and np.array_equal(mref.ola_stretch_map(noise, 1025, cu, tref.ola_window(win_len), hop), want)
