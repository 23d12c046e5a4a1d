"""CPU: the host half of the transient-preserving stretch (pg_hpss, pg_ola_stretch, pg_ola_window; phasegen.ops.hpss / ola_stretch;
phasegen.track transients="ola"): the exported symbols and the structs, every argument error in the documented order (validation
runs before any launch), the window table bit for bit, the Python surface, the combinations refused before any device work,
properties of the numpy restatements (tests/_transient_ref.py), and -- in float64 -- what the split buys on a signal with clicks.

The crest condition.  _transient_ref.clicky_melody is the project's melody (6 s at 16 kHz) over stationary noise 26 dB under a note,
plus five 2 ms noise bursts.  The figure is the crest of each burst in the output: the peak within +-96 samples of where the burst
belongs over the rms of +-2048 samples; the input's is 8.4, 9.8, 8.4, 7.9, 9.5.  The float64 chain at 2048 / 512 with
phase="vocoder_locked" (floor 0.2), 17 x 17 medians and overlap-add at 256 / 64 gives

    stretch   whole plane through the vocoder          harmonic part through the vocoder, percussive part moved
    1.5       2.91, 5.01, 2.18, 2.41, 6.96  (2.91)     6.63, 7.14, 6.44, 4.93, 7.26  (6.63)
    0.75      3.27, 5.06, 4.24, 2.37, 5.14  (4.24)     7.27, 6.86, 6.89, 3.82, 7.39  (6.89)

(medians in brackets; test_the_split_keeps_the_clicks prints them).  WITHOUT the background noise the bins between the melody's
partials are silent before every burst, the vocoder's reset floor hands them the analysis phase, and the bursts that sit well on the
output grid come through by themselves: 1.96, 8.77, 2.20, 2.24, 9.23 (2.24) against 6.77, 5.70, 5.19, 4.96, 7.48 (5.70) at 1.5, but
2.10, 7.11, 9.73, 2.33, 7.48 (7.11) against 7.30, 5.11, 6.13, 3.85, 7.30 (6.13) at 0.75.  The split's figures hardly depend on the
background or on where a burst sits; the vocoder's do.  The condition is therefore stated on the dense signal, the case the split
is for.  At stretch 1 the two chains agree to 5e-9 of a signal that peaks at 0.67 (the masks partition the cells and overlap-add at
ratio 1 is the identity)."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import _transient_ref as tref


# ---- the C entry points --------------------------------------------------------------------------------------------------

def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in ("pg_hpss", "pg_ola_stretch", "pg_ola_window"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4
    assert _lib.HPSS_MAX_WIN == 31


def test_struct_layouts():
    from phasegen import _lib
    H, O = _lib.HpssArgs, _lib.OlaStretchArgs
    assert ctypes.sizeof(H) == 56
    assert (H.n_ch.offset, H.bins.offset, H.F.offset, H.win_t.offset, H.win_f.offset) == (0, 4, 8, 16, 20)
    assert (H.M.offset, H.m_stride.offset, H.harm.offset, H.perc.offset) == (24, 32, 40, 48)
    assert not any(f[0] == "workspace" for f in H._fields_ + O._fields_)            # neither takes a workspace
    assert ctypes.sizeof(O) == 96
    assert (O.n_sig.offset, O.win_len.offset, O.hop.offset, O.n_in.offset, O.n_out.offset, O.src_per_out.offset) == (0, 4, 8, 16, 24, 32)
    assert (O.x.offset, O.x_stride.offset, O.win.offset, O.base.offset, O.base_stride.offset, O.y.offset, O.y_stride.offset) == (40, 48, 56, 64, 72, 80, 88)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "phasegen.h")).read()
    assert re.search(r"\}\s*pg_hpss_args;\s*/\*\s*56 bytes\s*\*/", h) and re.search(r"\}\s*pg_ola_stretch_args;\s*/\*\s*96 bytes\s*\*/", h)
    assert re.search(r"#define\s+PG_HPSS_MAX_WIN\s+31\b", h)


def _hpss_args(_lib):
    """2 channels of 5 bins and 19 frames; pointers are fake and never dereferenced."""
    a = _lib.HpssArgs()
    a.n_ch, a.bins, a.F, a.win_t, a.win_f = 2, 5, 19, 17, 17
    a.M = a.harm = a.perc = 4096
    a.m_stride = 5 * 19
    return a


def _ola_args(_lib):
    a = _lib.OlaStretchArgs()
    a.n_sig, a.win_len, a.hop, a.n_in, a.n_out, a.src_per_out = 2, 256, 64, 1000, 1500, 1 / 1.5
    a.x = a.win = a.base = a.y = 4096
    a.x_stride, a.base_stride, a.y_stride = 1000, 1500, 1500
    return a


def _classes(lib, f, make, prefix, classes):
    """each class alone, then every pair of classes in one call: the earlier class wins"""
    def code(**fields):
        a = make()
        for k, v in fields.items():
            setattr(a, k, v)
        rc = f(ctypes.byref(a), None)
        msg = lib.pg_last_error_string()
        assert rc != 0 and msg.startswith(prefix), (fields, rc, msg)
        return rc, msg

    for cases, want, word in classes:
        for c in cases:
            rc, msg = code(**c)
            assert rc == want and word in msg, (c, rc, msg)
    for i, (first, want, _) in enumerate(classes):
        for later, _, _ in classes[i + 1:]:
            for c1 in first[:4]:
                for c2 in later[:4]:
                    if not set(c1) & set(c2):
                        assert code(**c1, **c2)[0] == want, (c1, c2)
    return code


def test_hpss_argument_errors_are_reported_before_any_launch_and_in_order():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_hpss(None, None) == _lib.ERR_NULL
    null = [dict(M=None), dict(harm=None), dict(perc=None)]
    shape = ([{k: bad} for k in ("n_ch", "bins", "F") for bad in (0, -3)]
             + [{k: bad} for k in ("win_t", "win_f") for bad in (0, -1, 2, 16, 30, 32, 33, 1 << 20)]
             + [dict(m_stride=5 * 19 - 1), dict(m_stride=0), dict(n_ch=1 << 30, bins=1 << 20, F=1 << 40, m_stride=1 << 60),
                dict(bins=1 << 30, F=1 << 40, m_stride=1 << 62)])
    align = [{k: 4096 + off} for k in ("M", "harm", "perc") for off in (1, 2, 3)]
    code = _classes(lib, lib.pg_hpss, lambda: _hpss_args(_lib), b"hpss: ",
                    ((null, _lib.ERR_NULL, b"required"), (shape, _lib.ERR_SHAPE, b""), (align, _lib.ERR_ALIGN, b"misaligned")))
    assert b"odd" in code(win_t=16)[1] and b"m_stride" in code(m_stride=94)[1] and b"2^62" in code(**shape[-1])[1]
    a = _hpss_args(_lib)                                                            # a single channel: its stride is still checked
    a.n_ch, a.m_stride = 1, 94
    assert lib.pg_hpss(ctypes.byref(a), None) == _lib.ERR_SHAPE


def test_ola_stretch_argument_errors_are_reported_before_any_launch_and_in_order():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_ola_stretch(None, None) == _lib.ERR_NULL
    null = [dict(x=None), dict(win=None), dict(y=None)]
    shape = ([{k: bad} for k in ("n_sig", "n_in", "n_out") for bad in (0, -3)]
             + [dict(win_len=bad) for bad in (0, 1, -2, 3, 255, 4097, 4098, 8192)]
             + [dict(hop=bad) for bad in (0, -1, 129, 256)] + [dict(win_len=2, hop=2)]
             + [dict(src_per_out=bad) for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan"))]
             + [dict(x_stride=999), dict(y_stride=1499), dict(base_stride=1499), dict(n_sig=1 << 30, n_out=1 << 40, y_stride=1 << 40, base_stride=1 << 40)])
    align = [{k: 4096 + off} for k in ("x", "win", "base", "y") for off in (1, 2, 3)]
    code = _classes(lib, lib.pg_ola_stretch, lambda: _ola_args(_lib), b"ola_stretch: ",
                    ((null, _lib.ERR_NULL, b"required"), (shape, _lib.ERR_SHAPE, b""), (align, _lib.ERR_ALIGN, b"misaligned")))
    assert b"x_stride" in code(x_stride=999)[1] and b"base_stride" in code(base_stride=1)[1] and b"2^62" in code(**shape[-1])[1]
    a = _ola_args(_lib)                                                             # base is optional: without it its stride is not looked at
    a.base, a.base_stride, a.x = None, 0, None
    assert lib.pg_ola_stretch(ctypes.byref(a), None) == _lib.ERR_NULL               # (x: the call still stops before any launch)
    a = _ola_args(_lib)
    a.base, a.base_stride, a.y_stride = None, 0, 1
    assert lib.pg_ola_stretch(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"y_stride" in lib.pg_last_error_string()


def test_ola_window_is_the_double_formula_rounded_once():
    from phasegen import _lib, ops
    lib = _lib.load()
    for w in (2, 4, 8, 30, 256, 1024, 4096):
        got = ops.ola_window_host(w)
        want = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * j / w) for j in range(w)], np.float64).astype(np.float32)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), w
        assert np.array_equal(want.view(np.uint32), tref.ola_window(w).view(np.uint32))
        assert got[0] == 0.0 and got[w // 2] == 1.0 and (got >= 0).all()
    buf = np.empty(8, np.float32)
    assert lib.pg_ola_window(None, 8) == _lib.ERR_NULL
    for bad in (0, 1, -2, 7, 4097, 4098):
        assert lib.pg_ola_window(buf.ctypes.data_as(ctypes.c_void_p), bad) == _lib.ERR_SHAPE, bad
    # at hop = w / 4 the shifted copies sum to 2 (float64: to rounding)
    w = tref.ola_window(256).astype(np.float64)
    assert np.abs(w.reshape(4, 64).sum(0) - 2.0).max() < 1e-7


# ---- the Python surface --------------------------------------------------------------------------------------------------

def test_python_surface():
    """Signatures and defaults only (the calls need a GPU), and what earlier features pinned stays as it was."""
    from phasegen import ops, track
    p = inspect.signature(ops.hpss).parameters
    assert list(p) == ["logmag", "win_t", "win_f", "out"] and (p["win_t"].default, p["win_f"].default, p["out"].default) == (17, 17, None)
    p = inspect.signature(ops.ola_stretch).parameters
    assert list(p) == ["x", "n_out", "src_per_out", "win_len", "hop", "base", "out"]
    assert [p[k].default for k in list(p)[2:]] == [1.0, 256, 64, None, None]
    assert (track.HPSS_WIN, track.TRANSIENT_WINDOW, track.TRANSIENT_HOP, track.TRANSIENTS) == ((17, 17), 256, 64, (None, "ola"))
    assert track.reconstruct_track.options == {"join": "waveform", "stretch": 1.0}
    assert track.reconstruct_track.later_options == {"link_channels": False} and track.reconstruct_track.newer_options == {"transients": None}
    assert track.evaluate_stretch.options == {} and track.evaluate_stretch.later_options == {"link_channels": False}
    assert track.evaluate_stretch.newer_options == {"transients": None}
    assert track.evaluate_track.newer_options == {}
    assert list(inspect.signature(track.reconstruct_track).parameters)[-2:] == ["phase", "normalize"]
    assert list(inspect.signature(track.evaluate_stretch).parameters)[-1] == "return_audio"
    p = inspect.signature(track.pitch_shift).parameters
    assert p["transients"].default is None and p["transients"].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["link_channels"].default is False and list(p)[:3] == ["model", "audio", "semitones"]
    x = np.zeros(1000, np.float32)
    with pytest.raises(TypeError):
        track.reconstruct_track(None, x, 32, 8, 24, 4, None, None, 16000, "kaiser_best", 64, "zero", True, "ola")     # keyword only
    with pytest.raises(ValueError):
        ops.hpss(None)                                                              # refused before anything is looked at
    with pytest.raises(ValueError):
        ops.ola_stretch(None, 5)


def test_bad_combinations_are_refused_before_any_device_work():
    from phasegen import track
    x = np.zeros(1000, np.float32)
    small = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
    for phase in ("zero", "original"):                                              # the waveform join has no whole-track plane to split
        for kw in (dict(), dict(join="waveform")):
            with pytest.raises(ValueError, match="transients='ola' needs join='spectral'"):
                track.reconstruct_track(None, x, phase=phase, transients="ola", **kw, **small)
    for bad in ("OLA", "wsola", True, 1, ""):
        with pytest.raises(ValueError, match="transients must be None or 'ola'"):
            track.reconstruct_track(None, x, phase="zero", join="spectral", transients=bad, **small)
        with pytest.raises(ValueError, match="transients must be None or 'ola'"):
            track.evaluate_stretch(None, x, 1.5, phases=("zero",), transients=bad, **small)
        with pytest.raises(ValueError, match="transients must be None or 'ola'"):
            track.pitch_shift(None, x, 3, phase="zero", transients=bad, **small)
    # what the other options refuse stays refused with the option
    with pytest.raises(ValueError, match="stretch 1.5 needs phase"):
        track.reconstruct_track(None, x, phase="original", join="spectral", stretch=1.5, transients="ola", **small)
    with pytest.raises(ValueError, match="link_channels needs"):
        track.reconstruct_track(None, x, phase="vocoder", join="spectral", link_channels=True, transients="ola", **small)
    with pytest.raises(ValueError, match="needs a model"):
        track.reconstruct_track(None, x, phase="unet", join="spectral", transients="ola", **small)
    with pytest.raises(TypeError):
        track.evaluate_track(None, x, phases=("zero",), join="spectral", transients="ola", **small)      # no such option there


# ---- the restatements themselves -------------------------------------------------------------------------------------------

def _planted(seed, shape):
    """uniform [0, 1) with -0, +-inf and NaNs of both signs planted"""
    rs = np.random.RandomState(seed)
    M = rs.uniform(0.0, 1.0, shape).astype(np.float32)
    flat = M.reshape(-1)
    specials = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x00000000], np.uint32).view(np.float32)
    at = rs.choice(flat.size, size=min(flat.size, max(8, flat.size // 10)), replace=False)
    flat[at] = specials[np.arange(at.size) % specials.size]
    return M


def test_ref_key_is_the_total_order():
    f = np.array([0xFFFFFFFF, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F800000,
                  0x7F800001, 0x7FC00000, 0x7FFFFFFF], np.uint32).view(np.float32)      # -NaN < -inf < -1 < -denormal < -0 < +0 < ... < +inf < +NaN
    k = tref.key(f)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert np.array_equal(tref.unkey(k).view(np.uint32), f.view(np.uint32))
    x = np.random.RandomState(0).standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(tref.key(x), kind="stable"), np.argsort(x, kind="stable"))


def test_ref_hpss_partitions_the_cells_bit_for_bit():
    for seed, shape, wins in ((1, (2, 17, 33), (17, 17)), (2, (1, 5, 7), (31, 31)), (3, (3, 1, 1), (3, 5)), (4, (1, 40, 3), (1, 31))):
        for M in (_planted(seed, shape), np.random.RandomState(seed).randint(0, 4, shape).astype(np.float32)):
            harm, perc = tref.hpss(M, *wins)
            hb, pb, mb = (a.view(np.uint32) for a in (harm, perc, M))
            in_h, in_p = hb == mb, pb == mb
            assert ((in_h & (pb == 0)) | (in_p & (hb == 0))).all()                  # every cell in one plane, +0.0 in the other
            assert np.array_equal(np.where(hb != 0, hb, pb), mb)                    # (a +0.0 cell is +0.0 in both)


def test_ref_hpss_all_harmonic_cases():
    M = _planted(5, (2, 9, 21))
    harm, perc = tref.hpss(M, 1, 1)
    assert np.array_equal(harm.view(np.uint32), M.view(np.uint32)) and not perc.view(np.uint32).any()
    rows = np.repeat(_planted(6, (2, 9, 1)), 21, axis=2)                            # constant along time, win_f == 1: H == M == P
    for wt in (1, 3, 17, 31):
        harm, perc = tref.hpss(rows, wt, 1)
        assert np.array_equal(harm.view(np.uint32), rows.view(np.uint32)) and not perc.view(np.uint32).any()
    cols = np.repeat(_planted(7, (2, 1, 21)), 9, axis=1)                            # constant along frequency, win_t == 1: the tie goes to harm
    for wf in (1, 5, 17, 31):
        harm, perc = tref.hpss(cols, 1, wf)
        assert np.array_equal(harm.view(np.uint32), cols.view(np.uint32)) and not perc.view(np.uint32).any()
    # and something does go to perc: one loud column in a quiet plane
    M = np.full((1, 21, 41), 0.1, np.float32)
    M[0, :, 20] = 2.0
    harm, perc = tref.hpss(M, 17, 17)
    assert (perc[0, :, 20] == 2.0).all() and not perc[0, :, :20].any() and not harm[0, :, 20].any()
    M = np.full((1, 21, 41), 0.1, np.float32)                                       # one loud row: harmonic
    M[0, 10, :] = 2.0
    harm, perc = tref.hpss(M, 17, 17)
    assert (harm[0, 10] == 2.0).all() and not perc[0, 10].any()


def test_ref_ola_identity_bound_and_independence_of_n_out():
    """src_per_out == 1: |r - x[t]| <= (2 k + 2) 2^-24 |x[t]| for k covering frames (the header's derivation)."""
    rs = np.random.RandomState(8)
    x = (rs.standard_normal((2, 1500)) * 3.0).astype(np.float32)
    for w, hop in ((256, 64), (256, 128), (8, 2), (2, 1), (64, 7)):
        win = tref.ola_window(w)
        y = tref.ola_stretch(x, 1500, 1.0, win, hop)
        g_lo, g_hi = tref.ola_frames(1500, w, hop)
        k = (g_hi - g_lo + 1).astype(np.float64)
        assert k.max() <= w // hop + 1
        live = tref.ola_stretch(np.ones((1, 1500), np.float32), 1500, 1.0, win, hop)[0] > 0      # den > 0
        err = np.abs(y.astype(np.float64) - x)
        assert (err[:, live] <= ((2 * k + 2) * 2.0 ** -24 * np.abs(x.astype(np.float64)))[:, live]).all(), (w, hop)
        assert not y[:, ~live].any()
        for spo in (1.0, 1 / 1.3, 2.0):
            a, b = tref.ola_stretch(x, 700, spo, win, hop), tref.ola_stretch(x, 1100, spo, win, hop)
            assert np.array_equal(a.view(np.uint32), b[:, :700].view(np.uint32))
    # the default 256 / 64: w / hop + 1 = 5 bounds k (12 2^-24); hop divides w, so exactly 4 frames cover an inner sample (10 2^-24)
    g_lo, g_hi = tref.ola_frames(5000, 256, 64)
    assert int((g_hi - g_lo + 1).max()) == 4 and int((g_hi - g_lo + 1)[128:].min()) == 4
    g_lo, g_hi = tref.ola_frames(5000, 64, 7)
    assert int((g_hi - g_lo + 1).max()) == 64 // 7 + 1


def test_ref_ola_relocates_a_click_and_a_nan_reaches_its_cone_only():
    x = np.zeros((1, 4000), np.float32)
    x[0, 2000] = 1.0
    win = tref.ola_window(256)
    for stretch in (1.5, 0.75, 2.0):
        y = tref.ola_stretch(x, int(4000 * stretch), 1.0 / stretch, win, 64)[0]
        at = np.flatnonzero(y)
        assert at.size and abs(int(np.argmax(np.abs(y))) - 2000 * stretch) <= 64 and at.max() - at.min() < 2 * 256      # moved, not spread
    x = np.random.RandomState(9).standard_normal((1, 1000)).astype(np.float32)
    clean, reads = tref.ola_stretch(x, 1300, 1 / 1.3, win, 64, return_reads=True)
    x[0, 500] = np.nan
    bad = tref.ola_stretch(x, 1300, 1 / 1.3, win, 64)
    # win[0] == 0 and 0 * NaN is NaN: a frame that reads the sample under a zero weight carries it too (the formula multiplies)
    cone = np.array([500 in r for r in reads])
    assert np.array_equal(np.isnan(bad[0]), cone) and 0 < cone.sum() < 500
    assert np.array_equal(bad[0, ~cone].view(np.uint32), clean[0, ~cone].view(np.uint32))


# ---- the input condition of the GPU ordering test, in float64 ---------------------------------------------------------------

@pytest.mark.parametrize("stretch", [1.5, 0.75])
def test_the_split_keeps_the_clicks(stretch):
    x, at = tref.clicky_melody()
    plain = tref.crests(tref.stretch64(x, stretch, split=False), at, stretch)
    split = tref.crests(tref.stretch64(x, stretch, split=True), at, stretch)
    print(f"\nclicky melody, stretch {stretch}: crest of the input {np.round(tref.crests(x, at, 1.0), 2)}, whole plane {np.round(plain, 2)} "
          f"(median {np.median(plain):.2f}), split {np.round(split, 2)} (median {np.median(split):.2f})")
    assert np.median(split) > np.median(plain), (plain, split)


def test_the_split_is_the_identity_at_stretch_one():
    """The masks partition the cells and overlap-add at ratio 1 is the identity in float64, so the two chains differ by the PHASE of
    the percussive cells alone: the analysis' fp32 angle on one side, the locked vocoder's at rate 1 on the other, angle_of(q(A)),
    which is A to half a step of the 2^32 grid (7.3e-10 rad) and one rounding to fp32 (2^-23 rad below 4): d = 1.2e-7 rad per cell.
    A frame's sample moves by at most d (2 / n_fft) sum_k m_k, and a sample of the ISTFT is sum_f w_f frame_f / sum_f w_f^2 with
    sum w / sum w^2 = 4 / 3 for the Hann window at 75 % overlap (below 2 at the ends): bound 2 d (2 / n_fft) max_f sum_k m_k."""
    from phasegen.track import spectral_plan
    import _vocoder_ref as ref
    x, _ = tref.clicky_melody()
    a, b = tref.stretch64(x, 1.0, split=False), tref.stretch64(x, 1.0, split=True)
    pl = spectral_plan(x.shape[0], 128, 512, 32, 1.0)
    logmag, _ = ref.analysis64(x.astype(np.float64)[None], pl.n_src, 2048, 512)
    bound = 2.0 * (2.0 ** -23 + math.pi / 2.0 ** 32) * (2.0 / 2048) * np.expm1(logmag).sum(1).max()
    print(f"\nstretch 1: max |split - whole| = {np.abs(a - b).max():.3g} (bound {bound:.3g}), peak {np.abs(a).max():.3g}")
    assert np.abs(a - b).max() <= bound
