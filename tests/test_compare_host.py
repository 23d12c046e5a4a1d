"""CPU: the host half of pg_wave_compare / pg_spec_compare (include/phasegen.h) and of the quality report built on them: exported
symbols, struct layouts against the header, every argument error (validation runs before any launch) with its message, the
workspace queries, and the Python signatures.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

COMPARE_SYMBOLS = ("pg_workspace_bytes_wave_compare", "pg_wave_compare", "pg_workspace_bytes_spec_compare", "pg_spec_compare")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in COMPARE_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert hasattr(_lib, "WaveCompareArgs") and hasattr(_lib, "SpecCompareArgs")
    assert _lib.SYMBOLS["pg_workspace_bytes_wave_compare"][0] is ctypes.c_int64
    assert _lib.SYMBOLS["pg_workspace_bytes_spec_compare"][0] is ctypes.c_int64
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def _header_fields(struct):
    """Field names of `struct` in declaration order, read from include/phasegen.h."""
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


def test_struct_layouts_match_the_header():
    from phasegen import _lib
    W, S = _lib.WaveCompareArgs, _lib.SpecCompareArgs
    assert [f[0] for f in W._fields_] == _header_fields("pg_wave_compare_args")
    assert [f[0] for f in S._fields_] == _header_fields("pg_spec_compare_args")
    assert ctypes.sizeof(W) == 80 and ctypes.sizeof(S) == 80                        # the sizes the header states
    assert (W.n_signals.offset, W.n.offset, W.x.offset, W.x_stride.offset, W.y.offset, W.y_stride.offset) == (0, 8, 16, 24, 32, 40)
    assert (W.gain.offset, W.out.offset, W.workspace.offset, W.workspace_bytes.offset) == (48, 56, 64, 72)
    assert (S.n_signals.offset, S.bins.offset, S.frames.offset, S.floor_power.offset) == (0, 4, 8, 12)
    assert (S.R.offset, S.r_stride.offset, S.E.offset, S.e_stride.offset) == (16, 24, 32, 40)
    assert (S.gain.offset, S.out.offset, S.workspace.offset, S.workspace_bytes.offset) == (48, 56, 64, 72)
    assert S.floor_power.size == 4 and W.n.size == 8


def _wave(_lib):
    """3 rows of 70001 samples, 70004 apart; pointers are fake and never dereferenced."""
    a = _lib.WaveCompareArgs()
    a.n_signals, a.n, a.x_stride, a.y_stride = 3, 70001, 70004, 70004
    a.x = a.y = a.out = a.gain = a.workspace = 4096
    a.workspace_bytes = 1 << 20
    return a


def _spec(_lib):
    """2 signals of 37 bins x 70 frames; pointers are fake and never dereferenced."""
    a = _lib.SpecCompareArgs()
    a.n_signals, a.bins, a.frames, a.floor_power = 2, 37, 70, 1e-10
    a.r_stride = a.e_stride = 2 * 37 * 70
    a.R = a.E = a.out = a.gain = a.workspace = 4096
    a.workspace_bytes = 1 << 20
    return a


def test_wave_compare_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    fn, err = lib.pg_wave_compare, lib.pg_last_error_string
    assert fn(None, None) == _lib.ERR_NULL and b"null args" in err()
    for field in ("n_signals", "n"):
        for bad in (0, -3):
            a = _wave(_lib)
            setattr(a, field, bad)
            assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"non-positive" in err(), (field, bad)
    for field in ("x_stride", "y_stride"):
        a = _wave(_lib)
        setattr(a, field, 70000)
        assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE and field.encode() + b" shorter than a row" in err(), field
    for field in ("x", "y", "out"):
        a = _wave(_lib)
        setattr(a, field, None)
        assert fn(ctypes.byref(a), None) == _lib.ERR_NULL and b"required" in err(), field
    for field, bad in (("x", 4098), ("y", 4097), ("out", 4100), ("gain", 4100)):
        a = _wave(_lib)
        setattr(a, field, bad)
        assert fn(ctypes.byref(a), None) == _lib.ERR_ALIGN and b"misaligned" in err(), field
    a = _wave(_lib)
    need = lib.pg_workspace_bytes_wave_compare(ctypes.byref(a))
    a.workspace = None
    assert fn(ctypes.byref(a), None) == _lib.ERR_WORKSPACE and b"pg_workspace_bytes_wave_compare" in err()
    a.workspace, a.workspace_bytes = 4096, need - 1
    assert fn(ctypes.byref(a), None) == _lib.ERR_WORKSPACE and b"workspace" in err()
    a.workspace, a.workspace_bytes = 4100, need
    assert fn(ctypes.byref(a), None) == _lib.ERR_ALIGN and b"workspace must be 8-byte aligned" in err()
    a = _wave(_lib)
    a.n_signals, a.n = 1 << 20, 1 << 40                                             # more workgroups than a grid holds
    a.x_stride = a.y_stride = 1 << 40
    assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"2^31" in err()


def test_spec_compare_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    fn, err = lib.pg_spec_compare, lib.pg_last_error_string
    assert fn(None, None) == _lib.ERR_NULL and b"null args" in err()
    for field in ("n_signals", "bins", "frames"):
        for bad in (0, -3):
            a = _spec(_lib)
            setattr(a, field, bad)
            assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"non-positive" in err(), (field, bad)
    for bad in (0.0, -1e-10, float("inf"), float("nan")):
        a = _spec(_lib)
        a.floor_power = bad
        assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"floor_power" in err(), bad
    for field in ("r_stride", "e_stride"):
        a = _spec(_lib)
        setattr(a, field, 2 * 37 * 70 - 1)
        assert fn(ctypes.byref(a), None) == _lib.ERR_SHAPE and field.encode() + b" shorter than a signal" in err(), field
    for field in ("R", "E", "out"):
        a = _spec(_lib)
        setattr(a, field, None)
        assert fn(ctypes.byref(a), None) == _lib.ERR_NULL and b"required" in err(), field
    for field, bad in (("R", 4098), ("E", 4097), ("out", 4100), ("gain", 4100)):
        a = _spec(_lib)
        setattr(a, field, bad)
        assert fn(ctypes.byref(a), None) == _lib.ERR_ALIGN and b"misaligned" in err(), field
    a = _spec(_lib)
    need = lib.pg_workspace_bytes_spec_compare(ctypes.byref(a))
    a.workspace = None
    assert fn(ctypes.byref(a), None) == _lib.ERR_WORKSPACE and b"pg_workspace_bytes_spec_compare" in err()
    a.workspace, a.workspace_bytes = 4096, need - 1
    assert fn(ctypes.byref(a), None) == _lib.ERR_WORKSPACE and b"workspace" in err()
    a.workspace, a.workspace_bytes = 4100, need
    assert fn(ctypes.byref(a), None) == _lib.ERR_ALIGN and b"workspace must be 8-byte aligned" in err()


def test_workspace_queries():
    """Pure host functions of the shapes: one 6-double partial per 8192 samples of a row; per (256-frame tile, 64-bin block) one
    partial, per tile one, and one double per frame and bin block."""
    from phasegen import _lib
    lib = _lib.load()
    w, s = lib.pg_workspace_bytes_wave_compare, lib.pg_workspace_bytes_spec_compare
    assert w(None) == _lib.ERR_NULL and s(None) == _lib.ERR_NULL
    assert w(ctypes.byref(_lib.WaveCompareArgs())) == _lib.ERR_SHAPE and s(ctypes.byref(_lib.SpecCompareArgs())) == _lib.ERR_SHAPE
    a = _lib.WaveCompareArgs()                                                      # pointers are not read
    for n_sig, n, chunks in ((1, 1, 1), (3, 8192, 1), (3, 8193, 2), (2, 70001, 9), (2, 4800000, 586)):
        a.n_signals, a.n = n_sig, n
        assert w(ctypes.byref(a)) == n_sig * chunks * 48, (n_sig, n)
    b = _lib.SpecCompareArgs()
    b.floor_power = 1e-10
    for n_sig, bins, frames, tiles, blocks in ((1, 16, 24, 1, 1), (2, 37, 70, 1, 1), (1, 1024, 5, 1, 16), (2, 16, 261, 2, 1), (2, 65, 257, 2, 2),
                                                (2, 1024, 9376, 37, 16)):
        b.n_signals, b.bins, b.frames = n_sig, bins, frames
        assert s(ctypes.byref(b)) == 8 * n_sig * (6 * tiles * blocks + 6 * tiles + blocks * frames), (n_sig, bins, frames)


def test_python_surface():
    """Signatures only (the calls need a GPU)."""
    from phasegen import audio, metrics, ops, track
    p = inspect.signature(ops.wave_compare).parameters
    assert list(p) == ["x", "y", "gain", "out"] and (p["gain"].default, p["out"].default) == (None, None)
    p = inspect.signature(ops.spec_compare).parameters
    assert list(p) == ["R", "E", "gain", "floor", "out"] and (p["gain"].default, p["floor"].default, p["out"].default) == (None, 1e-10, None)
    assert ops._compare_ws in ops._caches
    p = inspect.signature(metrics.compare_audio).parameters
    assert list(p) == ["ref", "est", "n_fft", "hop_length", "floor"]
    assert [p[k].default for k in list(p)[2:]] == [2048, 512, 1e-10]
    assert metrics.KEYS == ("si_sdr_db", "snr_db", "gain", "spectral_convergence", "lsd_db", "mag_gain", "max_abs_error", "n_samples",
                            "n_frames", "channels")
    p = inspect.signature(track.evaluate_track).parameters
    assert list(p) == ["model", "audio", "n_fft", "hop_length", "frames", "overlap_frames", "stats", "osr", "sr", "res_type", "clip_batch",
                       "phases", "gl_iters", "gl_seed", "floor", "return_audio"]
    assert [p[k].default for k in list(p)[2:]] == [2048, 512, 128, 32, None, None, 16000, "kaiser_best", 64, ("unet", "zero", "original"),
                                                   250, 0, 1e-10, False]
    p = inspect.signature(audio.griffin_lim_batch).parameters
    assert list(p) == ["mag", "n_fft", "hop_length", "n_iter", "init", "seed", "normalize"] and p["normalize"].default is True
    assert track.PHASES == ("unet", "zero", "original", "griffinlim")
