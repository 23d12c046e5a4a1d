"""CPU: the host half of pg_stitch (crossfaded overlap-add of clips into tracks, include/phasegen.h) and of the whole-track
pipeline built on it: exported symbols, struct layout, every argument error (validation runs before any launch), the ramp against
its float64 formula, the clip plan, and the Python signatures.  Nothing here needs a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

STITCH_SYMBOLS = ("pg_stitch_ramp", "pg_workspace_bytes_stitch", "pg_stitch")     # what include/phasegen.h declares for the feature


def test_symbols_are_exported_and_listed():
    from phasegen import _lib
    lib = _lib.load()
    for name in STITCH_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert hasattr(_lib, "StitchArgs")
    assert _lib.SYMBOLS["pg_workspace_bytes_stitch"][0] is ctypes.c_int64
    assert lib.pg_version() == 400                                                  # additive within ABI 0.4


def test_stitch_args_layout():
    from phasegen import _lib
    A = _lib.StitchArgs
    assert ctypes.sizeof(A) == 112
    assert (A.n_tracks.offset, A.n_clips.offset, A.clip_len.offset, A.step.offset) == (0, 4, 8, 12)
    assert (A.n_out.offset, A.clips.offset, A.clip_stride.offset, A.track_stride.offset) == (16, 24, 32, 40)
    assert (A.out.offset, A.out_stride.offset, A.ramp.offset, A.normalize.offset) == (48, 56, 64, 72)
    assert (A.peak.offset, A.n_nonfinite.offset, A.workspace.offset, A.workspace_bytes.offset) == (80, 88, 96, 104)


def _args(_lib):
    """5 clips of 184 samples, 120 apart (V = 64), cut 37 short; pointers are fake and never dereferenced."""
    a = _lib.StitchArgs()
    a.n_tracks, a.n_clips, a.clip_len, a.step, a.n_out = 2, 5, 184, 120, 4 * 120 + 184 - 37
    a.clips = a.out = a.ramp = 4096
    a.clip_stride, a.track_stride, a.out_stride = 184, 5 * 184, 4 * 120 + 184 - 37
    return a


def test_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    st = lib.pg_stitch
    assert st(None, None) == _lib.ERR_NULL
    for field in ("n_tracks", "n_clips", "clip_len", "step"):
        for bad in (0, -3):
            a = _args(_lib)
            setattr(a, field, bad)
            assert st(ctypes.byref(a), None) == _lib.ERR_SHAPE, (field, bad)
            assert b"non-positive" in lib.pg_last_error_string()
    a = _args(_lib)
    a.step, a.n_out = 91, 4 * 91 + 184                                              # 2 V = 186 > T
    assert st(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"overlap" in lib.pg_last_error_string()
    a.step, a.n_out = 92, 4 * 92 + 184                                              # 2 V = T: the largest overlap, accepted this far
    a.out_stride = a.n_out - 1
    assert st(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"out_stride" in lib.pg_last_error_string()
    a = _args(_lib)
    a.step, a.n_out = 185, 4 * 185 + 1                                              # step > T: gaps
    assert st(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"step" in lib.pg_last_error_string()
    for n_out in (4 * 120, 4 * 120 + 185, 0, -1):                                   # (n_clips-1) step < n_out <= (n_clips-1) step + T
        a = _args(_lib)
        a.n_out = a.out_stride = n_out
        assert st(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"n_out" in lib.pg_last_error_string(), n_out
    a = _args(_lib)
    a.clip_stride = 183
    assert st(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"clip_stride" in lib.pg_last_error_string()
    a = _args(_lib)
    a.out_stride = a.n_out - 1
    assert st(ctypes.byref(a), None) == _lib.ERR_SHAPE and b"out_stride" in lib.pg_last_error_string()
    for field in ("clips", "out", "ramp"):
        a = _args(_lib)
        setattr(a, field, None)
        assert st(ctypes.byref(a), None) == _lib.ERR_NULL and b"required" in lib.pg_last_error_string(), field
    # normalize / peak / n_nonfinite need the workspace
    for field in ("normalize", "peak", "n_nonfinite"):
        a = _args(_lib)
        setattr(a, field, 1 if field == "normalize" else 4096)
        assert st(ctypes.byref(a), None) == _lib.ERR_WORKSPACE, field
        a.workspace, a.workspace_bytes = 4096, lib.pg_workspace_bytes_stitch(ctypes.byref(a)) - 1
        assert st(ctypes.byref(a), None) == _lib.ERR_WORKSPACE and b"workspace" in lib.pg_last_error_string(), field


def test_workspace_query_and_ramp_errors():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_workspace_bytes_stitch(ctypes.byref(_args(_lib))) > 0
    assert lib.pg_workspace_bytes_stitch(ctypes.byref(_lib.StitchArgs())) == _lib.ERR_SHAPE      # zeroed struct
    assert lib.pg_workspace_bytes_stitch(None) == _lib.ERR_NULL
    assert lib.pg_stitch_ramp(None, 5) == _lib.ERR_NULL
    buf = np.full(8, np.float32(-77.0))
    assert lib.pg_stitch_ramp(buf.ctypes.data_as(ctypes.c_void_p), -1) == _lib.ERR_SHAPE
    assert lib.pg_stitch_ramp(buf.ctypes.data_as(ctypes.c_void_p), 0) == _lib.OK and (buf == -77.0).all()    # writes nothing
    assert lib.pg_stitch_ramp(None, 0) == _lib.OK
    assert lib.pg_stitch_ramp(buf.ctypes.data_as(ctypes.c_void_p), 5) == _lib.OK and (buf[5:] == -77.0).all() and (buf[:5] > 0).all()


@pytest.mark.parametrize("V", [1, 8, 11, 64, 92, 16384])
def test_ramp_is_float32_of_the_float64_formula(V):
    from phasegen import ops
    r = ops.stitch_ramp_host(V)
    assert r.dtype == np.float32 and r.shape == (V,)
    want = np.sin(np.pi * (np.arange(V, dtype=np.float64) + 0.5) / (2.0 * V)) ** 2
    w32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    assert (np.abs(r.astype(np.float64) - want) <= ulp).all(), np.abs(r.astype(np.float64) - want).max()
    assert (r > 0).all() and r.min() >= np.finfo(np.float32).tiny                   # strictly positive NORMAL floats
    assert np.abs((r.astype(np.float64) + r[::-1].astype(np.float64)) - 1.0).max() <= 2.0 ** -23
    assert ops.stitch_ramp_host(0).shape == (0,)


def test_track_plan():
    from phasegen.track import track_plan
    assert track_plan(160000, 128, 512, 32) == (65024, 48640, 3)
    assert track_plan(1000, 24, 8, 8) == (184, 120, 8)
    assert track_plan(1, 24, 8, 8) == (184, 120, 1) and track_plan(184, 24, 8, 8) == (184, 120, 1)
    assert track_plan(185, 24, 8, 8) == (184, 120, 2)
    assert track_plan(184 + 120, 24, 8, 8)[2] == 2 and track_plan(184 + 121, 24, 8, 8)[2] == 3
    assert track_plan(1000, 24, 8, 0) == (184, 184, 6)                              # no overlap: ceil(1000 / 184)
    assert track_plan(1000, 24, 8, 11) == (184, 96, 10)                             # 2 * 11 <= 23: the largest overlap
    for a_len in (1, 100, 184, 185, 1000, 160000):                                  # the stitch contract holds for every plan
        T, step, n = track_plan(a_len, 24, 8, 8)
        assert (n - 1) * step < a_len <= (n - 1) * step + T
    with pytest.raises(ValueError):
        track_plan(1000, 24, 8, 12)                                                 # 2 * 12 > 23
    with pytest.raises(ValueError):
        track_plan(1000, 24, 8, -1)
    with pytest.raises(ValueError):
        track_plan(1000, 100, 8, 8)                                                 # frames the U-Net cannot concatenate
    with pytest.raises(ValueError):
        track_plan(0, 24, 8, 8)


def test_python_surface():
    """Signatures only (the calls need a GPU)."""
    from phasegen import ops, preproc, track
    p = inspect.signature(track.reconstruct_track).parameters
    assert list(p) == ["model", "audio", "n_fft", "hop_length", "frames", "overlap_frames", "stats", "osr", "sr", "res_type",
                       "clip_batch", "phase", "normalize"]
    assert [p[k].default for k in list(p)[2:]] == [2048, 512, 128, 32, None, None, 16000, "kaiser_best", 64, "unet", True]
    assert list(inspect.signature(track.track_plan).parameters) == ["a_len", "frames", "hop_length", "overlap_frames"]
    p = inspect.signature(ops.stitch).parameters
    assert list(p) == ["clips", "step", "n_out", "normalize", "out", "return_status"]
    assert (p["normalize"].default, p["out"].default, p["return_status"].default) == (False, None, False)
    assert list(inspect.signature(ops.stitch_ramp_host).parameters) == ["overlap"]
    assert list(inspect.signature(ops.standardize_with_).parameters) == ["x", "mean", "std"]
    p = inspect.signature(preproc.build_dataset).parameters
    assert p["return_stats"].default is False and list(p)[0] == "tracks"
    assert ops._stitch_ws in ops._caches
