"""CPU: pg_clipnorm_fwd (BatchNorm forward with per-clip statistics) is exported and bound, its argument struct has the layout
include/phasegen.h declares, and its argument validation runs on the host before any launch.  An additive change within ABI 0.4:
pg_version() and pg_bn_args are what they were."""
import ctypes

import pytest


def test_clipnorm_is_exported_and_bound():
    from phasegen import _lib
    lib = _lib.load()
    assert hasattr(lib, "pg_clipnorm_fwd") and hasattr(lib, "pg_workspace_bytes_clipnorm")
    assert "pg_clipnorm_fwd" in _lib.SYMBOLS and "pg_workspace_bytes_clipnorm" in _lib.SYMBOLS
    assert lib.pg_version() == 400
    assert ctypes.sizeof(_lib.BnArgs) == 232                       # pg_bn_args untouched


def test_clipnorm_args_layout():
    """Layout by hand from the header: B, C, L, eps, momentum, _pad0 (6 x 4) | x, x_bs | y, y_bs, y2, y2_bs | y_act, y2_act (2 x 4) |
    yh, yh_bs, yh_pitch, yh_act | yh2, yh2_bs, yh2_pitch, yh2_act | gamma, beta | save_mean, save_invstd | running_mean, running_var |
    num_batches_tracked | workspace, workspace_bytes."""
    from phasegen import _lib
    A = _lib.ClipNormArgs
    size = 6 * 4 + 2 * 8 + 4 * 8 + 2 * 4 + (8 + 8 + 4 + 4) + (8 + 8 + 4 + 4) + 2 * 8 + 2 * 8 + 2 * 8 + 8 + 2 * 8
    assert size == 200 and ctypes.sizeof(A) == size
    assert A.x.offset == 24 and A.y.offset == 40 and A.y2.offset == 56 and A.y_act.offset == 72 and A.y2_act.offset == 76
    assert A.yh.offset == 80 and A.yh_pitch.offset == 96 and A.yh_act.offset == 100
    assert A.yh2.offset == 104 and A.yh2_pitch.offset == 120 and A.yh2_act.offset == 124
    assert A.gamma.offset == 128 and A.beta.offset == 136 and A.save_mean.offset == 144 and A.save_invstd.offset == 152
    assert A.running_mean.offset == 160 and A.running_var.offset == 168 and A.num_batches_tracked.offset == 176
    assert A.workspace.offset == 184 and A.workspace_bytes.offset == 192


def _args(_lib):
    a = _lib.ClipNormArgs()
    a.B, a.C, a.L = 3, 8, 29
    a.eps, a.momentum = 1e-5, 0.1
    a.x = a.y = a.gamma = a.beta = 4096                            # never dereferenced: every call below fails before a launch
    a.x_bs = a.y_bs = 8 * 29
    return a


def test_clipnorm_argument_errors_are_reported_before_any_launch():
    from phasegen import _lib
    lib = _lib.load()
    fwd = lib.pg_clipnorm_fwd
    assert fwd(None, None) == _lib.ERR_NULL
    for dim in ("B", "C", "L"):
        a = _args(_lib)
        setattr(a, dim, 0)
        assert fwd(ctypes.byref(a), None) == _lib.ERR_SHAPE, dim
        assert b"non-positive" in lib.pg_last_error_string()
        setattr(a, dim, -4)
        assert fwd(ctypes.byref(a), None) == _lib.ERR_SHAPE, dim
    for field in ("x", "y", "gamma", "beta"):                      # y is the only output here: missing outputs
        a = _args(_lib)
        setattr(a, field, None)
        assert fwd(ctypes.byref(a), None) == _lib.ERR_NULL, field
        assert b"required" in lib.pg_last_error_string()
    a = _args(_lib)                                                # y2 alone is not an output set either
    a.y, a.y2, a.y2_bs = None, 4096, 8 * 29
    assert fwd(ctypes.byref(a), None) == _lib.ERR_NULL
    for which in ("yh", "yh2"):
        a = _args(_lib)
        setattr(a, which, 4096)
        setattr(a, which + "_bs", 8 * 28)
        setattr(a, which + "_pitch", 28)                           # below L = 29
        assert fwd(ctypes.byref(a), None) == _lib.ERR_SHAPE, which
        assert b"pitch" in lib.pg_last_error_string()
    # running buffers need the workspace of the second launch
    a = _args(_lib)
    a.running_mean = a.running_var = 4096
    assert lib.pg_workspace_bytes_clipnorm(ctypes.byref(a)) == 2 * 3 * 8 * 4
    assert fwd(ctypes.byref(a), None) == _lib.ERR_WORKSPACE
    a.workspace, a.workspace_bytes = 4096, 2 * 3 * 8 * 4 - 1
    assert fwd(ctypes.byref(a), None) == _lib.ERR_WORKSPACE
    z = _lib.ClipNormArgs()
    assert lib.pg_workspace_bytes_clipnorm(ctypes.byref(z)) == _lib.ERR_SHAPE


def test_engine_surface_has_the_statistics_mode():
    """Signatures only (constructing an engine needs a GPU)."""
    import inspect
    from phasegen import ops
    from phasegen.model import UNetModel
    from phasegen.unet import UNetEngine
    from phasegen.validate import validation_metrics
    assert inspect.signature(UNetEngine.forward).parameters["stats"].default == "batch"
    assert inspect.signature(UNetModel.forward).parameters["per_clip"].default is False
    p = inspect.signature(validation_metrics).parameters
    assert p["batched"].default is False and p["clip_batch"].default == 64
    p = inspect.signature(ops.clipnorm_fwd).parameters
    assert [k for k in p][:4] == ["x", "y", "gamma", "beta"] and p["save_mean"].default is None and p["running_mean"].default is None
