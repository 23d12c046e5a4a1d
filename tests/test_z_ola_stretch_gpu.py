"""GPU: pg_ola_stretch (ops.ola_stretch) BIT FOR BIT against the numpy restatement of its contract (tests/_transient_ref.py: fp32
sums over the covering frames in ascending g) -- signal and output lengths from one sample to several windows, six time ratios,
five window / hop pairs, a table with zero entries (den == 0), with and without ``base``, offset views and row strides (both store
paths), the identity bound at ratio 1, independence of n_out, the cone of a NaN, and the stream contract of the entry point
(tests/test_z_streams_gpu.py counts it as reached).

Bounds.  The kernel performs the contract's fp32 operations in the contract's order (nothing is contracted or reassociated), so
every comparison with the restatement is exact.  The identity bound is the header's: (2 k + 2) 2^-24 |x[t]| for k covering frames."""
import ctypes

import numpy as np
import pytest
import torch

import _transient_ref as tref
from test_z_lock_gpu import offset_view, same_bits

pytestmark = pytest.mark.gpu
N_IN = (1, 2, 255, 256, 1000, 5000)
N_OUT = (1, 3, 255, 1024, 1025, 4100)
RATIOS = (1.0, 0.5, 2.0, 1 / 1.3, 4.0, 0.25)
WINDOWS = ((2, 1), (8, 2), (256, 64), (256, 128), (4096, 1024))


def signal(seed, n_sig, n):
    return (np.random.RandomState(seed).standard_normal((n_sig, n)) * 2.0).astype(np.float32)


def raw(x, n_out, spo, win, hop, base=None):
    """pg_ola_stretch with a window table of the caller's: the wrapper always passes pg_ola_window's"""
    from phasegen import _lib, ops
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(win).cuda()
    bd = None if base is None else torch.from_numpy(base).cuda()
    y = torch.full((x.shape[0], n_out), -77.0, device="cuda")
    a = _lib.OlaStretchArgs()
    a.n_sig, a.win_len, a.hop, a.n_in, a.n_out, a.src_per_out = x.shape[0], win.shape[0], hop, x.shape[1], n_out, spo
    a.x, a.x_stride, a.win, a.y, a.y_stride = xd.data_ptr(), x.shape[1], wd.data_ptr(), y.data_ptr(), n_out
    if bd is not None:
        a.base, a.base_stride = bd.data_ptr(), n_out
    _lib.check(_lib.load().pg_ola_stretch(ctypes.byref(a), ops._stream()), "ola_stretch")
    return y


@pytest.mark.parametrize("w,hop", WINDOWS, ids=lambda v: str(v))
def test_bitwise_against_the_restatement(w, hop):
    from phasegen import ops
    win = tref.ola_window(w)
    for n_in in N_IN:
        x = signal(n_in + w, 2, n_in)
        xd = torch.from_numpy(x).cuda()
        for n_out in N_OUT:
            base = signal(n_out + hop, 2, n_out)
            bd = torch.from_numpy(base).cuda()
            for spo in RATIOS:
                got = ops.ola_stretch(xd, n_out, spo, w, hop)
                assert tuple(got.shape) == (2, n_out) and got.dtype == torch.float32
                assert same_bits(got, tref.ola_stretch(x, n_out, spo, win, hop)), (n_in, n_out, spo)
                assert same_bits(ops.ola_stretch(xd, n_out, spo, w, hop, base=bd), tref.ola_stretch(x, n_out, spo, win, hop, base=base)), (n_in, n_out, spo, "base")


def test_a_table_with_zero_entries():
    """den == 0 where every covering frame has a zero weight: r = 0 there, with and without base.  The entries j = 0, hop, 2 hop, ...
    are zero, so the samples t with (t + w / 2) % hop == 0 see nothing but zero weights; a third of the others are zero too."""
    rs = np.random.RandomState(3)
    for w, hop in ((8, 4), (16, 3), (256, 64)):
        win = rs.uniform(0.0, 1.0, w).astype(np.float32)
        win[rs.rand(w) < 0.33] = 0.0
        win[::hop] = 0.0
        x, base = signal(w, 2, 700), signal(w + 1, 2, 900)
        dead = tref.ola_stretch(np.ones((1, 900), np.float32), 900, 1.0, win, hop)[0] == 0     # (ratio 1 reads x[t] = 1: zero iff den == 0)
        assert dead[(np.arange(900) + w // 2) % hop == 0].all() and not dead.all()
        for spo in (1.0, 1 / 1.3, 2.0):
            want = tref.ola_stretch(x, 900, spo, win, hop)
            assert not want[:, dead].any()
            assert same_bits(raw(x, 900, spo, win, hop), want), (w, hop, spo)
            assert same_bits(raw(x, 900, spo, win, hop, base), tref.ola_stretch(x, 900, spo, win, hop, base=base)), (w, hop, spo)
    zero = np.zeros(8, np.float32)                                                          # an all-zero table: the output is `base` + 0
    assert not bool(raw(x, 50, 1.0, zero, 2).view(torch.int32).any())


@pytest.mark.parametrize("n_out", [1024, 1023, 1025, 7])
def test_offset_views_and_row_strides_give_the_same_bits(n_out):
    """16-byte stores need y on the grid and a row stride that is a multiple of 4; everything else goes sample by sample"""
    from phasegen import ops
    x, base = signal(1, 3, 900), signal(2, 3, n_out)
    want = tref.ola_stretch(x, n_out, 1 / 1.3, tref.ola_window(256), 64, base=base)
    xd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(base).cuda()
    assert same_bits(ops.ola_stretch(xd, n_out, 1 / 1.3, base=bd), want)
    y = offset_view(torch.full((3, n_out), -77.0, device="cuda"))
    assert ops.ola_stretch(offset_view(xd), n_out, 1 / 1.3, base=offset_view(bd), out=y) is y and same_bits(y, want)
    for pitch in (n_out + 1, n_out + 4, n_out + 6):                                         # rows of out, x and base further apart
        big, bx, bb = (torch.full((3, p), -77.0, device="cuda") for p in (pitch, 900 + 3, pitch + 1))
        bx[:, :900], bb[:, :n_out] = xd, bd
        got = ops.ola_stretch(bx[:, :900], n_out, 1 / 1.3, base=bb[:, :n_out], out=big[:, :n_out])
        assert same_bits(got, want) and bool((big[:, n_out:] == -77.0).all()), pitch
    one = ops.ola_stretch(xd[1], n_out, 1 / 1.3, base=bd[1])                                # a 1-D signal
    assert tuple(one.shape) == (n_out,) and same_bits(one, want[1])


def test_rows_do_not_depend_on_n_sig_or_position():
    from phasegen import ops
    x = signal(4, 5, 1200)
    want = tref.ola_stretch(x, 1700, 1 / 1.4, tref.ola_window(256), 64)
    xd = torch.from_numpy(x).cuda()
    for n in (1, 2, 5):
        assert same_bits(ops.ola_stretch(xd[:n], 1700, 1 / 1.4), want[:n])
    for r in range(5):
        assert same_bits(ops.ola_stretch(xd[r:r + 1], 1700, 1 / 1.4)[0], want[r])
    assert same_bits(ops.ola_stretch(xd.flip(0).contiguous(), 1700, 1 / 1.4), want[::-1])


@pytest.mark.parametrize("w,hop", [(256, 64), (256, 128), (8, 2), (64, 7)])
def test_identity_bound_at_ratio_one(w, hop):
    from phasegen import ops
    x = signal(w + hop, 2, 3000)
    y = ops.ola_stretch(torch.from_numpy(x).cuda(), 3000, 1.0, w, hop).cpu().numpy()
    g_lo, g_hi = tref.ola_frames(3000, w, hop)
    k = (g_hi - g_lo + 1).astype(np.float64)
    err = np.abs(y.astype(np.float64) - x)
    den = tref.ola_stretch(np.ones((1, 3000), np.float32), 3000, 1.0, tref.ola_window(w), hop)[0] > 0
    print(f"\n{w} / {hop}: max |y - x| / |x| = {(err[:, den] / np.abs(x[:, den])).max() * 2 ** 24:.2f} x 2^-24 (bound {2 * k.max() + 2:.0f})")
    assert (err[:, den] <= ((2 * k + 2) * 2.0 ** -24 * np.abs(x.astype(np.float64)))[:, den]).all()
    assert not y[:, ~den].any()


def test_a_sample_does_not_depend_on_n_out():
    from phasegen import ops
    xd = torch.from_numpy(signal(6, 2, 2000)).cuda()
    for spo in RATIOS:
        a, b = ops.ola_stretch(xd, 1001, spo), ops.ola_stretch(xd, 3000, spo)
        assert same_bits(a, b[:, :1001]), spo


def test_a_nan_reaches_exactly_the_restatements_cone():
    from phasegen import ops
    x = signal(7, 1, 1000)
    win = tref.ola_window(256)
    clean, reads = tref.ola_stretch(x, 1300, 1 / 1.3, win, 64, return_reads=True)
    cone = np.array([500 in r for r in reads])
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[0, 500] = bad
        got = ops.ola_stretch(torch.from_numpy(xb).cuda(), 1300, 1 / 1.3).cpu().numpy()
        assert same_bits(got, tref.ola_stretch(xb, 1300, 1 / 1.3, win, 64))
        assert np.array_equal(~np.isfinite(got[0]), cone) and 0 < cone.sum() < 500, bad       # R1: nothing swallowed
        assert same_bits(got[0, ~cone], clean[0, ~cone])                                       # R2: nothing spreads


def ola_case():
    import test_z_workspace_gpu as W
    from phasegen import ops
    ins = {"x": W.cuda(signal(8, 2, 1000)), "base": W.cuda(signal(9, 2, 1500))}
    return W.Case("ola_stretch", ins, lambda: {"y": W.sent(2, 1500)}, lambda i, o: [ops.ola_stretch(i["x"], 1500, 1 / 1.5, base=i["base"], out=o["y"])],
                  symbol="pg_ola_stretch", needs_ws=False)


def test_the_stream_contract():
    """pg_ola_stretch on a busy side stream: the same bits, no wait for the device, nothing on another stream, no workspace."""
    import test_z_streams_gpu as S
    from _strict import strict_workspaces
    case = ola_case()
    with strict_workspaces(0xFF) as s:
        got = case.run(case.ins, case.make_outs())
    assert s.requests == [] and "pg_ola_stretch" in s.symbols()
    assert same_bits(got[0], tref.ola_stretch(case.ins["x"].cpu().numpy(), 1500, 1 / 1.5, tref.ola_window(256), 64, base=case.ins["base"].cpu().numpy()))
    S.reach(case)
    assert "pg_ola_stretch" in S.REACHED


def test_argument_errors():
    from phasegen import _lib, ops
    x = torch.zeros(2, 100, device="cuda")
    for bad in (dict(n_out=0), dict(src_per_out=0.0), dict(src_per_out=float("nan")), dict(src_per_out=float("inf")), dict(win_len=255), dict(win_len=0),
                dict(win_len=4098), dict(hop=0), dict(hop=129), dict(base=torch.zeros(2, 149, device="cuda")), dict(base=torch.zeros(2, 150)),
                dict(out=torch.zeros(2, 151, device="cuda")), dict(out=torch.zeros(2, 300, device="cuda")[:, ::2])):
        with pytest.raises(ValueError):
            ops.ola_stretch(**{**dict(x=x, n_out=150), **bad})
    for view in (x[:, ::2], x.double(), x.cpu(), x[None], x.t()):
        with pytest.raises(ValueError):
            ops.ola_stretch(view, 150)
    # real pointers, a bad hop: refused before any launch, nothing written
    lib = _lib.load()
    y = torch.full((2, 150), 7.0, device="cuda")
    win = torch.zeros(256, device="cuda")
    a = _lib.OlaStretchArgs()
    a.n_sig, a.win_len, a.hop, a.n_in, a.n_out, a.src_per_out = 2, 256, 129, 100, 150, 1.0
    a.x, a.x_stride, a.win, a.y, a.y_stride = x.data_ptr(), 100, win.data_ptr(), y.data_ptr(), 150
    assert lib.pg_ola_stretch(ctypes.byref(a), None) == _lib.ERR_SHAPE
    a.hop, a.y_stride = 64, 149
    assert lib.pg_ola_stretch(ctypes.byref(a), None) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
