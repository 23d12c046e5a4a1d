"""GPU: pg_hpss (ops.hpss) BIT FOR BIT against the numpy restatement of its contract (tests/_transient_ref.py: medians by sorting
the keys) -- every window size, planes smaller and larger than any halo and on both sides of the 32 x 64 tile edge, more tiles than
workgroups, ties, -0, infinities and NaNs of both signs, both store paths, strided channel views, and the stream contract of the
entry point (tests/test_z_streams_gpu.py counts it as reached).

Bounds.  The kernel selects among bit patterns and copies them: every comparison with the restatement is exact."""
import ctypes

import numpy as np
import pytest
import torch

import _transient_ref as tref
from test_z_lock_gpu import offset_view, same_bits

pytestmark = pytest.mark.gpu
BINS = (1, 2, 16, 17, 63, 64, 65, 130)
FRAMES = (1, 3, 31, 64, 65, 257)
WINDOWS = ((1, 1), (3, 5), (17, 17), (31, 31), (1, 31), (31, 1))
SPECIALS = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x00000000], np.uint32).view(np.float32)


def uniform(seed, shape):
    return np.random.RandomState(seed).uniform(0.0, 3.0, shape).astype(np.float32)


def levels(seed, shape):
    """quantised to 4 levels: windows full of ties"""
    return (np.random.RandomState(seed).randint(0, 4, shape) * np.float32(0.5)).astype(np.float32)


def planted(seed, shape):
    """uniform, with -0, +-inf and NaNs of both signs (and two payloads) in a tenth of the cells"""
    rs = np.random.RandomState(seed)
    M = rs.uniform(0.0, 3.0, shape).astype(np.float32)
    flat = M.reshape(-1)
    at = rs.choice(flat.size, size=min(flat.size, max(8, flat.size // 10)), replace=False)
    flat[at] = SPECIALS[np.arange(at.size) % SPECIALS.size]
    return M


def run(M, win_t, win_f, **kw):
    from phasegen import ops
    return ops.hpss(torch.from_numpy(M).cuda(), win_t, win_f, **kw)


def check(M, win_t, win_f, tag):
    harm, perc = run(M, win_t, win_f)
    wh, wp = tref.hpss(M, win_t, win_f)
    assert tuple(harm.shape) == tuple(perc.shape) == M.shape and harm.dtype == perc.dtype == torch.float32
    assert same_bits(harm, wh) and same_bits(perc, wp), tag
    return harm, perc


@pytest.mark.parametrize("wins", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_bitwise_against_the_restatement(wins):
    for bins in BINS:
        for F in FRAMES:
            for make in (uniform, levels, planted):
                check(make(bins * 1000 + F, (2, bins, F)), *wins, (bins, F, make.__name__))


@pytest.mark.parametrize("win", range(1, 32, 2))
def test_every_window_size(win):
    """each of the 16 selection networks, along time and along frequency, on a plane with ties and specials"""
    for M in (planted(win, (1, 37, 70)), levels(win, (1, 37, 70))):
        check(M, win, 1, win)
        check(M, 1, win, win)
        check(M, win, 32 - win if win != 1 else 31, win)


def test_more_tiles_than_workgroups():
    """3 x 2 x 350 = 2100 tiles; a launch has at most 2048 workgroups, so some walk a second tile"""
    from phasegen import _lib  # noqa: F401
    M = levels(77, (3, 33, 64 * 350))
    M[:, :, ::7] = uniform(78, (3, 33, 3200))
    harm, perc = check(M, 3, 5, "tiles")
    assert bool((perc != 0).any()) and bool((harm != 0).any())


def test_partition_on_the_device_output():
    for M, wins in ((planted(5, (2, 65, 130)), (17, 17)), (levels(6, (2, 65, 130)), (31, 3)), (uniform(7, (1, 130, 65)), (5, 31))):
        harm, perc = run(M, *wins)
        hb, pb, mb = (t.cpu().numpy().view(np.uint32) for t in (harm, perc, torch.from_numpy(M)))
        assert (((hb == mb) & (pb == 0)) | ((pb == mb) & (hb == 0))).all()
        assert np.array_equal(np.where(hb != 0, hb, pb), mb)
        assert 0.05 < float(((pb == mb) & (mb != 0)).mean()) < 0.95                 # both planes get their share


def test_all_harmonic_cases():
    M = planted(8, (2, 40, 70))
    harm, perc = run(M, 1, 1)
    assert same_bits(harm, M) and not bool(perc.view(torch.int32).any())
    rows = np.ascontiguousarray(np.repeat(planted(9, (2, 40, 1)), 70, axis=2))
    cols = np.ascontiguousarray(np.repeat(planted(10, (2, 1, 70)), 40, axis=1))
    for w in (3, 17, 31):
        harm, perc = run(rows, w, 1)
        assert same_bits(harm, rows) and not bool(perc.view(torch.int32).any()), w
        harm, perc = run(cols, 1, w)
        assert same_bits(harm, cols) and not bool(perc.view(torch.int32).any()), w


@pytest.mark.parametrize("F", [64, 65, 66, 67, 3])
def test_both_store_paths_give_the_same_bits(F):
    """16-byte stores need aligned outputs and F % 4 == 0; a view one element off the grid and every other F take the scalar path"""
    from phasegen import ops
    M = planted(F, (2, 33, F))
    wh, wp = tref.hpss(M, 17, 5)
    Md = torch.from_numpy(M).cuda()
    harm, perc = ops.hpss(Md, 17, 5)
    assert same_bits(harm, wh) and same_bits(perc, wp)
    oh, op = offset_view(torch.full_like(harm, -77.0)), offset_view(torch.full_like(perc, -77.0))
    got = ops.hpss(offset_view(Md), 17, 5, out=(oh, op))
    assert got[0] is oh and got[1] is op and same_bits(oh, wh) and same_bits(op, wp)
    got = ops.hpss(Md, 17, 5, out=(oh, torch.full_like(perc, -77.0)))               # one of the two off the grid
    assert same_bits(got[0], wh) and same_bits(got[1], wp)


def test_strided_channel_view_and_independence_of_n_ch_and_position():
    from phasegen import ops
    pol = torch.from_numpy(planted(11, (5, 2, 21, 70))).cuda()                      # a polar tensor: pol[:, 0] is read in place
    M = pol[:, 0]
    assert not M.is_contiguous()
    want = tref.hpss(M.cpu().numpy(), 17, 17)
    for n_ch in (1, 2, 3, 5):
        harm, perc = ops.hpss(M[:n_ch], 17, 17)
        assert same_bits(harm, want[0][:n_ch]) and same_bits(perc, want[1][:n_ch]), n_ch
    for c in range(5):
        harm, perc = ops.hpss(M[c:c + 1], 17, 17)
        assert same_bits(harm[0], want[0][c]) and same_bits(perc[0], want[1][c]), c
    harm, perc = ops.hpss(M.flip(0).contiguous(), 17, 17)
    assert same_bits(harm, want[0][::-1]) and same_bits(perc, want[1][::-1])
    sub = ops.hpss(pol[1:4, 1], 3, 31)                                              # the other plane, inner channels
    assert same_bits(sub[0], tref.hpss(pol[1:4, 1].cpu().numpy(), 3, 31)[0])


def hpss_case():
    import test_z_workspace_gpu as W
    from phasegen import ops

    def run_case(i, o):
        ops.hpss(i["M"], 17, 5, out=(o["harm"], o["perc"]))
        return [o["harm"], o["perc"]]

    return W.Case("hpss", {"M": W.cuda(uniform(12, (2, 33, 70)))}, lambda: {"harm": W.sent(2, 33, 70), "perc": W.sent(2, 33, 70)}, run_case,
                  symbol="pg_hpss", needs_ws=False)


def test_the_stream_contract():
    """pg_hpss on a busy side stream: the same bits, no wait for the device, nothing on another stream, and no workspace asked for."""
    import test_z_streams_gpu as S
    from _strict import strict_workspaces
    case = hpss_case()
    with strict_workspaces(0xFF) as s:
        got = case.run(case.ins, case.make_outs())
    assert s.requests == [] and "pg_hpss" in s.symbols()
    want = tref.hpss(case.ins["M"].cpu().numpy(), 17, 5)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    S.reach(case)
    assert "pg_hpss" in S.REACHED


def test_argument_errors():
    from phasegen import _lib, ops
    M = torch.zeros(2, 5, 19, device="cuda")
    for bad in (dict(win_t=0), dict(win_t=2), dict(win_f=16), dict(win_t=33), dict(win_f=-1), dict(out=torch.zeros(2, 5, 19, device="cuda")),
                dict(out=(torch.zeros(2, 5, 19, device="cuda"), torch.zeros(2, 5, 18, device="cuda")))):
        with pytest.raises(ValueError):
            ops.hpss(**{**dict(logmag=M), **bad})
    for view in (M[:, :, ::2], M.transpose(1, 2), M.double(), M[0], M.cpu()):
        with pytest.raises(ValueError):
            ops.hpss(view)
    # real pointers, a bad window: refused before any launch, nothing written
    lib = _lib.load()
    harm, perc = torch.full((2, 5, 19), 7.0, device="cuda"), torch.full((2, 5, 19), 7.0, device="cuda")
    a = _lib.HpssArgs()
    a.n_ch, a.bins, a.F, a.win_t, a.win_f = 2, 5, 19, 17, 18
    a.M, a.m_stride, a.harm, a.perc = M.data_ptr(), 95, harm.data_ptr(), perc.data_ptr()
    assert lib.pg_hpss(ctypes.byref(a), None) == _lib.ERR_SHAPE
    a.win_f, a.m_stride = 17, 94
    assert lib.pg_hpss(ctypes.byref(a), None) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((harm == 7.0).all()) and bool((perc == 7.0).all())
