"""GPU: tempo maps -- the five mapped entry points (pg_spec_clips_map, pg_phase_vocoder_map, pg_phase_lock_map,
pg_phase_lock_linked_map, pg_ola_stretch_map) BIT FOR BIT against their uniform twins on uniform tables and against the numpy
restatement of their contract (tests/_map_ref.py) on real ones, at the chunk boundaries of each kernel, with hostile tables, under the
workspace and stream contracts, and the track level built on them (phasegen.track.TimeMap as ``stretch``, reconstruct.py --tempo_map).

Bounds.  A position is read from the table, clamped by two comparisons and floored; from there on every kernel does what its twin does:
fp32 sums in a fixed order, integer sums modulo 2^32, plain IEEE comparisons.  Every comparison here is therefore exact.

The module is named to be collected before tests/test_z_streams_gpu.py and tests/test_z_workspace_gpu.py, whose completeness tests count
an entry point as reached only through ``S.reach`` / ``W.check`` called from here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _link_ref as kref
import _map_ref as mref
import _transient_ref as tref
import _vocoder_ref as ref
from phasegen import detgen
from test_z_lock_gpu import offset_view, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)
SPOS = [1.0, 0.5, 2.0, 1 / 1.3, 4.0, 0.25]
NAN, INF = float("nan"), float("inf")
FLOOR = 0.5
# the shapes of the issue: spec_clips 2 ch x 5 bins, F_src 23, 3 clips of 8 frames, sf 5; vocoder 2 x 3 rows, F_out 1029 (crosses the
# 1024-frame chunk), F_src 700; lock and linked F_out 70 (crosses two 32-frame chunks), n_ch 2; overlap-add (256, 64) and (8, 2)
SC = dict(n_ch=2, bins=5, F_src=23, n_clips=3, frames=8, sf=5)
SC_N = (SC["n_clips"] - 1) * SC["sf"] + SC["frames"]
PV = dict(n_ch=2, bins=3, F_out=1029, F_src=700)
LK_F_OUT, LK_F_SRC = 70, 90
LK_BINS = [1, 5, 65, 130, 1100]
OLA = [(256, 64), (8, 2)]
OLA_N_OUT = [1025, 7]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def planes(seed, n_ch, bins, F_src):
    rs = np.random.RandomState(seed)
    A = rs.uniform(-np.pi, np.pi, (n_ch, bins, F_src)).astype(np.float32)
    M = rs.uniform(0.0, 1.0, (n_ch, bins, F_src)).astype(np.float32)
    return A, M


@pytest.fixture(scope="module")
def data():
    """every input of the kernel tests, made once and left unchanged"""
    d = {"sc": planes(1, SC["n_ch"], SC["bins"], SC["F_src"])[1], "pv": planes(2, PV["n_ch"], PV["bins"], PV["F_src"])}
    for bins in LK_BINS + [1024]:
        A, M = planes(10 + bins, 2, bins, LK_F_SRC)
        Ar, Mr = planes(20 + bins, 1, bins, LK_F_SRC)
        d["lk", bins] = (A, M, Ar[0], Mr[0])
    d["ola"] = np.random.RandomState(3).standard_normal((2, 1500)).astype(np.float32)
    return d


# ---- tables ------------------------------------------------------------------------------------------------------------------

def uniform(n, spo):
    return np.arange(n, dtype=np.float64) * spo


def two_slope(n, gb):
    """stretch 0.5 (two source frames per output frame) up to frame gb, stretch 2 from there"""
    g = np.arange(n, dtype=np.float64)
    return np.where(g <= gb, g * 2.0, gb * 2.0 + (g - gb) * 0.5)


def ramp(n, F_src):
    return (F_src - 1.5) * (np.arange(n, dtype=np.float64) / (n - 1)) ** 1.3


def wild(n, jump=12.6):
    """a freeze (equal neighbours), a backward step and a jump wider than the staged window (8 source frames at 1024 bins)"""
    p = np.arange(n, dtype=np.float64) * 0.75
    a, b, c = n // 4, n // 2, 3 * n // 4
    p[a:a + 4] = p[a]
    p[b:] -= 3.3
    p[c:] += jump
    return p


def beyond(n, F_src):
    return np.arange(n, dtype=np.float64) * ((F_src + 5.0) / (n - 1))


def real_maps(n, F_src, gb):
    return {"two_slope": two_slope(n, gb), "ramp": ramp(n, F_src), "wild": wild(n), "beyond": beyond(n, F_src)}


def hostile(n, F_src):
    p = ramp(n, F_src)
    for at, v in zip(np.linspace(1, n - 1, 8).astype(int), (NAN, -1.0, INF, 1e300, -INF, -0.0, 2.0 ** 52 + 2.0, 5e-324)):
        p[at] = v
    return p


def grain_table(n_out, w, hop, kind):
    n = mref.n_grains(n_out, w, hop)
    g = np.arange(n, dtype=np.float64) * hop
    if kind == "two_slope":
        return two_slope(n, n // 3) * hop
    if kind == "ramp":
        return g ** 1.1
    if kind == "wild":
        return wild(n, 400.3) * hop
    if kind == "beyond":
        return g * (1700.0 / max(g[-1], 1.0))
    assert kind == "hostile"
    p = g * 0.9 + 0.5                                                      # (x.5: rint rounds half to even)
    for at, v in zip(np.linspace(0, n - 1, 8).astype(int), (NAN, -1.0, INF, 1e300, -INF, -1e300, 2.0 ** 62, -(2.0 ** 62))):
        p[at] = v
    return p


# ---- the five calls, uniform twin and mapped ------------------------------------------------------------------------------------

def sc_run(P, spo=None, pos=None, **kw):
    from phasegen import ops
    grid = dict(src_per_out=spo) if pos is None else dict(pos=dev(pos) if isinstance(pos, np.ndarray) else pos)
    return ops.spec_clips(P if torch.is_tensor(P) else dev(P), SC["n_clips"], SC["frames"], SC["sf"], **grid, **kw)


def pv_run(A, M, F_out, spo=None, pos=None, **kw):
    from phasegen import ops
    grid = dict(src_per_out=spo) if pos is None else dict(pos=dev(pos) if isinstance(pos, np.ndarray) else pos)
    return ops.phase_vocoder(A if torch.is_tensor(A) else dev(A), F_out, logmag=None if M is None else (M if torch.is_tensor(M) else dev(M)),
                             reset_below=FLOOR, **grid, **kw)


def lk_run(A, M, F_out, spo=None, pos=None, **kw):
    from phasegen import ops
    grid = dict(src_per_out=spo) if pos is None else dict(pos=dev(pos) if isinstance(pos, np.ndarray) else pos)
    return ops.phase_lock(A if torch.is_tensor(A) else dev(A), F_out, logmag=M if torch.is_tensor(M) else dev(M), reset_below=FLOOR, **grid, **kw)


def ln_run(A, Ar, Mr, F_out, spo=None, pos=None, **kw):
    from phasegen import ops
    grid = dict(src_per_out=spo) if pos is None else dict(pos=dev(pos) if isinstance(pos, np.ndarray) else pos)
    t = lambda v: v if torch.is_tensor(v) else dev(v)
    return ops.phase_lock_linked(t(A), t(Ar), t(Mr), F_out, reset_below=FLOOR, **grid, **kw)


def ol_run(x, n_out, w, hop, spo=None, pos=None, **kw):
    from phasegen import ops
    grid = dict(src_per_out=spo) if pos is None else dict(pos=dev(pos) if isinstance(pos, np.ndarray) else pos)
    return ops.ola_stretch(x if torch.is_tensor(x) else dev(x), n_out, win_len=w, hop=hop, **grid, **kw)


# ---- uniform tables: the bits of the uniform twin ---------------------------------------------------------------------------------

@pytest.mark.parametrize("spo", SPOS)
def test_a_uniform_table_gives_the_bits_of_the_uniform_twin(data, spo):
    P = data["sc"]
    assert same_bits(sc_run(P, pos=uniform(SC_N, spo)), sc_run(P, spo)), "spec_clips"
    A, M = data["pv"]
    for m in (M, None):
        assert same_bits(pv_run(A, m, PV["F_out"], pos=uniform(PV["F_out"], spo)), pv_run(A, m, PV["F_out"], spo)), "vocoder"
    for bins in LK_BINS:
        A, M, Ar, Mr = data["lk", bins]
        pos = uniform(LK_F_OUT, spo)
        assert same_bits(lk_run(A, M, LK_F_OUT, pos=pos), lk_run(A, M, LK_F_OUT, spo)), ("lock", bins)
        assert same_bits(ln_run(A, Ar, Mr, LK_F_OUT, pos=pos), ln_run(A, Ar, Mr, LK_F_OUT, spo)), ("linked", bins)
    x = data["ola"]
    for w, hop in OLA:
        for n_out in OLA_N_OUT:
            c = (np.arange(mref.n_grains(n_out, w, hop), dtype=np.int64) * hop).astype(np.float64) * spo
            base = dev(x[:, :n_out] * np.float32(0.5))
            assert same_bits(ol_run(x, n_out, w, hop, pos=c), ol_run(x, n_out, w, hop, spo)), ("ola", w, hop, n_out)
            assert same_bits(ol_run(x, n_out, w, hop, pos=c, base=base), ol_run(x, n_out, w, hop, spo, base=base)), ("ola+base", w, hop, n_out)


# ---- real tables: bit for bit against the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["two_slope", "ramp", "wild", "beyond"])
def test_spec_clips_and_vocoder_against_the_restatement(data, kind):
    P = data["sc"]
    pos = real_maps(SC_N, SC["F_src"], 7)[kind]
    want = mref.spec_clips_map(P, SC["n_clips"], SC["frames"], SC["sf"], pos)
    assert same_bits(sc_run(P, pos=pos), want)
    A, M = data["pv"]
    pos = real_maps(PV["F_out"], PV["F_src"], 100)[kind]
    if kind != "wild":
        assert pos.max() > PV["F_src"] // 2                                  # the table spans the plane
    for m in (M, None):
        assert same_bits(pv_run(A, m, PV["F_out"], pos=pos), mref.phase_vocoder_map(A, pos, m, FLOOR)), (kind, m is None)


@pytest.mark.parametrize("bins", LK_BINS)
def test_lock_and_linked_against_the_restatement(data, bins):
    A, M, Ar, Mr = data["lk", bins]
    for kind, pos in real_maps(LK_F_OUT, LK_F_SRC, 21).items():
        want, T = mref.phase_lock_map(A, pos, M, FLOOR, return_rotation=True)
        assert T.any()
        assert same_bits(lk_run(A, M, LK_F_OUT, pos=pos), want), (kind, bins)
        assert same_bits(ln_run(A, Ar, Mr, LK_F_OUT, pos=pos), mref.phase_lock_linked_map(A, Ar, Mr, pos, FLOOR)), (kind, bins)


def test_a_jump_wider_than_the_staged_window(data):
    """bins 1024 stages 8 source frames: the table's jump of 12.6 frames reads the rows, its backward step reloads the window"""
    A, M, Ar, Mr = data["lk", 1024]
    pos = wild(40)
    i0, _, _ = mref.positions(pos, LK_F_SRC)
    assert np.abs(np.diff(i0)).max() >= 9 and (np.diff(i0) < 0).any() and (np.diff(pos) == 0).any()
    assert same_bits(lk_run(A, M, 40, pos=pos), mref.phase_lock_map(A, pos, M, FLOOR))
    assert same_bits(ln_run(A, Ar, Mr, 40, pos=pos), mref.phase_lock_linked_map(A, Ar, Mr, pos, FLOOR))


@pytest.mark.parametrize("kind", ["two_slope", "ramp", "wild", "beyond", "hostile"])
def test_overlap_add_against_the_restatement(data, kind):
    x = data["ola"]
    for w, hop in OLA:
        win = tref.ola_window(w)
        for n_out in OLA_N_OUT:
            c = grain_table(n_out, w, hop, kind)
            base = x[:, 100:100 + n_out] * np.float32(0.25)
            assert same_bits(ol_run(x, n_out, w, hop, pos=c), mref.ola_stretch_map(x, n_out, c, win, hop)), (kind, w, hop, n_out)
            assert same_bits(ol_run(x, n_out, w, hop, pos=c, base=dev(base)), mref.ola_stretch_map(x, n_out, c, win, hop, base=base)), (kind, w, n_out)


# ---- the prefix property ----------------------------------------------------------------------------------------------------------

def test_the_frames_before_the_first_break_have_the_uniform_bits(data):
    P = data["sc"]
    gb = 7
    got, uni = sc_run(P, pos=two_slope(SC_N, gb)).cpu(), sc_run(P, 2.0).cpu()
    for k in range(SC["n_clips"]):
        for f in range(SC["frames"]):
            if k * SC["sf"] + f <= gb:
                assert same_bits(got[k, :, :, f], uni[k, :, :, f]), (k, f)
    assert not same_bits(got, uni)
    A, M = data["pv"]
    gb = 100
    got, uni = pv_run(A, M, PV["F_out"], pos=two_slope(PV["F_out"], gb)), pv_run(A, M, PV["F_out"], 2.0)
    assert same_bits(got[..., :gb + 1], uni[..., :gb + 1]) and not same_bits(got, uni)
    A, M, Ar, Mr = data["lk", 130]
    gb = 21
    pos = two_slope(LK_F_OUT, gb)
    got, uni = lk_run(A, M, LK_F_OUT, pos=pos), lk_run(A, M, LK_F_OUT, 2.0)
    assert same_bits(got[..., :gb + 1], uni[..., :gb + 1]) and not same_bits(got, uni)
    got, uni = ln_run(A, Ar, Mr, LK_F_OUT, pos=pos), ln_run(A, Ar, Mr, LK_F_OUT, 2.0)
    assert same_bits(got[..., :gb + 1], uni[..., :gb + 1]) and not same_bits(got, uni)


# ---- linked exactness -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [5, 130])
def test_linked_keeps_the_analysis_phase_difference_in_every_cell(data, bins):
    A, _M, Ar, Mr = data["lk", bins]
    for kind, pos in real_maps(LK_F_OUT, LK_F_SRC, 21).items():
        out = ln_run(A, Ar, Mr, LK_F_OUT, pos=pos).cpu().numpy()
        i0, _, _ = mref.positions(pos, LK_F_SRC)
        qa = ref.q(A)
        want = (qa[0] - qa[1])[:, i0]
        got = ref.q(out[0]) - ref.q(out[1])
        # the outputs are rounded once to fp32: half an ulp below pi is 1.2e-7 rad = 82 steps of the 2^32 grid per output
        d = (got - want).view(np.int32)
        assert np.abs(d).max() <= 2 * 82 + 2, (kind, bins, np.abs(d).max())
        T = mref.phase_lock_map(Ar, pos, Mr, FLOOR, return_rotation=True)[1]
        assert same_bits(out, ref.angle_of(T[None] + qa[..., i0]))           # and exactly, before that rounding


# ---- hostile tables and cells -----------------------------------------------------------------------------------------------------

GUARD, SENT = 64, -77.0


def interior(a):
    """a device copy of ``a`` as an interior view of a buffer of sentinels -> (view, buffer)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((GUARD + t.numel() + GUARD,), SENT, dtype=t.dtype).cuda()
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def guards_hold(buf, a):
    n = int(np.asarray(a).size)
    inner = buf[GUARD:GUARD + n].cpu().numpy().reshape(np.asarray(a).shape)
    same = np.array_equal(np.ascontiguousarray(inner).view(np.uint8), np.ascontiguousarray(a).view(np.uint8))
    return same and bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


def test_hostile_positions_read_nothing_outside_the_planes(data):
    """NaN, -1, +-inf, 1e300, -0.0, beyond 2^52 and a denormal in single frames: the restatement's bits, and the sentinels around
    every plane, the table and the output stay as they were"""
    P = data["sc"]
    pos = hostile(SC_N, SC["F_src"])
    (Pv, Pb), (pv, pb) = interior(P), interior(pos)
    ov, ob = interior(np.zeros((SC["n_clips"], SC["n_ch"], SC["bins"], SC["frames"]), np.float32))
    want = mref.spec_clips_map(P, SC["n_clips"], SC["frames"], SC["sf"], pos)
    assert same_bits(sc_run(Pv, pos=pv, out=ov), want)
    assert guards_hold(Pb, P) and guards_hold(pb, pos) and guards_hold(ob, want)
    A, M = data["pv"]
    pos = hostile(PV["F_out"], PV["F_src"])
    (Av, Ab), (Mv, Mb), (pv, pb) = interior(A), interior(M), interior(pos)
    ov, ob = interior(np.zeros((PV["n_ch"], PV["bins"], PV["F_out"]), np.float32))
    want = mref.phase_vocoder_map(A, pos, M, FLOOR)
    assert same_bits(pv_run(Av, Mv, PV["F_out"], pos=pv, out=ov), want)
    assert guards_hold(Ab, A) and guards_hold(Mb, M) and guards_hold(pb, pos) and guards_hold(ob, want)
    for bins in (5, 130, 1100):
        A, M, Ar, Mr = data["lk", bins]
        pos = hostile(LK_F_OUT, LK_F_SRC)
        (Av, Ab), (Mv, Mb), (Arv, Arb), (Mrv, Mrb), (pv, pb) = interior(A), interior(M), interior(Ar), interior(Mr), interior(pos)
        ov, ob = interior(np.zeros((2, bins, LK_F_OUT), np.float32))
        want = mref.phase_lock_map(A, pos, M, FLOOR)
        assert same_bits(lk_run(Av, Mv, LK_F_OUT, pos=pv, out=ov), want), bins
        assert guards_hold(Ab, A) and guards_hold(Mb, M) and guards_hold(pb, pos) and guards_hold(ob, want)
        want = mref.phase_lock_linked_map(A, Ar, Mr, pos, FLOOR)
        assert same_bits(ln_run(Av, Arv, Mrv, LK_F_OUT, pos=pv, out=ov), want), bins
        assert guards_hold(Ab, A) and guards_hold(Arb, Ar) and guards_hold(Mrb, Mr) and guards_hold(pb, pos) and guards_hold(ob, want)
    x = data["ola"]
    for (w, hop), n_out in zip(OLA, OLA_N_OUT):
        c = grain_table(n_out, w, hop, "hostile")
        (xv, xb), (cv, cb) = interior(x), interior(c)
        ov, ob = interior(np.zeros((2, n_out), np.float32))
        want = mref.ola_stretch_map(x, n_out, c, tref.ola_window(w), hop)
        assert same_bits(ol_run(xv, n_out, w, hop, pos=cv, out=ov), want)
        assert guards_hold(xb, x) and guards_hold(cb, c) and guards_hold(ob, want)


def test_nan_cells_in_the_planes_do_what_the_twins_do(data):
    """q(NaN) = 0, a NaN magnitude neither resets nor is a peak, a NaN plane cell is interpolated like any other: the twins' rules,
    so the restatement on a real table and the twin on a uniform one"""
    rs = np.random.RandomState(5)
    P = data["sc"].copy()
    P[rs.uniform(size=P.shape) < 0.1] = NAN
    P[0, 0, 3], P[1, 2, 4] = -0.0, INF
    pos = ramp(SC_N, SC["F_src"])
    assert same_bits(sc_run(P, pos=pos), mref.spec_clips_map(P, SC["n_clips"], SC["frames"], SC["sf"], pos))
    assert same_bits(sc_run(P, pos=uniform(SC_N, 1.0)), sc_run(P, 1.0))      # (w == 0 copies: -0.0 and the NaN payloads survive)
    A, M, Ar, Mr = (v.copy() for v in data["lk", 65])
    for t in (A, M, Ar, Mr):
        t[rs.uniform(size=t.shape) < 0.05] = NAN
    A[0, 1, 2], M[1, 3, 4], Mr[5, 6] = INF, -INF, INF
    for pos in (ramp(LK_F_OUT, LK_F_SRC), wild(LK_F_OUT)):
        assert same_bits(pv_run(A, M, LK_F_OUT, pos=pos), mref.phase_vocoder_map(A, pos, M, FLOOR))
        assert same_bits(lk_run(A, M, LK_F_OUT, pos=pos), mref.phase_lock_map(A, pos, M, FLOOR))
        assert same_bits(ln_run(A, Ar, Mr, LK_F_OUT, pos=pos), mref.phase_lock_linked_map(A, Ar, Mr, pos, FLOOR))
    pos = uniform(LK_F_OUT, 1 / 1.3)
    assert same_bits(lk_run(A, M, LK_F_OUT, pos=pos), lk_run(A, M, LK_F_OUT, 1 / 1.3))
    x = data["ola"].copy()
    x[0, 300], x[1, 700] = NAN, INF
    c = grain_table(1025, 256, 64, "ramp")
    assert same_bits(ol_run(x, 1025, 256, 64, pos=c), mref.ola_stretch_map(x, 1025, c, tref.ola_window(256), 64))


# ---- the workspace and stream contracts ----------------------------------------------------------------------------------------

def lock_map_case(F_out, bins, n_ch=2, linked=False):
    import test_z_workspace_gpu as W
    from phasegen import ops
    F_src = F_out + 7
    A, M = planes(4000 + F_out + bins, n_ch, bins, F_src)
    Ar, Mr = planes(5000 + F_out + bins, 1, bins, F_src)
    pos = wild(F_out) if F_out >= 8 else uniform(F_out, 0.7)
    ins = {"A": W.cuda(A), "M": W.cuda(M), "Aref": W.cuda(Ar[0]), "Mref": W.cuda(Mr[0]), "pos": W.cuda(pos)}
    if linked:
        return W.Case(f"link-map-F{F_out}-b{bins}", ins, lambda: {"out": W.sent(n_ch, bins, F_out)},
                      lambda i, o: [ops.phase_lock_linked(i["A"], i["Aref"], i["Mref"], F_out, reset_below=FLOOR, out=o["out"], pos=i["pos"])],
                      poisons=(0x00,), symbol="pg_phase_lock_linked_map", lock=True)
    return W.Case(f"lock-map-F{F_out}-b{bins}", ins, lambda: {"out": W.sent(n_ch, bins, F_out)},
                  lambda i, o: [ops.phase_lock(i["A"], F_out, logmag=i["M"], reset_below=FLOOR, out=o["out"], pos=i["pos"])],
                  poisons=(0x00,), symbol="pg_phase_lock_map", lock=True)


def streaming_cases():
    import test_z_workspace_gpu as W
    from phasegen import ops
    P = planes(6001, 2, 5, 40)[1]
    A, M = planes(6002, 2, 5, 40)
    x, base = np.random.RandomState(6).standard_normal((2, 1000)).astype(np.float32), np.random.RandomState(7).standard_normal((2, 1500)).astype(np.float32)
    return [
        W.Case("spec_clips_map", {"plane": W.cuda(P), "pos": W.cuda(ramp(28, 40))}, lambda: {"out": W.sent(3, 2, 5, 12)},
               lambda i, o: [ops.spec_clips(i["plane"], 3, 12, 8, out=o["out"], pos=i["pos"])], symbol="pg_spec_clips_map", needs_ws=False),
        W.Case("phase_vocoder_map", {"A": W.cuda(A), "M": W.cuda(M), "pos": W.cuda(wild(50))}, lambda: {"out": W.sent(2, 5, 50)},
               lambda i, o: [ops.phase_vocoder(i["A"], 50, logmag=i["M"], reset_below=FLOOR, out=o["out"], pos=i["pos"])],
               symbol="pg_phase_vocoder_map", needs_ws=False),
        W.Case("ola_stretch_map", {"x": W.cuda(x), "base": W.cuda(base), "pos": W.cuda(grain_table(1500, 256, 64, "two_slope") * 0.6)},
               lambda: {"y": W.sent(2, 1500)}, lambda i, o: [ops.ola_stretch(i["x"], 1500, base=i["base"], out=o["y"], pos=i["pos"])],
               symbol="pg_ola_stretch_map", needs_ws=False)]


def test_exact_poisoned_stale_and_misaligned_workspaces_and_the_stream():
    """pg_phase_lock_map and pg_phase_lock_linked_map under the helpers of tests/test_z_workspace_gpu.py: a workspace of EXACTLY the
    queried size between guards, zeroed or holding the maps of another, larger problem, 4 bytes off its alignment -- the same bits,
    nothing written outside.  All five mapped entry points on a busy side stream (tests/test_z_streams_gpu.py): the same bits, no wait
    for the device, nothing on another stream.  Both modules count the seven new symbols' five stream entry points as reached."""
    import test_z_streams_gpu as S
    import test_z_workspace_gpu as W
    from _strict import strict_workspaces
    for linked in (False, True):
        for F_out, bins, n_ch in ((1, 1, 2), (33, 5, 3), (65, 64, 2), (33, 1025, 2)):
            case = lock_map_case(F_out, bins, n_ch, linked)
            W.check(case)
            big = lock_map_case(F_out + 70, min(2 * bins + 3, 4096), n_ch, linked)
            with strict_workspaces(0x00, keep=True) as s:
                big.run(big.ins, big.make_outs())
            (stale,) = s.contents
            assert bool((stale != 0).any())
            want = case.run(case.ins, case.make_outs())
            with strict_workspaces(0x00, stale=stale) as s:
                got = case.run(case.ins, case.make_outs())
            assert same_bits(got[0], want[0]), (linked, F_out, bins)
            assert s.requests == [12 * (1 if linked else n_ch) * bins * -(-F_out // 32)]       # the twin's size
        W.check(lock_map_case(33, 5, 2, linked), offset=4)
        S.reach(lock_map_case(33, 5, 2, linked))
    for case in streaming_cases():
        W.check(case)                                                        # (no workspace: the guards of none, the same bits)
        S.reach(case)
    new = {"pg_spec_clips_map", "pg_phase_vocoder_map", "pg_phase_lock_map", "pg_phase_lock_linked_map", "pg_ola_stretch_map"}
    assert new <= S.REACHED and {"pg_phase_lock_map", "pg_phase_lock_linked_map"} <= W.REACHED and new <= W.REACHED


# ---- independence -----------------------------------------------------------------------------------------------------------------

def test_a_rows_bits_do_not_depend_on_its_company_or_its_layout(data):
    A, M, Ar, Mr = data["lk", 65]
    pos = dev(wild(LK_F_OUT))
    rs = np.random.RandomState(8)
    A3, M3 = (np.concatenate([v, planes(9, 1, 65, LK_F_SRC)[k]]) for k, v in enumerate((A, M)))
    pol = dev(np.stack([M3, A3], 1))                                         # (3, 2, bins, F): channels 2 bins rows apart
    assert not pol[:, 1].is_contiguous()
    runs = {"vocoder": lambda a, m, **kw: pv_run(a, m, LK_F_OUT, pos=pos, **kw), "lock": lambda a, m, **kw: lk_run(a, m, LK_F_OUT, pos=pos, **kw),
            "linked": lambda a, m, **kw: ln_run(a, Ar, Mr, LK_F_OUT, pos=pos, **kw)}
    for name, run in runs.items():
        both = run(dev(A3), dev(M3))
        assert same_bits(run(pol[:, 1], pol[:, 0]), both), name              # a plane of a polar tensor, read in place
        for c in range(3):
            assert same_bits(run(dev(A3[c:c + 1]), dev(M3[c:c + 1]))[0], both[c]), (name, c)
        assert same_bits(run(dev(A3[1:]), dev(M3[1:])), both[1:]), name
        out = offset_view(torch.zeros_like(both))                            # 4 bytes off: the frame-by-frame store path
        assert run(dev(A3), dev(M3), out=out) is out and same_bits(out, both), name
        assert same_bits(run(offset_view(dev(A3)), offset_view(dev(M3))), both), name
    odd = LK_F_OUT - 1                                                       # F_out % 4 != 0: element-wise stores, the same head
    assert same_bits(lk_run(A, M, odd, pos=pos[:odd].clone()), lk_run(A, M, LK_F_OUT, pos=pos)[..., :odd])
    P3 = rs.uniform(0, 1, (3, SC["bins"], SC["F_src"])).astype(np.float32)
    sp = dev(ramp(SC_N, SC["F_src"]))
    both = sc_run(P3, pos=sp)
    for c in range(3):
        assert same_bits(sc_run(P3[c:c + 1], pos=sp)[:, 0], both[:, c]), c
    pol = dev(np.stack([P3, P3 + 1], 1))
    assert same_bits(sc_run(pol[:, 0], pos=sp), both) and same_bits(sc_run(offset_view(dev(P3)), pos=sp), both)
    from phasegen import ops
    one = ops.spec_clips(dev(P3), 1, SC_N, SC_N, pos=sp)                     # one clip of every frame: the clips are windows of it
    for k in range(SC["n_clips"]):
        assert same_bits(both[k], one[0, :, :, k * SC["sf"]:k * SC["sf"] + SC["frames"]]), k
    x = data["ola"]
    c = dev(grain_table(1025, 256, 64, "wild"))
    both = ol_run(x, 1025, 256, 64, pos=c)
    assert same_bits(ol_run(x[1], 1025, 256, 64, pos=c), both[1])
    wide = dev(np.concatenate([x, x], 1))[:, :1500]                          # rows 3000 apart
    assert wide.stride(0) == 3000 and same_bits(ol_run(wide, 1025, 256, 64, pos=c), both)
    out = offset_view(torch.zeros_like(both))
    assert same_bits(ol_run(x, 1025, 256, 64, pos=c, out=out), both)


def test_argument_errors(data):
    from phasegen import ops
    A, M, Ar, Mr = (dev(v) for v in data["lk", 5])
    good = dev(uniform(LK_F_OUT, 0.7))
    for bad in (good[:-1], good.float(), good.cpu(), good[None], torch.cat([good, good])[::2], list(range(LK_F_OUT))):
        for call in (lambda p: ops.phase_vocoder(A, LK_F_OUT, pos=p), lambda p: ops.phase_lock(A, LK_F_OUT, logmag=M, pos=p),
                     lambda p: ops.phase_lock_linked(A, Ar, Mr, LK_F_OUT, pos=p)):
            with pytest.raises(ValueError):
                call(bad)
    for call in (lambda: ops.phase_vocoder(A, LK_F_OUT, 0.7, pos=good), lambda: ops.phase_lock(A, LK_F_OUT, 0.7, logmag=M, pos=good),
                 lambda: ops.phase_lock_linked(A, Ar, Mr, LK_F_OUT, 0.7, pos=good),
                 lambda: ops.spec_clips(M, 1, LK_F_OUT, LK_F_OUT, 0.7, pos=good),
                 lambda: ops.ola_stretch(dev(data["ola"]), 7, 0.7, 8, 2, pos=dev(uniform(6, 1.0)))):
        with pytest.raises(ValueError, match="two time grids"):
            call()
    with pytest.raises(ValueError):
        ops.spec_clips(M, 3, 8, 5, pos=good)                                 # 18 entries wanted
    with pytest.raises(ValueError):
        ops.ola_stretch(dev(data["ola"]), 7, win_len=8, hop=2, pos=dev(uniform(5, 1.0)))
    with pytest.raises(ValueError):
        ops.phase_lock(A, LK_F_OUT, pos=good)                                # logmag is still required
    wide = torch.zeros(1, 4097, 3, device="cuda")
    with pytest.raises(RuntimeError, match="4096 bins"):
        ops.phase_lock(wide, 4, logmag=wide, pos=dev(uniform(4, 0.5)))


# ---- track level ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def melody():
    return ref.melody(seconds=3.0)


@pytest.fixture(scope="module")
def stereo():
    return kref.stereo_melody(seconds=3.0)


@pytest.fixture(scope="module")
def model():
    from phasegen.model import UNetModel
    return UNetModel(16, 32, gpu_ids=[0]).load_numpy(detgen.make_params(16, seed=0))


@pytest.mark.parametrize("R", [0.5, 2.0])
def test_a_one_segment_map_is_the_uniform_stretch_bit_for_bit(melody, stereo, model, R):
    from phasegen import track
    tm = track.TimeMap([(0, 0), (1, R)])
    for phase in track.STRETCH_PHASES:
        kw = dict(phase=phase, join="spectral", normalize=False, **SMALL)
        m = model if phase == "unet" else None
        got, want = track.reconstruct_track(m, melody, stretch=tm, **kw), track.reconstruct_track(m, melody, stretch=R, **kw)
        assert tuple(got.shape) == (round(melody.shape[0] * R),) and same_bits(got, want), (phase, R)
        got, want = (track.reconstruct_track(m, melody, stretch=s, transients="ola", **kw) for s in (tm, R))
        assert same_bits(got, want), (phase, R, "ola")
    kw = dict(phase="vocoder_locked", join="spectral", link_channels=True, **SMALL)
    got, want = (track.reconstruct_track(None, stereo, stretch=s, **kw) for s in (tm, R))
    assert tuple(got.shape) == (2, round(stereo.shape[1] * R)) and same_bits(got, want)
    got, want = (track.reconstruct_track(None, stereo, stretch=s, transients="ola", formant_semitones=3.0, **kw) for s in (tm, R))
    assert same_bits(got, want)


def test_a_two_slope_map_equals_the_ops_composition(melody, stereo):
    from phasegen import ops, track
    anchors = [(0, 0), (1.0, 0.5), (3.0, 4.5)]
    tm = track.TimeMap(anchors)
    floor = track.VOCODER_RESET_BELOW
    out = track.reconstruct_track(None, melody, phase="vocoder_locked", join="spectral", stretch=tm, normalize=False, **SMALL)
    an = track._analyse_spectral(melody, 32, 8, 24, 4, None, None, 16000, "kaiser_best", tm)
    pl = an.plan
    want_plan = mref.mapped_plan(mref.TimeMap(anchors), melody.shape[0], 24, 8, 4)
    assert pl.a_out == 72000 == want_plan["a_out"] and all(want_plan[k] == getattr(pl, k) for k in ("n_clips", "F_out", "F_src", "n_src"))
    assert np.array_equal(pl.pos, want_plan["pos"]) and np.array_equal(pl.grains, want_plan["grains"])
    assert tuple(out.shape) == (pl.a_out,) and bool(torch.isfinite(out).all())
    pos = dev(pl.pos)
    assert same_bits(an.pos.cpu().numpy().view(np.float32), pl.pos.view(np.float32))
    with torch.no_grad():
        ph = ops.phase_lock(an.pol[:, 1], pl.F_out, logmag=an.pol[:, 0], reset_below=floor, pos=pos)
        mag = ops.spec_clips(an.pol[:, 0], 1, pl.F_out, pl.F_out, pos=pos)[0]
        want = track._trim_spectral(an, ops.istft(mag, ph, 8, mode=0, normalize=False), False)
    assert same_bits(out, want[0])
    pol = an.pol.cpu().numpy()
    assert same_bits(ph, mref.phase_lock_map(pol[:, 1], pl.pos, pol[:, 0], floor))
    assert same_bits(mag, mref.spec_clips_map(pol[:, 0], 1, pl.F_out, pl.F_out, pl.pos)[0])
    # the transient path and the linked stereo path, written out the same way
    out = track.reconstruct_track(None, stereo, phase="vocoder_locked", join="spectral", stretch=tm, normalize=False, link_channels=True,
                                  transients="ola", **SMALL)
    an = track._analyse_spectral(stereo, 32, 8, 24, 4, None, None, 16000, "kaiser_best", tm, True)
    with torch.no_grad():
        harm, perc = ops.hpss(an.pol[:, 0], *track.HPSS_WIN)
        ph = ops.phase_lock_linked(an.pol[:2, 1], an.pol[2, 1], harm[2], pl.F_out, reset_below=floor, pos=pos)
        mag = ops.spec_clips(harm[:2], 1, pl.F_out, pl.F_out, pos=pos)[0]
        audio = ops.istft(mag, ph, 8, mode=0, normalize=False)
        p_audio = ops.istft(perc[:2], an.pol[:2, 1], 8, mode=0, normalize=False)
        audio = ops.ola_stretch(p_audio, audio.shape[1], 1.0, track.TRANSIENT_WINDOW, track.TRANSIENT_HOP, base=audio, pos=dev(pl.grains))
        want = track._trim_spectral(an, audio, False)
    assert tuple(out.shape) == (2, pl.a_out) and bool(torch.isfinite(out).all()) and same_bits(out, want)
    normal = track.reconstruct_track(None, melody, phase="vocoder", join="spectral", stretch=tm, **SMALL)
    assert float(normal.abs().max()) == 1.0


def test_evaluate_stretch_takes_a_map(melody):
    from phasegen import track
    tm = track.TimeMap.ramp(3.0, 1.0, 1.5, 16)
    x = melody[8000:24000]
    rep = track.evaluate_stretch(None, x, tm, phases=("vocoder_locked", "spsi", "zero"), return_audio=True, **SMALL)
    assert list(rep) == ["n_samples", "n_out", "sr", "stretch", "n_clips", "reset_below", "metrics", "audio"]
    a_out = int(round(tm.out_of_src(16000)))
    assert (rep["n_samples"], rep["n_out"]) == (16000, a_out) and rep["stretch"] == a_out / 16000
    for p, m in rep["metrics"].items():
        assert set(m) == {"spectral_convergence", "lsd_db", "n_frames", "channels"} and np.isfinite(m["spectral_convergence"]), p
    raw = track.reconstruct_track(None, x, phase="spsi", join="spectral", stretch=tm, normalize=False, **SMALL)
    assert tuple(raw.shape) == (a_out,) and same_bits(rep["audio"]["spsi"], raw)


def test_a_map_is_refused_where_it_cannot_work(melody):
    from phasegen import track
    tm = track.TimeMap([(0, 0), (1, 1.5)])
    x = melody[:4000]
    with pytest.raises(ValueError, match="join='spectral'"):
        track.reconstruct_track(None, x, phase="zero", stretch=tm, **SMALL)
    with pytest.raises(ValueError, match="TimeMap needs phase"):
        track.reconstruct_track(None, x, phase="original", join="spectral", stretch=tm, **SMALL)
    with pytest.raises(ValueError, match="TimeMap"):
        track.pitch_shift(None, x, tm, phase="zero", **SMALL)
    with pytest.raises(ValueError, match="link_channels"):
        track.reconstruct_track(None, x, phase="vocoder", join="spectral", stretch=tm, link_channels=True, **SMALL)


# ---- command line -----------------------------------------------------------------------------------------------------------------

def _cli(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--channels", "16", "--hop", "8",
                           "--frames", "24", "--overlap_frames", "4", *map(str, flags)], capture_output=True, text=True, timeout=300)


def test_reconstruct_cli_with_a_tempo_map(tmp_path):
    from scipy.io import wavfile
    wav, out, tmap = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "map.txt"
    wavfile.write(str(wav), 16000, detgen.normal(99, (4000,)).astype(np.float32) * 0.1)
    tmap.write_text("# source output\n0 0\n0.1 0.05   # twice as fast\n0.25, 0.35\n")
    a_out = int(round(mref.TimeMap([(0, 0), (0.1, 0.05), (0.25, 0.35)]).out_of_src(4000)))
    assert a_out == 5600
    r = _cli("--input", wav, "--output", out, "--phase", "vocoder_locked", "--tempo_map", tmap, "--transients", "ola")      # no --weight
    assert r.returncode == 0, r.stderr[-2000:]
    sr, y = wavfile.read(str(out))
    assert sr == 16000 and y.shape == (a_out,) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    for flags, msg in ((("--stretch", "1.5"), "--tempo_map"), (("--pitch", "3"), "--tempo_map")):
        r = _cli("--input", wav, "--output", out, "--phase", "vocoder", "--tempo_map", tmap, *flags)
        assert r.returncode == 2 and msg in r.stderr, (flags, r.stderr[-500:])
