"""GPU: channel-linked phase locking -- pg_phase_lock_linked BIT FOR BIT against the numpy restatement of its contract
(tests/_link_ref.py) at every chunk boundary of the scan it shares with pg_phase_lock, its widths (every size of the three-plane
staged window), layouts, store paths and special inputs, the equalities with pg_phase_lock and pg_phase_vocoder, the workspace and
stream contract of the entry point, and the track level built on it (phasegen.track link_channels, evaluate_stretch's mid_metrics,
reconstruct.py --link_channels).

Bounds.  The kernel's sums are integers modulo 2^32 and its comparisons plain IEEE fp32 comparisons, so every comparison with the
restatement is exact.  The mid signal: the float64 chain at n_fft 512 / hop 128 gives a mid spectral convergence of 0.0715 linked
against 0.3194 independent at stretch 1.5 (tests/test_link_host.py: ratio 0.224), so "below half" holds with room."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _link_ref as kref
import _lock_ref as lref
import _vocoder_ref as ref
from phasegen import detgen
from test_z_lock_gpu import f_src_for, offset_view, same_bits, sparse_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)


def L():
    from phasegen import ops
    return ops.PHASE_LOCK_CHUNK


def planes(seed, n_ch, bins, F_src):
    """A (n_ch, bins, F_src) and Aref (bins, F_src) uniform in (-pi, pi], Mref uniform in [0, 1): with reset_below at Mref's median
    about half of the peaks reset."""
    rs = np.random.RandomState(seed)
    A = rs.uniform(-np.pi, np.pi, (n_ch, bins, F_src)).astype(np.float32)
    Aref = rs.uniform(-np.pi, np.pi, (bins, F_src)).astype(np.float32)
    Mref = rs.uniform(0.0, 1.0, (bins, F_src)).astype(np.float32)
    return A, Aref, Mref


def run(A, Aref, Mref, F_out, spo, floor=0.0, **kw):
    from phasegen import ops
    return ops.phase_lock_linked(torch.from_numpy(A).cuda(), torch.from_numpy(Aref).cuda(), torch.from_numpy(Mref).cuda(), F_out, spo,
                                 reset_below=floor, **kw)


def both_floors(A, Aref, Mref, F_out, spo, tag):
    """reset_below at a floor that cuts through the data, and at 0 (nothing resets after frame 0)"""
    floor = float(np.median(Mref))
    got = run(A, Aref, Mref, F_out, spo, floor)
    assert tuple(got.shape) == (A.shape[0], A.shape[1], F_out) and got.dtype == torch.float32
    want = kref.phase_lock_linked(A, Aref, Mref, F_out, spo, floor)
    assert np.abs(want).max() <= np.float32(np.pi)
    assert same_bits(got, want), tag
    assert same_bits(run(A, Aref, Mref, F_out, spo), kref.phase_lock_linked(A, Aref, Mref, F_out, spo, 0.0)), tag


# ---- bit for bit against the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("spo", [1.0, 0.5, 2.0, 1 / 1.3, 4.0, 0.25])
def test_bitwise_against_the_restatement_at_every_chunk_boundary(spo):
    for F_out in (1, 31, 32, 33, 64, 65, 97):
        A, Aref, Mref = planes(1000 + F_out, 2, 5, f_src_for(F_out, spo))
        both_floors(A, Aref, Mref, F_out, spo, (spo, F_out))


@pytest.mark.parametrize("bins", [1, 2, 3, 5, 63, 64, 65, 130])
def test_bitwise_for_every_narrow_width(bins):
    for spo in (1 / 1.3, 2.0):
        A, Aref, Mref = planes(2000 + bins, 2, bins, f_src_for(40, spo))
        both_floors(A, Aref, Mref, 40, spo, (bins, spo))


@pytest.mark.parametrize("bins", [260, 1024, 2048, 3000, 4096])
def test_bitwise_for_every_size_of_the_staged_window(bins):
    """37 frames (two chunks) of 2 channels: a window of the whole chunk (260), of 8 source frames (1024), of 2 with two bins per
    thread (2048), and none with three and four bins per thread (3000, 4096).  The reference's magnitudes leave long runs of empty
    words in the peak mask (tests/test_z_lock_gpu.py: sparse_planes), so bins gather from peaks many words away."""
    F_out, spo = 37, 1 / 1.5
    F_src = f_src_for(F_out, spo)
    Aref, Mref = (p[0] for p in sparse_planes(13 + bins, bins, F_src))
    A = np.random.RandomState(14 + bins).uniform(-np.pi, np.pi, (2, bins, F_src)).astype(np.float32)
    want, T = kref.phase_lock_linked(A, Aref, Mref, F_out, spo, 5e-4), lref.phase_lock(Aref, F_out, spo, Mref, 5e-4, return_rotation=True)[1]
    assert T[:, -1].any() and not np.array_equal(want, ref.angle_of(ref.q(A[..., ref.positions(F_out, spo, F_src)[0]])))      # it rotates
    assert same_bits(run(A, Aref, Mref, F_out, spo, 5e-4), want)
    never = run(A, Aref, Mref, F_out, spo)
    assert same_bits(never, kref.phase_lock_linked(A, Aref, Mref, F_out, spo, 0.0)) and not same_bits(never, want)


def test_positions_further_apart_than_the_staged_window():
    """src_per_out = 9 at 1024 bins: the two positions of a frame are 8 source frames apart and the window holds 8, so every frame
    but the first is read by the threads from their own rows; 40: likewise, and the last frames sit on the source's end."""
    F_out = L() + 3
    A, Aref, Mref = planes(22, 2, 1024, f_src_for(F_out, 9.0))
    for spo in (9.0, 40.0):
        assert same_bits(run(A, Aref, Mref, F_out, spo, 0.5), kref.phase_lock_linked(A, Aref, Mref, F_out, spo, 0.5)), spo
    A, Aref, Mref = planes(23, 2, 5, 700)
    for spo in (40.0, 1e300):
        assert same_bits(run(A, Aref, Mref, F_out, spo, 0.5), kref.phase_lock_linked(A, Aref, Mref, F_out, spo, 0.5)), spo


def test_the_source_ends_early():
    """Positions 0 .. 2 L + 2 of 7 source frames at half rate: from frame 12 on i1 == i0, the advance is zero and every frame repeats."""
    A, Aref, Mref = planes(11, 2, 37, 7)
    F_out = 2 * L() + 3
    got = run(A, Aref, Mref, F_out, 0.5, 0.4)
    assert same_bits(got, kref.phase_lock_linked(A, Aref, Mref, F_out, 0.5, 0.4))
    g = got.cpu().numpy()
    assert np.array_equal(g[..., 13:], np.repeat(g[..., 13:14], F_out - 13, -1)) and not np.array_equal(g[..., 11], g[..., 12])


# ---- channels ------------------------------------------------------------------------------------------------------------

def test_channel_counts_and_a_channel_alone_has_the_bits_it_has_in_a_batch():
    from phasegen import ops
    F_out = 2 * L() + 1
    A, Aref, Mref = planes(17, 5, 21, f_src_for(F_out, 0.8))
    Ad, Rd, Md = (torch.from_numpy(x).cuda() for x in (A, Aref, Mref))
    want = kref.phase_lock_linked(A, Aref, Mref, F_out, 0.8, 0.5)
    for n_ch in (1, 2, 3, 5):
        got = ops.phase_lock_linked(Ad[:n_ch], Rd, Md, F_out, 0.8, reset_below=0.5)
        assert tuple(got.shape) == (n_ch, 21, F_out) and same_bits(got, want[:n_ch]), n_ch
    for c in range(5):
        assert same_bits(ops.phase_lock_linked(Ad[c:c + 1], Rd, Md, F_out, 0.8, reset_below=0.5)[0], want[c]), c
    assert same_bits(ops.phase_lock_linked(Ad[3:], Rd[None], Md[None], F_out, 0.8, reset_below=0.5), want[3:])     # (1, bins, F_src) references
    back = ops.phase_lock_linked(Ad.flip(0).contiguous(), Rd, Md, F_out, 0.8, reset_below=0.5)
    assert same_bits(back, want[::-1])                                      # nor does it depend on the channel's position


def test_the_rotation_cancels_between_two_channels():
    """q(out_c) - q(out_d) is q(A_c) - q(A_d) on the output grid to within the two roundings to fp32 and back: half an ulp of a value
    below 4, 2^-23 rad = 81.5 steps of the 2^32 grid, plus half a step for q's rint, per channel: 164 steps."""
    F_out, spo = 2 * L() + 7, 1 / 1.5
    A, Aref, Mref = planes(31, 2, 65, f_src_for(F_out, spo))
    got = run(A, Aref, Mref, F_out, spo, 0.5).cpu().numpy()
    i0, _ = ref.positions(F_out, spo, A.shape[-1])
    qa = ref.q(A)[..., i0]
    d = (ref.q(got[0]) - ref.q(got[1]) - (qa[0] - qa[1])).view(np.int32)
    assert np.abs(d.astype(np.int64)).max() <= 164 and lref.phase_lock(Aref, F_out, spo, Mref, 0.5, return_rotation=True)[1].any()


def test_planes_of_a_polar_tensor_are_read_in_place_with_the_reference_from_another_tensor():
    from phasegen import ops
    rs = np.random.RandomState(16)
    F = 2 * L() + 9
    pol = np.stack([rs.uniform(0, 1, (3, 21, F)), rs.uniform(-np.pi, np.pi, (3, 21, F))], 1).astype(np.float32)     # (n_ch, 2, bins, F)
    mid = np.stack([rs.uniform(0, 1, (1, 21, F)), rs.uniform(-np.pi, np.pi, (1, 21, F))], 1).astype(np.float32)
    pd, md = torch.from_numpy(pol).cuda(), torch.from_numpy(mid).cuda()
    assert not pd[:, 1].is_contiguous() and pd[:, 1].stride(0) == 2 * 21 * F
    for F_out, spo in ((F, 1.0), (3 * L() + 2, 1 / 1.5)):
        got = ops.phase_lock_linked(pd[:, 1], md[0, 1], md[0, 0], F_out, spo, reset_below=0.5)
        assert same_bits(got, kref.phase_lock_linked(pol[:, 1], mid[0, 1], mid[0, 0], F_out, spo, 0.5))
        assert same_bits(got, ops.phase_lock_linked(pd[:, 1].contiguous(), md[:, 1], md[:, 0], F_out, spo, reset_below=0.5))
    # the reference as the last row of the SAME polar tensor (the track layer's layout)
    got = ops.phase_lock_linked(pd[:2, 1], pd[2, 1], pd[2, 0], 3 * L() + 2, 1 / 1.5, reset_below=0.5)
    assert same_bits(got, kref.phase_lock_linked(pol[:2, 1], pol[2, 1], pol[2, 0], 3 * L() + 2, 1 / 1.5, 0.5))
    assert same_bits(pd.cpu(), pol) and same_bits(md.cpu(), mid)            # (and nothing of them was written)


def test_element_wise_store_path_equals_the_16_byte_path():
    from phasegen import ops
    A, Aref, Mref = planes(18, 2, 21, 3 * L())
    Ad, Rd, Md = (torch.from_numpy(x).cuda() for x in (A, Aref, Mref))
    for F_out in (L(), 2 * L() + 4):                                        # multiples of 4: the 16-byte path when aligned
        wide = ops.phase_lock_linked(Ad, Rd, Md, F_out, 0.9, reset_below=0.5)
        assert wide.data_ptr() % 16 == 0 and same_bits(wide, kref.phase_lock_linked(A, Aref, Mref, F_out, 0.9, 0.5))
        out = offset_view(torch.zeros_like(wide))                           # `out` offset by 4 bytes: frame by frame
        assert ops.phase_lock_linked(Ad, Rd, Md, F_out, 0.9, reset_below=0.5, out=out) is out
        assert same_bits(out, wide)
        assert same_bits(ops.phase_lock_linked(offset_view(Ad), offset_view(Rd[None]), offset_view(Md[None]), F_out, 0.9, reset_below=0.5), wide)
        odd = ops.phase_lock_linked(Ad, Rd, Md, F_out + 1, 0.9, reset_below=0.5)          # F_out % 4 == 1: frame by frame
        assert same_bits(odd[..., :F_out], wide) and same_bits(odd, kref.phase_lock_linked(A, Aref, Mref, F_out + 1, 0.9, 0.5))


# ---- special inputs ------------------------------------------------------------------------------------------------------

def test_plateaus_ties_infinities_and_nans_in_the_reference_magnitude():
    inf, nan = np.inf, np.nan
    rows = [[1, 3, 3, 3, 1, 0, 0, 2, 0, 0, 0],                              # a plateau: its first bin is the peak
            [5, 0, 0, 0, 5, 0, 0, 0, 5, 0, 0],                              # exact ties between equal peaks: the lower one
            [0, inf, inf, 0, -inf, -inf, 1, 0, inf, 0, 0],                  # +-inf
            [0, 0, 7, nan, 0, 0, 9, 0, nan, 0, 8],                          # a NaN next to a peak disqualifies it
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],                              # all equal: bin 0 is the only peak
            [nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan]]        # no peak at all: every bin on its own
    F_out = L() + 5
    rs = np.random.RandomState(19)
    Mref = np.ascontiguousarray(np.array(rows, np.float32)[np.arange(F_out + 1) % 6].T)       # source frame f shows row f % 6
    assert Mref.shape == (11, F_out + 1)
    Aref = rs.uniform(-np.pi, np.pi, Mref.shape).astype(np.float32)
    A = rs.uniform(-np.pi, np.pi, (2,) + Mref.shape).astype(np.float32)
    for floor in (0.0, 2.5):
        assert same_bits(run(A, Aref, Mref, F_out, 1 / 1.2, floor), kref.phase_lock_linked(A, Aref, Mref, F_out, 1 / 1.2, floor)), floor


def test_nans_and_values_that_quantise_to_zero_in_the_angle_planes():
    pi = np.float32(np.pi)
    row = np.array([0.5, np.nan, 1.0, np.inf, -np.inf, 2.0, 2.0 ** 20 * (1 + 2.0 ** -23), -3e6, 2.5, pi, -pi, pi, 2.0 ** 20, -7.0], np.float32)
    A = np.stack([np.stack([np.roll(row, k + 3 * c) for k in range(5)]) for c in range(2)])      # (2, 5, 14)
    Aref = np.stack([np.roll(row, 7 - k) for k in range(5)])
    Mref = np.random.RandomState(20).uniform(0, 1, Aref.shape).astype(np.float32)
    for F_out, spo in ((14, 1.0), (28, 0.5), (40, 1 / 3.0)):
        got = run(A, Aref, Mref, F_out, spo, 0.3)
        want = kref.phase_lock_linked(A, Aref, Mref, F_out, spo, 0.3)
        assert same_bits(got, want) and np.isfinite(want).all() and np.abs(want).max() <= pi
    clean = np.where(np.isfinite(A) & (np.abs(A) <= 2.0 ** 20), A, 0).astype(np.float32)
    assert same_bits(run(A, Aref, Mref, 14, 1.0), ref.angle_of(ref.q(clean)))                   # a stretch of 1 returns q(A)


# ---- equalities between entry points -------------------------------------------------------------------------------------------

def test_a_channel_equal_to_the_reference_has_phase_locks_bits_and_an_all_nan_magnitude_the_plain_vocoders():
    from phasegen import ops
    F_out = 3 * L() + 5
    A, Aref, Mref = planes(14, 3, 65, f_src_for(F_out, 0.7))
    A[1] = Aref
    Ad, Rd, Md = (torch.from_numpy(x).cuda() for x in (A, Aref, Mref))
    got = ops.phase_lock_linked(Ad, Rd, Md, F_out, 0.7, reset_below=0.5)
    lock = ops.phase_lock(Rd[None], F_out, 0.7, logmag=Md[None], reset_below=0.5)
    assert same_bits(got[1], lock[0]) and not same_bits(got[0], lock[0])
    assert same_bits(ops.phase_lock_linked(Rd[None], Rd, Md, F_out, 0.7, reset_below=0.5), lock)         # n_ch == 1 with A == Aref
    assert not same_bits(got[0], ops.phase_lock(Ad[:1], F_out, 0.7, logmag=Md[None], reset_below=0.5)[0])   # (linking does change a channel)
    nan = torch.full_like(Md, float("nan"))
    got = ops.phase_lock_linked(Ad, Rd, nan, F_out, 0.7, reset_below=0.5)
    assert same_bits(got[1], ops.phase_vocoder(Rd[None], F_out, 0.7)[0])
    assert same_bits(ops.phase_lock_linked(Ad, Rd, Md, A.shape[-1], 1.0, reset_below=0.5), ref.angle_of(ref.q(A)))


# ---- the workspace and stream contract of the entry point ----------------------------------------------------------------------

def link_case(F_out, bins, n_ch=2, spo=1 / 1.5):
    import test_z_workspace_gpu as W
    from phasegen import ops
    A, Aref, Mref = planes(3000 + F_out + bins, n_ch, bins, f_src_for(F_out, spo))
    return W.Case(f"link-F{F_out}-b{bins}", {"A": W.cuda(A), "Aref": W.cuda(Aref), "Mref": W.cuda(Mref)}, lambda: {"out": W.sent(n_ch, bins, F_out)},
                  lambda i, o: [ops.phase_lock_linked(i["A"], i["Aref"], i["Mref"], F_out, spo, reset_below=0.5, out=o["out"])],
                  poisons=(0x00,), symbol="pg_phase_lock_linked", lock=True)


def test_exact_poisoned_and_stale_workspaces_and_the_stream():
    """pg_phase_lock_linked under the helpers of tests/test_z_workspace_gpu.py and tests/test_z_streams_gpu.py: a workspace of EXACTLY
    the queried size -- one channel's worth -- between guards, zeroed or holding the maps of another, larger problem (the workspace
    holds gather indices, so a mistake has to show as wrong values, never as wrong addresses), 4 bytes off its alignment, and a busy
    side stream: the same bits, nothing written outside, no wait for the device.  Both modules count the entry point as reached."""
    import test_z_streams_gpu as S
    import test_z_workspace_gpu as W
    from _strict import strict_workspaces
    for F_out, bins, n_ch in ((1, 1, 2), (33, 5, 3), (65, 64, 2), (33, 1025, 2)):
        case = link_case(F_out, bins, n_ch)
        W.check(case)
        big = link_case(F_out + 70, min(2 * bins + 3, 4096), n_ch)
        with strict_workspaces(0x00, keep=True) as s:
            big.run(big.ins, big.make_outs())
        (stale,) = s.contents
        assert bool((stale != 0).any())
        want = case.run(case.ins, case.make_outs())
        with strict_workspaces(0x00, stale=stale) as s:
            got = case.run(case.ins, case.make_outs())
        assert s.requests == [12 * bins * ((F_out + 31) // 32)] and stale.numel() > s.requests[0]      # whatever n_ch
        assert same_bits(got[0], want[0]), (F_out, bins)
        assert same_bits(want[0], kref.phase_lock_linked(*(case.ins[k].cpu().numpy() for k in ("A", "Aref", "Mref")), F_out, 1 / 1.5, 0.5))
    W.check(link_case(33, 5), offset=4)
    S.reach(link_case(33, 5))
    assert "pg_phase_lock_linked" in W.REACHED and "pg_phase_lock_linked" in S.REACHED


def test_argument_errors():
    from phasegen import _lib, ops
    A = torch.zeros(2, 5, 19, device="cuda")
    Rf, Mf = torch.zeros(5, 19, device="cuda"), torch.zeros(5, 19, device="cuda")
    for bad in (dict(F_out=0), dict(src_per_out=0.0), dict(src_per_out=float("nan")), dict(reset_below=-1.0), dict(reset_below=float("inf")),
                dict(ref_logmag=torch.zeros(5, 18, device="cuda")), dict(ref_angle=torch.zeros(2, 5, 19, device="cuda")), dict(ref_logmag=torch.zeros(5, 19)),
                dict(ref_angle=None), dict(out=torch.zeros(2, 5, 24, device="cuda"))):
        with pytest.raises(ValueError):
            ops.phase_lock_linked(**{**dict(angle=A, ref_angle=Rf, ref_logmag=Mf, F_out=25), **bad})
    for view in (A[:, :, ::2], A.transpose(1, 2), A.double(), A[0]):
        with pytest.raises(ValueError):
            ops.phase_lock_linked(view, Rf, Mf, 25)
    wide = torch.zeros(1, 4097, 3, device="cuda")
    with pytest.raises(RuntimeError, match="4096 bins"):
        ops.phase_lock_linked(wide, wide[0], wide[0], 3)
    # the workspace one byte short, with real pointers: refused before any launch
    lib = _lib.load()
    out = torch.full((2, 5, 25), 7.0, device="cuda")
    a = _lib.PhaseLockLinkedArgs()
    a.n_ch, a.bins, a.F_src, a.F_out, a.src_per_out, a.reset_below = 2, 5, 19, 25, 0.75, 0.05
    a.A, a.Aref, a.Mref, a.out, a.a_stride = A.data_ptr(), Rf.data_ptr(), Mf.data_ptr(), out.data_ptr(), 95
    need = lib.pg_workspace_bytes_phase_lock_linked(ctypes.byref(a))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert lib.pg_phase_lock_linked(ctypes.byref(a), None) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    a.bins, a.workspace_bytes = 4097, 1 << 40
    assert lib.pg_phase_lock_linked(ctypes.byref(a), None) == _lib.ERR_SHAPE


# ---- track level ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stereo():
    return kref.stereo_melody()


@pytest.mark.parametrize("stats", [None, (0.1, 2.0)], ids=["own-moments", "stats"])
def test_the_linked_analysis_leaves_the_channels_planes_as_they_are(stereo, stats):
    from phasegen import track
    args = (stereo, 32, 8, 24, 4, stats, None, 16000, "kaiser_best", 1.5)
    plain, linked = track._analyse_spectral(*args), track._analyse_spectral(*args, True)
    assert not plain.link and linked.link and plain.n_ch == linked.n_ch == 2
    assert tuple(plain.pol.shape) == (2, 2, 16, plain.plan.F_src) and tuple(linked.pol.shape) == (3, 2, 16, plain.plan.F_src)
    assert same_bits(linked.pol[:2], plain.pol)
    # the third row is the analysis of the channel mean under the same (mean, std)
    mid = torch.from_numpy(stereo).cuda().mean(0, keepdim=True)
    if stats is not None:
        alone = track._analyse_spectral(mid, 32, 8, 24, 4, stats, None, 16000, "kaiser_best", 1.5)
        assert same_bits(linked.pol[2:], alone.pol)
    assert bool(torch.isfinite(linked.pol).all()) and not same_bits(linked.pol[2], linked.pol[0])


@pytest.mark.parametrize("stretch", [1.5, 0.8])
def test_reconstruct_track_linked_equals_the_ops_composition(stereo, stretch):
    from phasegen import ops, track
    out = track.reconstruct_track(None, stereo, phase="vocoder_locked", join="spectral", stretch=stretch, normalize=False, link_channels=True, **SMALL)
    assert out.is_cuda and tuple(out.shape) == (2, round(stereo.shape[1] * stretch)) and bool(torch.isfinite(out).all())
    an = track._analyse_spectral(stereo, 32, 8, 24, 4, None, None, 16000, "kaiser_best", stretch, True)
    pl = an.plan
    with torch.no_grad():
        ph = ops.phase_lock_linked(an.pol[:2, 1], an.pol[2, 1], an.pol[2, 0], pl.F_out, 1 / stretch, reset_below=track.VOCODER_RESET_BELOW)
        mag = ops.spec_clips(an.pol[:2, 0], 1, pl.F_out, pl.F_out, 1 / stretch)[0]
        want = track._trim_spectral(an, ops.istft(mag, ph, 8, mode=0, normalize=False), False)
    assert same_bits(out, want)
    pol = an.pol.cpu().numpy()
    assert same_bits(ph, kref.phase_lock_linked(pol[:2, 1], pol[2, 1], pol[2, 0], pl.F_out, 1 / stretch, track.VOCODER_RESET_BELOW))
    unlinked = track.reconstruct_track(None, stereo, phase="vocoder_locked", join="spectral", stretch=stretch, normalize=False, **SMALL)
    assert not same_bits(out, unlinked)
    normal = track.reconstruct_track(None, stereo, phase="vocoder_locked", join="spectral", stretch=stretch, link_channels=True, **SMALL)
    assert same_bits(normal, track.peak_normalize(out))


def test_mono_input_linked_equals_the_unlinked_result(stereo):
    from phasegen import track
    for x, stats in ((stereo[0], None), (stereo[:1], (0.1, 2.0))):
        kw = dict(phase="vocoder_locked", join="spectral", stretch=1.5, stats=stats, **SMALL)
        a, b = track.reconstruct_track(None, x, link_channels=True, **kw), track.reconstruct_track(None, x, **kw)
        assert a.shape == b.shape and a.dim() == x.ndim and same_bits(a, b)


def test_pitch_shift_forwards_the_option():
    from phasegen import track
    x = kref.stereo_melody(seconds=1.2)[:, 8000:9000]
    out = track.pitch_shift(None, x, 5, stats=(0.1, 2.0), phase="vocoder_locked", link_channels=True, **SMALL)
    assert tuple(out.shape) == (2, 1000) and bool(torch.isfinite(out).all()) and float(out.abs().max()) == 1.0
    assert not same_bits(out, track.pitch_shift(None, x, 5, stats=(0.1, 2.0), phase="vocoder_locked", **SMALL))


def test_evaluate_stretch_reports_a_mid_signal_twice_as_consistent_when_linked(stereo):
    """n_fft 512 / hop 128, stretch 1.5: the report's mid_metrics of the linked locked vocoder against the mid consistency of the
    UNLINKED audio (from return_audio: the trimmed track, so the frames its samples cover; the linked audio measured the same way
    is printed beside the report's own figure)."""
    from phasegen import metrics, ops, track
    kw = dict(n_fft=512, hop_length=128, phases=("vocoder_locked", "vocoder"))
    rep = track.evaluate_stretch(None, stereo, 1.5, link_channels=True, return_audio=True, **kw)
    assert rep["link_channels"] is True and list(rep["mid_metrics"]) == ["vocoder_locked", "vocoder"] == list(rep["metrics"])
    for m in rep["mid_metrics"].values():
        assert set(m) == {"spectral_convergence", "lsd_db", "n_frames", "channels"} and m["channels"] == 1
    plain = track.evaluate_stretch(None, stereo, 1.5, return_audio=True, **kw)
    assert set(plain) == {"n_samples", "n_out", "sr", "stretch", "n_clips", "reset_below", "metrics", "audio"}
    assert same_bits(rep["audio"]["vocoder"], plain["audio"]["vocoder"])         # the option changes the locked vocoder alone
    assert plain["metrics"]["vocoder"] == rep["metrics"]["vocoder"]
    assert same_bits(rep["audio"]["vocoder_locked"], track.reconstruct_track(None, stereo, 512, 128, phase="vocoder_locked", normalize=False,
                                                                             join="spectral", stretch=1.5, link_channels=True))
    # the mid magnitudes on the output grid, cut to the frames the trimmed audio covers
    an = track._analyse_spectral(stereo, 512, 128, 128, 32, None, None, 16000, "kaiser_best", 1.5, True)
    F = rep["n_out"] // 128 + 1
    with torch.no_grad():
        mid_mag = ops.spec_clips(an.pol[2:, 0], 1, an.plan.F_out, an.plan.F_out, 1 / 1.5)[0][:, :, :F].contiguous()
    mid = lambda audio: metrics.consistency(mid_mag, audio.mean(0, keepdim=True)[:, :128 * (F - 1)].contiguous(), 512, 128)["spectral_convergence"]
    unlinked, linked_cut = mid(plain["audio"]["vocoder_locked"]), mid(rep["audio"]["vocoder_locked"])
    linked = rep["mid_metrics"]["vocoder_locked"]["spectral_convergence"]
    print(f"\nstereo melody, 512 / 128, stretch 1.5, mid SC on the device: linked {linked:.4f} (on the trimmed audio {linked_cut:.4f}), "
          f"unlinked {unlinked:.4f}; per-channel SC linked {rep['metrics']['vocoder_locked']['spectral_convergence']:.4f}, "
          f"unlinked {plain['metrics']['vocoder_locked']['spectral_convergence']:.4f}")
    assert linked < 0.5 * unlinked


def test_the_report_has_todays_keys_with_the_option_off(stereo):
    from phasegen import track
    x = stereo[:, 8000:12000]
    rep = track.evaluate_stretch(None, x, 1.5, phases=("vocoder_locked", "zero"), **SMALL)
    assert list(rep) == ["n_samples", "n_out", "sr", "stretch", "n_clips", "reset_below", "metrics"]
    off = track.evaluate_stretch(None, x, 1.5, phases=("vocoder_locked", "zero"), link_channels=False, **SMALL)
    assert off == rep
    on = track.evaluate_stretch(None, x, 1.5, phases=("vocoder_locked", "zero"), link_channels=True, **SMALL)
    assert list(on) == ["n_samples", "n_out", "sr", "stretch", "n_clips", "reset_below", "metrics", "link_channels", "mid_metrics"]
    assert on["metrics"]["zero"] == rep["metrics"]["zero"] and list(on["mid_metrics"]) == ["vocoder_locked", "zero"]


# ---- command line --------------------------------------------------------------------------------------------------------

def test_reconstruct_cli_links_the_channels_of_a_stereo_file(tmp_path):
    from scipy.io import wavfile
    wav, out, rep = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "stretch.json"
    x = kref.stereo_melody(seconds=1.2)[:, 8000:12000]
    wavfile.write(str(wav), 16000, np.ascontiguousarray(x.T * np.float32(0.25)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--input", str(wav), "--output", str(out),
                        "--channels", "16", "--hop", "8", "--frames", "24", "--overlap_frames", "4", "--stereo", "--stretch", "1.5",
                        "--phase", "vocoder_locked", "--link_channels", "--stretch_report", str(rep)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Stretch report" in r.stdout and "consistency of the channel mean" in r.stdout
    sr, y = wavfile.read(str(out))
    assert sr == 16000 and y.shape == (6000, 2) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    report = json.load(open(rep))
    assert report["link_channels"] is True and list(report["mid_metrics"]) == list(report["metrics"]) == ["vocoder_locked", "vocoder", "zero"]
    assert (report["n_samples"], report["n_out"], report["stretch"]) == (4000, 6000, 1.5) and report["flags"]["link_channels"] is True
    assert "audio" not in report
