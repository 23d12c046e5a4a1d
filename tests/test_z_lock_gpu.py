"""GPU: identity phase locking -- pg_phase_lock BIT FOR BIT against the numpy restatement of its contract (tests/_lock_ref.py) at every
chunk boundary of its three-launch scan, its layouts, store paths and special inputs, and the track level built on it
(phasegen.track phase="vocoder_locked", evaluate_stretch, pitch_shift, reconstruct.py --phase vocoder_locked).

Bounds.  The kernel's sums are integers modulo 2^32 and its comparisons are plain IEEE fp32 comparisons, so every comparison with the
restatement is exact.  The ordering on the melody: the float64 chain gives SC(locked) / SC(plain) = 0.0631 / 0.2022 = 0.31 at stretch
1.5 with the module's floor (tests/test_lock_host.py), so 0.5 holds with room.  The locked figure against the float64 chain: the
margin of tests/test_z_vocoder_gpu.py::test_consistency_against_the_float64_chain, 1e-5 relative, between metrics.consistency on the
device and _vocoder_ref.consistency64 of the restatement's phase -- the restatement run on the device's analysis planes (whose bits the
kernel reproduces) and imposed on the device's magnitudes, the ISTFT and the STFT in float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lock_ref as lref
import _vocoder_ref as ref
from phasegen import detgen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(n_fft=32, hop_length=8, frames=24, overlap_frames=4)


def bits(t):
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def same_bits(got, want):
    return torch.equal(torch.from_numpy(bits(got)), torch.from_numpy(bits(want)))


def offset_view(t):
    """The same values one element off the allocation's 16-byte grid: the element-wise path."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def planes(seed, n_ch, bins, F_src):
    """A uniform in (-pi, pi], M uniform in [0, 1): with reset_below at M's median about half of the peaks reset."""
    rs = np.random.RandomState(seed)
    A = (-rs.uniform(-np.pi, np.pi, (n_ch, bins, F_src))).astype(np.float32)
    M = rs.uniform(0.0, 1.0, (n_ch, bins, F_src)).astype(np.float32)
    return A, M


def f_src_for(F_out, spo):
    """Enough source frames that no position is clamped: floor((F_out - 1) spo) + 2."""
    return int(np.floor((F_out - 1) * spo)) + 2


def L():
    from phasegen import ops
    return ops.PHASE_LOCK_CHUNK


# ---- bit for bit against the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("spo", [1.0, 0.5, 2.0, 1 / 1.3, 4.0, 0.25])
def test_bitwise_against_the_restatement_at_every_chunk_boundary(spo):
    from phasegen import ops
    for F_out in (1, 2, L() - 1, L(), L() + 1, 3 * L() + 5):
        for n_ch, bins in ((1, 5), (3, 5), (1, 130), (3, 65)):
            F_src = f_src_for(F_out, spo)
            A, M = planes(1000 + F_out + bins, n_ch, bins, F_src)
            floor = float(np.median(M))
            got = ops.phase_lock(torch.from_numpy(A).cuda(), F_out, spo, logmag=torch.from_numpy(M).cuda(), reset_below=floor)
            assert tuple(got.shape) == (n_ch, bins, F_out) and got.dtype == torch.float32
            want = lref.phase_lock(A, F_out, spo, M, floor)
            assert np.abs(want).max() <= np.float32(np.pi)
            assert same_bits(got, want), (spo, F_out, n_ch, bins)


@pytest.mark.parametrize("bins", [1, 2, 3, 5, 63, 64, 65, 130])
def test_bitwise_for_every_width(bins):
    from phasegen import ops
    F_out = 3 * L() + 5
    for spo in (1 / 1.3, 2.0):
        A, M = planes(2000 + bins, 2, bins, f_src_for(F_out, spo))
        floor = float(np.median(M))
        Ad, Md = torch.from_numpy(A).cuda(), torch.from_numpy(M).cuda()
        assert same_bits(ops.phase_lock(Ad, F_out, spo, logmag=Md, reset_below=floor), lref.phase_lock(A, F_out, spo, M, floor)), (bins, spo)
        assert same_bits(ops.phase_lock(Ad, F_out, spo, logmag=Md), lref.phase_lock(A, F_out, spo, M, 0.0)), (bins, spo)      # never resets


def test_the_source_ends_early():
    """Positions 0 .. 2 L + 2 of 7 source frames at half rate: from frame 12 on i1 == i0, the advance is zero and -- the peaks being
    those of one and the same source frame -- every frame repeats."""
    from phasegen import ops
    A, M = planes(11, 2, 37, 7)
    F_out = 2 * L() + 3
    got = ops.phase_lock(torch.from_numpy(A).cuda(), F_out, 0.5, logmag=torch.from_numpy(M).cuda(), reset_below=0.4)
    assert same_bits(got, lref.phase_lock(A, F_out, 0.5, M, 0.4))
    g = got.cpu().numpy()
    assert np.array_equal(g[..., 13:], np.repeat(g[..., 13:14], F_out - 13, -1)) and not np.array_equal(g[..., 11], g[..., 12])


def test_an_odd_width_of_several_bins_per_thread():
    """bins = 1025 (two bins per thread, a last word of the peak mask with one bin in it) x 2 L + 1 frames, once."""
    from phasegen import ops
    F_out = 2 * L() + 1
    A, M = planes(12, 1, 1025, f_src_for(F_out, 1 / 1.5))
    floor = float(np.median(M))
    got = ops.phase_lock(torch.from_numpy(A).cuda(), F_out, 1 / 1.5, logmag=torch.from_numpy(M).cuda(), reset_below=floor)
    assert same_bits(got, lref.phase_lock(A, F_out, 1 / 1.5, M, floor))


def sparse_planes(seed, bins, F_src):
    """Planes whose peak bitmask has long runs of EMPTY 64-bin words, so that a bin's nearest peak lies many words away: random
    magnitudes, 1000 times smaller in bins [bins / 40, 3 bins / 4) (with the floor 5e-4 about half of the peaks there reset, and
    none outside), and exactly zero in bins [bins / 6, 5 bins / 8) -- no bin of that plateau is a peak (its first bin has a larger
    neighbour below), and its middle is equally far from the peaks on either side only by chance."""
    A, M = planes(seed, 1, bins, F_src)
    M[:, bins // 40:3 * bins // 4] *= 1e-3
    M[:, bins // 6:5 * bins // 8] = 0.0
    return A, M


@pytest.mark.parametrize("bins", [4096, 3000, 1024, 260])
def test_wide_planes_with_empty_words_in_the_peak_mask(bins):
    """Four bins per thread without a staged window (4096: all 64 words of the mask, the largest LDS footprint), three (3000), one
    with a window (1024, 260), each at a rate != 1 over three chunks, so that the advances are not zero and the output depends on
    the peak maps, on their composition and on the carry; 29 (21, 7, 1) words of the mask are empty in every frame and the bins under
    them gather from the nearest non-empty word on either side."""
    from phasegen import ops
    F_out, spo = 2 * L() + 3, 1 / 1.5
    A, M = sparse_planes(13 + bins, bins, f_src_for(F_out, spo))
    empty = [not lref.peaks(M[0, :, f])[w * 64:(w + 1) * 64].any() for f in range(M.shape[2]) for w in range(-(-bins // 64))]
    assert sum(empty) >= M.shape[2] * {4096: 27, 3000: 19, 1024: 6, 260: 1}[bins]
    want, T = lref.phase_lock(A, F_out, spo, M, 5e-4, return_rotation=True)
    b, P = bins // 3, lref.peak_map(M[0, :, ref.positions(F_out, spo, A.shape[-1])[0][-1]])
    assert abs(P[b] - b) >= min(64, bins // 8) and T[0, b].any() and T[0, b, -1] == T[0, P[b], -1]      # a bin locked to a peak far off
    assert T[0, :, -1].any() and not T[0, bins // 20:3 * bins // 4, 1:].all()                          # regions rotate, and some reset
    assert not np.array_equal(want, ref.angle_of(ref.q(A[..., ref.positions(F_out, spo, A.shape[-1])[0]])))     # not the analysis phase
    got = ops.phase_lock(torch.from_numpy(A).cuda(), F_out, spo, logmag=torch.from_numpy(M).cuda(), reset_below=5e-4)
    assert same_bits(got, want)
    never = ops.phase_lock(torch.from_numpy(A).cuda(), F_out, spo, logmag=torch.from_numpy(M).cuda())
    assert same_bits(never, lref.phase_lock(A, F_out, spo, M, 0.0)) and not same_bits(never, got)


def test_two_bins_per_thread_with_a_window():
    """bins = 2048: two bins per thread and still a staged window of source frames (the widest plane has none)."""
    from phasegen import ops
    F_out = L() + 8
    A, M = planes(21, 1, 2048, f_src_for(F_out, 1 / 1.5))
    floor = float(np.median(M))
    got = ops.phase_lock(torch.from_numpy(A).cuda(), F_out, 1 / 1.5, logmag=torch.from_numpy(M).cuda(), reset_below=floor)
    assert same_bits(got, lref.phase_lock(A, F_out, 1 / 1.5, M, floor))


def test_positions_further_apart_than_the_staged_window():
    """src_per_out = 40 (the two positions of a frame are 39 source frames apart: no window holds them), a rate that mixes such
    frames with the clamped end of the source, and a position beyond the int64 range."""
    from phasegen import ops
    F_out = L() + 3
    for bins in (5, 130):
        A, M = planes(22 + bins, 2, bins, 700)
        Ad, Md = torch.from_numpy(A).cuda(), torch.from_numpy(M).cuda()
        for spo in (40.0, 33.0, 1e300):                                     # 40 (L + 2) > 700: the last frames sit on the source's end
            got = ops.phase_lock(Ad, F_out, spo, logmag=Md, reset_below=0.5)
            assert same_bits(got, lref.phase_lock(A, F_out, spo, M, 0.5)), (bins, spo)


# ---- where no locking can occur: pg_phase_vocoder's bits ----------------------------------------------------------------------

def test_one_bin_and_an_all_nan_magnitude_equal_the_plain_vocoder():
    from phasegen import ops
    F_out = 3 * L() + 5
    A, M = planes(14, 3, 5, f_src_for(F_out, 0.7))
    Ad, Md = torch.from_numpy(A).cuda(), torch.from_numpy(M).cuda()
    A1, M1 = Ad[:, :1].contiguous(), Md[:, :1].contiguous()
    assert same_bits(ops.phase_lock(A1, F_out, 0.7, logmag=M1, reset_below=0.5), ops.phase_vocoder(A1, F_out, 0.7, logmag=M1, reset_below=0.5))
    nan = torch.full_like(Md, float("nan"))
    assert same_bits(ops.phase_lock(Ad, F_out, 0.7, logmag=nan, reset_below=0.5), ops.phase_vocoder(Ad, F_out, 0.7, logmag=nan, reset_below=0.5))
    assert same_bits(ops.phase_lock(Ad, F_out, 0.7, logmag=nan, reset_below=0.5), ops.phase_vocoder(Ad, F_out, 0.7))
    # and it DOES lock otherwise
    assert not same_bits(ops.phase_lock(Ad, F_out, 0.7, logmag=Md), ops.phase_vocoder(Ad, F_out, 0.7, logmag=Md))


def test_rate_one_returns_the_analysis_phase():
    from phasegen import ops
    A, M = planes(15, 2, 65, 2 * L() + 7)
    got = ops.phase_lock(torch.from_numpy(A).cuda(), 2 * L() + 7, 1.0, logmag=torch.from_numpy(M).cuda(), reset_below=0.5)
    assert same_bits(got, ref.angle_of(ref.q(A)))


# ---- layouts -------------------------------------------------------------------------------------------------------------

def test_planes_of_a_polar_tensor_are_read_in_place():
    from phasegen import ops
    rs = np.random.RandomState(16)
    F = 2 * L() + 9
    pol = np.stack([rs.uniform(0, 1, (3, 21, F)), rs.uniform(-np.pi, np.pi, (3, 21, F))], 1).astype(np.float32)     # (n_ch, 2, bins, F)
    pd = torch.from_numpy(pol).cuda()
    assert not pd[:, 1].is_contiguous() and pd[:, 1].stride(0) == 2 * 21 * F
    for F_out, spo in ((F, 1.0), (3 * L() + 2, 1 / 1.5)):
        got = ops.phase_lock(pd[:, 1], F_out, spo, logmag=pd[:, 0], reset_below=0.5)
        assert same_bits(got, lref.phase_lock(pol[:, 1], F_out, spo, pol[:, 0], 0.5))
        assert same_bits(got, ops.phase_lock(pd[:, 1].contiguous(), F_out, spo, logmag=pd[:, 0].contiguous(), reset_below=0.5))


def test_a_channel_alone_has_the_bits_it_has_in_a_batch():
    from phasegen import ops
    F_out = 2 * L() + 1
    A, M = planes(17, 3, 21, f_src_for(F_out, 0.8))
    Ad, Md = torch.from_numpy(A).cuda(), torch.from_numpy(M).cuda()
    both = ops.phase_lock(Ad, F_out, 0.8, logmag=Md, reset_below=0.5)
    for c in range(3):
        alone = ops.phase_lock(Ad[c:c + 1], F_out, 0.8, logmag=Md[c:c + 1], reset_below=0.5)
        assert same_bits(alone[0], both[c]), c
    assert same_bits(ops.phase_lock(Ad[1:], F_out, 0.8, logmag=Md[1:], reset_below=0.5), both[1:])


def test_element_wise_store_path_equals_the_16_byte_path():
    from phasegen import ops
    A, M = planes(18, 2, 21, 3 * L())
    Ad, Md = torch.from_numpy(A).cuda(), torch.from_numpy(M).cuda()
    for F_out in (L(), 2 * L() + 4):                                        # multiples of 4: the 16-byte path when aligned
        wide = ops.phase_lock(Ad, F_out, 0.9, logmag=Md, reset_below=0.5)
        assert wide.data_ptr() % 16 == 0
        out = offset_view(torch.zeros_like(wide))
        assert ops.phase_lock(Ad, F_out, 0.9, logmag=Md, reset_below=0.5, out=out) is out
        assert same_bits(out, wide)
        assert same_bits(ops.phase_lock(offset_view(Ad), F_out, 0.9, logmag=offset_view(Md), reset_below=0.5), wide)
        assert same_bits(wide, lref.phase_lock(A, F_out, 0.9, M, 0.5))
        odd = ops.phase_lock(Ad, F_out + 1, 0.9, logmag=Md, reset_below=0.5)          # F_out % 4 == 1: element-wise
        assert same_bits(odd[..., :F_out], wide) and same_bits(odd, lref.phase_lock(A, F_out + 1, 0.9, M, 0.5))


# ---- special inputs ------------------------------------------------------------------------------------------------------

def test_plateaus_ties_infinities_and_nans_in_the_magnitude():
    from phasegen import ops
    inf, nan = np.inf, np.nan
    rows = [[1, 3, 3, 3, 1, 0, 0, 2, 0, 0, 0],                              # a plateau: its first bin is the peak
            [5, 0, 0, 0, 5, 0, 0, 0, 5, 0, 0],                              # exact ties between equal peaks: the lower one
            [0, inf, inf, 0, -inf, -inf, 1, 0, inf, 0, 0],                  # +-inf
            [0, 0, 7, nan, 0, 0, 9, 0, nan, 0, 8],                          # a NaN next to a peak disqualifies it
            [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],                              # all equal: bin 0 is the only peak
            [nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan]]        # no peak at all: every bin on its own
    F_out = L() + 5
    rs = np.random.RandomState(19)
    M = np.ascontiguousarray(np.array(rows, np.float32)[np.arange(F_out + 1) % 6].T[None])      # source frame f shows row f % 6
    assert M.shape == (1, 11, F_out + 1) and np.array_equal(M[0, :, 7], np.array(rows[1], np.float32), equal_nan=True)
    A = rs.uniform(-np.pi, np.pi, M.shape).astype(np.float32)
    assert list(lref.peak_map(M[0, :, 0])) == [1, 1, 1, 1, 1, 7, 7, 7, 7, 7, 7] and list(lref.peak_map(M[0, :, 1])) == [0, 0, 0, 4, 4, 4, 4, 8, 8, 8, 8]
    for floor in (0.0, 2.5):
        got = ops.phase_lock(torch.from_numpy(A).cuda(), F_out, 1 / 1.2, logmag=torch.from_numpy(M).cuda(), reset_below=floor)
        assert same_bits(got, lref.phase_lock(A, F_out, 1 / 1.2, M, floor)), floor


def test_values_that_quantise_to_zero_and_the_branch_cut():
    from phasegen import ops
    pi = np.float32(np.pi)
    row = np.array([0.5, np.nan, 1.0, np.inf, -np.inf, 2.0, 2.0 ** 20 * (1 + 2.0 ** -23), -3e6, 2.5, pi, -pi, pi, 2.0 ** 20, -7.0], np.float32)
    A = np.stack([np.roll(row, k) for k in range(5)])[None]                 # (1, 5, 14)
    M = np.random.RandomState(20).uniform(0, 1, A.shape).astype(np.float32)
    Ad, Md = torch.from_numpy(A).cuda(), torch.from_numpy(M).cuda()
    for F_out, spo in ((14, 1.0), (28, 0.5), (40, 1 / 3.0)):
        got = ops.phase_lock(Ad, F_out, spo, logmag=Md, reset_below=0.3)
        want = lref.phase_lock(A, F_out, spo, M, 0.3)
        assert same_bits(got, want) and np.isfinite(want).all() and np.abs(want).max() <= pi
    clean = np.where(np.isfinite(A) & (np.abs(A) <= 2.0 ** 20), A, 0).astype(np.float32)
    assert same_bits(ops.phase_lock(Ad, 14, 1.0, logmag=Md), ref.angle_of(ref.q(clean)))


# ---- argument errors -----------------------------------------------------------------------------------------------------

def test_argument_errors():
    import ctypes
    from phasegen import _lib, ops
    A = torch.zeros(2, 5, 19, device="cuda")
    with pytest.raises(ValueError, match="logmag"):
        ops.phase_lock(A, 25)
    for bad in (dict(F_out=0), dict(src_per_out=0.0), dict(src_per_out=float("nan")), dict(reset_below=-1.0), dict(reset_below=float("inf")),
                dict(logmag=torch.zeros(2, 5, 18, device="cuda")), dict(logmag=torch.zeros(2, 5, 19)), dict(out=torch.zeros(2, 5, 24, device="cuda"))):
        with pytest.raises(ValueError):
            ops.phase_lock(A, **{**dict(F_out=25, logmag=torch.zeros_like(A)), **bad})
    for view in (A[:, :, ::2], A.transpose(1, 2), A.double(), A[0]):
        with pytest.raises(ValueError):
            ops.phase_lock(view, 25, logmag=view)
    wide = torch.zeros(1, 4097, 3, device="cuda")
    with pytest.raises(RuntimeError, match="4096 bins"):
        ops.phase_lock(wide, 3, logmag=wide)
    # the workspace one byte short, with real pointers: refused before any launch
    lib = _lib.load()
    M, out = torch.zeros_like(A), torch.full((2, 5, 25), 7.0, device="cuda")
    a = _lib.PhaseLockArgs()
    a.n_ch, a.bins, a.F_src, a.F_out, a.src_per_out, a.reset_below = 2, 5, 19, 25, 0.75, 0.05
    a.A, a.M, a.out, a.a_stride, a.m_stride = A.data_ptr(), M.data_ptr(), out.data_ptr(), 95, 95
    need = lib.pg_workspace_bytes_phase_lock(ctypes.byref(a))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert lib.pg_phase_lock(ctypes.byref(a), None) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    a.bins, a.workspace_bytes = 4097, 1 << 40
    assert lib.pg_phase_lock(ctypes.byref(a), None) == _lib.ERR_SHAPE


# ---- track level ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def melody():
    return ref.melody()


@pytest.mark.parametrize("stretch", [1.0, 1.5, 0.75])
def test_reconstruct_track_with_the_locked_vocoder(melody, stretch):
    from phasegen.track import reconstruct_track
    out = reconstruct_track(None, melody, phase="vocoder_locked", join="spectral", stretch=stretch)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (round(melody.shape[0] * stretch),)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) == 1.0
    if stretch == 1.0:          # the analysis phase's track: phase="vocoder" returns the same phase there, so the same bits
        assert same_bits(out, reconstruct_track(None, melody, phase="vocoder", join="spectral"))
        x = melody[:20000]
        a = reconstruct_track(None, x, phase="vocoder_locked", join="spectral", normalize=False, stats=(0.0, 2.0)).cpu().numpy().astype(np.float64)
        b = reconstruct_track(None, x, phase="original", join="spectral", normalize=False, stats=(0.0, 2.0)).cpu().numpy().astype(np.float64)
        e = np.abs(a - b).max() / np.abs(b).max()
        print(f"\nlocked vocoder at stretch 1 against the analysis' own phase: {e:.3e} of max-abs (bound 5e-5)")
        assert e < 5e-5         # (the round trip's tolerance of tests/test_z_spectral_gpu.py, as for phase="vocoder")


def test_evaluate_stretch_orders_locked_before_plain_before_zero(melody):
    from phasegen import metrics, ops, track
    rep = track.evaluate_stretch(None, melody, 1.5, phases=("vocoder_locked", "vocoder", "zero"), return_audio=True)
    assert list(rep["metrics"]) == ["vocoder_locked", "vocoder", "zero"] and rep["reset_below"] == track.VOCODER_RESET_BELOW
    lk, v, z = (rep["metrics"][p]["spectral_convergence"] for p in ("vocoder_locked", "vocoder", "zero"))
    print(f"\nmelody at stretch 1.5 on the device: SC locked {lk:.4f}, vocoder {v:.4f}, zero {z:.4f}")
    assert lk < 0.5 * v and v < z
    assert tuple(rep["audio"]["vocoder_locked"].shape) == (144000,)
    raw = track.reconstruct_track(None, melody, phase="vocoder_locked", join="spectral", stretch=1.5, normalize=False)
    assert same_bits(rep["audio"]["vocoder_locked"], raw)
    # against the float64 chain on the restatement's phase: the restatement on the device's analysis, imposed on the device's magnitudes
    an = track._analyse_spectral(melody, 2048, 512, 128, 32, None, None, 16000, "kaiser_best", 1.5)
    F_out = an.plan.F_out
    with torch.no_grad():
        dmag, full = track._invert_spectral(an, None, "vocoder_locked", 512, 128, 64)
        dph = ops.phase_lock(an.pol[:, 1], F_out, 1 / 1.5, logmag=an.pol[:, 0], reset_below=track.VOCODER_RESET_BELOW)
    pol = an.pol.cpu().numpy()
    ph = lref.phase_lock(pol[:, 1], F_out, 1 / 1.5, pol[:, 0], track.VOCODER_RESET_BELOW)
    assert same_bits(dph, ph)
    want = ref.consistency64(dmag.cpu().numpy(), 2048, 512, phase=ph)["spectral_convergence"]
    again = metrics.consistency(dmag, full, 2048, 512)["spectral_convergence"]
    print(f"locked SC: device {lk:.7f} (again {again:.7f}), float64 chain on the restatement's phase {want:.7f}")
    assert again == lk
    assert abs(lk - want) <= 1e-5 * want


def test_pitch_shift_with_the_locked_vocoder():
    from phasegen.track import pitch_shift
    x = detgen.normal(98, (2, 1000))
    out = pitch_shift(None, x, 5, stats=(0.1, 2.0), phase="vocoder_locked", **SMALL)
    assert tuple(out.shape) == (2, 1000) and bool(torch.isfinite(out).all()) and float(out.abs().max()) == 1.0


# ---- command line --------------------------------------------------------------------------------------------------------

def test_reconstruct_cli_with_the_locked_vocoder_and_a_stretch_report(tmp_path):
    from scipy.io import wavfile
    wav, out, rep = tmp_path / "in.wav", tmp_path / "out.wav", tmp_path / "stretch.json"
    wavfile.write(str(wav), 16000, detgen.normal(99, (4000,)).astype(np.float32) * 0.1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "unet-phasegen_amd", "reconstruct.py"), "--input", str(wav), "--output", str(out),
                        "--channels", "16", "--hop", "8", "--frames", "24", "--overlap_frames", "4", "--phase", "vocoder_locked",
                        "--stretch", "1.5", "--stretch_report", str(rep)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Stretch report" in r.stdout and "vocoder_locked spectral convergence" in r.stdout and "zero spectral convergence" in r.stdout
    sr, y = wavfile.read(str(out))
    assert sr == 16000 and y.shape == (6000,) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() == 1.0
    report = json.load(open(rep))
    assert list(report["metrics"]) == ["vocoder_locked", "vocoder", "zero"] and "audio" not in report
    assert (report["n_samples"], report["n_out"], report["stretch"]) == (4000, 6000, 1.5)
    for m in report["metrics"].values():
        assert set(m) == {"spectral_convergence", "lsd_db", "n_frames", "channels"}
