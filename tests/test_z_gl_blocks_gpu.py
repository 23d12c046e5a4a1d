"""GPU: the Griffin-Lim building blocks of csrc/stft.hip one by one -- the projection onto the target magnitudes (gl_project_kernel),
the overlap-add of (n_fft, frames)-major frames (ola_nt_kernel with its per-clip peak words) -- and the phase range of ISTFT mode 0
(pg_sincos, pg_fastmath.h).  tests/test_signal_gpu.py reaches the first two only through audio.griffin_lim, after several iterations.

References are numpy float64 of the fp32 inputs; the bounds follow from the kernels' operation order and are derived in the
docstrings; DESIGN.md section 4.2 lists the largest errors observed next to them, and each test prints them before it asserts.
Inputs and outputs sit in the middle of sentinel-filled 1-D buffers whose guards are checked.

Named test_z_* so that it is collected behind the older modules."""
import functools

import numpy as np
import pytest
import torch

from phasegen import detgen

pytestmark = pytest.mark.gpu
F32 = np.float32
SENT = -77.0


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _embedded(shape, guard, fill=SENT, inner=None):
    """(buffer, view): a tensor of `shape` in the middle of a 1-D buffer of `fill`, `guard` elements on either side; the view itself
    starts as `inner` (NaN by default)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), fill, device=_dev())
    v = buf[guard:guard + n].view(*shape)
    v.fill_(float("nan") if inner is None else inner)
    return buf, v


def _guards_intact(buf, guard, fill=SENT):
    return bool((buf[:guard] == fill).all()) and bool((buf[buf.numel() - guard:] == fill).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# gl_project
# ---------------------------------------------------------------------------------------------------------------------
# (bins, frames, clips; 0 = the unbatched 2-D form).  1025 x 1031 = 1 056 775 cells > 4096 * 256: the grid-stride loop runs
PROJECT_CASES = [(3, 1, 0), (3, 7, 3), (17, 33, 2), (1025, 128, 1), (1025, 1031, 1)]
# planted (re, im): zeros of either sign (angle(0) = 0), the negative real axis with im = -0.0 (np.angle of re + 1j * im gives +pi:
# the imaginary -0.0 becomes +0.0), tiny and huge cells (|S| <= 1e30: hypotf overflows above), fp32 denormals
PLANTED = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-1.0, -0.0), (1e-30, 1e-30), (-1e30, 1e30), (1e-40, 0.0), (1e-40, 1.0)]


@functools.lru_cache(maxsize=None)
def _project_inputs(case):
    bins, frames, clips = case
    n = max(clips, 1)
    cells = bins * frames
    S = detgen.normal(351, (n, 2, bins, frames)) * (F32(10.0) ** detgen.uniform(352, (n, 2, bins, frames), -3.0, 3.0))
    mag = np.abs(detgen.normal(353, (n, bins, frames))).astype(F32)
    mag.reshape(n, -1)[:, 2::5] = 0.0                      # exact zeros
    where = []
    if cells >= 4 * len(PLANTED):
        for i, (re, im) in enumerate(PLANTED):
            e = 3 + i * (cells // len(PLANTED))
            S.reshape(n, 2, -1)[:, 0, e], S.reshape(n, 2, -1)[:, 1, e] = re, im
            mag.reshape(n, -1)[:, e] = 0.5 + i
            where.append(e)
    return S.astype(F32), mag, tuple(where)


def _project_ref(S, mag):
    """new_spec = mag * exp(1j * angle(re + 1j * im)) in float64, with pg_complex_from_parts' signed-zero arithmetic (pg_common.h)"""
    re, im = S[:, 0].astype(np.float64), S[:, 1].astype(np.float64)
    t = im * 0.0 - 0.0
    re2, im2 = re + t, 0.0 + (im + 0.0)
    th = np.arctan2(im2, re2)
    m = mag.astype(np.float64)
    return m * np.cos(th), m * np.sin(th)


@pytest.mark.parametrize("case", PROJECT_CASES, ids=lambda c: "bins%d-frames%d-n%d" % c)
def test_gl_project(case):
    """nr = m re / hypotf(re, im), ni = m im / hypotf(re, im): hypotf is within 1 ulp, then one division and one product, three
    roundings of 6e-8: |nr - m cos(theta)| and |ni - m sin(theta)| <= 3e-7 m per cell (exactly 0 where m = 0).
    Layout of the GEMM operand x (2 bins - 2, frames): rows 0 .. bins-1 are the real plane, rows bins .. 2 bins - 3 the imaginary
    rows 1 .. bins-2 -- every row of x is compared bit for bit with its row of spec_out, so the imaginary parts of DC and Nyquist
    appear nowhere in it."""
    from phasegen import ops
    bins, frames, clips = case
    n = max(clips, 1)
    S, mag, where = _project_inputs(case)
    guard = max(64, frames)
    lead = (n,) if clips else ()
    Sd, md = _cuda(S).view(*lead, 2, bins, frames), _cuda(mag).view(*lead, bins, frames)
    xbuf, x = _embedded(lead + (2 * bins - 2, frames), guard)
    sbuf, so = _embedded(lead + (2, bins, frames), guard)
    ops.gl_project(Sd, md, x, so)
    xa, sa = x.view(n, 2 * bins - 2, frames), so.view(n, 2, bins, frames)
    assert _guards_intact(xbuf, guard) and _guards_intact(sbuf, guard)
    assert torch.equal(_bits(xa[:, :bins]), _bits(sa[:, 0]))
    assert torch.equal(_bits(xa[:, bins:]), _bits(sa[:, 1, 1:bins - 1]))
    nr, ni = sa[:, 0].cpu().numpy(), sa[:, 1].cpu().numpy()
    wr, wi = _project_ref(S, mag)
    m = mag.astype(np.float64)
    pos = m > 0
    err = max(float((np.abs(nr - wr)[pos] / m[pos]).max()), float((np.abs(ni - wi)[pos] / m[pos]).max()))
    print(f"gl_project {case}: max |error| / m = {err:.3g} (3e-7)")
    assert err <= 3e-7
    assert not nr[~pos].any() and not ni[~pos].any()
    if where:
        fr, fi, fm = nr.reshape(n, -1), ni.reshape(n, -1), mag.reshape(n, -1)
        for i in range(3):                                                    # angle(0) = 0
            assert np.array_equal(fr[:, where[i]], fm[:, where[i]]) and not fi[:, where[i]].any()
        assert np.array_equal(fr[:, where[3]], -fm[:, where[3]])              # (-1, -0.0): angle +pi ...
        assert not fi[:, where[3]].any() and not np.signbit(fi[:, where[3]]).any()      # ... so ni = m * (+0 / 1) = +0, not -0
    # without the [re; im] copy: the same x
    x2buf, x2 = _embedded(lead + (2 * bins - 2, frames), guard)
    ops.gl_project(Sd, md, x2)
    assert torch.equal(_bits(x2), _bits(x)) and _guards_intact(x2buf, guard)
    # a clip of a batch == the clip alone
    if clips > 1:
        for c in range(clips):
            x1 = torch.full((2 * bins - 2, frames), float("nan"), device=_dev())
            ops.gl_project(Sd[c].contiguous(), md[c].contiguous(), x1)
            assert torch.equal(_bits(x1), _bits(xa[c]))


# ---------------------------------------------------------------------------------------------------------------------
# ola_nt
# ---------------------------------------------------------------------------------------------------------------------
# (n_fft, hop, frames, clips; 0 = the unbatched form); hops that do not divide n_fft; the Griffin-Lim shape; 263 168 samples >
# 1024 * 256: the grid-stride loop.  hop <= n_fft / 2 throughout, so that every sample's window-sum-square is >= 0.25.
OLA_CASES = [(4, 2, 2, 0), (6, 3, 4, 1), (16, 5, 11, 3), (30, 7, 9, 2), (64, 16, 7, 64), (2046, 512, 128, 2), (2046, 512, 515, 1)]


@functools.lru_cache(maxsize=None)
def _ola_frames(case):
    N, hop, frames, clips = case
    return detgen.normal(361, (max(clips, 1), N, frames))


def _ola_ref(fr, hop):
    """y[i] = sum_t fr[n, t] / sum_t w(n)^2, n = i + n_fft / 2 - t hop in [0, n_fft), w the periodic Hann window; float64.
    Returns y and the bound's scale sum_t |fr[n, t]| / sum_t w(n)^2."""
    n, N, frames = fr.shape
    length = hop * (frames - 1)
    w2 = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)) ** 2
    f64 = fr.astype(np.float64)
    num, mass, wss = np.zeros((n, length)), np.zeros((n, length)), np.zeros(length)
    for t in range(frames):
        i0, i1 = max(0, t * hop - N // 2), min(length, t * hop - N // 2 + N)
        if i1 <= i0:
            continue
        n0, n1 = i0 + N // 2 - t * hop, i1 + N // 2 - t * hop
        num[:, i0:i1] += f64[:, n0:n1, t]
        mass[:, i0:i1] += np.abs(f64[:, n0:n1, t])
        wss[i0:i1] += w2[n0:n1]
    assert wss.min() >= 0.25
    return num / wss, mass / wss


def _ola(fr_np, case, normalize, scale=1.0):
    """run ops.ola_nt on frames embedded between sentinel guards (a frame index one past a clip's rows would read the sentinel);
    returns the (clips, length) output as numpy"""
    from phasegen import ops
    N, hop, frames, clips = case
    n = max(clips, 1)
    lead = (n,) if clips else ()
    guard = max(64, 2 * frames)
    fbuf, fr = _embedded(lead + (N, frames), guard, fill=1e30)
    fr.copy_(_cuda(fr_np * F32(scale)).view(*lead, N, frames))
    abuf, audio = _embedded(lead + (hop * (frames - 1),), 64)
    ops.ola_nt(fr, hop, audio, normalize=normalize)
    assert _guards_intact(abuf, 64)
    return audio.view(n, -1).cpu().numpy()


@pytest.mark.parametrize("case", OLA_CASES, ids=lambda c: "nfft%d-hop%d-frames%d-n%d" % c)
def test_ola_nt(case):
    """The kernel adds the <= ceil(n_fft / hop) frame values of a sample in sequence, adds the squares of the fp32 window
    (0.5 - 0.5 cospif: ~1e-7 absolute, harmless against a sum >= 0.25) and divides: a few roundings of 6e-8 on sum|fr| / wss and
    <= 1e-6 relative on wss: |y - ref| <= 2e-6 sum_t|fr| / wss per sample.
    Normalised: the kernel divides its own un-normalised output by its own per-clip peak in fp32 (correctly rounded), so that output
    is reproduced bit for bit, every clip's peak is exactly 1, and an all-zero clip (peak 0: left as it is) stays zero.
    A clip of a batch equals the clip alone bit for bit (the sum order of a sample depends on nothing else)."""
    N, hop, frames, clips = case
    n = max(clips, 1)
    fr = _ola_frames(case).copy()
    zero_clip = 1 if n >= 3 else None
    if zero_clip is not None:
        fr[zero_clip] = 0.0
    want, scale = _ola_ref(fr, hop)
    y = _ola(fr, case, False)
    live = scale > 0
    err = float((np.abs(y - want)[live] / scale[live]).max())
    print(f"ola_nt {case}: max |error| / (sum|fr| / wss) = {err:.3g} (2e-6)")
    assert err <= 2e-6
    yn = _ola(fr, case, True)
    pk = np.abs(y).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        expect = np.where(pk > 0, y / pk, y).astype(F32)
    assert np.array_equal(yn.view(np.int32), expect.view(np.int32))
    for c in range(n):
        assert np.abs(yn[c]).max() == (0.0 if c == zero_clip else 1.0)
    if zero_clip is not None:
        assert not y[zero_clip].any() and not yn[zero_clip].any()
    if clips > 1:
        for c in sorted({0, zero_clip or 0, n - 1}):
            one = _ola(fr[c:c + 1], (N, hop, frames, 0), False)
            assert np.array_equal(one.view(np.int32), y[c:c + 1].view(np.int32))


@pytest.mark.parametrize("case", [(30, 7, 9, 2), (2046, 512, 128, 2)], ids=lambda c: "nfft%d-hop%d-frames%d-n%d" % c)
def test_ola_nt_peak_words_do_not_outlive_a_call(case):
    """The per-clip peak words live in a workspace that the next call on the stream reuses: after a call on frames scaled by 1000,
    the same call at scale 1 must still normalise to a peak of exactly 1 (and to the bits of a first call)."""
    fr = _ola_frames(case)
    fresh = _ola(fr, case, True)
    loud = _ola(fr, case, True, scale=1000.0)
    after = _ola(fr, case, True)
    assert (np.abs(loud).max(axis=1) == 1.0).all()
    assert (np.abs(after).max(axis=1) == 1.0).all()
    assert np.array_equal(after.view(np.int32), fresh.view(np.int32))


def test_ola_nt_refuses_more_than_64_clips():
    from phasegen import ops
    fr = torch.zeros(65, 4, 2, device=_dev())
    audio = torch.full((65, 2), SENT, device=_dev())
    with pytest.raises(RuntimeError, match="64 clips"):
        ops.ola_nt(fr, 2, audio)
    torch.cuda.synchronize()
    assert bool((audio == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# ISTFT mode 0 over the documented phase range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,frames,hop", [(64, 36, 32), (1024, 16, 512)])
def test_istft_mode0_phase_range(bins, frames, hop):
    """pg_sincos documents <= 2.5e-7 + 6e-8 |phi| absolute (the rounding of phi / pi) and |phi| <= 100.  With phi uniform in
    +-100 -- and one bin row of exact multiples of pi / 2 rounded to fp32 -- mode 0 ((exp(m) - 1) e^{j phi} formed on the device)
    must equal mode 1 fed the spectrum formed in float64 within the transform tolerance of test_istft_synthesis_arithmetic plus twice
    the reduction term: relmax <= 1e-5 + 2 * 6e-8 * 100 = 2.2e-5."""
    from phasegen import ops
    nsig = 2
    m = np.abs(detgen.normal(41, (nsig, bins, frames))).astype(F32) * F32(2.0)
    phi = detgen.uniform(371, (nsig, bins, frames), -100.0, 100.0)
    k = (np.arange(nsig * frames).reshape(nsig, frames) * 7) % 127 - 63          # |k pi / 2| <= 99
    phi[:, bins // 3, :] = (k * (np.pi / 2)).astype(F32)
    assert np.abs(phi).max() <= 100.0
    amp = np.expm1(m.astype(np.float64))
    zr = (amp * np.cos(phi.astype(np.float64))).astype(F32)
    zi = (amp * np.sin(phi.astype(np.float64))).astype(F32)
    for norm in (False, True):
        y0 = ops.istft(_cuda(m), _cuda(phi), hop, mode=0, normalize=norm).cpu().numpy().astype(np.float64)
        y1 = ops.istft(_cuda(zr), _cuda(zi), hop, mode=1, normalize=norm).cpu().numpy().astype(np.float64)
        err = float(np.abs(y0 - y1).max() / np.abs(y1).max())
        print(f"istft mode 0 vs 1, bins {bins} frames {frames} normalize {norm}: relmax {err:.3g} (2.2e-5)")
        assert err <= 2.2e-5
