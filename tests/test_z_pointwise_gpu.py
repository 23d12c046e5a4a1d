"""GPU: the streaming kernels of csrc/pointwise.hip at the sizes where their loops take another trip and on the values where their
arithmetic can go wrong -- the fused loss (loss_partial_kernel / loss_final_kernel), Adam (adam_kernel / adam_thin_kernel) and the
bf16 row cast (cast_rows_kernel).

References are numpy float64 of the fp32 inputs the device gets (loss), a numpy float32 emulation with one rounding per operation
in the kernel's order (Adam: the library is built with -ffp-contract=off and `/` and sqrtf are correctly rounded, so the update is
pinned bit for bit), and fp32 torch on the CPU followed by .to(bfloat16) (row cast, bit patterns).  Every tolerance is derived in
the docstring of the test that uses it; DESIGN.md section 4.2 lists the largest errors observed next to the bounds.  Each test
prints the figures it is about to assert (pytest -s shows them).

Named test_z_* so that it is collected behind the older modules."""
import functools
import math

import numpy as np
import pytest
import torch

from phasegen import detgen

pytestmark = pytest.mark.gpu
SENT = -77.0
GUARD = 64
F32 = np.float32


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _embedded(n, fill=SENT, dtype=torch.float32):
    """(buffer, middle): n elements in the middle of a 1-D buffer that holds `fill` everywhere, GUARD elements on either side"""
    buf = torch.full((n + 2 * GUARD,), fill, device=_dev(), dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=SENT):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


# ---------------------------------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------------------------------
# (1, 1, 1); (2, 3, 5); 79 partials: lanes 0..14 of the final kernel add two each; 265 893 > 1024 * 256 elements: every one of the 1024
# workgroups runs, some threads take a second grid-stride trip, the final loop takes 16 trips
LOSS_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 40, 251), (3, 337, 263)]


@functools.lru_cache(maxsize=None)
def _loss_inputs(shape):
    """pred (B, 2C, L) = [phase; magnitude] and batch (B, 2, C, L) = [logmag; angle] as fp32 numpy arrays.  Phases ~ N(0, 4^2); every
    hundredth one (flat index 7, 107, ...) is +-1e4 (1 + u) or +-1e6 (1 + u), u in [0, 1): the network's output is unbounded and
    sincosf must still reduce it.  Target angles in (-pi, pi]."""
    B, C, L = shape
    n = B * C * L
    ph = (detgen.normal(301, (n,)) * 4.0).astype(F32)
    idx = np.arange(7, n, 100)
    big = np.array([1e4, -1e4, 1e6, -1e6], F32)[np.arange(idx.size) % 4]
    ph[idx] = big * (F32(1.0) + detgen.uniform(302, (idx.size,), 0.0, 1.0))
    mh = detgen.normal(303, (n,)) * F32(1.5)
    m = np.abs(detgen.normal(304, (n,))).astype(F32) * F32(2.0)
    th = -detgen.uniform(305, (n,), -3.1415925, 3.1415925)              # [lo, hi) negated: (-pi, pi]
    pred = np.concatenate([ph.reshape(B, C, L), mh.reshape(B, C, L)], axis=1)
    batch = np.stack([m.reshape(B, C, L), th.reshape(B, C, L)], axis=1)
    return np.ascontiguousarray(pred, F32), np.ascontiguousarray(batch, F32)


@functools.lru_cache(maxsize=None)
def _loss_ref(shape, mag_weight):
    """include/phasegen.h: loss = MSE(cos p, cos th) + MSE(sin p, sin th) + mag_weight * MSE(m^, m) and its gradient, in float64"""
    B, C, L = shape
    pred, batch = (a.astype(np.float64) for a in _loss_inputs(shape))
    p, mh, m, th = pred[:, :C], pred[:, C:], batch[:, 0], batch[:, 1]
    N = B * C * L
    dc, ds, dm = np.cos(p) - np.cos(th), np.sin(p) - np.sin(th), mh - m
    cos_l, sin_l, mag_l = (dc * dc).sum() / N, (ds * ds).sum() / N, (dm * dm).sum() / N
    s = 2.0 / N
    dphase = s * (ds * np.cos(p) - dc * np.sin(p))
    dmag = mag_weight * s * dm
    return np.array([cos_l + sin_l + mag_weight * mag_l, cos_l + sin_l, mag_l]), dphase, dmag, float(np.abs(dm).max())


@pytest.mark.parametrize("mag_weight", [0.2, 0.7])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_loss_against_float64(shape, mag_weight):
    """Bounds, with s = 2 / N:
    phase half of dpred = s (ds cos p - dc sin p).  sincosf is within OpenCL's 4 ulp (<= 2.4e-7 for values <= 1), so ds and dc (one
    subtraction each, |.| <= 2) carry <= 5e-7 + one rounding, each product <= 1.2e-6 with the factor's own error, their difference and
    the product with fl(s) three more roundings of values <= 2.9: |dpred - ref| <= 4e-6 s elementwise.
    magnitude half = fl(mag_weight) fl(s) (mh - m): the subtraction, the product of the scalars and the product with dm are three
    roundings, fl(mag_weight) and fl(s) two more conversions, 5 * 6e-8 = 3e-7: |dpred - ref| <= 1e-6 mag_weight s max|dm|.
    losses: sums of non-negative terms (squares of values that carry <= 5e-7) with <= 1e-6 relative error each in the sum, <= 2 fp32
    additions per thread and ~10 in the block tree (12 * 6e-8 = 7e-7 relative on a sum of non-negative terms), the sum over the
    partials and the division in double: 4e-6 relative on each of the three."""
    from phasegen import ops
    B, C, L = shape
    pred, batch = _loss_inputs(shape)
    want, dphase, dmag, dm_max = _loss_ref(shape, mag_weight)
    n = pred.size
    buf, mid = _embedded(n)
    dpred = mid.view(B, 2 * C, L)
    pd, bd = torch.from_numpy(pred).to(_dev()), torch.from_numpy(batch).to(_dev())
    out = ops.loss_fwd_bwd(pd, bd, dpred, mag_weight=mag_weight)
    got = out.cpu().numpy().astype(np.float64)
    d = dpred.cpu().numpy().astype(np.float64)
    s = 2.0 / (B * C * L)
    e_phase = float(np.abs(d[:, :C] - dphase).max()) / s
    e_mag = float(np.abs(d[:, C:] - dmag).max()) / (mag_weight * s * dm_max)
    e_loss = np.abs(got - want) / want
    print(f"loss {shape} w={mag_weight}: phase {e_phase:.3g} (4e-6)  mag {e_mag:.3g} (1e-6)  losses {e_loss.max():.3g} (4e-6)")
    assert _guards_intact(buf, n)
    assert e_phase <= 4e-6
    assert e_mag <= 1e-6
    assert (e_loss <= 4e-6).all(), (got, want)
    # evaluation: no gradient buffer -> the same three floats, bit for bit
    out_eval = ops.loss_fwd_bwd(pd, bd, None, mag_weight=mag_weight)
    assert torch.equal(out_eval.view(torch.int32), out.view(torch.int32))


def test_loss_does_not_read_stale_partials():
    """A call with 1024 partials, then one with a single partial on the same stream and workspace; then the workspace is filled with a
    NaN pattern and the small call is repeated.  All small results are bit-identical (and equal the float64 reference within the
    bound of test_loss_against_float64, checked there): loss_final_kernel reads the `blocks` partials of its own call only."""
    from phasegen import ops
    big, small = LOSS_SHAPES[3], LOSS_SHAPES[1]
    first = ops.loss_fwd_bwd(*(torch.from_numpy(a).to(_dev()) for a in _loss_inputs(small)))
    ops.loss_fwd_bwd(*(torch.from_numpy(a).to(_dev()) for a in _loss_inputs(big)))
    second = ops.loss_fwd_bwd(*(torch.from_numpy(a).to(_dev()) for a in _loss_inputs(small)))
    ws = ops._loss_ws.get(_dev(), lambda: 0)
    assert ws.numel() >= 1024 * 3 * 4
    ws.fill_(0xFF)
    third = ops.loss_fwd_bwd(*(torch.from_numpy(a).to(_dev()) for a in _loss_inputs(small)))
    assert bool(torch.isfinite(first).all())
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert torch.equal(first.view(torch.int32), third.view(torch.int32))
    want = _loss_ref(small, 0.2)[0]
    assert (np.abs(first.cpu().numpy() - want) <= 4e-6 * want).all()


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
# tails only; the old test's size; odd and more than one trip per thread on the thin kernel's <= 256 workgroups (2 values per thread and
# trip); a second trip on the plain kernel's <= 4096 workgroups (4 values per thread and trip)
ADAM_SIZES = [1, 2, 3, 5, 100003, 131072 + 2 * 256 + 1, 4194304 + 4 * 256 + 3]
ADAM_HYPER = {"default": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0),
              "custom": dict(lr=3e-4, beta1=0.8, beta2=0.95, eps=1e-6, grad_scale=0.125)}


def _adam_scalars(step, lr, beta1, beta2, eps, grad_scale):
    """pg_adam_scalars: formed in double, each rounded to fp32 once"""
    return (F32(1.0 - beta1), F32(beta2), F32(1.0 - beta2), F32(lr / (1.0 - math.pow(beta1, step))),
            F32(math.sqrt(1.0 - math.pow(beta2, step))), F32(eps), F32(grad_scale))


def _adam_emulated(p, g, m, v, step, **hyper):
    """pg_adam_one on float32 numpy arrays: every operation rounds once, in the kernel's order"""
    omb1, b2, omb2, step_size, bc2_sqrt, eps, gs = _adam_scalars(step, **hyper)
    g = g * gs
    m = m + omb1 * (g - m)
    v = v * b2 + omb2 * (g * g)
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


@functools.lru_cache(maxsize=2)
def _adam_inputs(n):
    p = detgen.uniform(311, (n,), -0.1, 0.1)
    g = detgen.uniform(312, (n,), -1e-2, 1e-2)
    g[::7] = 0.0
    m = detgen.uniform(313, (n,), -1e-2, 1e-2)
    v = detgen.uniform(314, (n,), 0.0, 2e-4)
    return p, g, m, v


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _run_adam(p, g, m, v, step, thin, hyper):
    from phasegen import ops
    pd, gd, md, vd = (torch.from_numpy(a).to(_dev()) for a in (p, g, m, v))
    ops.adam_step(pd, gd, md, vd, step, thin=thin, **hyper)
    return pd, md, vd


@pytest.mark.parametrize("state", ["zero-step1", "random-step1000"])
@pytest.mark.parametrize("hyper", list(ADAM_HYPER))
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_bit_exact(n, hyper, state):
    """pg_adam_one is IEEE basic operations only (*, +, -, /, sqrt; no contraction), so a float32 emulation in the same order must
    give the same BITS of p, m and v -- from both kernels, which thereby equal each other at every size (the thin kernel's pairs
    and odd tail, the plain kernel's quads and n & 3 tail).  The gradients hold exact zeros; no value here is small enough for a
    denormal intermediate (|g| >= 1e-2 * 2^-24 where it is not 0), which test_adam_tiny_gradients covers."""
    h = ADAM_HYPER[hyper]
    p, g, m, v = _adam_inputs(n)
    step = 1 if state == "zero-step1" else 1000
    if step == 1:
        m, v = np.zeros_like(m), np.zeros_like(v)
    pw, mw, vw = _adam_emulated(p, g, m, v, step, **h)
    for thin in (False, True):
        pd, md, vd = _run_adam(p, g, m, v, step, thin, h)
        for name, got, want in (("p", pd, pw), ("m", md, mw), ("v", vd, vw)):
            bad = np.flatnonzero(_bits(got) != want.view(np.int32))
            assert bad.size == 0, f"thin={thin} {name}: {bad.size} of {n} differ, first at {bad[0]}"
    if step == 1:          # zero gradient on zero state: nothing moves
        z = g == 0.0
        assert z.any() or n < 7
        assert np.array_equal(pw[z].view(np.int32), p[z].view(np.int32)) and not mw[z].any() and not vw[z].any()


@pytest.mark.parametrize("thin", [False, True])
def test_adam_zero_gradient_block_on_zero_state_changes_nothing(thin):
    """g = 0, m = v = 0: m = 0 + omb1 (0 - 0) = 0, v = 0 b2 + omb2 0 = 0, denom = 0 / bc2 + eps = eps, p = p - step_size (0 / eps) = p."""
    n = 2 * 1024 + 3
    p = detgen.uniform(315, (n,), -0.1, 0.1)
    z = np.zeros(n, F32)
    pd, md, vd = _run_adam(p, z, z, z, 1, thin, ADAM_HYPER["default"])
    assert np.array_equal(_bits(pd), p.view(np.int32))
    assert not _bits(md).any() and not _bits(vd).any()          # +0.0 bit patterns


@pytest.mark.parametrize("thin", [False, True])
def test_adam_tiny_gradients(thin):
    """g = +-1e-20 on zero state, step 1: g^2 = 1e-40 and v = 1e-43 are fp32 denormals.  The device keeps them (include/phasegen.h,
    "Magnitude range": the update is IEEE basic operations, denormals included), so p, m and v have the bits of the float32
    emulation; and whether or not it did,
    denom = sqrt(v) / bc2_sqrt + eps = 1e-8 (1 + 1e-12) and the update step_size * m / denom = 1e-16 is far below half an ulp of
    p ~ 0.1 or 1e-6 step_size: p, m and v must be finite and within 1e-6 * step_size of the float64 formula."""
    n = 4 * 256 + 3
    h = ADAM_HYPER["default"]
    p = detgen.uniform(316, (n,), -0.1, 0.1)
    g = np.where(np.arange(n) % 2 == 0, F32(1e-20), F32(-1e-20)).astype(F32)
    z = np.zeros(n, F32)
    pd, md, vd = _run_adam(p, g, z, z, 1, thin, h)
    omb1, b2, omb2, step_size, bc2_sqrt, eps, gs = (float(s) for s in _adam_scalars(1, **h))
    g64 = g.astype(np.float64) * gs
    m64, v64 = omb1 * g64, omb2 * g64 * g64
    p64 = p.astype(np.float64) - step_size * (m64 / (np.sqrt(v64) / bc2_sqrt + eps))
    pe, me, ve = _adam_emulated(p, g, z, z, 1, **h)
    same = all(np.array_equal(_bits(a), b.view(np.int32)) for a, b in ((pd, pe), (md, me), (vd, ve)))
    print(f"adam tiny gradients thin={thin}: device bits {'equal' if same else 'differ from'} the numpy float32 emulation (which keeps denormals); "
          f"device v[0] = {float(vd[0]):.3e}, numpy {float(ve[0]):.3e}")
    for got, want in ((pd, p64), (md, m64), (vd, v64)):
        got = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        assert np.abs(got - want).max() <= 1e-6 * step_size
    assert same, "pg_adam_step keeps fp32 denormals (include/phasegen.h, Magnitude range): g^2 and v must have the emulation's bits"


def test_adam_thin_matches_torch_optim():
    """The cross-check of tests/test_ops_gpu.py::test_adam_matches_torch_optim at its tolerance, on the thin kernel."""
    from phasegen import ops
    n = 100003
    p0 = torch.from_numpy(detgen.uniform(13, (n,), -0.1, 0.1))
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3)
    p, m, v = p0.to(_dev()), torch.zeros(n, device=_dev()), torch.zeros(n, device=_dev())
    for step in range(1, 4):
        g = torch.from_numpy(detgen.uniform(20 + step, (n,), -1e-2, 1e-2))
        g[::7] = 0.0
        pr.grad = g.clone()
        opt.step()
        ops.adam_step(p, g.to(_dev()), m, v, step, thin=True)
    st = opt.state[pr]
    for got, want in ((p, pr), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
        got, want = got.cpu().double(), want.detach().double()
        assert float((got - want).abs().max() / want.abs().max()) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# fp32 -> bf16 row cast
# ---------------------------------------------------------------------------------------------------------------------
def _cast_values(n):
    """N(0, 1) with the special values in front: signed zeros and infinities, fp32 denormals, FLT_MAX (rounds to inf), exact ties of
    the bf16 rounding (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6: to even) with their negatives, and one fp32 ulp to either side of each"""
    x = detgen.normal(321, (n,)).astype(F32)
    fmax = np.finfo(F32).max
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)], F32)
    special = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, fmax, -fmax], F32), ties,
                              np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf))]).astype(F32)
    assert n >= special.size
    x[:special.size] = special
    return x


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "leaky", "relu"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (3, 7, 61, 64), (2, 5, 64, 72)], ids=lambda s: "B%d-C%d-L%d-pitch%d" % s)
def test_cast_rows_bf16_bits(shape, act):
    """Reference: torch.where(x >= 0, x, slope * x) in fp32 on the CPU, then .to(torch.bfloat16) (round to nearest even), compared as
    bit patterns (+-0 alike after relu).  The source is a channel slice of a wider NaN buffer, the destination sits between guard
    elements in a buffer of 0x7fff patterns: the tails [L, pitch) of every row must come out as zero bits, the guards stay.
    Under relu the reference turns -inf into the NaN of 0 * -inf; a kernel that applied fmaxf(x, slope * x) stored -inf there."""
    from phasegen import ops
    B, C, L, pitch = shape
    slope = {0: 1.0, 1: 0.2, 2: 0.0}[act]
    x = torch.from_numpy(_cast_values(B * C * L).reshape(B, C, L))
    wide = torch.full((B, 2 + C + 3, L), float("nan"), device=_dev())
    xv = wide[:, 2:2 + C]
    xv.copy_(x)
    n = B * C * pitch
    buf, mid = _embedded(n, 0x7fff, torch.int16)
    out = mid.view(torch.bfloat16).view(B, C, pitch)
    ops.cast_rows_bf16(xv, out, act=act)
    want = torch.where(x >= 0, x, torch.tensor(slope, dtype=torch.float32) * x).to(torch.bfloat16).view(torch.int16).numpy()
    got = mid.view(B, C, pitch).cpu().numpy()
    assert _guards_intact(buf, n, 0x7fff)
    assert not got[:, :, L:].any(), "row tails must be zero"
    g, w = got[:, :, :L].copy(), want.copy()
    for a in (g, w):          # a NaN is a NaN: torch's own conversion writes 0x7fc0 or 0xffff depending on the code path it takes
        a[(a & 0x7fff) > 0x7f80] = 0x7fc0
    if act == 2:
        g[g == np.int16(-0x8000)] = 0
        w[w == np.int16(-0x8000)] = 0
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{len(bad)} differ, first {tuple(bad[0])}: x = {float(x[tuple(bad[0])])!r}, got {int(g[tuple(bad[0])]) & 0xffff:#06x}, want {int(w[tuple(bad[0])]) & 0xffff:#06x}"
