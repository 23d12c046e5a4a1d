"""GPU: train-mode BatchNorm (csrc/norm.hip, pg_bn_fwd / pg_bn_bwd) where the statistics are hard or exact.

tests/test_ops_gpu.py covers every unit width and view layout with x = 2 rnd + 0.3, data on which a one-pass variance
(E[x^2] - E[x]^2) is as good as the two-pass arithmetic the kernels use.  Here channels with mean 1000 and sigma 1, and mean -1000
and sigma 0.1, share a launch with ordinary ones: the one-pass form is off by 6 % on the first and negative on the second.  The
reference is numpy float64 of the fp32 x; the bounds are worst cases of the kernels' fixed summation order, derived in the
docstrings.  The second half pins channels whose statistics are exactly representable -- constant channels, one value per channel --
bit for bit against a float32 emulation.  DESIGN.md section 4.2 lists the largest errors observed next to the bounds; each test
prints them before it asserts.

Named test_z_* so that it is collected behind the older modules."""
import numpy as np
import pytest
import torch

from phasegen import detgen

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24                     # unit roundoff of fp32
EPS, MOM = F32(1e-5), F32(0.1)     # as the fp32 fields of pg_bn_args hold them


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _np(t):
    return t.cpu().numpy()


# (B, C, L, P): P = values a thread sums before the block tree = ceil(B L / 256) rounded up to the unit width.
# 16-byte units, 64 floats per thread; scalar units; 18 000 > 16 384 values: the three-pass kernel (scalar, 71 per thread)
HARD_CASES = [(64, 8, 256, 64), (5, 6, 61, 2), (3, 4, 6000, 71)]
MEAN_SIGMA = [(0.3, 2.0), (30.0, 1.0), (1000.0, 1.0), (-1000.0, 0.1)]


@pytest.mark.parametrize("case", HARD_CASES, ids=lambda c: "B%d-C%d-L%d" % c[:3])
def test_bn_ill_conditioned_channels(case):
    """Channel c holds M + sigma rnd with (M, sigma) cycling through (0.3, 2), (30, 1), (1000, 1), (-1000, 0.1).

    Forward.  A thread adds P values in sequence (P - 1 roundings, each <= u = 2^-24 of the running sum <= sum|x|), the wave butterfly
    adds 6 levels, the four wave sums 3 more, the division by n one: |save_mean - mean64| <= E = (P + 10) u mean|x_c|.
    The variance is the mean of (x - mean)^2 around the DEVICE's mean: a shift d of the mean adds d^2, i.e. (E / sigma)^2 relative,
    half of that in invstd; the centred squares are summed in the same order, plus the subtraction, the square, eps, sqrt and the
    division: save_invstd within 0.5 (E / sigma)^2 + (P + 12) u relative.
    y = (x - mean) invstd gamma + beta: the shift of the mean moves y by |gamma| E / sigma, the relative error of invstd (below
    E / sigma) scales |gamma xhat|, and four roundings of |gamma xhat| and |beta| remain:
    |y - y64| <= |gamma| E / sigma (1 + |xhat|) + 4e-6 (|gamma| |xhat| + |beta|).
    The running buffers take the same terms times the momentum, plus the six roundings of the step itself
    ((1 - m), two products, the sum; n / (n - 1) and its product for the variance).

    Backward (dy = rnd + 0.5 xhat, so mean(dy xhat) ~ 0.5), float64 from the DEVICE's save_mean / save_invstd, which the kernel reads:
    dgamma = sum(dy xhat) and dbeta = sum(dy) in the same summation order: within (P + 10) u sum|terms|; dx within 2e-5 of the
    channel's max-abs (the two means carry (P + 10) u = 4.4e-6 of mean|terms| at P = 64, xhat <= 4.5 multiplies one of them)."""
    from phasegen import ops
    B, C, L, P = case
    n = B * L
    M = np.array([MEAN_SIGMA[c % 4][0] for c in range(C)], F32)
    S = np.array([MEAN_SIGMA[c % 4][1] for c in range(C)], F32)
    x = (M[None, :, None] + S[None, :, None] * detgen.normal(331, (B, C, L))).astype(F32)
    gamma = detgen.uniform(332, (C,), 0.5, 1.5) * np.where(np.arange(C) % 3 == 2, F32(-1), F32(1)).astype(F32)
    beta = detgen.uniform(333, (C,), -0.5, 0.5)
    rm0, rv0 = detgen.uniform(334, (C,), -0.5, 0.5), detgen.uniform(335, (C,), 0.5, 1.5)

    x64 = x.astype(np.float64)
    mean64 = x64.mean(axis=(0, 2))
    var64 = ((x64 - mean64[None, :, None]) ** 2).mean(axis=(0, 2))
    sig64, inv64 = np.sqrt(var64), 1.0 / np.sqrt(var64 + float(EPS))
    xhat = (x64 - mean64[None, :, None]) * inv64[None, :, None]
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    y64 = xhat * g64[None, :, None] + b64[None, :, None]
    E = (P + 10) * U * np.abs(x64).mean(axis=(0, 2))
    r_inv = 0.5 * (E / sig64) ** 2 + (P + 12) * U
    mom = float(MOM)
    unb64 = var64 * n / (n - 1)
    rm0_64, rv0_64 = rm0.astype(np.float64), rv0.astype(np.float64)
    rm64, rv64 = (1 - mom) * rm0_64 + mom * mean64, (1 - mom) * rv0_64 + mom * unb64

    xd = _cuda(x)
    y = torch.full_like(xd, float("nan"))
    sm, si = torch.empty(C, device=_dev()), torch.empty(C, device=_dev())
    rm, rv, cnt = _cuda(rm0), _cuda(rv0), torch.tensor(5, dtype=torch.int64, device=_dev())
    gd, bd = _cuda(gamma), _cuda(beta)
    ops.bn_fwd(xd, y, gd, bd, sm, si, rm, rv, eps=float(EPS), momentum=mom, num_batches_tracked=cnt)
    smh, sih = _np(sm).astype(np.float64), _np(si).astype(np.float64)
    e_mean = np.abs(smh - mean64) / E
    e_inv = np.abs(sih / inv64 - 1) / r_inv
    y_bound = np.abs(g64)[None, :, None] * (E / sig64)[None, :, None] * (1 + np.abs(xhat)) + 4e-6 * (np.abs(g64)[None, :, None] * np.abs(xhat) + np.abs(b64)[None, :, None])
    e_y = (np.abs(_np(y).astype(np.float64) - y64) / y_bound).max(axis=(0, 2))
    rm_bound = mom * E + 6 * U * (np.abs((1 - mom) * rm0_64) + np.abs(mom * mean64))
    rv_bound = mom * unb64 * 2 * r_inv + 6 * U * (np.abs((1 - mom) * rv0_64) + mom * unb64)
    e_rm, e_rv = np.abs(_np(rm) - rm64) / rm_bound, np.abs(_np(rv) - rv64) / rv_bound
    print(f"bn hard {case[:3]}: as fractions of the bounds, per channel\n  mean {e_mean}\n  invstd {e_inv}\n  y {e_y}\n  running_mean {e_rm}\n  running_var {e_rv}")
    print(f"  |save_mean - mean64| / ulp(M): {np.abs(smh - mean64) / np.spacing(np.abs(M))}   relative error of the device variance: {np.abs(1 / sih ** 2 - float(EPS) - var64) / var64}")
    assert int(cnt) == 6
    assert (e_mean <= 1).all() and (e_inv <= 1).all()
    assert (e_y <= 1).all()
    assert (e_rm <= 1).all() and (e_rv <= 1).all()

    dy = (detgen.normal(336, (B, C, L)) + F32(0.5) * xhat.astype(F32)).astype(F32)
    dx = torch.full_like(xd, float("nan"))
    dg, db = torch.empty(C, device=_dev()), torch.empty(C, device=_dev())
    ops.bn_bwd(xd, _cuda(dy), dx, gd, sm, si, dg, db)
    dy64 = dy.astype(np.float64)
    xh_dev = (x64 - smh[None, :, None]) * sih[None, :, None]
    t = dy64 * xh_dev
    dg64, db64 = t.sum(axis=(0, 2)), dy64.sum(axis=(0, 2))
    dx64 = (g64 * sih)[None, :, None] * (dy64 - (db64 / n)[None, :, None] - xh_dev * (dg64 / n)[None, :, None])
    e_dg = np.abs(_np(dg) - dg64) / ((P + 10) * U * np.abs(t).sum(axis=(0, 2)))
    e_db = np.abs(_np(db) - db64) / ((P + 10) * U * np.abs(dy64).sum(axis=(0, 2)))
    e_dx = np.abs(_np(dx).astype(np.float64) - dx64).max(axis=(0, 2)) / np.abs(dx64).max(axis=(0, 2))
    print(f"  dgamma {e_dg}\n  dbeta {e_db}  (fractions of the bounds)\n  dx / max|dx| {e_dx} (2e-5)")
    assert (e_dg <= 1).all() and (e_db <= 1).all()
    assert (e_dx <= 2e-5).all()


def _running_step(r0, value):
    """norm_running_step in float32: (1 - momentum) * r + momentum * value, one rounding per operation"""
    return (F32(1) - MOM) * r0 + MOM * value


def test_bn_exact_channels():
    """(4, 6, 64): n = 256 values per channel, so the sums of the constant channels x = 0, x = 1, x = -2 are exact in any order (and
    so is the division by n).  They share the call with three random channels.  Expected for a constant c: save_mean == c, every
    centred value 0, var 0, save_invstd == fl(1 / fl(sqrt(fl(0 + eps)))), y = 0 * invstd * gamma + beta == beta and each stored copy
    == its activation of beta (fp32 y plain, y2 leaky, bf16 yh relu, yh2 plain; the betas are bf16 values), running_mean ==
    fl(fl((1 - m) rm) + fl(m c)), running_var == fl((1 - m) rv) (the unbiased variance is 0).  Backward: xhat == 0, so dgamma == 0
    and dx == fl(k * fl(dy - m1)) with k = fl(gamma * invstd), m1 = fl(dbeta / n) from the device's own dbeta."""
    from phasegen import ops
    B, C, L = 4, 6, 64
    n = B * L
    consts = [0.0, 1.0, -2.0]
    x = (F32(1.5) * detgen.normal(341, (B, C, L)) + F32(0.4)).astype(F32)
    for c, val in enumerate(consts):
        x[:, c] = val
    gamma = np.array([1.25, -0.75, 0.5, 1.0, 0.8, 1.3], F32)
    beta = np.array([0.25, -0.5, -1.5, 0.1, -0.2, 0.3], F32)
    rm0, rv0 = detgen.uniform(342, (C,), -0.5, 0.5), detgen.uniform(343, (C,), 0.5, 1.5)
    xd, gd, bd = _cuda(x), _cuda(gamma), _cuda(beta)
    y, y2 = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    yh, yh2 = ops.h_alloc(B, C, L, _dev()), ops.h_alloc(B, C, L, _dev())
    sm, si = torch.empty(C, device=_dev()), torch.empty(C, device=_dev())
    rm, rv, cnt = _cuda(rm0), _cuda(rv0), torch.tensor(0, dtype=torch.int64, device=_dev())
    ops.bn_fwd(xd, y, gd, bd, sm, si, rm, rv, eps=float(EPS), momentum=float(MOM), y_act=ops.ACT_NONE, y2=y2, y2_act=ops.ACT_LEAKY,
               yh=yh, yh_act=ops.ACT_RELU, yh2=yh2, yh2_act=ops.ACT_NONE, num_batches_tracked=cnt)
    inv0 = F32(1) / np.sqrt(F32(0) + EPS)
    assert inv0.dtype == np.float32 and int(cnt) == 1
    k = len(consts)
    cs = np.array(consts, F32)
    assert np.array_equal(_np(sm)[:k], cs)
    assert np.array_equal(_np(si)[:k].view(np.int32), np.full(k, inv0).view(np.int32))
    bk = beta[:k, None]
    leaky = np.maximum(bk, F32(0.2) * bk)
    for b in range(B):
        assert np.array_equal(_np(y)[b, :k], np.broadcast_to(bk, (k, L)))
        assert np.array_equal(_np(y2)[b, :k], np.broadcast_to(leaky, (k, L)))
        assert np.array_equal(_np(yh.float())[b, :k, :L], np.broadcast_to(np.maximum(bk, F32(0)), (k, L)))
        assert np.array_equal(_np(yh2.float())[b, :k, :L], np.broadcast_to(bk, (k, L)))
    assert not _np(yh.float())[:, :, L:].any() and not _np(yh2.float())[:, :, L:].any()          # the zero tails stay zero
    assert np.array_equal(_np(rm)[:k], _running_step(rm0[:k], cs))
    assert np.array_equal(_np(rv)[:k], (F32(1) - MOM) * rv0[:k])
    # the random channels next to them: float64, at the everyday bound
    x64 = x[:, k:].astype(np.float64)
    mu, var = x64.mean(axis=(0, 2), keepdims=True), x64.var(axis=(0, 2), keepdims=True)
    y64 = (x64 - mu) / np.sqrt(var + float(EPS)) * gamma[None, k:, None] + beta[None, k:, None]
    assert np.abs(_np(y)[:, k:] - y64).max() <= 1e-5 * np.abs(y64).max()

    dy = detgen.normal(344, (B, C, L))
    dx = torch.full_like(xd, float("nan"))
    dg, db = torch.empty(C, device=_dev()), torch.empty(C, device=_dev())
    ops.bn_bwd(xd, _cuda(dy), dx, gd, sm, si, dg, db)
    assert not _np(dg)[:k].any()
    dbh = _np(db)
    assert np.abs(dbh - dy.astype(np.float64).sum(axis=(0, 2))).max() <= 20 * U * np.abs(dy).sum(axis=(0, 2)).max()
    kk, m1 = gamma[:k] * inv0, dbh[:k] / F32(n)
    want = kk[None, :, None] * (dy[:, :k] - m1[None, :, None])
    assert want.dtype == np.float32
    assert np.array_equal(_np(dx)[:, :k], want)


def test_bn_one_value_per_channel():
    """(1, 3, 1): n = 1.  mean == x, var == 0, y == beta; the header's max(n - 1, 1) rule makes the unbiased variance 0 * (1 / 1), so
    running_var == fl((1 - m) rv); the counter advances by one."""
    from phasegen import ops
    x = np.array([[[0.7], [-3.0], [1000.0]]], F32)
    gamma, beta = np.array([1.5, -0.5, 2.0], F32), np.array([0.25, -0.125, 3.0], F32)
    rm0, rv0 = np.array([0.1, -0.2, 0.3], F32), np.array([1.0, 0.7, 1.3], F32)
    xd = _cuda(x)
    y = torch.full_like(xd, float("nan"))
    sm, si = torch.empty(3, device=_dev()), torch.empty(3, device=_dev())
    rm, rv, cnt = _cuda(rm0), _cuda(rv0), torch.tensor(41, dtype=torch.int64, device=_dev())
    ops.bn_fwd(xd, y, _cuda(gamma), _cuda(beta), sm, si, rm, rv, eps=float(EPS), momentum=float(MOM), num_batches_tracked=cnt)
    assert np.array_equal(_np(y).ravel(), beta)
    assert np.array_equal(_np(sm), x.ravel())
    assert np.array_equal(_np(si), np.full(3, F32(1) / np.sqrt(F32(0) + EPS)))
    assert np.array_equal(_np(rm), _running_step(rm0, x.ravel()))
    assert np.array_equal(_np(rv), (F32(1) - MOM) * rv0)
    assert int(cnt) == 42
