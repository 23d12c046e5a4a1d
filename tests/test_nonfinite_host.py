"""CPU: is the comparison of tests/_nonfinite.py honest?

(1) the cones it states by index arithmetic are those of the float64 restatements evaluated with IEEE arithmetic on a poisoned input:
    convolutions against a loop over the terms that exist (padding is no term), STFT and ISTFT against tests/_signal_ref64.py;
(2) float32 stand-ins built differently from the float64 references -- a tap loop for the convolutions, running sums for BatchNorm,
    float32 numpy for loss, Adam and polar, the fp32 torch.fft transforms of tests/_signal_ref64.py -- pass `check` on the cases of
    tests/test_z_nonfinite_gpu.py (the convolutions on the tiny geometries of tests/test_conv_bounds_host.py, where a tap loop is
    affordable; the GPU module's own rows are held to (4));
(3) planted faults -- in a stand-in, never in library code -- are rejected: ReLU as fmax(x, 0), nan_to_num on the input, a peak by
    fmax.reduce used as a divisor, padding zeros multiplied in, the angle by the fmaxf / fminf formulation;
(4) a condition, not a measurement: in every case of the GPU module the cone of the poisoned element holds at least one output
    element and at most half of them, so that R1 and R2 both have content.  Whole-cone cases, by definition of the operation and
    listed here by name: the three losses, moments / standardize, the statistics and running buffers of a BatchNorm channel;
    and WIDE_WINDOWS, the conv rows whose window is wider than half of a one-sample output."""
import numpy as np
import pytest

import _conv_ref64 as cref
import _nonfinite as nf
import _signal_ref64 as sig
import test_z_nonfinite_gpu as gpu
from test_conv_bounds_host import TINY

F32 = np.float32
ERR = dict(invalid="ignore", over="ignore", divide="ignore")


def rejected(*args, **kw):
    try:
        nf.check(*args, **kw)
    except AssertionError as e:
        return str(e)
    return None


# ---- the checker itself -------------------------------------------------------------------------------------------------------------
def test_check_counts_and_rules():
    rc = np.arange(6, dtype=np.float64)
    rp = rc.copy()
    rp[1], rp[2] = np.nan, 7.0                          # one in the cone, one changed
    gc = rc.astype(F32)
    good = gc.copy()
    good[1], good[2] = np.inf, 123.0                    # inf for NaN is fine; a changed element is held to neither rule
    assert nf.check(good, gc, rp, rc) == {"cone": 1, "outside": 4, "changed": 1, "swallowed": 0, "spread": 0, "allowed": 0}
    swallow = good.copy()
    swallow[1] = 1.0
    assert "R1" in rejected(swallow, gc, rp, rc)
    spread = good.copy()
    spread[4] = np.nan
    assert "R2" in rejected(spread, gc, rp, rc)
    ulp = good.copy()
    ulp[5] = np.nextafter(ulp[5], F32(9))
    assert "R2" in rejected(ulp, gc, rp, rc)            # bits, not a tolerance
    zero = good.copy()
    zero[0] = -0.0
    assert "R2" in rejected(zero, gc, rp, rc)
    allow = np.zeros(6, bool)
    allow[4] = True
    assert nf.check(spread, gc, rp, rc, allow=allow)["allowed"] == 1
    assert "R1" in rejected(swallow, gc, rp, rc, allow=np.ones(6, bool))         # no exception from R1
    with pytest.raises(AssertionError):
        nf.check(good, good, rp, rc)                    # a clean call that is not finite proves nothing
    assert nf.cone_is_a_proper_part(rp, rc) and not nf.cone_is_a_proper_part(rc, rc) and not nf.cone_is_a_proper_part(np.full(6, np.nan), rc)
    assert nf.cone_is_a_proper_part(np.full(6, np.nan), rc, whole=True)


# ---- convolutions -------------------------------------------------------------------------------------------------------------------
def _poisoned_operands(t, operand, index, value):
    T = {k: t[k] for k in ("x", "w", "dy")}
    T[operand] = nf.poison(t[operand], index, value)
    return T


@pytest.mark.parametrize("geom", TINY)
def test_conv_cone_is_the_cone_of_the_tap_loop_and_a_float32_tap_loop_passes(geom):
    t = cref.make_inputs(geom, "white")
    for op in ("fwd", "dgrad", "wgrad"):
        ref_c = nf.conv_direct(op, geom, t["x"], t["w"], t["dy"])
        value, mag = cref.conv64(op, geom, t["x"], t["w"], t["dy"])
        assert np.all(np.abs(ref_c - value) <= 1e-13 * mag)                              # the tap loop is the GEMM of _conv_ref64
        s32 = lambda T: nf.conv_direct(op, geom, T["x"], T["w"], T["dy"]).astype(F32)    # (float64 sums rounded once: another order)
        got_c = s32(t)
        for operand in nf.conv_operands(op):
            if operand in ("add", "ref"):
                continue
            for site, index in nf.conv_sites(geom, operand).items():
                cone = nf.conv_cone(op, geom, operand, index)
                for vname, v in nf.VALUES:
                    T = _poisoned_operands(t, operand, index, v)
                    ref_p = nf.conv_direct(op, geom, T["x"], T["w"], T["dy"])
                    assert np.array_equal(~np.isfinite(ref_p), cone), (geom, op, operand, site, vname)
                    assert np.array_equal(ref_p[~cone], ref_c[~cone])
                    n = nf.check(s32(T), got_c, np.where(cone, np.nan, ref_c), ref_c, tag=f"host {geom} {op} {operand} {site} {vname}")
                    assert n["cone"] == int(cone.sum())


def test_conv_planted_faults_are_rejected():
    geom = (False, 3, 4, 4, 2, 1, 9, 2)
    t = cref.make_inputs(geom, "white")
    ref_c = nf.conv_direct("fwd", geom, t["x"], t["w"], t["dy"])
    clean = ref_c.astype(F32)
    # ReLU as fmax(x, 0) on the second output: a NaN comes out as 0
    idx = nf.conv_sites(geom, "x")["interior"]
    cone = nf.conv_cone("fwd", geom, "x", idx)
    with np.errstate(**ERR):
        y = nf.conv_direct("fwd", geom, nf.poison(t["x"], idx, nf.NAN), t["w"], t["dy"]).astype(F32)
    relu_ref, relu_ref_p = nf.act64(ref_c, 2), np.where(cone, np.nan, nf.act64(ref_c, 2))
    assert rejected(np.fmax(y, F32(0)), np.fmax(clean, F32(0)), relu_ref_p, relu_ref) is not None
    with np.errstate(**ERR):
        select = lambda a: np.where(a >= 0, a, F32(0) * a)
        assert nf.check(select(y), select(clean), relu_ref_p, relu_ref)["cone"] == int(cone.sum())
    # nan_to_num on the input
    for v in (nf.NAN, nf.PINF):
        y = nf.conv_direct("fwd", geom, np.nan_to_num(nf.poison(t["x"], idx, v)), t["w"], t["dy"]).astype(F32)
        assert "R1" in rejected(y, clean, np.where(cone, np.nan, ref_c), ref_c)
    # zero taps multiplied in, not skipped: the GEMM over the zero-padded input (_conv_ref64.standin) with a poisoned tap 0
    idx = nf.conv_sites(geom, "w")["edge"]
    cone = nf.conv_cone("fwd", geom, "w", idx)
    assert not cone[:, :, 0].any() and cone[:, idx[0], 1:].all()                 # tap 0 of the first window lies on the padding
    for vname, v in nf.VALUES:
        with np.errstate(**ERR):
            y = cref.standin("fwd", geom, t["x"], nf.poison(t["w"], idx, v), t["dy"])
        ref_p = np.where(cone, np.nan, ref_c)
        assert "R2" in rejected(y, cref.standin("fwd", geom, t["x"], t["w"], t["dy"]), ref_p, ref_c)
        # ... which is what the header's exception names: with the row's mates allowed it passes
        assert nf.check(y, cref.standin("fwd", geom, t["x"], t["w"], t["dy"]), ref_p, ref_c, allow=nf.conv_row_mates("fwd", geom, "w", idx))["allowed"] > 0


# rows of the GPU module whose poisoned x (or dy) reaches more than half of the outputs: one sample, and a window of k = 32 taps over
# 13 output frames -- no element of x lies in fewer than 9 of them, the interior one in all (R2 rests on the other two sites there)
WIDE_WINDOWS = {((False, 8, 16, 32, 2, 16, 24, 1), "fwd", "x")}


def _gpu_conv_rows():
    import test_z_conv_values_gpu as cv
    return list(dict.fromkeys([(c[0], c[1]) for c in cv.CASES] + [(r[0], "fwd") for r in cv.H_ROWS]))


def test_every_conv_case_of_the_gpu_module_has_a_proper_cone():
    seen = set()
    for geom, op in _gpu_conv_rows():
        for operand in nf.conv_operands(op):
            for site, index in nf.conv_sites(geom, operand).items():
                cone = nf.conv_cone(op, geom, operand, index)
                n = int(cone.sum())
                if operand == "ref":
                    assert n == 0
                    continue
                assert n >= 1, (geom, op, operand, site)
                if 2 * n > cone.size:
                    seen.add((geom, op, operand))
                assert n < cone.size or (site == "interior" and (geom, op, operand) in WIDE_WINDOWS), (geom, op, operand, site)
                mates = nf.conv_row_mates(op, geom, operand, index)
                assert not mates.any() or (mates | cone).sum() == mates.sum()            # the exception lies around the cone
    assert seen == WIDE_WINDOWS, seen ^ WIDE_WINDOWS


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------
def bn_fwd32(x, gamma, beta, rm0, rv0, per_clip):
    """float32 with running sums along the frames (np.cumsum), one rounding per operation: built differently from nf.bn_fwd64"""
    x = np.asarray(x, F32)
    B, C, L = x.shape
    with np.errstate(**ERR):
        if per_clip:
            mean = np.cumsum(x, axis=2, dtype=F32)[:, :, -1] / F32(L)
            d = x - mean[:, :, None]
            var = np.cumsum(d * d, axis=2, dtype=F32)[:, :, -1] / F32(L)
            xh = d / np.sqrt(var + F32(gpu.EPS))[:, :, None]
            rm, rv = rm0.copy(), rv0.copy()
            for i in range(B):
                rm = F32(1 - gpu.MOM) * rm + F32(gpu.MOM) * mean[i]
                rv = F32(1 - gpu.MOM) * rv + F32(gpu.MOM) * (var[i] * F32(L / max(L - 1, 1)))
            inv = F32(1) / np.sqrt(var + F32(gpu.EPS))
        else:
            n = B * L
            flat = x.transpose(1, 0, 2).reshape(C, n)
            mean = np.cumsum(flat, axis=1, dtype=F32)[:, -1] / F32(n)
            d = x - mean[None, :, None]
            var = np.cumsum((d * d).transpose(1, 0, 2).reshape(C, n), axis=1, dtype=F32)[:, -1] / F32(n)
            inv = F32(1) / np.sqrt(var + F32(gpu.EPS))
            xh = d * inv[None, :, None]
            rm = F32(1 - gpu.MOM) * rm0 + F32(gpu.MOM) * mean
            rv = F32(1 - gpu.MOM) * rv0 + F32(gpu.MOM) * (var * F32(n / max(n - 1, 1)))
        y = xh * gamma[None, :, None] + beta[None, :, None]
    return {"y": y.astype(F32), "save_mean": mean, "save_invstd": inv, "running_mean": rm, "running_var": rv}


@pytest.mark.parametrize("per_clip", [False, True])
@pytest.mark.parametrize("shape", gpu.NORM_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_norm_standins_pass_and_cones_are_a_channel(shape, per_clip):
    x, dy, gamma, beta, rm0, rv0 = gpu.norm_inputs(shape)
    B, C, L = shape
    ref_c, got_c = nf.bn_fwd64(x, gamma, beta, rm0, rv0, gpu.EPS, gpu.MOM, per_clip), bn_fwd32(x, gamma, beta, rm0, rv0, per_clip)
    for site, index in gpu.norm_sites(shape).items():
        for vname, v in nf.VALUES:
            xp = nf.poison(x, index, v)
            ref_p, got_p = nf.bn_fwd64(xp, gamma, beta, rm0, rv0, gpu.EPS, gpu.MOM, per_clip), bn_fwd32(xp, gamma, beta, rm0, rv0, per_clip)
            for n in ref_c:
                nf.check(got_p[n], got_c[n], ref_p[n], ref_c[n], tag=f"host norm {shape} per_clip={per_clip} {site} {vname} {n}")
                # y: one channel (row) of C (B C); the statistics of that channel: whole by definition, the others untouched
                assert nf.cone_is_a_proper_part(ref_p[n], ref_c[n], whole=n != "y")
                assert int((~np.isfinite(ref_p[n])).sum()) == {"y": L if per_clip else B * L}.get(n, 1)
    if not per_clip:
        sm, si = ref_c["save_mean"], ref_c["save_invstd"]
        bc = nf.bn_bwd64(x, dy, gamma, sm, si)
        for operand in ("x", "dy"):
            for site, index in gpu.norm_sites(shape).items():
                for vname, v in nf.VALUES:
                    bp = nf.bn_bwd64(nf.poison(x, index, v) if operand == "x" else x, nf.poison(dy, index, v) if operand == "dy" else dy, gamma, sm, si)
                    assert int((~np.isfinite(bp["dx"])).sum()) == B * L and int((~np.isfinite(bp["dgamma"])).sum()) == 1
                    assert int((~np.isfinite(bp["dbeta"])).sum()) == (1 if operand == "dy" else 0)
                    assert np.array_equal(bp["dbeta"], bc["dbeta"]) or operand == "dy"


def test_a_variance_clamped_by_fmax_is_rejected():
    """planted: var = fmax(var, 0) drops the NaN of an infinite sample, save_invstd comes out as 1 / sqrt(eps)"""
    shape = gpu.NORM_SHAPES[0]
    x, dy, gamma, beta, rm0, rv0 = gpu.norm_inputs(shape)
    xp = nf.poison(x, (0, 0, 0), nf.PINF)
    ref_c, ref_p = (nf.bn_fwd64(a, gamma, beta, rm0, rv0, gpu.EPS, gpu.MOM)["save_invstd"] for a in (x, xp))
    with np.errstate(**ERR):
        x64 = xp.astype(np.float64)
        var = ((x64 - x64.mean(axis=(0, 2), keepdims=True)) ** 2).mean(axis=(0, 2))
        assert np.isnan(var[0])
        bad = (1.0 / np.sqrt(np.fmax(var, 0.0) + gpu.EPS)).astype(F32)
    assert "R1" in rejected(bad, ref_c.astype(F32), ref_p, ref_c)


# ---- loss, Adam, polar ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gpu.LOSS_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_loss_standin_passes(shape):
    pred, batch = gpu.loss_inputs(shape)

    def f32(pred, batch):
        B, C2, L = pred.shape
        C = C2 // 2
        p, mh, m, th = pred[:, :C], pred[:, C:], batch[:, 0], batch[:, 1]
        N = F32(B * C * L)
        with np.errstate(**ERR):
            dc, ds, dm = np.cos(p) - np.cos(th), np.sin(p) - np.sin(th), mh - m
            parts = [np.cumsum((d * d).ravel(), dtype=F32)[-1] / N for d in (dc, ds, dm)]
            s = F32(2) / N
            dpred = np.concatenate([s * (ds * np.cos(p) - dc * np.sin(p)), F32(0.2) * s * dm], axis=1)
        return np.array([parts[0] + parts[1] + F32(0.2) * parts[2], parts[0] + parts[1], parts[2]], F32), dpred.astype(F32)

    (rl, rd), (gl, gd) = nf.loss64(pred, batch), f32(pred, batch)
    for site, (which, index) in gpu.loss_sites(shape).items():
        for vname, v in nf.VALUES:
            pp, bp = (nf.poison(pred, index, v), batch) if which == "pred" else (pred, nf.poison(batch, index, v))
            (pl, pdp), (gpl, gpd) = nf.loss64(pp, bp), f32(pp, bp)
            nf.check(gpl, gl, pl, rl, tag=f"host loss {shape} {site} {vname} losses")
            nf.check(gpd, gd, pdp, rd, tag=f"host loss {shape} {site} {vname} dpred")
            assert nf.cone_is_a_proper_part(pl, rl, whole=True) and int((~np.isfinite(pl)).sum()) == 2           # (scalars: by definition)
            assert nf.cone_is_a_proper_part(pdp, rd) and int((~np.isfinite(pdp)).sum()) == 1
            assert np.isfinite(pl[1 if site in ("magnitude", "target logmag") else 2])


def test_adam_standin_passes():
    arrays = dict(zip("pgmv", gpu.adam_inputs()))
    ref_c = nf.adam64(arrays["p"], arrays["g"], arrays["m"], arrays["v"], 7)
    got_c = nf.adam64(arrays["p"], arrays["g"], arrays["m"], arrays["v"], 7, dtype=F32)
    for operand in "gmvp":
        for site, i in gpu.ADAM_SITES.items():
            for vname, v in nf.VALUES:
                T = dict(arrays)
                T[operand] = nf.poison(arrays[operand], i, v)
                ref_p, got_p = nf.adam64(T["p"], T["g"], T["m"], T["v"], 7), nf.adam64(T["p"], T["g"], T["m"], T["v"], 7, dtype=F32)
                cone = 0
                for a, b, c, d in zip(got_p, got_c, ref_p, ref_c):
                    cone += nf.check(a, b, c, d, tag=f"host adam {operand} {site} {vname}")["cone"]
                    assert (~np.isfinite(c)).sum() <= 1 and np.isfinite(np.delete(c, i)).all()
                assert 1 <= cone <= 3


def test_polar_standin_passes_and_the_minmax_angle_is_rejected():
    d = gpu.detgen.normal(951, (2, 2, 5, 7))
    where = [(0, 0, 0), (0, 2, 3), (0, 4, 6), (1, 0, 1), (1, 1, 1), (1, 3, 5), (1, 4, 6)]
    dp = d.copy()
    for (n, b, f), (re, im) in zip(where, nf.POLAR_CELLS):
        dp[n, 0, b, f], dp[n, 1, b, f] = re, im
    ref_c, ref_p = np.stack(nf.polar64(d[:, 0], d[:, 1]), 1), np.stack(nf.polar64(dp[:, 0], dp[:, 1]), 1)
    with np.errstate(**ERR):
        def s32(a, ang):
            z = (a[:, 0] + np.complex64(1j) * a[:, 1]).astype(np.complex64)              # complex64: data.py:40 in the device's precision
            return np.stack([np.log1p(np.hypot(z.real, z.imag)), ang(z.imag, z.real)], 1).astype(F32)

        n = nf.check(s32(dp, np.arctan2), s32(d, np.arctan2), ref_p, ref_c, tag="host polar")
        assert n["cone"] == 12 and nf.cone_is_a_proper_part(ref_p, ref_c)
        # the formulation is the honest one on finite data ...
        assert np.abs(nf.atan2_minmax32(d[:, 1], d[:, 0]) - np.arctan2(d[:, 1], d[:, 0])).max() <= 1e-6
        # ... and swallows a NaN in either argument
        assert np.isfinite(nf.atan2_minmax32(F32("nan"), F32(1))) and np.isfinite(nf.atan2_minmax32(F32(1), F32("nan")))
        assert "R1" in rejected(s32(dp, nf.atan2_minmax32), s32(d, nf.atan2_minmax32), ref_p, ref_c)


# ---- STFT / ISTFT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", gpu.STFT_ROWS + [(r[0], r[1], r[2], 1 + r[3] // r[2], r[4]) for r in gpu.CROP_ROWS], ids=lambda r: r[0])
def test_stft_cone_and_standin(row):
    id, n_fft, hop, frames, single = row
    n = hop * (frames - 1) if not id.startswith("crops") else dict((r[0], r[3]) for r in gpu.CROP_ROWS)[id]
    signals = 3 if id.startswith("crops") else 2
    y = sig.white(961, signals, n)
    ref_c = gpu.stft_refs(y, n_fft, hop, False)
    got_c = sig.standin_stft(y, n_fft, hop)
    sites = nf.stft_sites(n, n_fft, hop)
    assert sites["first"] == 0 and sites["last"] == n - 1 and 0 < sites["two-frames"] < n - 1
    for site, i in sites.items():
        cone = nf.stft_cone(n, n_fft, hop, i)
        assert 1 <= cone.sum() and 2 * cone.sum() <= signals * cone.size, (id, site, int(cone.sum()))
        for vname, v in nf.VALUES:
            yp = nf.poison(y, (1, i), v)
            with np.errstate(**ERR):
                X = sig.stft64(yp, n_fft, hop)
                got_p = sig.standin_stft(yp, n_fft, hop)
            ref_p = gpu.stft_poisoned_ref(ref_c, 1, n, n_fft, hop, i, vname == "nan", False)
            held, unheld, bad = np.isnan(ref_p), ref_p == nf.UNHELD, ~np.isfinite(X)
            # float64 rfft: non-finite wherever the coefficient of the sample is not exactly zero, untouched outside the frames that
            # hold it; where the coefficient is zero (the imaginary part of the Nyquist bin among them) a real transform may do either
            assert bad[held].all() and not bad[~held & ~unheld].any() and np.array_equal(X[~held & ~unheld], ref_c[~held & ~unheld])
            assert np.array_equal((held | unheld)[1].any(axis=(0, 1)), cone) and not (held | unheld)[0].any()
            assert 2 * held.sum() <= held.size and held[1].any(axis=0)[:, cone].all()           # every bin of those frames: a held part
            nf.check(got_p, got_c, ref_p, ref_c, tag=f"host stft {id} {site} {vname}")
            pol = gpu.stft_poisoned_ref(gpu.stft_refs(y, n_fft, hop, True), 1, n, n_fft, hop, i, vname == "nan", True)
            with np.errstate(**ERR):
                m, a = nf.polar64(X[:, 0], X[:, 1])
            assert not np.isfinite(m[np.isnan(pol[:, 0])]).any() and not np.isfinite(a[np.isnan(pol[:, 1])]).any()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("row", gpu.ISTFT_ROWS, ids=lambda r: r[0])
def test_istft_cone_standin_and_the_fmax_peak(row, mode):
    id, bins, hop, frames = row
    a, b = gpu.istft_inputs(bins, frames, mode)
    ref_c = sig.istft64(a, b, hop, mode)[0]
    got_c = sig.standin_istft(a, b, hop, mode)
    length = hop * (frames - 1)
    for plane in (0, 1):
        for frame in (frames // 2, frames - 1):
            for vname, v in gpu.istft_values(mode, plane):
                ap, bp = (nf.poison(a, (1, 3, frame), v), b) if plane == 0 else (a, nf.poison(b, (1, 3, frame), v))
                with np.errstate(**ERR):
                    y64 = sig.istft64(ap, bp, hop, mode)[0]
                    got_p = sig.standin_istft(ap, bp, hop, mode)
                ref_p = np.stack([ref_c[0], nf.istft_poisoned(ref_c[1], 2 * bins, hop, frame, 3, plane, mode)])
                held, unheld, bad = np.isnan(ref_p), ref_p == nf.UNHELD, ~np.isfinite(y64)
                assert bad[held].all() and not bad[~held & ~unheld].any(), (id, mode, plane, frame, vname)
                assert np.array_equal((held | unheld)[1], nf.istft_cone(2 * bins, hop, frames, frame)) and not (held | unheld)[0].any()
                assert 1 <= held.sum() and 2 * held.sum() <= held.size and 2 * held.sum() > (held | unheld).sum()
                nf.check(got_p, got_c, ref_p, ref_c, tag=f"host istft {id} mode {mode} plane {plane} frame {frame} {vname}")
                with np.errstate(**ERR):
                    norm = lambda yy, mx: (yy / mx(np.abs(yy), axis=1, keepdims=True)).astype(yy.dtype)
                    ref_pn, ref_cn = nf.normalised(ref_p, vname == "nan"), norm(ref_c, np.max)
                    nf.check(norm(got_p, np.max), norm(got_c, np.max), ref_pn, ref_cn, tag="host istft normalised")
                    if vname == "nan":                   # planted: a peak that drops the NaN leaves the rest of the signal finite
                        assert "R1" in rejected(norm(got_p, np.fmax.reduce), norm(got_c, np.max), ref_pn, ref_cn)
    if mode == 0:
        with np.errstate(**ERR):
            assert np.isfinite(sig.istft64(nf.poison(a, (1, 3, 2), nf.NINF), b, hop, 0)[0]).all()      # expm1(-inf) = -1: why it is left out


def test_gl_and_ola_cases_have_proper_cones():
    import test_z_gl_blocks_gpu as gl
    for case in gpu.OLA_CASES:
        N, hop, frames, clips = case
        fr = gpu.detgen.normal(991, (clips, N, frames))
        for index in ((clips - 1, N // 2 + 1, frames // 2), (clips - 1, N // 2 - 1, frames - 1)):
            with np.errstate(**ERR):
                assert int((~np.isfinite(gl._ola_ref(nf.poison(fr, index, nf.NAN), hop)[0])).sum()) == 1


def test_spec_clips_and_resample_standins_pass():
    """the fp32 restatement of tests/_spectral_ref.py and a float32 direct sum against the float64 references, on the GPU module's cases"""
    import _spectral_ref as spec
    import test_resample_gpu as rs
    n_ch, bins, F_src, n_clips, frames, sf = 2, 5, 40, 3, 12, 8
    P = gpu.detgen.normal(1011, (n_ch, bins, F_src))
    for spo in (1.0, 1 / 1.5):
        ref_c, got_c = spec.spec_clips(P, n_clips, frames, sf, spo), spec.spec_clips_f32(P, n_clips, frames, sf, spo)
        for f in (0, 10, int(np.floor((2 * sf + frames - 1) * spo))):
            for vname, v in nf.VALUES:
                Pp = nf.poison(P, (1, 2, f), v)
                with np.errstate(**ERR):
                    ref_p = spec.spec_clips(Pp, n_clips, frames, sf, spo)
                assert nf.cone_is_a_proper_part(ref_p, ref_c)
                nf.check(spec.spec_clips_f32(Pp, n_clips, frames, sf, spo), got_c, ref_p, ref_c, tag=f"host spec_clips {spo:.3f} {f} {vname}")
    for up, down in ((160, 441), (1000, 3101)):
        edge = rs.TILE[(up, down)] * down // up
        n_in = 2 * edge + 1
        x = sig.white(1001, 3, n_in)[1]
        b64 = rs.bank64(up, down, 0)
        b32 = b64.astype(F32)
        s32 = lambda a: rs.direct64(a, up, down, 0, bank=b32).astype(F32)               # (the bank rounded first: another arithmetic)
        ref_c, got_c = rs.direct64(x, up, down, 0, bank=b64), s32(x)
        for i in (0, edge, n_in - 1):
            for vname, v in nf.VALUES:
                with np.errstate(**ERR):
                    ref_p, got_p = rs.direct64(nf.poison(x, i, v), up, down, 0, bank=b64), s32(nf.poison(x, i, v))
                assert 1 <= (~np.isfinite(ref_p)).sum() and 6 * (~np.isfinite(ref_p)).sum() <= 3 * ref_p.size     # (one of three signals)
                nf.check(got_p, got_c, ref_p, ref_c, tag=f"host resample {up}/{down} {i} {vname}")
