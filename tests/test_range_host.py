"""CPU: the checkers of tests/_range.py are honest, and every case of tests/test_z_range_gpu.py's table meets the condition of its rule
on the float64 reference alone.

numpy keeps fp32 denormals, so numpy float32 stand-ins -- the k-ordered float32 convolution and the bf16x3 split of
tests/_conv_ref64.py, a direct float32 DFT, the per-cell arithmetic of pg_spec_compare and of pg_abs2 -- must pass every rule; and
each planted fault must fail the rule meant for it:
  outputs flushed to zero below FLT_MIN (M2), operands flushed where the header says kept (M3), + 1e-30f in an epilogue (M1), a
  float16 intermediate (M1), a product formed in fp32 where the formula says double (M1), a 0x1p-60 ladder that forgets to scale back
  (M1), an overflowed output clamped to FLT_MAX (M4)."""
import numpy as np
import pytest

import _conv_ref64 as cref
import _range as rg
import test_z_conv_values_gpu as cv
from test_kernel_families import BF16_FAMILIES

F32 = np.float32
# two small rows (a Conv1d forward / dgrad and a ConvTranspose1d wgrad) for the stand-ins; the conditions are asserted on EVERY row
GEOMS = [((False, 8, 8, 4, 2, 1, 30, 2), "fwd"), ((False, 8, 16, 8, 1, 2, 61, 2), "dgrad"), ((True, 36, 17, 5, 2, 1, 9, 2), "wgrad")]
PRECS = ("fp32", "bf16", "bf16x3")


def variants(op):
    from test_z_nonfinite_gpu import _conv_variants
    return rg.conv_variants(op, _conv_variants(op))


def standin(t, geom, op, variant, prec):
    """the numpy float32 "device": {name: float32 array}"""
    return {n: np.asarray(r[2], F32) for n, r in rg.conv_rows(t, geom, op, variant, prec).items()}


# ---- scaled ---------------------------------------------------------------------------------------------------------------------------
def test_scaled_is_exact_or_raises():
    a = np.array([1.0, -0.75, 3e-5, 0.0, -0.0], F32)
    assert np.array_equal(rg.scaled(a, -100), a * F32(2.0) ** -100) and rg.scaled(a, 100).dtype == F32
    assert np.signbit(rg.scaled(a, 7)[4]) and rg.scaled(a, 7)[3] == 0
    with pytest.raises(AssertionError):
        rg.scaled(a, 128)                      # overflows
    with pytest.raises(AssertionError):
        rg.scaled(np.array([1.0 + 2.0 ** -23], F32), -127)       # a denormal that drops a bit
    assert rg.scaled(np.array([1.0], F32), -149)[0] == F32(2.0 ** -149)          # an exact denormal is fine
    assert rg.stored(np.array([1.0 + 2.0 ** -23], F32), -127)[0] == F32(2.0 ** -127)
    assert np.array_equal(rg.flushed(np.array([1e-39, -1e-39, 1e-37], F32)).view(np.uint32), np.array([0.0, -0.0, 1e-37], F32).view(np.uint32))


# ---- the stand-ins pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("row", GEOMS, ids=lambda r: r[1])
def test_conv_standins_pass_every_rule(row, prec):
    geom, op = row
    t = cv.inputs(geom, "white")
    K = rg.conv_k(geom, op)
    R = rg.conv_roundings(K, prec)
    for variant in variants(op):
        clean_rows = rg.conv_rows(t, geom, op, variant, prec)
        clean = standin(t, geom, op, variant, prec)
        for ex, ew in rg.CONV_M1:
            scales, e = rg.conv_scales(op, ex, ew)
            T = rg.conv_operands(t, op, scales)
            got = standin(T, geom, op, variant, prec)
            for n in got:
                rg.check_m1(got[n], clean[n], clean_rows[n][0], e, operands=[T[k if k != "ref" else "refz"] for k in scales], cast_bf16=prec != "fp32",
                            tag=f"stand-in {prec} {op} [{variant[0]}] {n} ({ex}, {ew})")
        T, operands, m2 = rg.conv_m2(t, geom, op, variant, prec, clean_rows)
        got = standin(T, geom, op, variant, prec)
        for n, (ref_s, bound_s, case_ref) in m2.items():
            rg.check_m2(got[n], ref_s, bound_s, R, operands=operands, cast_bf16=prec != "fp32", case_ref=case_ref, tag=f"stand-in {prec} {op} [{variant[0]}] {n}")
        for ex, ew in rg.conv_m3(prec, op, t):
            scales, e = rg.conv_scales(op, ex, ew)
            den = rg.m3_denormal(scales)
            T = rg.conv_operands(t, op, scales, how=den)
            Tf = dict(T, **{k: rg.flushed(T[k]) for k in den})
            got, rk, rf = standin(T, geom, op, variant, prec), rg.conv_rows(T, geom, op, variant, prec), rg.conv_rows(Tf, geom, op, variant, prec)
            if prec == "bf16x3":            # (as the GPU module states it: the operands as the split sees them, B from the row's clean call)
                rk, rf = rg.conv_rows(T, geom, op, variant, prec, False, True), rg.conv_rows(Tf, geom, op, variant, prec, False, True)
                rk = {n: (rk[n][0], rk[n][1], clean_rows[n][2]) for n in rk}
            for n in got:
                _, b_rel = rg.conv_bound(*clean_rows[n])
                rg.check_m3(got[n], rk[n][0], rf[n][0], b_rel * rk[n][1], R, "kept", tag=f"stand-in {prec} {op} [{variant[0]}] {n} ({ex}, {ew})")
    m4 = m4_case(geom, op, prec)
    got = standin(m4["T"], geom, op, m4["variant"], prec)[m4["name"]]
    rg.check_m4(got, m4["ref"], m4["S"], m4["bound"], m4["B_rel"], nan_ok=prec == "bf16x3", tag=f"stand-in {prec} {op}")


def m4_case(geom, op, prec):
    """the M4 case of a row as tests/test_z_range_gpu.py runs it"""
    return rg.conv_m4_case(geom, op, prec)


# ---- the planted faults fail ----------------------------------------------------------------------------------------------------------
def test_flushed_outputs_fail_m2():
    geom, op = GEOMS[0]
    t = cv.inputs(geom, "white")
    variant = variants(op)[0]
    scales, e = rg.conv_scales(op, *rg.CONV_M2)
    got = standin(rg.conv_operands(t, op, scales), geom, op, variant, "fp32")["y"]
    value, mag, base = rg.conv_rows(t, geom, op, variant, "fp32")["y"]
    bound, _ = rg.conv_bound(value, mag, base)
    R = rg.conv_roundings(rg.conv_k(geom, op), "fp32")
    rg.check_m2(got, np.ldexp(value, e), np.ldexp(bound, e), R, tag="honest")
    with pytest.raises(AssertionError, match="flushed to zero"):
        rg.check_m2(rg.flushed(got), np.ldexp(value, e), np.ldexp(bound, e), R, tag="fault: outputs flushed")


def test_flushed_operands_fail_m3_where_the_header_says_kept():
    geom, op = GEOMS[0]
    t = cv.inputs(geom, "white")
    variant = variants(op)[0]
    scales, e = rg.conv_scales(op, *rg.CONV_M3[0])
    T = rg.conv_operands(t, op, scales, how=["x"])
    Tf = dict(T, x=rg.flushed(T["x"]))
    assert not Tf["x"].any() and T["x"].any()
    rk, rf = rg.conv_rows(T, geom, op, variant, "fp32")["y"], rg.conv_rows(Tf, geom, op, variant, "fp32")["y"]
    bound, _ = rg.conv_bound(*rk)
    R = rg.conv_roundings(rg.conv_k(geom, op), "fp32")
    rg.check_m3(rk[2], rk[0], rf[0], bound, R, "kept", tag="honest")
    rg.check_m3(rf[2], rk[0], rf[0], bound, R, "flushed", tag="a device that flushes, stated as such")
    with pytest.raises(AssertionError, match="M3"):
        rg.check_m3(rf[2], rk[0], rf[0], bound, R, "kept", tag="fault: operands flushed")
    with pytest.raises(AssertionError, match="M3"):
        rg.check_m3(rk[2], rk[0], rf[0], bound, R, "flushed", tag="fault: kept where the header says flushed")


def test_an_absolute_epsilon_and_a_float16_intermediate_fail_m1():
    geom, op = GEOMS[1]
    t = cv.inputs(geom, "white")
    variant = variants(op)[1]
    ref = rg.conv_rows(t, geom, op, variant, "fp32")["dx"][0]
    clean = standin(t, geom, op, variant, "fp32")["dx"]
    for (ex, ew), fault, name in (((-40, -40), lambda a: a + F32(1e-30), "+ 1e-30f"), ((40, 40), lambda a: a.astype(np.float16).astype(F32), "float16")):
        scales, e = rg.conv_scales(op, ex, ew)
        T = rg.conv_operands(t, op, scales)
        got = standin(T, geom, op, variant, "fp32")["dx"]
        rg.check_m1(got, clean, ref, e, tag="honest")
        with np.errstate(over="ignore"):
            bad, bad_clean = fault(got), fault(clean)
        with pytest.raises(AssertionError, match="M1"):
            rg.check_m1(bad, bad_clean, ref, e, tag=f"fault: {name}")


# ---- pg_spec_compare's cell arithmetic --------------------------------------------------------------------------------------------------
def spec_cells32(R, E, gain, widen):
    """slots 0-3 of pg_spec_compare in numpy: mR, mE0 as float32 magnitudes; the products formed in double (widen) or in fp32"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if widen:
            mR = np.sqrt(R[:, 0].astype(np.float64) ** 2 + R[:, 1].astype(np.float64) ** 2).astype(F32)
            mE0 = np.sqrt(E[:, 0].astype(np.float64) ** 2 + E[:, 1].astype(np.float64) ** 2).astype(F32)
            d = (mR - F32(gain) * mE0).astype(np.float64)
            a, b = mR.astype(np.float64), mE0.astype(np.float64)
            terms = (a * a, b * b, a * b, d * d)
        else:
            mR, mE0 = np.sqrt(R[:, 0] * R[:, 0] + R[:, 1] * R[:, 1]), np.sqrt(E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1])
            d = mR - F32(gain) * mE0
            terms = tuple(v.astype(np.float64) for v in (mR * mR, mE0 * mE0, mR * mE0, d * d))
        return np.stack([v.sum((1, 2)) for v in terms], 1)


@pytest.mark.parametrize("e", [-100, -40, 40, 70, 100])
def test_fp32_products_fail_m1_where_the_formula_says_double(e):
    from phasegen import detgen
    from test_compare_gpu import spec_ref
    R, E = detgen.normal(7, (2, 2, 16, 24), std=3.0), detgen.normal(8, (2, 2, 16, 24), std=2.0)
    ref = spec_ref(R, E, 0.81)[:, :4]
    Rs, Es = rg.scaled(R, e), rg.scaled(E, e)
    clean, got = spec_cells32(R, E, 0.81, True), spec_cells32(Rs, Es, 0.81, True)
    rg.check_m1(got, clean, ref, 2 * e, operands=[Rs, Es], out64=True, tag=f"spec cells, widened, 2^{e}")
    if abs(e) > 40:          # squares of 2^+-40 are still normal fp32 numbers: the fault shows past 2^63.5 and below 2^-63
        with pytest.raises(AssertionError, match="M1"):
            rg.check_m1(spec_cells32(Rs, Es, 0.81, False), spec_cells32(R, E, 0.81, False), ref, 2 * e, operands=[Rs, Es], out64=True, tag=f"fault: fp32 products, 2^{e}")


# ---- |z| by scaled squares --------------------------------------------------------------------------------------------------------------
def abs2_32(re, im, lo=F32(2.0 ** -60), up=F32(2.0 ** 90), back=True):
    """csrc/pg_fastmath.h's pg_abs2 in numpy float32; back=False forgets to scale back"""
    re, im = np.asarray(re, F32), np.asarray(im, F32)
    m = np.maximum(np.abs(re), np.abs(im))
    sc = np.where(m < lo, up, np.where(m > F32(2.0 ** 60), F32(2.0 ** -64), F32(1))).astype(F32)
    isc = (F32(1) / sc).astype(F32) if back else F32(1)
    with np.errstate(under="ignore"):
        a, b = re * sc, im * sc
        return (np.sqrt(a * a + b * b) * isc).astype(F32)


def test_a_ladder_that_forgets_to_scale_back_fails_m1():
    rng = np.random.default_rng(3)
    re, im = rng.standard_normal(500).astype(F32), rng.standard_normal(500).astype(F32)
    ref = np.hypot(re.astype(np.float64), im.astype(np.float64))
    for e in (-100, -40, 40, 100):
        rs, ims = rg.scaled(re, e), rg.scaled(im, e)
        rg.check_m1(abs2_32(rs, ims), abs2_32(re, im), ref, e, operands=[rs, ims], tag=f"|z| 2^{e}")
        if abs(e) == 100:
            with pytest.raises(AssertionError, match="M1"):
                rg.check_m1(abs2_32(rs, ims, back=False), abs2_32(re, im, back=False), ref, e, operands=[rs, ims], tag=f"fault: no scale back, 2^{e}")


# ---- a direct float32 DFT ---------------------------------------------------------------------------------------------------------------
def test_a_direct_dft_is_equivariant_and_an_invariant_normalisation_keeps_its_bits():
    from phasegen import detgen
    N = 16
    x = detgen.normal(5, (6, N))
    k, m = np.arange(1, N // 2)[:, None], np.arange(N)[None, :]            # (the Nyquist bin's sine is 1e-16: not a normal output)
    C, S = np.cos(2 * np.pi * k * m / N).astype(F32), (-np.sin(2 * np.pi * k * m / N)).astype(F32)

    def dft(a):
        out = np.zeros((2, len(a), N // 2 - 1), F32)
        for j in range(N):                       # k-ordered, one rounding per product and per addition
            out[0] += a[:, j, None] * C[None, :, j]
            out[1] += a[:, j, None] * S[None, :, j]
        return out

    ref = np.stack([x.astype(np.float64) @ C.astype(np.float64).T, x.astype(np.float64) @ S.astype(np.float64).T])
    assert (np.abs(ref) > 1e-6).all()
    clean = dft(x)
    for e in (-100, -40, 40, 100):
        xs = rg.scaled(x, e)
        rg.check_m1(dft(xs), clean, ref, e, operands=[xs], tag=f"direct DFT 2^{e}")
        peak = lambda a: a / np.abs(a).max()
        rg.check_m1_invariant(peak(dft(xs)), peak(clean), operands=[xs], tag=f"direct DFT / peak 2^{e}")
        if e == -100:           # an absolute epsilon of 1e-35 is 1e-5 of data at 2^-100 and hides behind anything larger
            with pytest.raises(AssertionError, match="invariant"):
                rg.check_m1_invariant(peak(dft(xs) + F32(1e-35)), peak(clean + F32(1e-35)), operands=[xs], tag=f"fault: hidden absolute epsilon 2^{e}")


# ---- tests/_signal_ref64.py cast down: the fp32 STFT and ISTFT stand-ins ------------------------------------------------------------------
def test_the_fp32_transform_standins_pass_m1_and_stay_unflushed_below_flt_min():
    """tests/_signal_ref64.standin_stft / standin_istft on the numpy Stockham FFT (float32 / complex64, denormals kept): equivariant bit
    for bit, and below FLT_MIN within the module's Tier A bound + R 2^-150, as tests/test_z_range_gpu.py asks of the kernels; the same
    outputs flushed to zero fail"""
    import _signal_ref64 as sig
    n_fft, hop, frames = 64, 16, 8
    y = sig.white(961, 2, hop * (frames - 1))
    ref = sig.stft64(y, n_fft, hop)
    keep = np.abs(ref) > 1e-6
    fwd = lambda a: sig.standin_stft(a, n_fft, hop, fft=sig.stockham_fft)
    clean = fwd(y)
    for e in (-100, -40, 40, 100):
        ys = rg.scaled(y, e)
        rg.check_m1(fwd(ys)[keep], clean[keep], ref[keep], e, operands=[ys], tag=f"fp32 STFT stand-in 2^{e}")
    ys = rg.stored(y, rg.den_exponent(ref))
    with np.errstate(under="ignore"):
        got = fwd(ys)
    want, bound = sig.stft64(ys, n_fft, hop), sig.forward_bound(sig.forward_scales(ys, n_fft, hop), "r2", n_fft)[:, None, None, :]
    rg.check_m2(got, want, bound, 16 * n_fft, tag="fp32 STFT stand-in below FLT_MIN")
    with pytest.raises(AssertionError, match="flushed to zero"):
        rg.check_m2(rg.flushed(got), want, bound, 16 * n_fft, tag="fault: STFT outputs flushed")
    bins = n_fft // 2
    from phasegen import detgen
    a, b = detgen.normal(971, (2, bins, frames)), detgen.normal(972, (2, bins, frames))
    inv = lambda p, q: sig.standin_istft(p, q, hop, 1, fft=sig.stockham_fft)
    y64 = sig.istft64(a, b, hop, 1)[0]
    clean = inv(a, b)
    for e in (-100, -40, 40, 100):
        a_s, b_s = rg.scaled(a, e), rg.scaled(b, e)
        rg.check_m1(inv(a_s, b_s), clean, y64, e, operands=[a_s, b_s], tag=f"fp32 ISTFT stand-in 2^{e}")


# ---- M4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_clamped_overflow_fails_m4():
    geom, op = GEOMS[0]
    m4 = m4_case(geom, op, "fp32")
    got = standin(m4["T"], geom, op, m4["variant"], "fp32")[m4["name"]]
    rg.check_m4(got, m4["ref"], m4["S"], m4["bound"], m4["B_rel"], tag="honest")
    with pytest.raises(AssertionError, match="overflow zone"):
        rg.check_m4(np.clip(got, -rg.FLT_MAX, rg.FLT_MAX), m4["ref"], m4["S"], m4["bound"], m4["B_rel"], tag="fault: clamped to FLT_MAX")
    with pytest.raises(AssertionError, match="overflow zone"):
        rg.check_m4(np.where(np.isinf(got), F32("inf"), got), m4["ref"], m4["S"], m4["bound"], m4["B_rel"], tag="fault: the sign is lost")
    nan = np.where(np.isinf(got), F32("nan"), got)
    rg.check_m4(nan, m4["ref"], m4["S"], m4["bound"], m4["B_rel"], nan_ok=True, tag="NaN where the split may answer NaN")
    with pytest.raises(AssertionError, match="overflow zone"):
        rg.check_m4(nan, m4["ref"], m4["S"], m4["bound"], m4["B_rel"], tag="fault: NaN from an fp32 path")
    half = np.where(np.isfinite(got), got * F32(0.5), got)
    with pytest.raises(AssertionError, match="finite zone"):
        rg.check_m4(half, m4["ref"], m4["S"], m4["bound"], m4["B_rel"], tag="fault: a wrong finite value")


# ---- every case of the table meets its conditions on the float64 reference alone -----------------------------------------------------------
def _rows():
    seen, out = set(), []
    for c in cv.CASES:
        for prec in PRECS:
            if prec != "fp32" and c[3] not in BF16_FAMILIES:
                continue
            if (c[0], c[1], prec) not in seen:
                seen.add((c[0], c[1], prec))
                out.append(pytest.param(c[0], c[1], prec, id=f"{cv.fixup_case_id(c)}-{prec}"))
    for geom in sorted({r[0] for r in cv.H_ROWS}):
        if (geom, "fwd", "bf16") not in seen:
            seen.add((geom, "fwd", "bf16"))
            out.append(pytest.param(geom, "fwd", "bf16", id=f"h-{geom}"))
    return out


@pytest.mark.parametrize("geom,op,prec", _rows())
def test_every_conv_case_meets_the_conditions_of_its_rules(geom, op, prec):
    """M1: every scaled operand and reference output normal; M2: all outputs below FLT_MIN, half above R 2^-150; M3: the kept and the
    flushed restatement apart; M4: both zones occupied, at most a quarter between them -- from float64 alone (no stand-in, no device)"""
    t = cv.inputs(geom, "white")
    rounded = "bf16" if prec == "bf16" else "fp32"
    R = rg.conv_roundings(rg.conv_k(geom, op), prec)
    for variant in variants(op):
        value, mag = cref.conv64(op, geom, t["x"], t["w"], t["dy"], variant[1], rounded)
        pre = value + t["add"].astype(np.float64) if op == "dgrad" and variant[2] is not None else value         # (the cap: before a mask or a ReLU)
        if op == "dgrad" and variant[2] is not None:
            value, mag = cref.dgrad_epilogue64(value, mag, t["add"], t["refz"], variant[2])
        for ex, ew in rg.CONV_M1:
            scales, e = rg.conv_scales(op, ex, ew)
            T = rg.conv_operands(t, op, scales)
            assert rg.operands_normal([T[k if k != "ref" else "refz"] for k in scales], prec != "fp32")
            assert rg.is_normal_or_zero(np.ldexp(value, e)).all(), (variant[0], ex, ew)
        scales, e = rg.conv_scales(op, *rg.CONV_M2)
        scales.pop("add", None)
        assert rg.operands_normal([rg.conv_operands(t, op, scales)[k if k != "ref" else "refz"] for k in scales], prec != "fp32")
        assert rg.m2_case_ok(np.ldexp(pre, e), R) and (np.abs(np.ldexp(value, e)) < rg.FLT_MIN).all(), (variant[0], float(np.median(np.abs(value))), R)
        for ex, ew in rg.conv_m3(prec, op, t):
            scales, e = rg.conv_scales(op, ex, ew)
            den = rg.m3_denormal(scales)
            T = rg.conv_operands(t, op, scales, how=den)
            assert all(np.all(np.abs(T[k]) < rg.FLT_MIN) and T[k].any() for k in den)
            vk, mk = cref.conv64(op, geom, T["x"], T["w"], T["dy"], variant[1], rounded)
            assert 2 * int((np.abs(vk) > 1e-3 * mk).sum()) >= vk.size          # (flushed: the sum is 0; the bound is ~1e-6 mag)
    m4 = rg.conv_m4_exponent(geom, op, prec)
    assert m4["e"] is not None, "no exponent leaves a quarter of the outputs in each zone"
    assert rg.m4_case_ok(np.ldexp(m4["value"], m4["e"]), np.ldexp(m4["mag"], m4["e"]), m4["B_worst"])
    assert np.array_equal(np.abs(m4["value"]), m4["mag"])                      # one sign per output: S = |ref|
