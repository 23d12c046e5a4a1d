"""GPU: what the exponent range -- fp32 denormals to FLT_MAX -- does to every entry point (include/phasegen.h, "Magnitude range").

The value modules feed the kernels numbers of order one.  Here the same geometries, shapes and inputs are multiplied by exact powers
of two and held to the four rules of tests/_range.py:
  M1  operands and reference outputs stay normal: the outputs are the clean call's times the scale, BIT FOR BIT (scale-free outputs:
      the clean call's bits).  No reference and no tolerance: a hidden absolute epsilon, a narrower intermediate, a flush or a scale
      ladder that is off by one fails it.
  M2  outputs below FLT_MIN: within B 2^e + R 2^-150 of float64 (gradual underflow, no flush).
  M3  denormal operands: the ONE outcome the header states for the mode, "kept" or "flushed", for every element.
  M4  overflow: finite and within bound where sum |a b| < FLT_MAX / 2, non-finite with the reference's sign where |ref| is beyond
      FLT_MAX (1 + B).
Entry points that are not homogeneous (BatchNorm, Adam, the loss, log-magnitudes) are held to their float64 restatements at scaled
inputs just inside the domain the header states.

Every bound is one an existing value module asserts (cited where it is used) or a count of roundings times 2^-150 (derived in
tests/_range.py); every exponent that is not the issue's is chosen on the CPU from the float64 reference.  Every row prints RANGE
lines (pytest -s).  tests/test_range_host.py shows on the CPU that the checkers have teeth and that every case meets the condition
of its rule.  No call here is meant to fault: tiny and huge floats are ordinary data to these kernels.
Named test_z_* so that it is collected behind the older modules."""
import functools

import numpy as np
import pytest
import torch

import _conv_ref64 as cref
import _range as rg
import _signal_ref64 as sig
from phasegen import detgen

pytestmark = pytest.mark.gpu
F32 = np.float32
NAN = float("nan")
SCALES = (-100, -40, 40, 100)               # M1 of the linear kernels


def _znf():
    import test_z_nonfinite_gpu as znf
    return znf


def _cv():
    import test_z_conv_values_gpu as cv
    return cv


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _np(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _nan(shape):
    return torch.full(tuple(shape), NAN, device=_dev())


class Failures:
    """collects the violations of a row, so that one run shows all of them"""

    def __init__(self):
        self.msgs = []

    def run(self, fn, *args, **kw):
        try:
            return fn(*args, **kw)
        except AssertionError as e:
            self.msgs.append(str(e))

    def done(self):
        assert not self.msgs, f"{len(self.msgs)} violations:\n" + "\n".join(self.msgs[:40])


# =====================================================================================================================================
# conv
# =====================================================================================================================================
# M3 as measured (include/phasegen.h, "Magnitude range"): what each operand mode does with a denormal operand
M3_OUTCOME = {"fp32": "kept", "bf16": "kept", "bf16x3": "kept", "h": "kept"}


def conv_clean_rows(geom, op, variant, prec):
    """rg.conv_rows of the row's white input, from the value module's own caches (one stand-in per row and precision for both modules)"""
    cv = _cv()
    value, mag = cv.exact(geom, op, "white", variant[1], prec == "bf16")
    return rg.conv_epilogue(cv.inputs(geom, "white"), op, variant, value, mag, cv.honest(geom, op, "white", variant[1], prec))


def conv_call(geom, op, sched, prec, variant, T):
    """one call of the variant on the host operand set T into NaN-filled outputs, every byte of the workspace 0xff: {name: numpy}"""
    from phasegen import ops
    znf = _znf()
    tr, Cin, Cout, k, s, p, Lin, B = geom
    kw = dict(transposed=tr, precision=prec, schedule=sched)
    xs, ws, dys = cref.shapes(geom)
    name, x_act, mask = variant
    with znf._FilledWorkspace():
        if op == "fwd":
            if x_act == cref.NONE or name.startswith("y("):
                outs = {"y": _nan(dys)}
                ops.conv_fwd(_to(T["x"]), _to(T["w"]), outs["y"], s, p, x_act=x_act, **kw)
            else:
                outs = {"y": _nan(dys), "y2": _nan(dys)}
                ops.conv_fwd(_to(T["x"]), _to(T["w"]), outs["y"], s, p, x_act=ops.ACT_LEAKY, y_act=ops.ACT_LEAKY, y2=outs["y2"], y2_act=ops.ACT_RELU, **kw)
        elif op == "dgrad":
            outs = {"dx": _nan(xs)}
            if mask is None:
                ops.conv_dgrad(_to(T["dy"]), _to(T["w"]), outs["dx"], s, p, **kw)
            else:
                ops.conv_dgrad(_to(T["dy"]), _to(T["w"]), outs["dx"], s, p, add=_to(T["add"]), ref=_to(T["refz"]), mask=mask, **kw)
        else:
            outs = {"dw": _nan(ws)}
            ops.conv_wgrad(_to(T["x"]), _to(T["dy"]), outs["dw"], s, p, x_act=x_act, **kw)
    return {n: _np(v) for n, v in outs.items()}


def _used(T, scales):
    return [T["refz" if k == "ref" else k] for k in scales]


def run_conv_rules(geom, op, prec, call, outcome, tagp, variants=None):
    """M1 - M4 of one row; `call(variant, T)` runs the kernel on a host operand set"""
    znf, cv = _znf(), _cv()
    t = cv.inputs(geom, "white")
    R = rg.conv_roundings(rg.conv_k(geom, op), prec)
    cast = prec != "fp32"
    fails = Failures()
    for variant in (variants or rg.conv_variants(op, znf._conv_variants(op))):
        rows = conv_clean_rows(geom, op, variant, prec)
        clean = call(variant, t)
        tag = f"{tagp} [{variant[0]}]"
        for ex, ew in rg.CONV_M1:
            scales, e = rg.conv_scales(op, ex, ew)
            T = rg.conv_operands(t, op, scales)
            got = call(variant, T)
            for n in rows:
                fails.run(rg.check_m1, got[n], clean[n], rows[n][0], e, operands=_used(T, scales), cast_bf16=cast, tag=f"{tag} {n} ({ex}, {ew})")
        T, operands, m2 = rg.conv_m2(t, geom, op, variant, prec, rows)       # B: tests/test_z_conv_values_gpu.check, MARGIN x the stand-in's r_max
        got = call(variant, T)
        for n, (ref_s, bound_s, case_ref) in m2.items():
            fails.run(rg.check_m2, got[n], ref_s, bound_s, R, operands=operands, cast_bf16=cast, case_ref=case_ref, tag=f"{tag} {n} {rg.CONV_M2}")
        for ex, ew in rg.conv_m3(prec, op, t):
            scales, e = rg.conv_scales(op, ex, ew)
            den = rg.m3_denormal(scales)
            T = rg.conv_operands(t, op, scales, how=den)
            Tf = dict(T, **{k: rg.flushed(T[k]) for k in den})
            got, rk, rf = call(variant, T), rg.conv_rows(T, geom, op, variant, prec, False, prec == "bf16x3"), rg.conv_rows(Tf, geom, op, variant, prec, False, prec == "bf16x3")
            for n in rk:
                _, b_rel = rg.conv_bound(*rows[n])                # B of the row's clean call (the stand-in on the white input), on this case's sum |a b|
                fails.run(rg.check_m3, got[n], rk[n][0], rf[n][0], b_rel * rk[n][1], R, outcome, tag=f"{tag} {n} ({ex}, {ew})")
    m4 = rg.conv_m4_case(geom, op, prec)
    got = call(m4["variant"], m4["T"])[m4["name"]]
    fails.run(rg.check_m4, got, m4["ref"], m4["S"], m4["bound"], m4["B_rel"], nan_ok=prec == "bf16x3", tag=f"{tagp} [{m4['variant'][0]}] total 2^{m4['e']}")
    fails.done()


def run_conv(case, prec):
    from phasegen import ops
    geom, op, sched, fam = case[:4]
    if op == "wgrad":           # (sizes the workspace)
        t = _cv().inputs(geom, "white")
        ops.conv_wgrad(_to(t["x"]), _to(t["dy"]), torch.empty(cref.shapes(geom)[1], device=_dev()), geom[4], geom[5], x_act=ops.ACT_LEAKY,
                       transposed=geom[0], precision=prec, schedule=sched)
    run_conv_rules(geom, op, prec, lambda variant, T: conv_call(geom, op, sched, prec, variant, T), M3_OUTCOME[prec], f"{prec} {fam} {op}")


@pytest.mark.parametrize("case", _znf()._conv_cases())
def test_conv_fp32(case):
    run_conv(case, "fp32")


@pytest.mark.parametrize("case", _znf()._conv_cases(_znf()._bf16_families()))
def test_conv_bf16(case):
    run_conv(case, "bf16")


@pytest.mark.parametrize("case", _znf()._conv_cases(_znf()._bf16_families()))
def test_conv_bf16x3(case):
    run_conv(case, "bf16x3")


@pytest.mark.parametrize("row", _znf()._h_rows()[0], ids=_znf()._h_rows()[1])
def test_conv_fwd_h(row):
    """pg_conv_fwd_h behind the device's own row cast and shadow weights: the fp32 y at the bf16 criterion; the bf16 copies
    yh = LeakyReLU and yh2 = ReLU are the kernel's own y activated and rounded once (tests/test_z_conv_values_gpu.run_values_h3), which
    carries every rule over to them wherever the rounded value is a normal bf16 number"""
    from phasegen import ops
    znf = _znf()
    geom, epi, sched = row
    tr, Cin, Cout, k, s, p, Lin, B = geom
    Lout = cref.out_len(tr, Lin, k, s, p)

    def call(variant, T):
        dev = _dev()
        xh = ops.h_alloc(B, Cin, Lin, dev)
        ops.cast_rows_bf16(_to(T["x"]), xh, act=variant[1])
        w = _to(T["w"])
        wh = ops.shadow_weights(w, tr, s)
        y, yh, yh2 = _nan((B, Cout, Lout)), ops.h_alloc(B, Cout, Lout, dev), ops.h_alloc(B, Cout, Lout, dev)
        with znf._FilledWorkspace():
            ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, transposed=tr, y=y, yh=yh, yh_act=ops.ACT_LEAKY, yh2=yh2, yh2_act=ops.ACT_RELU, schedule=sched)
        yc = _np(y)
        with np.errstate(over="ignore"):
            lk, rl = cref.bf16(cref.act32(yc, cref.LEAKY)), cref.bf16(cref.act32(yc, cref.RELU))
        fin = np.isfinite(yc)
        assert np.array_equal(_np(yh)[:, :, :Lout][fin], lk[fin]) and np.array_equal(_np(yh2)[:, :, :Lout][fin], rl[fin]), "yh / yh2 are not y activated and rounded"
        assert not np.isfinite(_np(yh)[:, :, :Lout][~fin]).any()
        return {"y": yc}

    variants = [("y", cref.NONE, None), ("y(leaky x)", cref.LEAKY, None), ("y(relu x)", cref.RELU, None)]
    run_conv_rules(geom, "fwd", "bf16", call, M3_OUTCOME["h"], f"bf16-resident conv_h3 {znf._h_rows()[1](row)}", variants=variants)


# =====================================================================================================================================
# the compare kernels
# =====================================================================================================================================
def _compare():
    import test_compare_gpu as tc
    return tc


WAVE_SHAPES = [(2, 3), (3, 184), (1, 1023), (3, 70001)]            # of tests/test_compare_gpu.py (its one-sample row has no second term)
SPEC_SHAPES = [(3, 16, 24), (2, 37, 70), (1, 1024, 5), (2, 16, 261), (2, 70, 264)]


@pytest.mark.parametrize("shape", WAVE_SHAPES)
def test_wave_compare(shape):
    """pg_wave_compare with a gain, x and y times 2^e: slots 0 - 3 times 2^(2 e), slot 4 times 2^e, slot 5 unchanged -- bit for bit, in
    double.  Then denormal inputs (M3, kept: the kernel widens before it multiplies) and inputs whose squares pass FLT_MAX, against
    float64 at the bounds tests/test_compare_gpu.check_wave asserts."""
    from phasegen import ops
    tc = _compare()
    rows, n = shape
    x, y = detgen.normal(5, shape, std=0.7), detgen.normal(6, shape, std=0.5)
    gain = torch.from_numpy(np.array([0.37, -1.25, 2.0])[:rows]).to(_dev())
    clean = _np(ops.wave_compare(_to(x), _to(y), gain=gain))
    ref = tc.wave_ref(x, y, gain.cpu().numpy())
    fails = Failures()
    for e in SCALES:
        xs, ys = rg.scaled(x, e), rg.scaled(y, e)
        got = _np(ops.wave_compare(_to(xs), _to(ys), gain=gain))
        fails.run(rg.check_m1, got[:, :4], clean[:, :4], ref[:, :4], 2 * e, operands=[xs, ys], out64=True, tag=f"wave_compare {shape} slots 0-3 2^{e}")
        fails.run(rg.check_m1, got[:, 4], clean[:, 4], ref[:, 4], e, out64=True, tag=f"wave_compare {shape} slot 4 2^{e}")
        fails.run(rg.check_m1_invariant, got[:, 5], clean[:, 5], tag=f"wave_compare {shape} slot 5 2^{e}")
    for e, how in ((-140, rg.stored), (126, rg.scaled)):
        xs, ys = how(x, e), how(y, e)
        fails.run(tc.check_wave, ops.wave_compare(_to(xs), _to(ys), gain=gain), tc.wave_ref(xs, ys, gain.cpu().numpy()), f"wave_compare {shape} at 2^{e}")
    fails.done()


@pytest.mark.parametrize("shape", SPEC_SHAPES)
def test_spec_compare(shape):
    """pg_spec_compare with a gain, R and E times 2^e: slots 0 - 3 times 2^(2 e) and slot 5 unchanged, bit for bit (the cells are
    widened before any product: csrc/compare.hip); with the floor scaled along, slot 4 against float64 at check_spec's 1e-4 dB inside
    its domain m^2 <= FLT_MAX.  Denormal cells and cells near FLT_MAX: slots 0 - 3 and 5 against float64 at check_spec's 1e-5."""
    from phasegen import ops
    tc = _compare()
    n, bins, frames = shape
    R, E = detgen.normal(7, (n, 2, bins, frames), std=3.0), detgen.normal(8, (n, 2, bins, frames), std=2.0)
    g = np.array([0.81, 1.7, 0.05])[:n]
    gain = torch.from_numpy(g).to(_dev())
    clean = _np(ops.spec_compare(_to(R), _to(E), gain=gain))
    ref = tc.spec_ref(R, E, g)
    fails = Failures()
    for e in SCALES:
        Rs, Es = rg.scaled(R, e), rg.scaled(E, e)
        got = _np(ops.spec_compare(_to(Rs), _to(Es), gain=gain))
        fails.run(rg.check_m1, got[:, :4], clean[:, :4], ref[:, :4], 2 * e, operands=[Rs, Es], out64=True, tag=f"spec_compare {shape} slots 0-3 2^{e}")
        fails.run(rg.check_m1_invariant, got[:, 5], clean[:, 5], tag=f"spec_compare {shape} slot 5 2^{e}")
    for e in (-40, 40):                                                       # slot 4: floor_power 2^(2 e) stays a normal float
        floor = float(rg.scaled(np.array([tc.FLOOR], F32), 2 * e)[0])
        Rs, Es = rg.scaled(R, e), rg.scaled(E, e)
        assert float(np.abs(Rs).max()) ** 2 * 2 < rg.FLT_MAX
        got = ops.spec_compare(_to(Rs), _to(Es), gain=gain, floor=floor)
        fails.run(tc.check_spec, got, tc.spec_ref(Rs, Es, g, floor), frames, f"spec_compare {shape} 2^{e}, the floor scaled along")
    for e, how in ((-140, rg.stored), (123, rg.scaled)):
        Rs, Es = how(R, e), how(E, e)
        got, want = _np(ops.spec_compare(_to(Rs), _to(Es), gain=gain)), tc.spec_ref(Rs, Es, g)
        rel = np.abs(got[:, :4] - want[:, :4]) / np.abs(want[:, :4])
        print(f"RANGE spec_compare {shape} at 2^{e}: slots 0-3 worst relative error {rel.max():.3e} (bound 1e-5, tests/test_compare_gpu.check_spec), slot 5 {got[:, 5]}")
        if not ((rel <= 1e-5).all() and np.array_equal(got[:, 5], want[:, 5])):
            fails.msgs.append(f"spec_compare {shape} at 2^{e}: slots 0-3 {got[:, :4]} against {want[:, :4]}, slot 5 {got[:, 5]}")
    fails.done()


# =====================================================================================================================================
# pg_polar
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def polar_cells():
    """(re, im) float32: re at every fp32 exponent from the smallest denormal to 2^127, im at exponent offsets -30, -1, 0, +1, +30 from
    it (where that is an fp32 exponent), all four sign pairs, four mantissas each (1, 1.25, 1.5 + 2^-12, 2 - 2^-23; a denormal keeps the bits
    it has): about 20 k cells"""
    mant = np.array([1.0, 1.25, 1.5 + 2.0 ** -12, 2.0 - 2.0 ** -23])
    re, im = [], []
    for e in range(-149, 128):
        for off in (-30, -1, 0, 1, 30):
            if not -149 <= e + off <= 127:
                continue
            for sr in (1.0, -1.0):
                for si in (1.0, -1.0):
                    re.append(sr * np.ldexp(mant, e))
                    im.append(si * np.ldexp(mant[::-1], e + off))
    with np.errstate(under="ignore"):
        return np.concatenate(re).astype(F32), np.concatenate(im).astype(F32)


@pytest.mark.parametrize("use_exp", [False, True], ids=["abs", "log1p"])
def test_polar_every_exponent(use_exp):
    """pg_polar over the whole exponent range against float64 on the stored fp32 cells, at the bounds csrc/pg_fastmath.h states and
    tests/test_signal_gpu.test_polar_arithmetic_against_float64 holds: the angle within 3e-7 rad, the magnitude within 6e-7 relative
    (log1p: of log1p|z|) plus, for |z| below FLT_MIN, the one rounding of the result into the denormals (R = 1: pg_abs2 scales by exact
    powers of two, and only its last product can be a denormal).  |z| beyond FLT_MAX: +inf (use_exp: outside the header's domain)."""
    from phasegen import ops
    re, im = polar_cells()
    assert 19000 < len(re) < 23000 and np.isfinite(re).all() and (re != 0).all() and (im != 0).all()
    pad = (-len(re)) % 8
    d = np.stack([np.concatenate([re, np.ones(pad, F32)]), np.concatenate([im, np.ones(pad, F32)])])[None, :, None, :]
    got = _np(ops.polar(_to(d), out=_nan(d.shape), use_exp=use_exp))[0, :, 0, :len(re)]
    z = np.hypot(re.astype(np.float64), im.astype(np.float64))
    ang = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    over = z > rg.FLT_MAX * (1 + 6e-7)
    inside = z <= rg.FLT_MAX * (1 - 6e-7)
    want = np.log1p(z) if use_exp else z
    bound = 6e-7 * np.maximum(want, 1e-37) + rg.HALF_DENORM
    err_m, err_a = np.abs(got[0].astype(np.float64) - want), np.abs(got[1].astype(np.float64) - ang)
    bad_m, bad_a = inside & ~(err_m <= bound), ~(err_a <= 3e-7)
    small = z < rg.FLT_MIN
    print(f"RANGE polar use_exp={use_exp}: {len(re)} cells, {int(small.sum())} with |z| below FLT_MIN, {int(over.sum())} beyond FLT_MAX; magnitude outside its bound "
          f"{int(bad_m.sum())} ({int((bad_m & small).sum())} below FLT_MIN, {int((bad_m & (got[0] == 0)).sum())} flushed to zero), worst error / bound "
          f"{float((err_m / bound)[inside].max()):.3f}; angle beyond 3e-7 rad {int(bad_a.sum())}, worst {float(err_a.max()):.3e}")
    assert not bad_m.any(), (int(bad_m.sum()), re[bad_m][:4], im[bad_m][:4], got[0][bad_m][:4], want[bad_m][:4])
    assert not bad_a.any(), (int(bad_a.sum()), re[bad_a][:4], im[bad_a][:4], got[1][bad_a][:4], ang[bad_a][:4])
    if not use_exp:
        assert np.isposinf(got[0][over]).all()


def test_polar_scale():
    """|z| (use_exp = 0) is equivariant and the angle invariant under a common power of two, across pg_abs2's and pg_atan2's switches
    at 2^-60 and 2^60; the fused epilogues of pg_stft and pg_stft_crops (always log1p|z|) are the standalone kernel on the
    transform's own (re, im), bit for bit, at every scale of the signal"""
    from phasegen import ops
    d = detgen.normal(951, (2, 2, 5, 7))
    clean = _np(ops.polar(_to(d), out=_nan(d.shape), use_exp=False))
    ref = np.hypot(d[:, 0].astype(np.float64), d[:, 1].astype(np.float64))
    fails = Failures()
    for e in (-100, -70, -59, -40, 40, 59, 70, 100):
        ds = rg.scaled(d, e)
        got = _np(ops.polar(_to(ds), out=_nan(d.shape), use_exp=False))
        fails.run(rg.check_m1, got[:, 0], clean[:, 0], ref, e, operands=[ds], tag=f"polar |z| 2^{e}")
        fails.run(rg.check_m1_invariant, got[:, 1], clean[:, 1], operands=[ds], tag=f"polar angle 2^{e}")
    n_fft, hop, frames = 128, 32, 8
    n = hop * (frames - 1)
    y = sig.white(961, 2, n)
    buf = sig.white(963, 1, 2 * n + 7)[0]
    bd, ed = _to(np.array([0, n + 5], np.int64)), _to(np.full(2, len(buf), np.int64))
    for e in (-120, -100, -40, 0, 40, 100):             # (the fused epilogues have one mode, log1p|z|: there is no use_exp to loop over)
        yd, bufd = _to(rg.stored(y, e)), _to(rg.stored(buf, e))
        fused, alone = _np(ops.stft(yd, n_fft, hop, polar=True)), _np(ops.polar(ops.stft(yd, n_fft, hop, polar=False), use_exp=True))
        fails.run(rg.check_m1_invariant, fused, alone, tag=f"stft polar epilogue against pg_polar of the same spectrum, signal 2^{e}")
        crops = lambda polar: ops.stft_crops(bufd, bd, ed, n, n_fft, hop, polar=polar, stats=None)
        fails.run(rg.check_m1_invariant, _np(crops(True)), _np(ops.polar(crops(False), use_exp=True)),
                  tag=f"stft_crops polar epilogue against pg_polar of the same spectrum, buffer 2^{e}")
    fails.done()


# =====================================================================================================================================
# linear signal and track kernels: M1
# =====================================================================================================================================
def linear_m1(what, run, inputs, ref, scale_of, out_exp, out64=False, scales=SCALES, fails=None, keep=None):
    """`run(*inputs) -> {name: numpy}` at the clean inputs and with input i times 2^(scale_of[i] e): output `name` is the clean one
    times 2^(out_exp[name] e) (0: the clean bits), `ref[name]` its float64 reference (the condition); keep[name]: the elements held (all
    but those the formula makes exactly zero and a transform only nearly: they are rounding noise, which may pass FLT_MIN on its way down)"""
    own = fails is None
    fails = fails or Failures()
    clean = run(*inputs)
    for e in scales:
        ins = [rg.scaled(a, k * e) if k else a for a, k in zip(inputs, scale_of)]
        ops_ = [a for a, k in zip(ins, scale_of) if k]
        got = run(*ins)
        for n, k in out_exp.items():
            if k == 0:
                fails.run(rg.check_m1_invariant, got[n], clean[n], operands=ops_, tag=f"{what} {n} 2^{e}")
            else:
                m = keep[n] if keep and n in keep else np.ones(got[n].shape, bool)
                fails.run(rg.check_m1, got[n][m], clean[n][m], np.asarray(ref[n])[m], k * e, operands=ops_, out64=out64, tag=f"{what} {n} 2^{e}")
    if own:
        fails.done()


@pytest.mark.parametrize("row", _znf().STFT_ROWS, ids=[r[0] for r in _znf().STFT_ROWS])
def test_stft(row):
    from phasegen import ops
    id, n_fft, hop, frames, single = row
    y = sig.white(961, 2, hop * (frames - 1))
    run = lambda a: {"X": _np(ops.stft(_to(a), n_fft, hop, polar=False, out=_nan((2, 2, n_fft // 2, frames)), single_frame=single))}
    ref = sig.stft64(y, n_fft, hop)
    # exact zeros of the formula, 1e-13 in an rfft and rounding noise on the device: the imaginary part of the Nyquist bin, and of every
    # bin of a frame that the reflect padding makes symmetric about its centre (frame 0).  Everything else is far above 1e-6.
    keep = np.abs(ref) > 1e-6
    assert not ((np.abs(ref) > 1e-11) & ~keep).any() and 4 * int(keep.sum()) >= 3 * ref.size
    linear_m1(f"stft {id}", run, [y], {"X": ref}, [1], {"X": 1}, keep={"X": keep})


@pytest.mark.parametrize("row", _znf().CROP_ROWS, ids=[r[0] for r in _znf().CROP_ROWS])
def test_stft_crops(row):
    from phasegen import ops
    id, n_fft, hop, crop_len, single = row
    frames = 1 + crop_len // hop
    buf = sig.white(963, 1, 3 * crop_len + 11)[0]
    begin = np.array([0, crop_len + 5, 2 * crop_len + 9], np.int64)
    bd, ed = _to(begin), _to(np.full(3, len(buf), np.int64))
    run = lambda a: {"X": _np(ops.stft_crops(_to(a), bd, ed, crop_len, n_fft, hop, polar=False, stats=None, out=_nan((3, 2, n_fft // 2, frames)), single_frame=single))}
    ref = sig.stft64(np.stack([buf[b:b + crop_len] for b in begin]), n_fft, hop)
    keep = np.abs(ref) > 1e-6                               # (as in test_stft: the exact zeros of the formula)
    assert not ((np.abs(ref) > 1e-11) & ~keep).any() and 4 * int(keep.sum()) >= 3 * ref.size
    linear_m1(f"stft_crops {id}", run, [buf], {"X": ref}, [1], {"X": 1}, keep={"X": keep})


@pytest.mark.parametrize("row", _znf().ISTFT_ROWS, ids=[r[0] for r in _znf().ISTFT_ROWS])
def test_istft_re_im(row):
    """mode 1 (re, im): un-normalised, the samples scale with the spectrum; normalised, they keep their bits"""
    from phasegen import ops
    znf = _znf()
    id, bins, hop, frames = row
    length = hop * (frames - 1)
    a, b = znf.istft_inputs(bins, frames, 1)
    ref = sig.istft64(a, b, hop, 1)[0]
    for single in ((0, 1) if id == "f4" else (0,)):
        run = lambda at, bt: {"y": _np(ops.istft(_to(at), _to(bt), hop, mode=1, normalize=False, single_frame=single, out=_nan((2, length)))),
                              "y / peak": _np(ops.istft(_to(at), _to(bt), hop, mode=1, normalize=True, single_frame=single, out=_nan((2, length))))}
        linear_m1(f"istft {id} single_frame={single}", run, [a, b], {"y": ref}, [1, 1], {"y": 1, "y / peak": 0})


@pytest.mark.parametrize("case", _znf().OLA_CASES, ids=lambda c: "nfft%d-hop%d-frames%d-n%d" % c)
def test_ola_nt(case):
    from phasegen import ops
    import test_z_gl_blocks_gpu as gl
    N, hop, frames, clips = case
    length = hop * (frames - 1)
    fr = detgen.normal(991, (clips, N, frames))
    run = lambda f: {"y": _np(ops.ola_nt(_to(f), hop, _nan((clips, length)), normalize=False)), "y / peak": _np(ops.ola_nt(_to(f), hop, _nan((clips, length)), normalize=True))}
    linear_m1(f"ola_nt {case}", run, [fr], {"y": gl._ola_ref(fr, hop)[0]}, [1], {"y": 1, "y / peak": 0})


@pytest.mark.parametrize("case", _znf().GL_CASES, ids=lambda c: "bins%d-frames%d-n%d" % c)
def test_gl_project(case):
    """new_spec = mag exp(j angle(S)): equivariant in mag, invariant in S, across the 2^-60 and 2^60 switches of the angle"""
    from phasegen import ops
    import test_z_gl_blocks_gpu as gl
    bins, frames, clips = case
    S, mag = detgen.normal(981, (clips, 2, bins, frames)), (np.abs(detgen.normal(982, (clips, bins, frames))) + F32(0.1)).astype(F32)

    def run(S_, m_):
        x, so = _nan((clips, 2 * bins - 2, frames)), _nan((clips, 2, bins, frames))
        ops.gl_project(_to(S_), _to(m_), x, so)
        return {"spec": _np(so), "x": _np(x)}

    ref = np.stack(gl._project_ref(S, mag), 1)
    ref = np.where(np.abs(ref) < 1e-9, 0.0, ref)                     # (the imaginary parts of DC and Nyquist)
    refx = np.concatenate([ref[:, 0], ref[:, 1, 1:bins - 1]], axis=1)
    fails = Failures()
    linear_m1(f"gl_project {case} mag", run, [S, mag], {"spec": ref, "x": refx}, [0, 1], {"spec": 1, "x": 1}, fails=fails)
    linear_m1(f"gl_project {case} S", run, [S, mag], {}, [1, 0], {"spec": 0, "x": 0}, scales=(-100, -61, -59, -40, 40, 59, 61, 100), fails=fails)
    fails.done()


@pytest.mark.parametrize("up,down", [(160, 441), (1000, 3101)], ids=["160-441", "1000-3101"])
def test_resample(up, down):
    from phasegen import ops
    import test_resample_gpu as rs
    tile = rs.TILE[(up, down)]
    n_in = 2 * (tile * down // up) + 1
    n_out = rs.out_len(n_in, up, down)
    x = sig.white(1001, 3, n_in)
    b64 = rs.bank64(up, down, 0)
    ref = np.stack([rs.direct64(x[s], up, down, 0, bank=b64) for s in range(3)])
    run = lambda a: {"y": _np(ops.resample(_to(a), down, up, res_type="kaiser_best", out=_nan((3, n_out))))}
    linear_m1(f"resample {up}/{down}", run, [x], {"y": ref}, [1], {"y": 1})


@pytest.mark.parametrize("src_per_out", [1.0, 1 / 1.5], ids=["1.0", "1/1.5"])
def test_spec_clips(src_per_out):
    from phasegen import ops
    import _spectral_ref as spec
    n_ch, bins, F_src, n_clips, frames, sf = 2, 5, 40, 3, 12, 8
    P = detgen.normal(1011, (n_ch, bins, F_src))
    run = lambda a: {"clips": _np(ops.spec_clips(_to(a), n_clips, frames, sf, src_per_out, out=_nan((n_clips, n_ch, bins, frames))))}
    linear_m1(f"spec_clips {src_per_out:.3f}", run, [P], {"clips": spec.spec_clips(P, n_clips, frames, sf, src_per_out)}, [1], {"clips": 1})


@pytest.mark.parametrize("shape", _znf().NORM_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_bn_bwd_in_dy(shape):
    """pg_bn_bwd is linear in dy: dx, dgamma and dbeta scale with it (x and the saved statistics stay)"""
    from phasegen import ops
    import _nonfinite as nf
    znf = _znf()
    B, C, L = shape
    x, dy, gamma, beta, rm0, rv0 = znf.norm_inputs(shape)
    xd, gd = _to(x), _to(gamma)
    sm, si = _nan((C,)), _nan((C,))
    ops.bn_fwd(xd, _nan(shape), gd, _to(beta), sm, si, eps=znf.EPS, momentum=znf.MOM)

    def run(dy_):
        dx, dg, db = _nan(shape), _nan((C,)), _nan((C,))
        ops.bn_bwd(xd, _to(dy_), dx, gd, sm, si, dg, db)
        return {"dx": _np(dx), "dgamma": _np(dg), "dbeta": _np(db)}

    ref = nf.bn_bwd64(x, dy, gamma, _np(sm), _np(si))
    linear_m1(f"bn_bwd {shape}", run, [dy], ref, [1], {"dx": 1, "dgamma": 1, "dbeta": 1})


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "leaky", "relu"])
def test_cast_rows_bf16(act):
    from phasegen import ops
    B, C, L = 2, 3, 21
    x = detgen.normal(931, (B, C, L))

    def run(a):
        out = ops.h_alloc(B, C, L, _dev())
        ops.cast_rows_bf16(_to(a), out, act=act)
        o = _np(out)
        assert not o[:, :, L:].any()
        return {"xh": o[:, :, :L]}

    ref = cref.act64(x, act)
    linear_m1(f"cast_rows_bf16 act={act}", run, [x], {"xh": ref}, [1], {"xh": 1})
    got, xs = run(rg.stored(x, -130))["xh"], rg.stored(x, -130)                      # M3: a denormal input, a denormal bf16 output
    want = cref.bf16(cref.act32(xs, act))
    kept = int(np.sum(got.view(np.uint32) == want.view(np.uint32)))
    print(f"RANGE M3 cast_rows_bf16 act={act}: x 2^-130, {kept} of {got.size} are the bf16 rounding of the stored value, {int((got == 0).sum())} zeros ({int((want == 0).sum())} in the rounding)")
    assert kept == got.size


@pytest.mark.parametrize("n", [5, 3 * 1024 + 7])
def test_moments_and_standardize(n):
    """(mean, std) scale with the data, in double; the standardised array keeps its bits"""
    from phasegen import ops
    x = (detgen.normal(941, (n,)) + F32(0.25)).astype(F32)

    def run(a):
        xd = _to(a)
        st = _np(ops.moments(xd))
        ops.standardize_(xd)
        return {"stats": st, "standardized": _np(xd)}

    x64 = x.astype(np.float64)
    linear_m1(f"moments / standardize n={n}", run, [x], {"stats": np.array([x64.mean(), x64.std()])}, [1], {"stats": 1, "standardized": 0}, out64=True)


# =====================================================================================================================================
# phases under a scaling of the magnitudes
# =====================================================================================================================================
@pytest.mark.parametrize("src_per_out", [1.0, 1 / 1.5], ids=["1.0", "1/1.5"])
def test_phases_do_not_depend_on_the_scale_of_the_magnitudes(src_per_out):
    """pg_phase_vocoder, pg_phase_lock, pg_phase_lock_linked (magnitude plane and reset floor scaled together) and pg_phase_spsi: the
    magnitudes enter through comparisons and ratios only, so the phases keep their bits"""
    from phasegen import ops
    n_ch, bins, F_src = 2, 6, 30
    F_out = int((F_src - 1) / src_per_out)
    A = detgen.uniform(1021, (n_ch, bins, F_src), -3.1415, 3.1415)
    M = (np.abs(detgen.normal(1022, (n_ch, bins, F_src))) + F32(0.01)).astype(F32)
    floor = 0.5
    Ad = _to(A)

    def run(M_, fl):
        Md = _to(M_)
        return {"vocoder": _np(ops.phase_vocoder(Ad, F_out, src_per_out, logmag=Md, reset_below=fl, out=_nan((n_ch, bins, F_out)))),
                "lock": _np(ops.phase_lock(Ad, F_out, src_per_out, logmag=Md, reset_below=fl, out=_nan((n_ch, bins, F_out)))),
                "linked": _np(ops.phase_lock_linked(Ad, Ad[0], Md[0], F_out, src_per_out, reset_below=fl, out=_nan((n_ch, bins, F_out)))),
                "spsi": _np(ops.phase_spsi(Md, 2 * bins, bins // 2, out=_nan((n_ch, bins, F_src))))}

    clean = run(M, floor)
    assert all(np.isfinite(v).all() for v in clean.values())
    fails = Failures()
    for e in (-100, -40, 40, 100):
        Ms = rg.scaled(M, e)
        got = run(Ms, float(np.ldexp(floor, e)))
        for n in clean:
            fails.run(rg.check_m1_invariant, got[n], clean[n], operands=[Ms], tag=f"phase {n} src_per_out={src_per_out:.3f}, magnitudes 2^{e}")
    fails.done()


# =====================================================================================================================================
# entry points that are not homogeneous: float64 / IEEE restatements just inside the domains the header states
# =====================================================================================================================================
@pytest.mark.parametrize("e", [-70, 60])
@pytest.mark.parametrize("thin", [False, True], ids=["adam_kernel", "adam_thin_kernel"])
def test_adam_step(thin, e):
    """pg_adam_step at g 2^-70 with state to match (m 2^-70, v 2^-130 stored as denormals: g^2 underflows through the denormals, v v
    beta2 + (1 - beta2) g^2 is a sum of denormals) and at g 2^60 (g^2 near 2^107, inside the header's |grad_scale g| < 2^63): the
    update is IEEE basic operations with denormals kept, so p, m and v have the BITS of the float32 emulation of
    tests/test_z_pointwise_gpu.py -- test_adam_bit_exact's criterion, whose inputs stay clear of the denormals"""
    import test_z_pointwise_gpu as pw
    p, g, m, v = _znf().adam_inputs()
    gs = rg.scaled(g, e)
    if e < 0:
        m, v = rg.scaled(m, e), rg.stored(v, 2 * e + 10)
        assert (np.abs(v) < rg.FLT_MIN).all() and v.all()
    h = pw.ADAM_HYPER["default"]
    pd, md, vd = pw._run_adam(p, gs, m, v, 7, thin, h)
    with np.errstate(under="ignore"):
        pe, me, ve = pw._adam_emulated(p, gs, m, v, 7, **h)
    got = {"p": _np(pd), "m": _np(md), "v": _np(vd)}
    differ = {n: int(np.sum(got[n].view(np.uint32) != w.view(np.uint32))) for n, w in (("p", pe), ("m", me), ("v", ve))}
    print(f"RANGE adam thin={thin} g 2^{e}: elements that differ from the float32 emulation {differ}; denormal v in the emulation "
          f"{int(((ve != 0) & (np.abs(ve) < rg.FLT_MIN)).sum())} of {ve.size}, p moved in {int((pe != p).sum())}")
    assert all(np.isfinite(a).all() for a in got.values()) and np.isfinite(pe).all()
    assert not any(differ.values()), differ


BN_CASES = [(5, 6, 61, 2), (3, 4, 6000, 71)]          # (B, C, L, values a thread adds in sequence): tests/test_z_norm_edges_gpu.HARD_CASES' shapes among NORM_SHAPES


@pytest.mark.parametrize("e", [-70, 50])
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "B%d-C%d-L%d" % c[:3])
def test_bn_fwd(case, e):
    """pg_bn_fwd at x 2^-70 (the centred squares are denormals or zero and eps alone normalises, as the formula says) and x 2^50
    (centred squares near 2^104, inside the header's |x - mean| < 2^63), against float64 at the bounds
    tests/test_z_norm_edges_gpu.test_bn_ill_conditioned_channels derives, restated for an eps that is not negligible: a shift d of the
    mean moves y by |gamma| d invstd and the variance by d^2, so E / sigma there reads E invstd here (the same number where eps is
    negligible); everything else is taken unchanged."""
    from phasegen import ops
    znf = _znf()
    B, C, L, P = case
    shape, n = (B, C, L), B * L
    x, dy, gamma, beta, rm0, rv0 = znf.norm_inputs(shape)
    xs = rg.scaled(x, e)
    eps, mom = float(F32(znf.EPS)), float(F32(znf.MOM))
    x64 = xs.astype(np.float64)
    mean64 = x64.mean(axis=(0, 2))
    var64 = ((x64 - mean64[None, :, None]) ** 2).mean(axis=(0, 2))
    inv64 = 1.0 / np.sqrt(var64 + eps)
    xhat = (x64 - mean64[None, :, None]) * inv64[None, :, None]
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    y64 = xhat * g64[None, :, None] + b64[None, :, None]
    E = (P + 10) * rg.U * np.abs(x64).mean(axis=(0, 2))
    r_inv = 0.5 * (E * inv64) ** 2 + (P + 12) * rg.U
    unb64 = var64 * n / (n - 1)
    rm64, rv64 = (1 - mom) * rm0.astype(np.float64) + mom * mean64, (1 - mom) * rv0.astype(np.float64) + mom * unb64
    y, sm, si = _nan(shape), _nan((C,)), _nan((C,))
    rm, rv = _to(rm0), _to(rv0)
    ops.bn_fwd(_to(xs), y, _to(gamma), _to(beta), sm, si, rm, rv, eps=znf.EPS, momentum=znf.MOM)
    smh, sih = _np(sm).astype(np.float64), _np(si).astype(np.float64)
    e_mean = np.abs(smh - mean64) / E
    e_inv = np.abs(sih / inv64 - 1) / r_inv
    y_bound = np.abs(g64)[None, :, None] * (E * inv64)[None, :, None] * (1 + np.abs(xhat)) + 4e-6 * (np.abs(g64)[None, :, None] * np.abs(xhat) + np.abs(b64)[None, :, None])
    e_y = (np.abs(_np(y).astype(np.float64) - y64) / y_bound).max(axis=(0, 2))
    rm_bound = mom * E + 6 * rg.U * (np.abs((1 - mom) * rm0) + np.abs(mom * mean64))
    rv_bound = mom * unb64 * 2 * r_inv + 6 * rg.U * (np.abs((1 - mom) * rv0) + mom * unb64)
    e_rm, e_rv = np.abs(_np(rm) - rm64) / rm_bound, np.abs(_np(rv) - rv64) / rv_bound
    print(f"RANGE bn_fwd {shape} x 2^{e}: as fractions of the bounds, worst channel: mean {e_mean.max():.3f}, invstd {e_inv.max():.3f}, y {e_y.max():.3f}, "
          f"running_mean {e_rm.max():.3f}, running_var {e_rv.max():.3f}; var64 / eps {float((var64 / eps).max()):.3e}")
    assert (e_mean <= 1).all() and (e_inv <= 1).all() and (e_y <= 1).all() and (e_rm <= 1).all() and (e_rv <= 1).all()


# =====================================================================================================================================
# pg_stitch, pg_ola_stretch, pg_hpss: M1
# =====================================================================================================================================
STITCH_SHAPES = [(2, 4, 184, 92, 0), (1, 9, 23, 11, 3), (1, 7, 184, 8, 183)]        # of tests/test_stitch_gpu.py: (tracks, clips, T, V, cut)


@pytest.mark.parametrize("shape", STITCH_SHAPES)
def test_stitch(shape):
    """the crossfaded join scales with the clips; normalised by its own peak it keeps its bits"""
    from phasegen import ops
    import test_stitch_gpu as st
    n_tracks, n_clips, T, V, cut = shape
    clips, n_out = st.make_clips(shape), st.n_out_of(shape)
    run = lambda c: {"track": _np(ops.stitch(_to(c), T - V, n_out)), "track / peak": _np(ops.stitch(_to(c), T - V, n_out, normalize=True))}
    linear_m1(f"stitch {shape}", run, [clips], {"track": st.ref64(clips, T - V, n_out)[0]}, [1], {"track": 1, "track / peak": 0})


@pytest.mark.parametrize("spo", [1.0, 1 / 1.3, 0.5], ids=["1.0", "1/1.3", "0.5"])
def test_ola_stretch(spo):
    """windowed overlap-add of x on top of a base: both scaled, the sum scales"""
    from phasegen import ops
    import _transient_ref as tr
    n_in, n_out, w, hop = 1000, 1025, 256, 64
    x = (np.random.RandomState(11).standard_normal((2, n_in)) * 2.0).astype(F32)
    base = (np.random.RandomState(12).standard_normal((2, n_out)) * 2.0).astype(F32)
    run = lambda a, b: {"y": _np(ops.ola_stretch(_to(a), n_out, spo, w, hop)), "y + base": _np(ops.ola_stretch(_to(a), n_out, spo, w, hop, base=_to(b)))}
    win = tr.ola_window(w)
    ref = {"y": tr.ola_stretch(x, n_out, spo, win, hop, dtype=np.float64), "y + base": tr.ola_stretch(x, n_out, spo, win, hop, base=base, dtype=np.float64)}
    keep = {n: np.abs(r) > 1e-6 for n, r in ref.items()}                 # (outputs no window covers are exact zeros; sums that cancel to rounding noise)
    assert all(4 * int(k.sum()) >= 3 * k.size for k in keep.values())
    linear_m1(f"ola_stretch {spo:.3f}", run, [x, base], ref, [1, 1], {"y": 1, "y + base": 1}, keep=keep)


@pytest.mark.parametrize("wins", [(17, 17), (3, 5), (31, 1)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_hpss(wins):
    """medians and a comparison: the harmonic and the percussive plane scale with the magnitudes"""
    from phasegen import ops
    import _transient_ref as tr
    M = np.random.RandomState(21).uniform(0.25, 3.0, (2, 65, 64)).astype(F32)

    def run(a):
        harm, perc = ops.hpss(_to(a), *wins)
        return {"harm": _np(harm), "perc": _np(perc)}

    wh, wp = tr.hpss(M, *wins)
    linear_m1(f"hpss {wins}", run, [M], {"harm": wh.astype(np.float64), "perc": wp.astype(np.float64)}, [1], {"harm": 1, "perc": 1})


# =====================================================================================================================================
# linear signal and track kernels below FLT_MIN: nothing is flushed
# =====================================================================================================================================
def test_transforms_and_track_kernels_below_flt_min():
    """pg_stft, pg_istft (mode 1), pg_ola_nt, pg_resample, pg_stitch, pg_spec_clips, pg_ola_stretch and pg_hpss on inputs stored at the
    exponent that puts the largest reference output just below FLT_MIN (chosen from the float64 reference of the clean input).  These
    kernels' gain is one or more, so outputs below FLT_MIN need inputs below it too: M3 on an fp32 path ("kept") with M2's
    comparison, |got - ref64| <= B 2^e + R 2^-150 on the STORED values.  B is the family's own bound (tests/_signal_ref64.forward_bound /
    inverse_bound, tests/test_z_gl_blocks_gpu.test_ola_nt's 2e-6 sum|fr| / wss, tests/test_resample_gpu.bound, tests/test_stitch_gpu's
    8 u max|clips|), or the bits of the fp32 restatement where the value module asserts those (spec_clips_f32, _transient_ref).  R: a
    transform's output collects the roundings of every operation in its cone, fewer than 2 N complex butterflies of at most 8
    roundings each: 16 N (+ the covering frames and the division of an inverse); a resampled sample `taps` products and sums;
    ola_nt its covering frames + 3; a crossfade 6."""
    from phasegen import ops
    import _spectral_ref as spec
    import _transient_ref as tr
    import test_resample_gpu as rs
    import test_stitch_gpu as st
    import test_z_gl_blocks_gpu as gl
    znf = _znf()
    fails = Failures()
    for id, n_fft, hop, frames, single in znf.STFT_ROWS:
        y = sig.white(961, 2, hop * (frames - 1))
        ys = rg.stored(y, rg.den_exponent(sig.stft64(y, n_fft, hop)))
        got = _np(ops.stft(_to(ys), n_fft, hop, polar=False, out=_nan((2, 2, n_fft // 2, frames)), single_frame=single))
        bound = sig.forward_bound(sig.forward_scales(ys, n_fft, hop), sig.family_of(n_fft, single), n_fft)
        fails.run(rg.check_m2, got, sig.stft64(ys, n_fft, hop), bound[:, None, None, :], 16 * n_fft, tag=f"stft {id} below FLT_MIN")
    for id, bins, hop, frames in znf.ISTFT_ROWS:
        a, b = znf.istft_inputs(bins, frames, 1)
        e = rg.den_exponent(sig.istft64(a, b, hop, 1)[0])
        a_s, b_s = rg.stored(a, e), rg.stored(b, e)
        y64, info = sig.istft64(a_s, b_s, hop, 1)
        got = _np(ops.istft(_to(a_s), _to(b_s), hop, mode=1, normalize=False, out=_nan((2, hop * (frames - 1)))))
        fails.run(rg.check_m2, got, y64, sig.inverse_bound(y64, info, sig.family_of(2 * bins), 2 * bins), 32 * bins + int(np.max(info["C"])) + 1,
                  tag=f"istft {id} below FLT_MIN")
    for case in znf.OLA_CASES:
        N, hop, frames, clips = case
        fr = detgen.normal(991, (clips, N, frames))
        frs = rg.stored(fr, rg.den_exponent(gl._ola_ref(fr, hop)[0]))
        want, scale = gl._ola_ref(frs, hop)
        got = _np(ops.ola_nt(_to(frs), hop, _nan((clips, hop * (frames - 1))), normalize=False))
        fails.run(rg.check_m2, got, want, 2e-6 * scale, -(-N // hop) + 3, tag=f"ola_nt {case} below FLT_MIN")
    for up, down in ((160, 441), (1000, 3101)):
        n_in = 2 * (rs.TILE[(up, down)] * down // up) + 1
        x = sig.white(1001, 3, n_in)
        b64 = rs.bank64(up, down, 0)
        direct = lambda a: np.stack([rs.direct64(a[i], up, down, 0, bank=b64) for i in range(3)])
        xs = rg.stored(x, rg.den_exponent(direct(x)))
        got = _np(ops.resample(_to(xs), down, up, res_type="kaiser_best", out=_nan((3, rs.out_len(n_in, up, down)))))
        fails.run(rg.check_m2, got, direct(xs), rs.bound(up, down, 0, float(np.abs(xs).max())), 2 * rs.geometry(up, down, 0)[3] + 2,
                  tag=f"resample {up}/{down} below FLT_MIN")
    for shape in STITCH_SHAPES:
        n_tracks, n_clips, T, V, cut = shape
        clips, n_out = st.make_clips(shape), st.n_out_of(shape)
        cs = rg.stored(clips, rg.den_exponent(clips))
        got = _np(ops.stitch(_to(cs), T - V, n_out))
        fails.run(rg.check_m2, got, st.ref64(cs, T - V, n_out)[0], 8 * rg.U * float(np.abs(cs).max()), 6, tag=f"stitch {shape} below FLT_MIN")
        # the normaliser's early return (include/phasegen.h): a peak at or below FLT_MIN leaves the track as it is
        fails.run(rg.check_m1_invariant, _np(ops.stitch(_to(cs), T - V, n_out, normalize=True)), got, tag=f"stitch {shape} normalize, peak below FLT_MIN")
    P = detgen.normal(1011, (2, 5, 40))
    Ps = rg.stored(P, rg.den_exponent(P))
    for spo in (1.0, 1 / 1.5):
        got = _np(ops.spec_clips(_to(Ps), 3, 12, 8, spo, out=_nan((3, 2, 5, 12))))
        with np.errstate(under="ignore"):
            want = spec.spec_clips_f32(Ps, 3, 12, 8, spo)
        fails.run(rg.check_m1_invariant, got, want, tag=f"spec_clips {spo:.3f} below FLT_MIN against its fp32 restatement")
    x = (np.random.RandomState(11).standard_normal((2, 1000)) * 2.0).astype(F32)
    xs = rg.stored(x, rg.den_exponent(x) - 1)
    with np.errstate(under="ignore"):
        want = tr.ola_stretch(xs, 1025, 1 / 1.3, tr.ola_window(256), 64)
    fails.run(rg.check_m1_invariant, _np(ops.ola_stretch(_to(xs), 1025, 1 / 1.3, 256, 64)), want, tag="ola_stretch below FLT_MIN against its fp32 restatement")
    M = rg.stored(np.random.RandomState(21).uniform(0.25, 3.0, (2, 65, 64)).astype(F32), -128)
    harm, perc = ops.hpss(_to(M), 17, 17)
    wh, wp = tr.hpss(M, 17, 17)
    fails.run(rg.check_m1_invariant, _np(harm), wh, tag="hpss harm below FLT_MIN against its restatement")
    fails.run(rg.check_m1_invariant, _np(perc), wp, tag="hpss perc below FLT_MIN against its restatement")
    fails.done()


def test_normalisers_below_flt_min():
    """pg_istft and pg_ola_nt with normalize on a signal whose peak is below FLT_MIN: the early return leaves the un-normalised bits
    (include/phasegen.h, the domain of the normalisers); three binades higher the peak is exactly 1"""
    from phasegen import ops
    import test_z_gl_blocks_gpu as gl
    znf = _znf()
    id, bins, hop, frames = znf.ISTFT_ROWS[1]
    a, b = znf.istft_inputs(bins, frames, 1)
    e = rg.den_exponent(sig.istft64(a, b, hop, 1)[0])
    for de, name in ((0, "below"), (3, "above")):
        a_s, b_s = _to(rg.stored(a, e + de)), _to(rg.stored(b, e + de))
        raw, nrm = _np(ops.istft(a_s, b_s, hop, mode=1, normalize=False)), _np(ops.istft(a_s, b_s, hop, mode=1, normalize=True))
        peak = np.abs(raw).max(axis=1)
        print(f"RANGE istft normalize, peak {name} FLT_MIN: peaks {peak}, normalised peaks {np.abs(nrm).max(axis=1)}")
        if de == 0:
            assert (peak <= rg.FLT_MIN).all() and np.array_equal(raw.view(np.uint32), nrm.view(np.uint32))
        else:
            assert (peak > rg.FLT_MIN).all() and (np.abs(nrm).max(axis=1) == 1.0).all() and np.array_equal(nrm, raw / peak[:, None])
    N, hop, frames, clips = znf.OLA_CASES[0]
    fr = detgen.normal(991, (clips, N, frames))
    e = rg.den_exponent(gl._ola_ref(fr, hop)[0])
    length = hop * (frames - 1)
    for de in (0, 3):
        frs = _to(rg.stored(fr, e + de))
        raw, nrm = _np(ops.ola_nt(frs, hop, _nan((clips, length)), normalize=False)), _np(ops.ola_nt(frs, hop, _nan((clips, length)), normalize=True))
        peak = np.abs(raw).max(axis=1)
        if de == 0:
            assert (peak <= rg.FLT_MIN).all() and np.array_equal(raw.view(np.uint32), nrm.view(np.uint32))
        else:
            assert (peak > rg.FLT_MIN).all() and (np.abs(nrm).max(axis=1) == 1.0).all()


# =====================================================================================================================================
# per-clip BatchNorm, the four output copies, the loss, log-magnitude ISTFT: just inside the domains the header states
# =====================================================================================================================================
@pytest.mark.parametrize("e", [-70, 50])
@pytest.mark.parametrize("per_clip", [False, True], ids=["bn_fwd", "clipnorm_fwd"])
def test_norm_fwd_four_copies(per_clip, e):
    """pg_bn_fwd / pg_clipnorm_fwd at x 2^-70 and x 2^50 with all four output copies (NORM_SHAPES[2]): y, save_mean, save_invstd and the
    running buffers against float64 at tests/test_clip_stats_gpu's bound (1e-4 of the tensor's largest value: test_kernel_vs_float64,
    test_running_buffers_bitwise_and_vs_torch; tests/test_z_norm_edges_gpu.test_bn_exact_channels holds pg_bn_fwd's y to 1e-5 of it,
    asserted here for pg_bn_fwd); y2, yh, yh2 are the fp32 y of the same call activated and, for the bf16 rows, rounded once, bit for
    bit (test_kernel_writes_all_four_outputs_at_once's criterion)."""
    import _nonfinite as nf
    import test_clip_stats_gpu as cs
    znf = _znf()
    shape = znf.NORM_SHAPES[2]
    x, dy, gamma, beta, rm0, rv0 = znf.norm_inputs(shape)
    xs = rg.scaled(x, e)
    got = znf._norm_call(per_clip, shape, _to(xs), _to(gamma), _to(beta), rm0, rv0, True)
    ref = nf.bn_fwd64(xs, gamma, beta, rm0, rv0, znf.EPS, znf.MOM, per_clip=per_clip)
    rel = {n: float(np.abs(got[n] - ref[n]).max() / np.abs(ref[n]).max()) for n in ("y", "save_mean", "save_invstd", "running_mean", "running_var")}
    print(f"RANGE {'clipnorm' if per_clip else 'bn'}_fwd {shape} x 2^{e}: max error / max value {rel} (bound {cs.TOL:g})")
    assert max(rel.values()) < cs.TOL and (per_clip or rel["y"] <= 1e-5)
    y = got["y"]
    assert znf.ACTS == {"y": 0, "y2": 1, "yh": 2, "yh2": 0}
    assert np.array_equal(got["y2"].view(np.uint32), cref.act32(y, cref.LEAKY).view(np.uint32))
    assert np.array_equal(got["yh"].view(np.uint32), cref.bf16(cref.act32(y, cref.RELU)).view(np.uint32))
    assert np.array_equal(got["yh2"].view(np.uint32), cref.bf16(y).view(np.uint32))


@pytest.mark.parametrize("e", [-40, 40])
@pytest.mark.parametrize("shape", _znf().LOSS_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_loss_magnitude_planes(shape, e):
    """pg_loss_fwd_bwd with the predicted and the target magnitude plane at 2^-40 and 2^40 (inside the header's |m^ - m| < 2^63), against
    float64 at tests/test_z_pointwise_gpu.test_loss_against_float64's bounds: phase gradients within 4e-6 s, magnitude gradients within
    1e-6 mag_weight s max|dm|, each of the three losses within 4e-6 relative"""
    from phasegen import ops
    import _nonfinite as nf
    znf = _znf()
    B, C, L = shape
    pred, batch = (a.copy() for a in znf.loss_inputs(shape))
    pred[:, C:], batch[:, 0] = rg.scaled(pred[:, C:], e), rg.scaled(batch[:, 0], e)
    dpred, losses = _nan(pred.shape), _nan((3,))
    ops.loss_fwd_bwd(_to(pred), _to(batch), dpred, losses=losses, mag_weight=0.2)
    want, dref = nf.loss64(pred, batch, 0.2)
    d, s = _np(dpred).astype(np.float64), 2.0 / (B * C * L)
    dm_max = float(np.abs(pred[:, C:].astype(np.float64) - batch[:, 0].astype(np.float64)).max())
    e_phase = float(np.abs(d[:, :C] - dref[:, :C]).max()) / s
    e_mag = float(np.abs(d[:, C:] - dref[:, C:]).max()) / (0.2 * s * dm_max)
    e_loss = np.abs(_np(losses) - want) / want
    print(f"RANGE loss {shape} magnitudes 2^{e}: phase {e_phase:.3g} (4e-6)  mag {e_mag:.3g} (1e-6)  losses {e_loss} (4e-6)")
    assert e_phase <= 4e-6 and e_mag <= 1e-6 and (e_loss <= 4e-6).all()


@pytest.mark.parametrize("row", _znf().ISTFT_ROWS[:4], ids=[r[0] for r in _znf().ISTFT_ROWS[:4]])
def test_istft_log_magnitude_near_the_last_finite_exp(row):
    """pg_istft mode 0 with one cell per frame at m = 87 (exp(m) = 2^125.5) among log-magnitudes of order one: inside the header's
    domain, sum over a frame's bins of exp(m) < FLT_MAX / 4.  Against float64 at Tier A of tests/_signal_ref64.inverse_bound, the
    derived bound tests/test_z_signal_values_gpu.test_istft_values asserts through `accept`."""
    from phasegen import ops
    znf = _znf()
    id, bins, hop, frames = row
    a, b = (v.copy() for v in znf.istft_inputs(bins, frames, 0))
    for t in range(frames):
        a[t % 2, (3 * t + 1) % bins, t] = F32(87.0)
    assert float(np.exp(a.astype(np.float64)).sum(axis=1).max()) < rg.FLT_MAX / 4
    y64, info = sig.istft64(a, b, hop, 0)
    got = _np(ops.istft(_to(a), _to(b), hop, mode=0, normalize=False, out=_nan((2, hop * (frames - 1)))))
    err = sig.inverse_errors(got, y64, info, sig.inverse_bound(y64, info, sig.family_of(2 * bins), 2 * bins))
    print(f"RANGE istft {id} log-magnitude, cells at m = 87: largest |error| / Tier A bound {err['a']:.3f}, peak {float(np.abs(y64).max()):.3e}")
    assert np.isfinite(got).all() and err["a"] <= 1.0
