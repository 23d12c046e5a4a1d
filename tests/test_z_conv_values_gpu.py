"""GPU: the VALUES of every conv kernel family, element by element, against float64 (tests/_conv_ref64.py).

The geometry modules hold an fp32 result to 1e-4 of the tensor's max-abs on dense noise of one scale.  The bf16x3 split sits about
5e-6 from exact, so an fp32 call that ran the split -- a wrong `prec` at a launcher, a plan that ignores `precision`, a copied
template argument -- passes them all; and an output that is small next to the tensor's maximum (a channel whose BatchNorm gain has
drifted down) is not looked at.  Here every element is measured in unit roundoffs of ITS OWN terms, r = |got - want| / (u sum |terms|),
and r_max and r_rms must stay within 4 x those of an honest CPU stand-in of the same precision on the same input: numpy float32 with
sequential accumulation for fp32 (and, on bf16-rounded operands, for bf16 and the bf16-resident forward), the emulated split for
bf16x3.  The stand-in is computed here on the CPU, never from the kernel; tests/test_conv_bounds_host.py shows that the stand-ins
built differently pass, that planted faults do not, and that on every row marked [precision] below (GEMM K <= 512) the split's r_rms
is at least 10 x sequential fp32's, so that the fp32 bound rejects it.  Rows with a longer K keep every check; the bound merely no
longer tells the two apart there (the CONVERR lines of those rows carry no [precision] mark, and the host test lists them by name).

Rows: VIEW_CASES of tests/test_kernel_families.py -- every family, epilogue and fixup form under both work splits, the column-tail
launch, the packed wgrads, a runtime (k, s), each pinned to its plan there --, ADDED_CASES below (conv_f's forward and conv_t's
dgrad under the stream-K split, which that table has only unsplit) and FIXUP_CASES_H under both work splits for the resident forward.  Inputs: "white" (the suite's noise) and "graded" (a power of two from 2^-12 .. 2^12 per channel of x, per output
row of w and per channel of dy).  Calls: forward with x_act none, and with x_act leaky storing y as LeakyReLU and y2 as ReLU; dgrad
plain, and with an addend and a mask source that holds exact 0.0 and -0.0 at one element in eight (act'(0) = slope), LeakyReLU and
ReLU; wgrad with x_act leaky.  One-hot inputs are checked BIT FOR BIT: a forward returns the weight slice the impulse selects (at
bf16 the rounded weights, at bf16x3 float32(hi) + float32(lo)) and zeros elsewhere, a dgrad likewise, a wgrad the slice of dy in
the selected rows -- through both work splits, whose fixup then adds exact zeros.

Outputs start as NaN and every byte of the conv workspace is 0xff when a checked call is enqueued, as in
tests/test_z_conv_views_gpu.py.  Named to be collected after the geometry modules: where both fail theirs is the broader finding."""
import functools

import numpy as np
import pytest
import torch

import _conv_ref64 as ref
from test_kernel_families import BF16_FAMILIES, FIXUP_CASES_H, VIEW_CASES, fixup_case_id

pytestmark = pytest.mark.gpu
NAN = float("nan")
KINDS = ("white", "graded")
H_SCHEDULES = (1, 2)            # one tile per workgroup, forced stream-K
H_ROWS = [(geom, epi, sched) for geom, epi, _ in FIXUP_CASES_H for sched in H_SCHEDULES]
# VIEW_CASES reaches the im2col forward of a Conv1d (conv_f) and its dgrad (conv_t) only unsplit (the runtime (k, s) rows): the smallest
# problem that puts each through the stream-K split and the fixup (schedule 6 = im2col | stream-K), in VIEW_CASES' row format;
# tests/test_conv_bounds_host.py pins their plans with pg_conv_describe
ADDED_CASES = [((False, 16, 32, 4, 2, 1, 3, 2), "fwd", 6, "conv_f", "F", "plain"), ((False, 16, 32, 4, 2, 1, 3, 2), "dgrad", 6, "conv_t", "T", "plain")]
CASES = VIEW_CASES + ADDED_CASES


def precision_row(geom, op):
    """does the fp32 bound of this row tell fp32 from the bf16x3 split?  (asserted on the CPU by tests/test_conv_bounds_host.py)"""
    return ref.gemm_k(geom, op) <= ref.PRECISION_K


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(shape):
    return torch.full(tuple(shape), NAN, device=_dev())


class _Poisoned:
    """every byte of this thread's conv workspace is 0xff when the body's call is enqueued, and the call does not replace the buffer"""

    def __enter__(self):
        from phasegen import ops
        self.ws = ops.conv_workspace(_dev())
        self.ws.fill_(0xFF)

    def __exit__(self, *exc):
        from phasegen import ops
        if exc[0] is None:
            assert ops.conv_workspace(_dev()).data_ptr() == self.ws.data_ptr()


# ---- the CPU side, once per (row geometry, op, input): shared by the schedules and, where the operands agree, by the precisions -----
@functools.lru_cache(maxsize=None)
def inputs(geom, kind):
    t = ref.make_inputs(geom, kind)
    t["refz"] = ref.with_zeros(t["ref"])
    assert 0.05 < float(np.mean(t["refz"] == 0)) < 0.25 and bool(np.any(np.signbit(t["refz"]) & (t["refz"] == 0)))
    return t


@functools.lru_cache(maxsize=None)
def exact(geom, op, kind, x_act, rounded):
    t = inputs(geom, kind)
    return ref.conv64(op, geom, t["x"], t["w"], t["dy"], x_act, "bf16" if rounded else "fp32")


@functools.lru_cache(maxsize=None)
def honest(geom, op, kind, x_act, prec):
    t = inputs(geom, kind)
    return ref.standin(op, geom, t["x"], t["w"], t["dy"], x_act, prec)


def check(tag, got, value, mag, standin):
    """print the CONVERR line, then hold `got` to MARGIN x the stand-in's r_max and r_rms"""
    got = got.detach().cpu().numpy()
    err, base = ref.errors(got, value, mag), ref.errors(standin, value, mag)
    print(f"CONVERR {tag} {err['r_max']:.3f} {err['r_rms']:.4f} (bound {ref.bound_text(base)}; stand-in {base['r_max']:.3f} {base['r_rms']:.4f})")
    assert base["zeros"], tag
    assert err["zeros"], f"{tag}: an element no term contributes to is not zero"
    assert ref.accept(err, base), (tag, err, base)


def run_values(case, prec):
    from phasegen import ops
    geom, op, sched, fam = case[:4]
    tr, Cin, Cout, k, s, p, Lin, B = geom
    kw = dict(transposed=tr, precision=prec, schedule=sched)
    rounded = prec == "bf16"
    mark = " [precision]" if prec == "fp32" and precision_row(geom, op) else ""
    for kind in KINDS:
        t = inputs(geom, kind)
        xs, ws, dys = ref.shapes(geom)
        tag = f"{prec} {fam} {op} {kind}{mark}"
        wd = _to(t["w"])
        if op == "fwd":
            xd = _to(t["x"])
            value, mag = exact(geom, op, kind, ref.NONE, rounded)
            y = _nan(dys)
            with _Poisoned():
                ops.conv_fwd(xd, wd, y, s, p, **kw)
            check(tag + " y", y, value, mag, honest(geom, op, kind, ref.NONE, prec))
            value, mag = exact(geom, op, kind, ref.LEAKY, rounded)
            base = honest(geom, op, kind, ref.LEAKY, prec)
            y, y2 = _nan(dys), _nan(dys)
            with _Poisoned():
                ops.conv_fwd(xd, wd, y, s, p, x_act=ops.ACT_LEAKY, y_act=ops.ACT_LEAKY, y2=y2, y2_act=ops.ACT_RELU, **kw)
            check(tag + " leaky(y(leaky x))", y, ref.act64(value, ref.LEAKY), mag, ref.act32(base, ref.LEAKY))
            check(tag + " y2=relu", y2, ref.act64(value, ref.RELU), mag, ref.act32(base, ref.RELU))
        elif op == "dgrad":
            dyd = _to(t["dy"])
            value, mag = exact(geom, op, kind, ref.NONE, rounded)
            base = honest(geom, op, kind, ref.NONE, prec)
            dx = _nan(xs)
            with _Poisoned():
                ops.conv_dgrad(dyd, wd, dx, s, p, **kw)
            check(tag + " dx", dx, value, mag, base)
            addd, refd = _to(t["add"]), _to(t["refz"])
            for mask, name in ((ref.LEAKY, "leaky"), (ref.RELU, "relu")):
                v2, m2 = ref.dgrad_epilogue64(value, mag, t["add"], t["refz"], mask)
                dx = _nan(xs)
                with _Poisoned():
                    ops.conv_dgrad(dyd, wd, dx, s, p, add=addd, ref=refd, mask=mask, **kw)
                check(tag + f" (dx+add)*{name}'(ref)", dx, v2, m2, ref.dgrad_epilogue32(base, t["add"], t["refz"], mask))
        else:
            xd, dyd = _to(t["x"]), _to(t["dy"])
            value, mag = exact(geom, op, kind, ref.LEAKY, rounded)
            ops.conv_wgrad(xd, dyd, torch.empty(ws, device=_dev()), s, p, x_act=ops.ACT_LEAKY, **kw)       # (sizes the workspace)
            dw = _nan(ws)
            with _Poisoned():
                ops.conv_wgrad(xd, dyd, dw, s, p, x_act=ops.ACT_LEAKY, **kw)
            check(tag + " dw(leaky x)", dw, value, mag, honest(geom, op, kind, ref.LEAKY, prec))


def seen_by(prec, t):
    """what a product with 1.0 returns of an fp32 operand, exactly"""
    return {"fp32": lambda a: np.asarray(a, np.float32), "bf16": ref.bf16, "bf16x3": ref.hilo}[prec](t)


def run_impulse(case, prec):
    from phasegen import ops
    geom, op, sched, fam = case[:4]
    tr, Cin, Cout, k, s, p, Lin, B = geom
    kw = dict(transposed=tr, precision=prec, schedule=sched)
    xs, ws, dys = ref.shapes(geom)
    t = inputs(geom, "white")
    first_only = op == "wgrad"
    hot_shape = dys if op == "dgrad" else xs
    for v in range(ref.impulse_variants(B, first_only)):
        hot = ref.impulses(*hot_shape, k, v, first_only)
        if op == "wgrad":
            want, terms = ref.conv64(op, geom, hot, None, seen_by(prec, t["dy"]))
        else:
            want, terms = ref.conv64(op, geom, hot, seen_by(prec, t["w"]), hot)
        want32 = want.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64), want) and float(np.abs(want).max()) > 0         # one term per element: exact
        out = _nan(want.shape)
        if op == "wgrad":
            ops.conv_wgrad(_to(hot), _to(t["dy"]), torch.empty(ws, device=_dev()), s, p, **kw)
        with _Poisoned():
            if op == "fwd":
                ops.conv_fwd(_to(hot), _to(t["w"]), out, s, p, **kw)
            elif op == "dgrad":
                ops.conv_dgrad(_to(hot), _to(t["w"]), out, s, p, **kw)
            else:
                ops.conv_wgrad(_to(hot), _to(t["dy"]), out, s, p, **kw)
        got = out.cpu().numpy()
        wrong = int(np.sum(got != want32))                                # (+0 == -0; a NaN differs from everything)
        print(f"CONVIMPULSE {prec} {fam} {op} variant {v}: {int(np.sum(terms > 0))} selected elements, {wrong} differ")
        assert wrong == 0, (prec, case, v, np.argwhere(got != want32)[:8].tolist())


def _cases(families=None):
    return [pytest.param(c, id=fixup_case_id(c)) for c in CASES if families is None or c[3] in families]


@pytest.mark.parametrize("case", _cases())
def test_values_fp32(case):
    run_values(case, "fp32")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_values_bf16(case):
    run_values(case, "bf16")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_values_bf16x3(case):
    run_values(case, "bf16x3")


@pytest.mark.parametrize("case", _cases())
def test_impulse_fp32(case):
    run_impulse(case, "fp32")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_impulse_bf16(case):
    run_impulse(case, "bf16")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_impulse_bf16x3(case):
    run_impulse(case, "bf16x3")


def _h_id(row):
    g, epi, sched = row
    return f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}-L{g[6]}-B{g[7]}-{epi}-{'stream-k' if sched == 2 else 'tile-per-wg'}"


def _h_call(geom, sched, x, w, x_act):
    """pg_conv_fwd_h on fp32 host data: (y fp32, yh = LeakyReLU, yh2 = ReLU as bf16 rows), the input cast (and activated) on the device"""
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, B = geom
    Lout = ref.out_len(tr, Lin, k, s, p)
    dev = _dev()
    xh = ops.h_alloc(B, Cin, Lin, dev)
    ops.cast_rows_bf16(_to(x), xh, act=x_act)
    wh = ops.shadow_weights(_to(w), tr, s)
    y = _nan((B, Cout, Lout))
    yh, yh2 = ops.h_alloc(B, Cout, Lout, dev), ops.h_alloc(B, Cout, Lout, dev)
    with _Poisoned():
        ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, transposed=tr, y=y, yh=yh, yh_act=ops.ACT_LEAKY, yh2=yh2, yh2_act=ops.ACT_RELU, schedule=sched)
    return y, yh[:, :, :Lout], yh2[:, :, :Lout]


def run_values_h3(geom, sched):
    """the resident forward at the bf16 criterion: float64 of the bf16 operands, 4 x sequential fp32 accumulation of the same; the bf16
    copies are the kernel's own fp32 result activated and rounded once"""
    for kind in KINDS:
        t = inputs(geom, kind)
        for x_act, name in ((ref.NONE, "y"), (ref.LEAKY, "y(leaky x)")):
            value, mag = exact(geom, "fwd", kind, x_act, True)
            y, yh, yh2 = _h_call(geom, sched, t["x"], t["w"], x_act)
            check(f"bf16-resident conv_h3 fwd {kind} {name}", y, value, mag, honest(geom, "fwd", kind, x_act, "bf16"))
            yc = y.cpu().numpy()
            assert np.array_equal(yh.float().cpu().numpy(), ref.bf16(ref.act32(yc, ref.LEAKY)))
            assert np.array_equal(yh2.float().cpu().numpy(), ref.bf16(ref.act32(yc, ref.RELU)))


def run_impulse_h3(geom, sched):
    tr, Cin, Cout, k, s, p, Lin, B = geom
    t = inputs(geom, "white")
    for v in range(ref.impulse_variants(B)):
        hot = ref.impulses(B, Cin, Lin, k, v)
        want, terms = ref.conv64("fwd", geom, hot, ref.bf16(t["w"]), None)
        want32 = want.astype(np.float32)
        y, yh, yh2 = _h_call(geom, sched, hot, t["w"], ref.NONE)
        got = y.cpu().numpy()
        wrong = int(np.sum(got != want32))
        print(f"CONVIMPULSE bf16-resident conv_h3 fwd variant {v}: {int(np.sum(terms > 0))} selected elements, {wrong} differ")
        assert wrong == 0, (geom, sched, v, np.argwhere(got != want32)[:8].tolist())
        assert np.array_equal(yh.float().cpu().numpy(), ref.bf16(ref.act32(want32, ref.LEAKY)))


@pytest.mark.parametrize("row", H_ROWS, ids=_h_id)
def test_values_conv_h3(row):
    run_values_h3(row[0], row[2])


@pytest.mark.parametrize("row", H_ROWS, ids=_h_id)
def test_impulse_conv_h3(row):
    run_impulse_h3(row[0], row[2])
