"""GPU: what a NaN or an infinity that enters an entry point does to its outputs (include/phasegen.h, "Non-finite values").

Every call poisons ONE element of one input and is compared with the same call on the clean input (tests/_nonfinite.py):
  R1  an output the float64 restatement of the poisoned call makes non-finite is non-finite on the device (nothing is swallowed);
  R2  an output the restatement leaves exactly as it was has the bits of the clean call (nothing spreads), but for the exceptions
      the header names, which reach `check` as `allow` in the rows they concern and nowhere else.
Outputs start as a finite sentinel, the conv workspace as 0xff bytes, and after every poisoned call one clean call into the same
buffers, on the same workspace, returns the clean bits.  Every row prints a NONFINITE line (pytest -s): the size of the cone, of its
complement, and the violations.  tests/test_nonfinite_host.py shows on the CPU that the comparison has teeth and that every case's
cone is neither empty nor everything.

No call here is meant to fault: non-finite floats are ordinary data to these kernels.
Named test_z_* so that it is collected behind the older modules."""
import functools

import numpy as np
import pytest
import torch

import _conv_ref64 as cref
import _nonfinite as nf
import _signal_ref64 as sig
import _spectral_ref as spec
import _vocoder_ref as voc
from phasegen import detgen

pytestmark = pytest.mark.gpu
SENT = -77.0
F32 = np.float32


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _np(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _sent(shape, dtype=torch.float32):
    return torch.full(tuple(shape), SENT, device=_dev(), dtype=dtype)


def _poked(t, index, value):
    """a device copy of t with one element replaced"""
    out = t.clone()
    out[tuple(index)] = float(value)
    return out


class Failures:
    """collects the violations of a row, so that one run shows all of them"""

    def __init__(self):
        self.msgs = []
        self.followed, self.matched = 0, 0

    def check(self, *args, **kw):
        try:
            return nf.check(*args, **kw)
        except AssertionError as e:
            self.msgs.append(str(e))

    def same(self, what, a, b):
        self.followed += 1
        if nf.same_bits(a, b):
            self.matched += 1
        else:
            self.msgs.append(f"{what}: the clean call after the poisoned one differs in {int(np.sum(nf._bits(a) != nf._bits(b)))} elements")

    def done(self):
        if self.followed:
            print(f"NONFINITE clean calls into the same buffers after a poisoned one: {self.matched} of {self.followed} returned the clean bits")
        assert not self.msgs, f"{len(self.msgs)} violations:\n" + "\n".join(self.msgs[:40])


# =====================================================================================================================================
# conv
# =====================================================================================================================================
def _conv_tables():
    import test_z_conv_values_gpu as cv
    return cv


class _FilledWorkspace:
    def __enter__(self):
        from phasegen import ops
        self.ws = ops.conv_workspace(_dev())
        self.ws.fill_(0xFF)

    def __exit__(self, *exc):
        from phasegen import ops
        if exc[0] is None:
            assert ops.conv_workspace(_dev()).data_ptr() == self.ws.data_ptr()


def conv_allow(fam, op, geom, operand, index):
    """the exceptions of the header's section that apply to a row (None: none).  C1, zeros multiplied in: a weight in every family,
    an operand of every wgrad.  C2, zero-weight phantom taps: conv_t where the stride does not divide the taps."""
    tr, k, s = geom[0], geom[3], geom[4]
    if operand == "w" or (op == "wgrad" and operand in ("x", "dy")):
        return nf.conv_row_mates(op, geom, operand, index)
    if fam == "conv_t" and k % s and (op, operand, tr) in (("fwd", "x", True), ("dgrad", "dy", False)):
        return nf.conv_phantom_taps(op, geom, operand, index)
    return None


def _conv_variants(op):
    """(name, x_act, mask) of the calls of an op"""
    if op == "fwd":
        return [("y", cref.NONE, None), ("leaky(y(leaky x)), y2=relu", cref.LEAKY, None)]
    if op == "dgrad":
        return [("dx", cref.NONE, None), ("(dx+add)*leaky'(ref)", cref.NONE, cref.LEAKY), ("(dx+add)*relu'(ref)", cref.NONE, cref.RELU)]
    return [("dw(leaky x)", cref.LEAKY, None)]


def conv_refs(cv, geom, op, variant, prec, t):
    """{output name: float64 clean reference} of a variant"""
    name, x_act, mask = variant
    value, mag = cv.exact(geom, op, "white", x_act, prec == "bf16")
    if op == "fwd" and x_act == cref.LEAKY:
        return {"y": nf.act64(value, 1), "y2": nf.act64(value, 2)}
    if op == "dgrad" and mask is not None:
        return {"dx": cref.dgrad_epilogue64(value, mag, t["add"], t["refz"], mask)[0]}
    return {{"fwd": "y", "dgrad": "dx", "wgrad": "dw"}[op]: value}


def run_conv(case, prec):
    from phasegen import ops
    cv = _conv_tables()
    geom, op, sched, fam = case[:4]
    tr, Cin, Cout, k, s, p, Lin, B = geom
    kw = dict(transposed=tr, precision=prec, schedule=sched)
    t = cv.inputs(geom, "white")
    xs, ws, dys = cref.shapes(geom)
    clean = {"x": _to(t["x"]), "w": _to(t["w"]), "dy": _to(t["dy"]), "add": _to(t["add"]), "ref": _to(t["refz"])}
    out_shape = {"fwd": dys, "dgrad": xs, "wgrad": ws}[op]
    fails = Failures()

    def call(variant, T, outs=None):
        """one call of the variant on the operand set T into `outs` (fresh sentinel-filled tensors when None): {name: tensor}"""
        name, x_act, mask = variant
        if op == "fwd":
            if x_act == cref.NONE:
                outs = outs or {"y": _sent(out_shape)}
                ops.conv_fwd(T["x"], T["w"], outs["y"], s, p, **kw)
            else:
                outs = outs or {"y": _sent(out_shape), "y2": _sent(out_shape)}
                ops.conv_fwd(T["x"], T["w"], outs["y"], s, p, x_act=ops.ACT_LEAKY, y_act=ops.ACT_LEAKY, y2=outs["y2"], y2_act=ops.ACT_RELU, **kw)
        elif op == "dgrad":
            outs = outs or {"dx": _sent(out_shape)}
            if mask is None:
                ops.conv_dgrad(T["dy"], T["w"], outs["dx"], s, p, **kw)
            else:
                ops.conv_dgrad(T["dy"], T["w"], outs["dx"], s, p, add=T["add"], ref=T["ref"], mask=mask, **kw)
        else:
            outs = outs or {"dw": _sent(out_shape)}
            ops.conv_wgrad(T["x"], T["dy"], outs["dw"], s, p, x_act=ops.ACT_LEAKY, **kw)
        return outs

    if op == "wgrad":
        ops.conv_wgrad(clean["x"], clean["dy"], torch.empty(ws, device=_dev()), s, p, x_act=ops.ACT_LEAKY, **kw)       # (sizes the workspace)
    for variant in _conv_variants(op):
        refs = conv_refs(cv, geom, op, variant, prec, t)
        with _FilledWorkspace():
            got_clean = {n: _np(v) for n, v in call(variant, clean).items()}
        for operand in nf.conv_operands(op):
            if operand in ("add", "ref") and variant[2] is None:
                continue
            for site, index in nf.conv_sites(geom, operand).items():
                cone = nf.conv_cone(op, geom, operand, index)
                allow = conv_allow(fam, op, geom, operand, index)
                for vname, value in nf.VALUES:
                    T = dict(clean)
                    T[operand] = _poked(clean[operand], index, value)
                    with _FilledWorkspace():
                        outs = call(variant, T)
                    tag = f"{prec} {fam} {op} [{variant[0]}] {operand}{list(index)}({site})={vname}"
                    for n, ref_clean in refs.items():
                        if operand == "ref":          # a NaN in the mask source is a comparison that fails: act' = slope, nothing else
                            rz = nf.poison(t["refz"], index, value)
                            ref_p = cref.dgrad_epilogue64(*cv.exact(geom, op, "white", cref.NONE, prec == "bf16"), t["add"], rz, variant[2])[0]
                            assert np.isfinite(ref_p).all()
                        else:
                            ref_p = np.where(cone, np.nan, ref_clean)
                        fails.check(_np(outs[n]), got_clean[n], ref_p, ref_clean, allow=allow, tag=f"{tag} {n}")
                    if operand == "ref":              # ... shown as such: the bits of the same call with a finite value of that sign
                        T2 = dict(clean)
                        T2["ref"] = _poked(clean["ref"], index, 1.0 if value == nf.PINF else -1.0)
                        same = call(variant, T2)
                        fails.same(f"{tag}: against a finite mask source of the same sign", _np(outs["dx"]), _np(same["dx"]))
                    again = call(variant, clean, outs)             # same buffers, same workspace, nothing refilled
                    for n in refs:
                        fails.same(f"{tag} {n}", _np(again[n]), got_clean[n])
    fails.done()


def _conv_cases(families=None):
    cv = _conv_tables()
    return [pytest.param(c, id=cv.fixup_case_id(c)) for c in cv.CASES if families is None or c[3] in families]


def _bf16_families():
    from test_kernel_families import BF16_FAMILIES
    return BF16_FAMILIES


@pytest.mark.parametrize("case", _conv_cases())
def test_conv_fp32(case):
    run_conv(case, "fp32")


@pytest.mark.parametrize("case", _conv_cases(_bf16_families()))
def test_conv_bf16(case):
    run_conv(case, "bf16")


@pytest.mark.parametrize("case", _conv_cases(_bf16_families()))
def test_conv_bf16x3(case):
    run_conv(case, "bf16x3")


def _h_rows():
    cv = _conv_tables()
    return cv.H_ROWS, cv._h_id


@pytest.mark.parametrize("row", _h_rows()[0], ids=_h_rows()[1])
def test_conv_fwd_h(row):
    """pg_conv_fwd_h: the poisoned element enters through the device's own row cast (x) or shadow weights (w); the fp32 y and the
    bf16 copies yh = LeakyReLU, yh2 = ReLU are held to the same cone"""
    from phasegen import ops
    cv = _conv_tables()
    geom, epi, sched = row
    tr, Cin, Cout, k, s, p, Lin, B = geom
    t = cv.inputs(geom, "white")
    Lout = cref.out_len(tr, Lin, k, s, p)
    fails = Failures()
    for x_act, aname in ((cref.NONE, "y"), (cref.LEAKY, "y(leaky x)")):
        value, _ = cv.exact(geom, "fwd", "white", x_act, True)
        refs = {"y": value, "yh": nf.act64(value, 1), "yh2": nf.act64(value, 2)}

        def call(x, w, outs=None):
            dev = _dev()
            xh = ops.h_alloc(B, Cin, Lin, dev)
            ops.cast_rows_bf16(x, xh, act=x_act)
            wh = ops.shadow_weights(w, tr, s)
            outs = outs or {"y": _sent((B, Cout, Lout)), "yh": ops.h_alloc(B, Cout, Lout, dev), "yh2": ops.h_alloc(B, Cout, Lout, dev)}
            ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, transposed=tr, y=outs["y"], yh=outs["yh"], yh_act=ops.ACT_LEAKY,
                           yh2=outs["yh2"], yh2_act=ops.ACT_RELU, schedule=sched)
            return outs

        view = lambda o: {"y": _np(o["y"]), "yh": _np(o["yh"])[:, :, :Lout], "yh2": _np(o["yh2"])[:, :, :Lout]}
        xd, wd = _to(t["x"]), _to(t["w"])
        with _FilledWorkspace():
            outs0 = call(xd, wd)
        got_clean = view(outs0)
        for operand in ("x", "w"):
            for site, index in nf.conv_sites(geom, operand).items():
                cone = nf.conv_cone("fwd", geom, operand, index)
                allow = conv_h_allow(geom, operand, index)
                for vname, v in nf.VALUES:
                    with _FilledWorkspace():
                        outs = call(_poked(xd, index, v) if operand == "x" else xd, _poked(wd, index, v) if operand == "w" else wd)
                    got = view(outs)
                    tag = f"bf16-resident conv_h3 {_h_rows()[1](row)} [{aname}] {operand}{list(index)}({site})={vname}"
                    for n in refs:
                        fails.check(got[n], got_clean[n], np.where(cone, np.nan, refs[n]), refs[n], allow=allow, tag=f"{tag} {n}")
                    assert not _np(outs["yh"])[:, :, Lout:].any() and not _np(outs["yh2"])[:, :, Lout:].any(), f"{tag}: the zero tails of the bf16 rows"
                    again = view(call(xd, wd, outs))
                    for n in refs:
                        fails.same(f"{tag} {n}", again[n], got_clean[n])
    fails.done()


def conv_h_allow(geom, operand, index):
    """header exception C1 for a weight (as above); conv_h3 needed none for x on these rows"""
    return nf.conv_row_mates("fwd", geom, operand, index) if operand == "w" else None


# =====================================================================================================================================
# BatchNorm, per-clip BatchNorm
# =====================================================================================================================================
NORM_SHAPES = [(5, 6, 61), (3, 4, 6000), (3, 24, 128)]
EPS, MOM = 1e-5, 0.1


@functools.lru_cache(maxsize=None)
def norm_inputs(shape):
    B, C, L = shape
    x = (detgen.normal(901, shape) * F32(1.5) + F32(0.3)).astype(F32)
    dy = detgen.normal(902, shape)
    gamma = (detgen.uniform(903, (C,), 0.5, 1.5) * np.where(np.arange(C) % 3 == 2, F32(-1), F32(1))).astype(F32)
    beta = detgen.uniform(904, (C,), -0.5, 0.5)
    rm0, rv0 = detgen.uniform(905, (C,), -0.5, 0.5), detgen.uniform(906, (C,), 0.5, 1.5)
    return x, dy, gamma, beta, rm0, rv0


def norm_sites(shape):
    B, C, L = shape
    return {"first": (0, 0, 0), "interior": (B // 2, C // 2, L // 2), "last": (B - 1, C - 1, L - 1)}


ACTS = {"y": 0, "y2": 1, "yh": 2, "yh2": 0}


def _norm_call(per_clip, shape, xd, gd, bd, rm0, rv0, four):
    """pg_bn_fwd / pg_clipnorm_fwd into fresh sentinel-filled outputs: {name: numpy}"""
    from phasegen import ops
    B, C, L = shape
    y = _sent(shape)
    stat = (B, C) if per_clip else (C,)
    sm, si = _sent(stat), _sent(stat)
    rm, rv = _to(rm0), _to(rv0)
    extra, outs = {}, {}
    if four:
        y2, yh, yh2 = _sent(shape), ops.h_alloc(B, C, L, _dev()), ops.h_alloc(B, C, L, _dev())
        extra = dict(y2=y2, y2_act=ACTS["y2"], yh=yh, yh_act=ACTS["yh"], yh2=yh2, yh2_act=ACTS["yh2"])
    fn = ops.clipnorm_fwd if per_clip else ops.bn_fwd
    fn(xd, y, gd, bd, sm, si, rm, rv, eps=EPS, momentum=MOM, y_act=ACTS["y"], **extra)
    outs = {"y": _np(y), "save_mean": _np(sm), "save_invstd": _np(si), "running_mean": _np(rm), "running_var": _np(rv)}
    if four:
        outs.update(y2=_np(y2), yh=_np(yh)[:, :, :L], yh2=_np(yh2)[:, :, :L])
        assert not _np(yh)[:, :, L:].any() and not _np(yh2)[:, :, L:].any()
    return outs


def _norm_refs(per_clip, x, gamma, beta, rm0, rv0, four):
    r = nf.bn_fwd64(x, gamma, beta, rm0, rv0, EPS, MOM, per_clip=per_clip)
    if four:
        r.update({n: nf.act64(r["y"], ACTS[n]) for n in ("y2", "yh", "yh2")})
    return r


@pytest.mark.parametrize("per_clip", [False, True], ids=["bn_fwd", "clipnorm_fwd"])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_norm_fwd(shape, per_clip):
    """the poisoned channel (clipnorm: the poisoned row, and its channel's running buffers) is non-finite everywhere -- y and its
    copies, save_mean, save_invstd, running_mean, running_var --, every other one has the clean bits"""
    x, dy, gamma, beta, rm0, rv0 = norm_inputs(shape)
    four = shape == NORM_SHAPES[2]
    gd, bd = _to(gamma), _to(beta)
    xd = _to(x)
    clean = _norm_call(per_clip, shape, xd, gd, bd, rm0, rv0, four)
    ref_clean = _norm_refs(per_clip, x, gamma, beta, rm0, rv0, four)
    fails = Failures()
    for site, index in norm_sites(shape).items():
        for vname, v in nf.VALUES:
            got = _norm_call(per_clip, shape, _poked(xd, index, v), gd, bd, rm0, rv0, four)
            ref_p = _norm_refs(per_clip, nf.poison(x, index, v), gamma, beta, rm0, rv0, four)
            b, c, _ = index
            for n in clean:
                hit = ref_p[n][b, c] if per_clip and ref_p[n].shape[:2] == shape[:2] else ref_p[n][:, c] if ref_p[n].ndim == 3 else ref_p[n][c]
                assert not np.isfinite(hit).any(), (n, index)                   # the whole channel (clipnorm: row), by the formula
                fails.check(got[n], clean[n], ref_p[n], ref_clean[n], tag=f"{'clipnorm' if per_clip else 'bn'}_fwd {shape} x{list(index)}({site})={vname} {n}")
            again = _norm_call(per_clip, shape, xd, gd, bd, rm0, rv0, four)
            for n in clean:
                fails.same(f"norm fwd {shape} {site} {vname} {n}", again[n], clean[n])
    fails.done()


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_bn_bwd(shape):
    """pg_bn_bwd on the clean forward's saved statistics.  A poisoned dy takes dgamma, dbeta and dx of its channel; a poisoned x takes
    dgamma and dx, and dbeta = sum dy keeps its clean bits."""
    from phasegen import ops
    B, C, L = shape
    x, dy, gamma, beta, rm0, rv0 = norm_inputs(shape)
    xd, dyd, gd = _to(x), _to(dy), _to(gamma)
    sm, si = _sent((C,)), _sent((C,))
    ops.bn_fwd(xd, _sent(shape), gd, _to(beta), sm, si, eps=EPS, momentum=MOM)
    smh, sih = _np(sm), _np(si)

    def call(xt, dyt):
        dx, dg, db = _sent(shape), _sent((C,)), _sent((C,))
        ops.bn_bwd(xt, dyt, dx, gd, sm, si, dg, db)
        return {"dx": _np(dx), "dgamma": _np(dg), "dbeta": _np(db)}

    clean = call(xd, dyd)
    ref_clean = nf.bn_bwd64(x, dy, gamma, smh, sih)
    fails = Failures()
    for operand in ("x", "dy"):
        for site, index in norm_sites(shape).items():
            for vname, v in nf.VALUES:
                got = call(_poked(xd, index, v) if operand == "x" else xd, _poked(dyd, index, v) if operand == "dy" else dyd)
                ref_p = nf.bn_bwd64(nf.poison(x, index, v) if operand == "x" else x, nf.poison(dy, index, v) if operand == "dy" else dy, gamma, smh, sih)
                for n in clean:
                    fails.check(got[n], clean[n], ref_p[n], ref_clean[n], tag=f"bn_bwd {shape} {operand}{list(index)}({site})={vname} {n}")
                again = call(xd, dyd)
                for n in clean:
                    fails.same(f"bn_bwd {shape} {operand} {site} {vname} {n}", again[n], clean[n])
    fails.done()


# =====================================================================================================================================
# pointwise
# =====================================================================================================================================
LOSS_SHAPES = [(2, 3, 5), (2, 40, 251)]


@functools.lru_cache(maxsize=None)
def loss_inputs(shape):
    B, C, L = shape
    n = B * C * L
    ph = (detgen.normal(911, (n,)) * 4.0).astype(F32)
    mh = detgen.normal(912, (n,)) * F32(1.5)
    m = np.abs(detgen.normal(913, (n,))).astype(F32) * F32(2.0)
    th = -detgen.uniform(914, (n,), -3.1415925, 3.1415925)
    pred = np.concatenate([ph.reshape(B, C, L), mh.reshape(B, C, L)], axis=1)
    batch = np.stack([m.reshape(B, C, L), th.reshape(B, C, L)], axis=1)
    return np.ascontiguousarray(pred, F32), np.ascontiguousarray(batch, F32)


def loss_sites(shape):
    """{name: (tensor, index)}: one element each of the phase half, the magnitude half, the target angle, the target log-magnitude"""
    B, C, L = shape
    return {"phase": ("pred", (B - 1, C - 1, L - 1)), "magnitude": ("pred", (0, C + C // 2, L // 2)),
            "target angle": ("batch", (B - 1, 1, C // 2, L // 2)), "target logmag": ("batch", (0, 0, 0, 0))}


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "B%d-C%d-L%d" % s)
def test_loss(shape):
    """which of [loss, angle loss, magnitude loss] and which element of dpred go non-finite follows the float64 formula: a poisoned
    phase or target angle takes losses 0 and 1 and one phase gradient, a poisoned magnitude or target log-magnitude losses 0 and 2 and
    one magnitude gradient; the third loss and every other gradient keep the clean bits"""
    from phasegen import ops
    pred, batch = loss_inputs(shape)
    pd, bd = _to(pred), _to(batch)

    def call(p, b):
        dpred = _sent(pred.shape)
        losses = _sent((3,))
        ops.loss_fwd_bwd(p, b, dpred, losses=losses)
        return {"losses": _np(losses), "dpred": _np(dpred)}

    clean = call(pd, bd)
    rl, rd = nf.loss64(pred, batch)
    fails = Failures()
    for site, (which, index) in loss_sites(shape).items():
        for vname, v in nf.VALUES:
            got = call(_poked(pd, index, v) if which == "pred" else pd, _poked(bd, index, v) if which == "batch" else bd)
            pl, pdp = nf.loss64(nf.poison(pred, index, v) if which == "pred" else pred, nf.poison(batch, index, v) if which == "batch" else batch)
            assert int((~np.isfinite(pl)).sum()) == 2 and int((~np.isfinite(pdp)).sum()) == 1
            fails.check(got["losses"], clean["losses"], pl, rl, tag=f"loss {shape} {site}={vname} losses")
            fails.check(got["dpred"], clean["dpred"], pdp, rd, tag=f"loss {shape} {site}={vname} dpred")
            again = call(pd, bd)
            fails.same(f"loss {shape} {site} {vname}", again["losses"], clean["losses"])
            fails.same(f"loss {shape} {site} {vname}", again["dpred"], clean["dpred"])
    fails.done()


ADAM_N = 4 * 256 * 3 + 3            # several workgroups of either kernel, and both tails


@functools.lru_cache(maxsize=None)
def adam_inputs():
    n = ADAM_N
    return (detgen.uniform(921, (n,), -0.1, 0.1), detgen.uniform(922, (n,), -1e-2, 1e-2), detgen.uniform(923, (n,), -1e-2, 1e-2),
            detgen.uniform(924, (n,), 1e-6, 2e-4))


ADAM_SITES = {"first": 0, "interior": 1027, "last": ADAM_N - 1}


@pytest.mark.parametrize("thin", [False, True], ids=["adam_kernel", "adam_thin_kernel"])
def test_adam(thin):
    """a poisoned g, m, v or p changes the class of that element's p / m / v as the float64 update says; every other element keeps
    the clean bits"""
    from phasegen import ops
    arrays = dict(zip("pgmv", adam_inputs()))

    def call(T):
        d = {k: _to(a) for k, a in T.items()}
        ops.adam_step(d["p"], d["g"], d["m"], d["v"], 7, thin=thin)
        return {k: _np(d[k]) for k in "pmv"}

    clean = call(arrays)
    ref_clean = dict(zip("pmv", nf.adam64(arrays["p"], arrays["g"], arrays["m"], arrays["v"], 7)))
    fails = Failures()
    for operand in "gmvp":
        for site, i in ADAM_SITES.items():
            for vname, v in nf.VALUES:
                T = dict(arrays)
                T[operand] = nf.poison(arrays[operand], i, v)
                got = call(T)
                ref_p = dict(zip("pmv", nf.adam64(T["p"], T["g"], T["m"], T["v"], 7)))
                for n in "pmv":
                    fails.check(got[n], clean[n], ref_p[n], ref_clean[n], tag=f"adam thin={thin} {operand}[{i}]({site})={vname} {n}")
    fails.done()


CAST_SPECIALS = np.array([0x7fffffff, 0xffffffff, 0x7f800001, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff], np.uint32).view(F32)


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "leaky", "relu"])
def test_cast_rows_bf16(act):
    """NaN payloads 0x7fffffff, 0xffffffff, 0x7f800001 stay NaN (the last one must not round to an infinity), infinities stay
    infinities, +-FLT_MAX round to +-inf as round-to-nearest-even says -- each after the activation x >= 0 ? x : slope x in fp32
    (relu: -inf -> NaN = 0 * -inf, -FLT_MAX -> -0) -- and every other element keeps the bits of the clean call"""
    from phasegen import ops
    B, C, L = 2, 3, 21
    x = detgen.normal(931, (B, C, L))
    where = [(0, 0, 0), (0, 1, 7), (0, 2, 20), (1, 0, 3), (1, 1, 10), (1, 2, 19), (1, 2, 20)]
    xp = x.copy()
    for idx, v in zip(where, CAST_SPECIALS):
        xp[idx] = v

    def call(a):
        out = ops.h_alloc(B, C, L, _dev())
        ops.cast_rows_bf16(_to(a), out, act=act)
        return _np(out)

    clean, got = call(x), call(xp)
    slope = {0: 1.0, 1: 0.2, 2: 0.0}[act]
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.where(xp >= 0, xp, F32(slope) * xp).astype(F32)
    want = cref.bf16(np.where(np.isnan(want), F32(0), want))                 # RNE of the non-NaN values: FLT_MAX -> inf
    nan = np.isnan(np.where(xp >= 0, xp, F32(slope) * xp))
    hit = np.zeros(x.shape, bool)
    for idx in where:
        hit[idx] = True
        print(f"NONFINITE cast_rows_bf16 act={act} x={xp[idx]!r} ({int(xp.view(np.uint32)[idx]):#010x}) -> {got[idx]!r}")
    assert np.array_equal(np.isnan(got[:, :, :L]), nan), "a NaN stays a NaN and nothing else becomes one"
    assert np.array_equal(got[:, :, :L][~nan], want[~nan]), "infinities stay, FLT_MAX rounds to inf"
    assert int(np.isinf(got[:, :, :L]).sum()) == {0: 4, 1: 3, 2: 2}[act]          # leaky: -FLT_MAX / 5 is finite; relu: the negatives are gone
    assert nf.same_bits(got[:, :, :L][~hit], clean[:, :, :L][~hit]) and not got[:, :, L:].any()


@pytest.mark.parametrize("n", [5, 3 * 1024 + 7])
def test_moments_and_standardize(n):
    """pg_moments / pg_standardize: mean and std over the whole array, so the statistics and every element are non-finite"""
    from phasegen import ops
    x = detgen.normal(941, (n,))
    for site, i in (("first", 0), ("interior", n // 2), ("last", n - 1)):
        for vname, v in nf.VALUES:
            xd = _to(nf.poison(x, i, v))
            st = ops.moments(xd).cpu().numpy()
            ops.standardize_(xd)
            got = _np(xd)
            print(f"NONFINITE moments/standardize n={n} x[{i}]({site})={vname}: stats {st}, finite elements {int(np.isfinite(got).sum())} of {n}")
            assert not np.isfinite(st).any() and not np.isfinite(got).any()
    xd = _to(x)
    st = ops.standardize_(xd).cpu().numpy()
    assert np.isfinite(st).all() and np.isfinite(_np(xd)).all()               # the workspace keeps nothing of the poisoned calls


# =====================================================================================================================================
# signal: polar, STFT, ISTFT, Griffin-Lim blocks
# =====================================================================================================================================
@pytest.mark.parametrize("use_exp", [True, False], ids=["log1p", "abs"])
def test_polar_cells(use_exp):
    """pg_polar on (NaN, 1), (1, NaN), (+-inf, 1), (1, +-inf), (inf, inf) among noise: both planes against np.abs / np.log1p /
    np.angle of re + 1j * im as data.py:40 forms it.  A NaN part makes both planes NaN; an infinite real part an infinite magnitude
    and the angle of its axis (0, pi); an infinite imaginary part makes the real part NaN on its way (1j * inf), so both planes."""
    from phasegen import ops
    d = detgen.normal(951, (2, 2, 5, 7))
    where = [(0, 0, 0), (0, 2, 3), (0, 4, 6), (1, 0, 1), (1, 1, 1), (1, 3, 5), (1, 4, 6)]
    dp = d.copy()
    for (n, b, f), (re, im) in zip(where, nf.POLAR_CELLS):
        dp[n, 0, b, f], dp[n, 1, b, f] = re, im
    clean, got = _np(ops.polar(_to(d), out=_sent(d.shape), use_exp=use_exp)), _np(ops.polar(_to(dp), out=_sent(d.shape), use_exp=use_exp))
    ref_c, ref_p = np.stack(nf.polar64(d[:, 0], d[:, 1], use_exp), 1), np.stack(nf.polar64(dp[:, 0], dp[:, 1], use_exp), 1)
    n = nf.check(got, clean, ref_p, ref_c, tag=f"polar use_exp={use_exp}")
    assert n["cone"] == 7 + 5                     # seven magnitudes; the angles of the NaN cells and of the cells with an infinite im
    for (s, b, f), (re, im) in zip(where, nf.POLAR_CELLS):
        ang, want = float(got[s, 1, b, f]), float(ref_p[s, 1, b, f])
        print(f"NONFINITE polar cell ({re}, {im}): magnitude {got[s, 0, b, f]}, angle {ang} (np.angle {want})")
        if np.isfinite(want):
            assert abs(ang - want) <= 3e-7
    again = _np(ops.polar(_to(d), out=_sent(d.shape), use_exp=use_exp))
    assert nf.same_bits(again, clean)


# (id, n_fft, hop, frames, single_frame): one per kernel family of tests/test_z_signal_values_gpu.py's table; two signals each
STFT_ROWS = [("w16", 2048, 512, 9, 0), ("w8", 1024, 256, 9, 0), ("f4", 128, 32, 8, 0), ("r2", 4096, 1024, 9, 0), ("r2-single", 64, 16, 8, 1)]
CHUNK_STARTS = (3, 8)


def stft_refs(y, n_fft, hop, polar, stats=None):
    """float64 (signals, 2, bins, frames) of the clean input"""
    X = sig.stft64(y, n_fft, hop)
    if stats:
        X = (X - stats[0]) / stats[1]
    return np.stack(nf.polar64(X[:, 0], X[:, 1]), 1) if polar else X


def stft_poisoned_ref(ref_clean, signal, n, n_fft, hop, sample, nan, polar):
    """the reference of the input with one poisoned sample in `signal` (tests/_nonfinite.stft_poisoned)"""
    out = ref_clean.copy()
    out[signal] = nf.stft_poisoned(ref_clean[signal], n, n_fft, hop, sample, nan, polar)
    return out


@pytest.mark.parametrize("row", STFT_ROWS, ids=[r[0] for r in STFT_ROWS])
def test_stft(row):
    """one poisoned sample -- the first, one that exactly two frames hold, the last -- changes the frames that hold it, every bin of
    them, and no other; plain, fused polar, and both again reading chunks in place"""
    from phasegen import ops
    import test_z_signal_values_gpu as sv
    id, n_fft, hop, frames, single = row
    n = hop * (frames - 1)
    y = sig.white(961, 2, n)
    shape = (2, 2, n_fft // 2, frames)
    kernel = sv.fcase(id, n_fft, hop, frames, single=single).kernel
    src = sig.white(962, 2, n + 64)
    gathered = np.stack([src[i, s:s + n] for i, s in enumerate(CHUNK_STARTS)])
    ckw = dict(chunk_len=n, chunk_start=torch.tensor(CHUNK_STARTS, dtype=torch.int64, device="cuda"),
               chunk_row=torch.tensor([0, 1], dtype=torch.int32, device="cuda"))
    fails = Failures()
    for chunked in (False, True):
        host, flat = (src, gathered) if chunked else (y, y)
        kw = dict(single_frame=single, **(ckw if chunked else {}))
        hd = _to(host)
        assert sv.describe_fields(ops.stft_describe(hd, n_fft, hop, **kw))[0] == kernel.format("true" if chunked else "false")
        for polar in (False, True):
            clean = _np(ops.stft(hd, n_fft, hop, polar=polar, out=_sent(shape), **kw))
            ref_c = stft_refs(flat, n_fft, hop, polar)
            for site, i in nf.stft_sites(n, n_fft, hop).items():
                for vname, v in nf.VALUES:
                    at = (1, CHUNK_STARTS[1] + i) if chunked else (1, i)
                    out = _sent(shape)
                    got = _np(ops.stft(_poked(hd, at, v), n_fft, hop, polar=polar, out=out, **kw))
                    ref_p = stft_poisoned_ref(ref_c, 1, n, n_fft, hop, i, vname == "nan", polar)
                    tag = f"stft {id}{' chunked' if chunked else ''}{' polar' if polar else ''} sample {i}({site})={vname}"
                    fails.check(got, clean, ref_p, ref_c, tag=tag)
                    fails.same(tag, _np(ops.stft(hd, n_fft, hop, polar=polar, out=out, **kw)), clean)
    fails.done()


# (id, n_fft, hop, crop_len, single_frame)
CROP_ROWS = [("crops-r2", 64, 16, 128, 1), ("crops-f4", 64, 16, 136, 0), ("crops-w8", 1024, 256, 2304, 0), ("crops-w16", 2048, 512, 4608, 0)]
CROP_STATS = (0.0123, 1.7)


@pytest.mark.parametrize("row", CROP_ROWS, ids=[r[0] for r in CROP_ROWS])
def test_stft_crops(row):
    """pg_stft_crops, with and without statistics and the polar epilogue: three disjoint crops of one buffer, a poisoned sample in the
    middle one (its first sample, one that two frames hold, its last) changes that crop's covering frames alone"""
    from phasegen import ops
    id, n_fft, hop, crop_len, single = row
    frames = 1 + crop_len // hop
    buf = sig.white(963, 1, 3 * crop_len + 11)[0]
    begin = np.array([0, crop_len + 5, 2 * crop_len + 9], np.int64)
    end = np.full(3, len(buf), np.int64)
    gathered = np.stack([buf[b:b + crop_len] for b in begin])
    bd, ed = _to(begin), _to(end)
    shape = (3, 2, n_fft // 2, frames)
    fails = Failures()
    for stats in (None, CROP_STATS):
        for polar in (False, True):
            run = lambda src, out: _np(ops.stft_crops(src, bd, ed, crop_len, n_fft, hop, polar=polar, stats=stats, out=out, single_frame=single))
            clean = run(_to(buf), _sent(shape))
            ref_c = stft_refs(gathered, n_fft, hop, polar, stats)
            for site, i in nf.stft_sites(crop_len, n_fft, hop).items():
                for vname, v in nf.VALUES:
                    out = _sent(shape)
                    got = run(_poked(_to(buf), (int(begin[1]) + i,), v), out)
                    ref_p = stft_poisoned_ref(ref_c, 1, crop_len, n_fft, hop, i, vname == "nan", polar)
                    tag = f"stft_crops {id} stats={stats is not None} polar={polar} sample {i}({site})={vname}"
                    fails.check(got, clean, ref_p, ref_c, tag=tag)
                    fails.same(tag, run(_to(buf), out), clean)
    fails.done()


# (id, bins, hop, frames): the generic frames + overlap-add kernels, the fused overlap-add of both wave widths with seams, radix-2
ISTFT_ROWS = [("f4", 16, 8, 8), ("f4-hop50", 64, 50, 7), ("w8", 512, 256, 12), ("w16", 1024, 512, 12), ("r2", 2048, 1024, 9)]


@functools.lru_cache(maxsize=None)
def istft_inputs(bins, frames, mode):
    shape = (2, bins, frames)
    if mode == 1:
        return detgen.normal(971, shape), detgen.normal(972, shape)
    return np.abs(detgen.normal(973, shape)), detgen.uniform(974, shape, -3.1415, 3.1415)


def istft_values(mode, plane):
    """-inf in the log-magnitude plane of mode 0 is the finite magnitude expm1(-inf) = -1: no cone, left out"""
    return [(n, v) for n, v in nf.VALUES if not (mode == 0 and plane == 0 and n == "-inf")]


@pytest.mark.parametrize("mode", [0, 1], ids=["logmag-phase", "re-im"])
@pytest.mark.parametrize("row", ISTFT_ROWS, ids=[r[0] for r in ISTFT_ROWS])
def test_istft(row, mode):
    """one poisoned cell of either plane (signal 1, an interior frame and the last one): without normalisation exactly the samples
    that frame overlaps change; with it the peak is a NaN (or an infinity) and R1 holds against y / max|y| -- a NaN peak takes the
    whole signal with it -- while the other signal keeps its bits"""
    from phasegen import ops
    id, bins, hop, frames = row
    N = 2 * bins
    length = hop * (frames - 1)
    a, b = istft_inputs(bins, frames, mode)
    ad, bd = _to(a), _to(b)
    fails = Failures()
    for single in ((0, 1) if id == "f4" else (0,)):
        run = lambda at, bt, norm, out: _np(ops.istft(at, bt, hop, mode=mode, normalize=norm, single_frame=single, out=out))
        clean, clean_n = run(ad, bd, False, _sent((2, length))), run(ad, bd, True, _sent((2, length)))
        ref_c = sig.istft64(a, b, hop, mode)[0]
        ref_cn = ref_c / np.abs(ref_c).max(axis=1, keepdims=True)
        for plane in (0, 1):
            for frame in (frames // 2, frames - 1):
                index = (1, 3, frame)
                for vname, v in istft_values(mode, plane):
                    ap, bp = (nf.poison(a, index, v), b) if plane == 0 else (a, nf.poison(b, index, v))
                    adp, bdp = (_poked(ad, index, v), bd) if plane == 0 else (ad, _poked(bd, index, v))
                    ref_p = np.stack([ref_c[0], nf.istft_poisoned(ref_c[1], N, hop, frame, index[1], plane, mode)])
                    tag = f"istft {id} mode {mode} single_frame={single} plane {plane} frame {frame}={vname}"
                    out = _sent((2, length))
                    fails.check(run(adp, bdp, False, out), clean, ref_p, ref_c, tag=tag)
                    fails.same(tag, run(ad, bd, False, out), clean)
                    ref_pn = nf.normalised(ref_p, vname == "nan")
                    got_n = run(adp, bdp, True, out)
                    assert not np.isfinite(got_n).all(), tag
                    fails.check(got_n, clean_n, ref_pn, ref_cn, tag=tag + " normalised")
                    fails.same(tag + " normalised", run(ad, bd, True, out), clean_n)
    fails.done()


GL_CASES = [(3, 7, 3), (17, 33, 2)]                     # (bins, frames, clips) of tests/test_z_gl_blocks_gpu.py


@pytest.mark.parametrize("case", GL_CASES, ids=lambda c: "bins%d-frames%d-n%d" % c)
def test_gl_project(case):
    """new_spec = mag exp(j angle(S)): a poisoned part of S or a poisoned magnitude takes that cell's (re, im) -- in spec_out and in
    the rows of the GEMM operand x that hold them -- and nothing else.  An infinite part of S against a finite one is the finite
    angle of its axis in float64; the device may answer NaN there (inf / inf), which is held to neither rule."""
    from phasegen import ops
    import test_z_gl_blocks_gpu as gl
    bins, frames, clips = case
    S, mag = detgen.normal(981, (clips, 2, bins, frames)), (np.abs(detgen.normal(982, (clips, bins, frames))) + F32(0.1)).astype(F32)

    def call(Sd, md):
        x, so = _sent((clips, 2 * bins - 2, frames)), _sent((clips, 2, bins, frames))
        ops.gl_project(Sd, md, x, so)
        xa, sa = _np(x), _np(so)
        assert nf.same_bits(xa[:, :bins], sa[:, 0]) and nf.same_bits(xa[:, bins:], sa[:, 1, 1:bins - 1])
        return sa

    def ref(S_, m_):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.stack(gl._project_ref(S_, m_), 1)

    Sd, md = _to(S), _to(mag)
    clean, ref_c = call(Sd, md), ref(S, mag)
    fails = Failures()
    cell = (clips - 1, bins // 2, frames - 1)
    for operand, index in (("S.re", (cell[0], 0) + cell[1:]), ("S.im", (cell[0], 1) + cell[1:]), ("mag", cell)):
        for vname, v in nf.VALUES:
            Sp, mp = (S, nf.poison(mag, index, v)) if operand == "mag" else (nf.poison(S, index, v), mag)
            ref_p = ref(Sp, mp)
            if operand != "mag" and vname != "nan":                     # finite in float64 (cos, sin of an axis angle): "changed"
                ref_p = np.where(np.isfinite(ref_p) & (ref_p != ref_c), 1e9, ref_p)
            got = call(_to(Sp), _to(mp))
            fails.check(got, clean, ref_p, ref_c, tag=f"gl_project {case} {operand}{list(index)}={vname}")
    fails.done()


OLA_CASES = [(16, 5, 11, 3), (30, 7, 9, 2), (64, 16, 7, 64)]        # (n_fft, hop, frames, clips) of tests/test_z_gl_blocks_gpu.py


@pytest.mark.parametrize("case", OLA_CASES, ids=lambda c: "nfft%d-hop%d-frames%d-n%d" % c)
def test_ola_nt(case):
    """one poisoned tap of one frame of the last clip: un-normalised, the one sample it is added into (none where the trim drops it);
    normalised, R1 against y / max|y| of that clip (a NaN peak takes the clip) and the other clips keep their bits"""
    from phasegen import ops
    import test_z_gl_blocks_gpu as gl
    N, hop, frames, clips = case
    length = hop * (frames - 1)
    fr = detgen.normal(991, (clips, N, frames))
    frd = _to(fr)
    run = lambda f, norm, out: _np(ops.ola_nt(f, hop, out, normalize=norm))
    clean, clean_n = run(frd, False, _sent((clips, length))), run(frd, True, _sent((clips, length)))
    ref_c = gl._ola_ref(fr, hop)[0]
    ref_cn = ref_c / np.abs(ref_c).max(axis=1, keepdims=True)
    fails = Failures()
    for site, index in (("interior", (clips - 1, N // 2 + 1, frames // 2)), ("last", (clips - 1, N // 2 - 1, frames - 1))):
        for vname, v in nf.VALUES:
            with np.errstate(invalid="ignore"):
                ref_p = gl._ola_ref(nf.poison(fr, index, v), hop)[0]
            assert int((~np.isfinite(ref_p)).sum()) == 1
            ref_p = np.where(np.isfinite(ref_p), ref_p, np.nan)
            ref_pn = nf.normalised(ref_p, vname == "nan")
            out = _sent((clips, length))
            tag = f"ola_nt {case} fr{list(index)}({site})={vname}"
            fails.check(run(_poked(frd, index, v), False, out), clean, ref_p, ref_c, tag=tag)
            fails.same(tag, run(frd, False, out), clean)
            fails.check(run(_poked(frd, index, v), True, out), clean_n, ref_pn, ref_cn, tag=tag + " normalised")
            fails.same(tag + " normalised", run(frd, True, out), clean_n)
    fails.done()


# =====================================================================================================================================
# resample, spec_clips, phase_vocoder
# =====================================================================================================================================
@pytest.mark.parametrize("up,down", [(160, 441), (1000, 3101)], ids=["160-441", "1000-3101"])
def test_resample(up, down):
    """three signals over three workgroup tiles; one poisoned sample of the middle signal -- the first, the last, the one at the edge
    of the first tile -- reaches the outputs whose taps hold it (the float64 direct sum of tests/test_resample_gpu.py) and no other"""
    from phasegen import ops
    import test_resample_gpu as rs
    tile = rs.TILE[(up, down)]
    edge = tile * down // up
    n_in = 2 * edge + 1
    n_out = rs.out_len(n_in, up, down)
    x = sig.white(1001, 3, n_in)
    b64 = rs.bank64(up, down, 0)
    run = lambda xd, out: _np(ops.resample(xd, down, up, res_type="kaiser_best", out=out))
    xd = _to(x)
    clean = run(xd, _sent((3, n_out)))
    ref_c = np.stack([rs.direct64(x[s], up, down, 0, bank=b64) for s in range(3)])
    fails = Failures()
    for site, i in (("first", 0), ("tile edge", edge), ("last", n_in - 1)):
        for vname, v in nf.VALUES:
            with np.errstate(invalid="ignore"):
                ref_p = ref_c.copy()
                ref_p[1] = rs.direct64(nf.poison(x[1], i, v), up, down, 0, bank=b64)
            assert nf.cone_is_a_proper_part(ref_p, ref_c)
            out = _sent((3, n_out))
            tag = f"resample {up}/{down} x[1, {i}]({site})={vname}"
            fails.check(run(_poked(xd, (1, i), v), out), clean, ref_p, ref_c, tag=tag)
            fails.same(tag, run(xd, out), clean)
    fails.done()


@pytest.mark.parametrize("src_per_out", [1.0, 1 / 1.5], ids=["1.0", "1/1.5"])
def test_spec_clips(src_per_out):
    """a poisoned source frame reaches the output frames that read it -- as the first neighbour, or as the second with a weight that
    is not zero -- in every clip that holds them"""
    from phasegen import ops
    n_ch, bins, F_src, n_clips, frames, sf = 2, 5, 40, 3, 12, 8
    P = detgen.normal(1011, (n_ch, bins, F_src))
    shape = (n_clips, n_ch, bins, frames)
    run = lambda Pd, out: _np(ops.spec_clips(Pd, n_clips, frames, sf, src_per_out, out=out))
    Pd = _to(P)
    clean = run(Pd, _sent(shape))
    ref_c = spec.spec_clips(P, n_clips, frames, sf, src_per_out)
    last = int(np.floor((2 * sf + frames - 1) * src_per_out))
    fails = Failures()
    for site, f in (("first", 0), ("interior", 10), ("last read", last)):
        for vname, v in nf.VALUES:
            with np.errstate(invalid="ignore"):
                ref_p = spec.spec_clips(nf.poison(P, (1, 2, f), v), n_clips, frames, sf, src_per_out)
            assert nf.cone_is_a_proper_part(ref_p, ref_c)
            out = _sent(shape)
            tag = f"spec_clips src_per_out={src_per_out:.3f} P[1, 2, {f}]({site})={vname}"
            fails.check(run(_poked(Pd, (1, 2, f), v), out), clean, ref_p, ref_c, tag=tag)
            fails.same(tag, run(Pd, out), clean)
    fails.done()


@pytest.mark.parametrize("src_per_out", [1.0, 1 / 1.5], ids=["1.0", "1/1.5"])
def test_phase_vocoder_follows_its_own_rule(src_per_out):
    """pg_phase_vocoder states its own rule (include/phasegen.h): an angle that is not finite counts as 0, a NaN in M does not reset
    (M < floor is false), -inf does, +inf does not.  So a poisoned call is still pinned BIT FOR BIT by the contract's restatement
    (tests/_vocoder_ref.py), output finite everywhere."""
    from phasegen import ops
    n_ch, bins, F_src = 2, 6, 30
    F_out = int((F_src - 1) / src_per_out)
    A = detgen.uniform(1021, (n_ch, bins, F_src), -3.1415, 3.1415)
    M = np.abs(detgen.normal(1022, (n_ch, bins, F_src))).astype(F32)
    floor = 0.5
    assert 0.2 < float(np.mean(M < floor)) < 0.8
    for plane in ("angle", "logmag"):
        for f in (0, F_src // 2, int(np.floor((F_out - 1) * src_per_out))):
            for vname, v in nf.VALUES:
                Ap, Mp = (nf.poison(A, (1, 3, f), v), M) if plane == "angle" else (A, nf.poison(M, (1, 3, f), v))
                got = _np(ops.phase_vocoder(_to(Ap), F_out, src_per_out, logmag=_to(Mp), reset_below=floor, out=_sent((n_ch, bins, F_out))))
                want = voc.phase_vocoder(Ap, F_out, src_per_out, Mp, floor)
                differ = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
                changed = int(np.sum(want.view(np.uint32) != voc.phase_vocoder(A, F_out, src_per_out, M, floor).view(np.uint32)))
                print(f"NONFINITE phase_vocoder src_per_out={src_per_out:.3f} {plane}[1, 3, {f}]={vname}: {changed} outputs move by the rule, "
                      f"{differ} differ from the restatement, all finite: {bool(np.isfinite(got).all())}")
                assert differ == 0 and np.isfinite(got).all()


# =====================================================================================================================================
# the pipeline
# =====================================================================================================================================
A_LEN = 400
RAISES = "Audio buffer is not finite everywhere"
TRACK_SITES = {"first": 0, "clip overlap": 150, "last": A_LEN - 1}
STATS = [(0.1, 2.0), None]


@functools.lru_cache(maxsize=None)
def track_audio():
    from phasegen.track import track_plan
    assert track_plan(A_LEN, 24, 8, 8) == (184, 120, 3) and 120 < TRACK_SITES["clip overlap"] < 184
    return detgen.normal(1031, (2, A_LEN))


@functools.lru_cache(maxsize=None)
def track_model(precision=None, which=None, index=0, value=None):
    """the small model of tests/test_track_gpu.py, optionally with one poisoned parameter element"""
    from phasegen.model import UNetModel
    p = detgen.make_params(16, seed=0)
    if which is not None:
        p[which] = nf.poison(p[which], index, value)
    return UNetModel(16, 32, gpu_ids=[0], precision=precision).load_numpy(p)


# (join, phase, link_channels, stretches)
RECONSTRUCT_ROWS = [("waveform", "unet", False, (1.0,)), ("waveform", "original", False, (1.0,)), ("waveform", "zero", False, (1.0,)),
                    ("spectral", "unet", False, (1.0, 1.5)), ("spectral", "original", False, (1.0,)), ("spectral", "zero", False, (1.0, 1.5)),
                    ("spectral", "vocoder", False, (1.0, 1.5)), ("spectral", "vocoder_locked", False, (1.0, 1.5)),
                    ("spectral", "vocoder_locked", True, (1.0, 1.5)), ("spectral", "spsi", False, (1.0, 1.5))]


@pytest.mark.parametrize("row", RECONSTRUCT_ROWS, ids=lambda r: f"{r[0]}-{r[1]}{'-linked' if r[2] else ''}")
def test_reconstruct_track_raises(row):
    """one poisoned input sample (NaN, +inf, -inf; the first, one in a clip overlap, the last) and reconstruct_track raises the
    documented ValueError, with the training set's statistics and with the track's own moments, at every stretch the phase allows"""
    from phasegen.track import reconstruct_track
    from test_track_gpu import SMALL
    join, phase, link, stretches = row
    model = track_model() if phase == "unet" else None
    audio = track_audio()
    n = 0
    for stretch in stretches:
        kw = dict(phase=phase, **SMALL)
        if join == "spectral":
            kw.update(join="spectral", stretch=stretch, **({"link_channels": True} if link else {}))
        for stats in STATS:
            assert bool(torch.isfinite(reconstruct_track(model, audio, stats=stats, **kw)).all())
            for site, i in TRACK_SITES.items():
                for vname, v in nf.VALUES:
                    with pytest.raises(ValueError, match=RAISES):
                        reconstruct_track(model, nf.poison(audio, (1, i), v), stats=stats, **kw)
                    n += 1
    print(f"NONFINITE reconstruct_track {row[:3]}: {n} poisoned tracks raised")


@pytest.mark.parametrize("phase", ["unet", "vocoder_locked"])
def test_pitch_shift_raises(phase):
    from phasegen.track import pitch_shift
    from test_track_gpu import SMALL
    model = track_model() if phase == "unet" else None
    audio = track_audio()
    assert bool(torch.isfinite(pitch_shift(model, audio, 2.0, stats=(0.1, 2.0), phase=phase, **SMALL)).all())
    for site, i in TRACK_SITES.items():
        for vname, v in nf.VALUES:
            with pytest.raises(ValueError, match=RAISES):
                pitch_shift(model, nf.poison(audio, (1, i), v), 2.0, stats=(0.1, 2.0), phase=phase, **SMALL)


def test_reports_raise():
    """evaluate_track and evaluate_stretch finite-check every synthesis before they measure it (their docstrings): no report comes
    back from a poisoned track"""
    from phasegen.track import evaluate_stretch, evaluate_track
    from test_track_gpu import SMALL
    model, audio = track_model(), track_audio()
    rep = evaluate_track(model, audio, stats=(0.1, 2.0), **SMALL)
    assert all(np.isfinite(v) for m in rep["metrics"].values() for v in m.values() if isinstance(v, float))
    for site, i in TRACK_SITES.items():
        for vname, v in nf.VALUES:
            bad = nf.poison(audio, (1, i), v)
            for join in ("waveform", "spectral"):
                with pytest.raises(ValueError, match=RAISES):
                    evaluate_track(model, bad, stats=(0.1, 2.0), join=join, **SMALL)
            with pytest.raises(ValueError, match=RAISES):
                evaluate_stretch(model, bad, 1.5, stats=(0.1, 2.0), phases=("unet", "vocoder", "zero", "vocoder_locked", "spsi"), **SMALL)


def _parameter_sites():
    keys = list(detgen.CONV_KEYS) + [k + s for k in detgen.BN_KEYS for s in (".weight", ".bias")]
    assert len(keys) == 8 + 12
    return keys


@pytest.mark.parametrize("precision", [None, "bf16"], ids=["fp32-engine", "bf16-resident-engine"])
def test_a_poisoned_parameter_raises(precision):
    """one poisoned element (the first: it feeds output channel 0, which the phase half holds) in each of the 8 conv weights and the
    12 BatchNorm weights and biases: the per-clip forward of either engine carries it into the audio"""
    from phasegen.track import reconstruct_track
    from test_track_gpu import SMALL
    audio = track_audio()
    clean = track_model(precision)
    if precision == "bf16":
        assert clean.engine.resident_ok()
    assert bool(torch.isfinite(reconstruct_track(clean, audio, stats=(0.1, 2.0), **SMALL)).all())
    for key in _parameter_sites():
        for vname, v in nf.VALUES:
            with pytest.raises(ValueError, match=RAISES):
                reconstruct_track(track_model(precision, key, 0, float(v)), audio, stats=(0.1, 2.0), **SMALL)
    print(f"NONFINITE reconstruct_track precision={precision}: {3 * len(_parameter_sites())} poisoned parameters raised")


@pytest.mark.parametrize("precision", [None, "bf16"], ids=["fp32-engine", "bf16-resident-engine"])
def test_running_statistics_are_not_read(precision):
    """negative control: train-mode (per-clip) BatchNorm never reads running_mean / running_var, so poisoning them changes no bit"""
    from phasegen.track import reconstruct_track
    from test_track_gpu import SMALL
    audio = track_audio()
    want = reconstruct_track(track_model(precision), audio, stats=(0.1, 2.0), **SMALL)
    for bn in detgen.BN_KEYS:
        for name in (".running_mean", ".running_var"):
            got = reconstruct_track(track_model(precision, bn + name, 0, float("nan")), audio, stats=(0.1, 2.0), **SMALL)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), bn + name


@pytest.mark.parametrize("plane", [0, 1], ids=["input-logmag", "target-angle"])
def test_trainer_step_matches_the_oracle(plane):
    """Trainer.step at (C, L, B) = (8, 24, 2) with one NaN in the batch: the three losses (which of them are finite, and the finite
    ones to the smoke run's tolerance) and, per parameter, whether its gradient holds a non-finite value, are the oracle's"""
    from oracle import unet_ref
    from phasegen.model import UNetModel
    from phasegen.trainer import Trainer
    C, L, B = 8, 24, 2
    pn = detgen.make_params(C, seed=0)
    batch = nf.poison(detgen.make_batch(B, C, L, seed=1), (1, plane, C // 2, L // 2), nf.NAN)
    model = UNetModel(C, 2 * C, gpu_ids=[0]).load_numpy(pn)
    trainer = Trainer(model, lr=1e-3)
    losses = trainer.step(torch.from_numpy(batch).cuda()).cpu().numpy()
    po = unet_ref.to_torch(pn)
    stats = {k: po[k] for k in po if "running" in k or "num_batches" in k}
    pp = {k: po[k] for k in detgen.param_order()}
    ost = unet_ref.new_opt_state(pp)
    pp.update(stats)
    lo, ao, mo, grads = unet_ref.train_step(pp, torch.from_numpy(batch), ost, stats)
    want = np.array([lo.item(), ao.item(), mo.item()])
    print(f"NONFINITE Trainer.step NaN in batch[:, {plane}]: losses {losses} (oracle {want})")
    assert np.array_equal(np.isfinite(losses), np.isfinite(want)) and not np.isfinite(want).all()
    fin = np.isfinite(want)
    assert np.allclose(losses[fin], want[fin], rtol=1e-4)
    flags = {}
    for k in detgen.param_order():
        flags[k] = (not bool(torch.isfinite(model.engine.arena.g(k)).all()), not bool(torch.isfinite(grads[k]).all()))
    print("NONFINITE Trainer.step gradient flags (device, oracle): " + ", ".join(f"{k}: {a}/{b}" for k, (a, b) in flags.items()))
    assert all(a == b for a, b in flags.values()), flags
