"""GPU: every conv kernel family in the argument patterns of the U-Net engine (phasegen/unet.py) -- operands that are channel slices
of wider buffers or batch[:, 0] of a (B, 2, C, L) batch, each with its own batch stride; an activation fused into the forward's
store and a second, differently activated output; the dgrad's addend and mask source as views, and the engine's in-place form (the
addend IS the dx view); the wgrad on a batch-strided x and a sliced dy.  tests/test_kernel_families.py holds the table (VIEW_CASES:
every fixup instantiation, every family's own epilogue, the column-tail launch, the packed wgrads, a runtime (k, s)) and pins on the
host that a row's plan does not depend on the strides.

Everything outside an input view is NaN, so a read outside the view -- which on a dense tensor falls outside the buffer descriptor
and returns zero, or is multiplied by a zero weight -- poisons the result.  Everything outside an output view is a finite sentinel
and the view itself starts as NaN.  Every byte of the thread's conv workspace is 0xff (a NaN pattern) when the checked call is
enqueued: the header calls its contents garbage between calls.

Each checked call is compared (1) with a CPU reference at the bounds of tests/test_ops_gpu.py -- fp32: fp32 torch, 1e-4 of max-abs;
bf16: float64 convolution of the bf16-rounded operands, 2e-5; bf16x3: float64 convolution of the unrounded operands, 2e-5 -- and
(2) BIT FOR BIT with the same op, schedule and precision on dense copies of the same data, without a store activation and with a
separate addend: the plan is the same, no kernel branches on alignment or stride, and the fixup adds a tile's segments in an order
that depends on (grid, tiles) alone, so nothing but addresses differs.

Like tests/test_z_fixup_cases_gpu.py the module is named to be collected after the other GPU modules: they cover the same kernels by
geometry on dense tensors, and where both fail theirs is the broader finding."""
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref  # noqa: F401  (disables oneDNN: see the bug note in oracle/unet_ref.py)
from test_kernel_families import BF16_FAMILIES, FIXUP_CASES_H, VIEW_CASES, VIEW_PAIRS, fixup_case_id, view_layout
from test_ops_gpu import TOL, act_cpu, bf16_round, relerr, rnd

pytestmark = pytest.mark.gpu
SENTINEL = -77.0
NAN = float("nan")
BOUND = {"fp32": TOL, "bf16": 2e-5, "bf16x3": 2e-5}
LEAKY, RELU = 1, 2


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _in_view(t, off, extra, outside=NAN):
    """t (CPU) as the channel slice [off, off + C) of a wider device buffer whose other channels hold `outside`"""
    B, C, L = t.shape
    buf = torch.full((B, off + C + extra, L), outside, device=_dev())
    v = buf[:, off:off + C]
    v.copy_(t)
    return buf, v


def _in_batch0(t):
    """t (CPU) as batch[:, 0] of a (B, 2, C, L) device batch whose other half is NaN"""
    B, C, L = t.shape
    batch = torch.full((B, 2, C, L), NAN, device=_dev())
    batch[:, 0].copy_(t)
    return batch[:, 0]


def _out_view(B, off, extra, C, L):
    """a NaN channel slice of a wider device buffer whose other channels hold the sentinel"""
    buf = torch.full((B, off + C + extra, L), SENTINEL, device=_dev())
    v = buf[:, off:off + C]
    v.fill_(NAN)
    return buf, v


def _untouched(buf, off, C):
    return bool((buf[:, :off] == SENTINEL).all()) and bool((buf[:, off + C:] == SENTINEL).all())


class _Poisoned:
    """``with _Poisoned():`` -- every byte of this thread's conv workspace (as sized by the calls made so far, a wgrad's packed
    operands included) is 0xff when the body's call is enqueued, and that call neither grows nor replaces the buffer"""

    def __enter__(self):
        from phasegen import ops
        self.ws = ops.conv_workspace(_dev())
        self.ws.fill_(0xFF)

    def __exit__(self, *exc):
        from phasegen import ops
        if exc[0] is None:
            ws = ops.conv_workspace(_dev())
            assert ws.data_ptr() == self.ws.data_ptr() and ws.numel() == self.ws.numel()


def _problem(case, prec):
    """the row's data (CPU, fp32) and a function act -> (reference of the row's op with x_act = act, in the reference's own dtype)"""
    (tr, Cin, Cout, k, s, p, Lin, B), op = case[0], case[1]
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    x, w, dy = rnd(61, B, Cin, Lin), rnd(62, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1, rnd(63, B, Cout, Lout)
    conv = (lambda a, b: F.conv_transpose1d(a, b, stride=s, padding=p)) if tr else (lambda a, b: F.conv1d(a, b, stride=s, padding=p))
    # operand as the MFMA sees it: fp32 torch for fp32; float64 of the bf16-rounded / of the unrounded values for bf16 / bf16x3
    see = {"fp32": lambda t: t.clone(), "bf16": lambda t: bf16_round(t).double(), "bf16x3": lambda t: t.double()}[prec]

    def reference(act):
        xa, wr = see(act_cpu(x, act)).requires_grad_(True), see(w).requires_grad_(True)
        yr = conv(xa, wr)
        if op == "fwd":
            return yr.detach()
        yr.backward(see(dy))
        return xa.grad if op == "dgrad" else wr.grad

    return x, w, dy, reference


def _cases(families=None):
    return [pytest.param(c, id=fixup_case_id(c)) for c in VIEW_CASES if families is None or c[3] in families]


def _report(prec, case, what, err):
    print(f"VIEWERR {prec} {case[3]} {case[1]} {what} {err:.3e} (bound {BOUND[prec]:.0e})")


def _run(case, prec):
    from phasegen import ops
    (tr, Cin, Cout, k, s, p, Lin, B), op, sched = case[:3]
    x, w, dy, reference = _problem(case, prec)
    kw = dict(transposed=tr, precision=prec, schedule=sched)
    tol = BOUND[prec]
    dev = _dev()
    wd, xd, dyd = w.to(dev), x.to(dev), dy.to(dev)
    # the references, once per row: the CPU's, and the same op on dense copies (fwd: no store activation; these calls also size the workspace)
    want = {a: reference(a) for a in ((0,) if op == "dgrad" else (0, LEAKY))}
    dense = {}
    for a in (0, LEAKY):
        if op == "fwd":
            dense[a] = ops.conv_fwd(xd, wd, torch.empty(want[a].shape, device=dev), s, p, x_act=a, **kw)
        elif op == "wgrad":
            dense[a] = ops.conv_wgrad(xd, dyd, torch.empty(w.shape, device=dev), s, p, x_act=a, **kw)
    for pair in range(len(VIEW_PAIRS)):
        lay = view_layout(case, pair)
        acts = (0, LEAKY) if pair == 0 else (LEAKY, 0)       # both input activations / masks in every row, swapped between the layouts
        if op == "fwd":
            # D0's form: x a view, y stored as LeakyReLU into a view, y2 as ReLU into another view of another width
            a = acts[0]
            _, xv = _in_view(x, *lay["x"][:2])
            ybuf, yv = _out_view(B, *lay["y"][:4])
            y2buf, y2v = _out_view(B, *lay["y2"][:4])
            assert len({xv.stride(0), yv.stride(0), y2v.stride(0)}) == 3 or B == 1
            with _Poisoned():
                ops.conv_fwd(xv, wd, yv, s, p, x_act=a, y_act=ops.ACT_LEAKY, y2=y2v, y2_act=ops.ACT_RELU, **kw)
            errs = relerr(yv, F.leaky_relu(want[a], 0.2)), relerr(y2v, F.relu(want[a]))
            _report(prec, case, f"pair{pair} y", errs[0])
            _report(prec, case, f"pair{pair} y2", errs[1])
            assert errs[0] < tol and errs[1] < tol, errs        # (each on its own: a NaN compares false, max() may drop it)
            assert not bool(torch.isnan(yv).any()) and not bool(torch.isnan(y2v).any())
            assert torch.equal(yv.cpu(), F.leaky_relu(dense[a].cpu(), 0.2)) and torch.equal(y2v.cpu(), F.relu(dense[a].cpu()))
            assert torch.equal(y2v, torch.relu(yv))          # exact: relu(leaky(v)) == relu(v)
            assert _untouched(ybuf, *lay["y"][0:3:2]) and _untouched(y2buf, *lay["y2"][0:3:2])
            # D3's form: y stored as ReLU, no second output; x as batch[:, 0] of a (B, 2, C, L) batch
            a = acts[1]
            xb = _in_batch0(x)
            ybuf, yv = _out_view(B, *lay["y"][:4])
            with _Poisoned():
                ops.conv_fwd(xb, wd, yv, s, p, x_act=a, y_act=ops.ACT_RELU, **kw)
            err = relerr(yv, F.relu(want[a]))
            _report(prec, case, f"pair{pair} y(relu)", err)
            assert err < tol
            assert not bool(torch.isnan(yv).any()) and torch.equal(yv.cpu(), F.relu(dense[a].cpu())) and _untouched(ybuf, *lay["y"][0:3:2])
        elif op == "dgrad":
            add, ref = rnd(64, B, Cin, Lin), rnd(65, B, Cin, Lin)
            assert bool((ref != 0).all())                    # (the mask's sign test would be ambiguous at 0)
            g = want[0]
            addd, refd = add.to(dev), ref.to(dev)
            for form, mask in zip("ab", (LEAKY, RELU) if pair == 0 else (RELU, LEAKY)):
                slope = 0.2 if mask == LEAKY else 0.0
                want_dx = (g + add.to(g.dtype)) * torch.where(ref > 0, torch.ones_like(g), torch.full_like(g, slope))
                dense_dx = ops.conv_dgrad(dyd, wd, torch.empty(B, Cin, Lin, device=dev), s, p, add=addd, ref=refd, mask=mask, **kw)
                _, dyv = _in_view(dy, *lay["dy"][:2])
                if form == "a":                              # every tensor a view of a buffer of its own width
                    dxbuf, dxv = _out_view(B, *lay["dx"][:4])
                    _, addv = _in_view(add, *lay["add"][:2])
                    _, refv = _in_view(ref, *lay["ref"][:2])
                    assert len({dyv.stride(0), dxv.stride(0), addv.stride(0), refv.stride(0)}) == 4 or B == 1
                else:                                        # the engine's in-place form: dx holds the skip gradient and is its own addend; ref dense
                    dxbuf, dxv = _in_view(add, *lay["dx"][:2], outside=SENTINEL)
                    addv, refv = dxv, refd
                with _Poisoned():
                    ops.conv_dgrad(dyv, wd, dxv, s, p, add=addv, ref=refv, mask=mask, **kw)
                err = relerr(dxv, want_dx)
                _report(prec, case, f"pair{pair} dx({form})", err)
                assert err < tol
                assert not bool(torch.isnan(dxv).any()) and torch.equal(dxv, dense_dx) and _untouched(dxbuf, *lay["dx"][0:3:2])
        else:
            for a in acts:                                   # D0's form: x batch-strided, dy the lower channels of a wider gradient buffer
                xb = _in_batch0(x)
                _, dyv = _in_view(dy, *lay["dy"][:2])
                assert xb.stride(0) != dyv.stride(0)
                dw = torch.full(w.shape, NAN, device=dev)
                with _Poisoned():
                    ops.conv_wgrad(xb, dyv, dw, s, p, x_act=a, **kw)
                err = relerr(dw, want[a])
                _report(prec, case, f"pair{pair} dw(act {a})", err)
                assert err < tol
                assert not bool(torch.isnan(dw).any()) and torch.equal(dw, dense[a])


@pytest.mark.parametrize("case", _cases())
def test_views_fp32(case):
    _run(case, "fp32")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_views_bf16(case):
    _run(case, "bf16")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_views_bf16x3(case):
    _run(case, "bf16x3")


def run_views_h3(geom, sched):
    """pg_conv_fwd_h under schedule word `sched`: yh / yh2 as channel slices of wider ops.h_alloc buffers (as the resident forward
    writes the concat halves), stored as LeakyReLU / ReLU, bit-identical to the call on dense outputs; the row tails [Lout, pitch) inside
    the views stay zero, the sibling channels untouched."""
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, B = geom
    dev = _dev()
    x = rnd(51, B, Cin, Lin)
    w = rnd(52, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    xh = ops.h_alloc(B, Cin, Lin, dev)
    ops.cast_rows_bf16(x.to(dev), xh)
    wh = ops.shadow_weights(w.to(dev), tr, s)
    kw = dict(transposed=tr, yh_act=ops.ACT_LEAKY, yh2_act=ops.ACT_RELU, schedule=sched)
    d1, d2 = ops.h_alloc(B, Cout, Lout, dev), ops.h_alloc(B, Cout, Lout, dev)
    ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, yh=d1, yh2=d2, **kw)
    assert float(d1[:, :, :Lout].float().abs().max()) > 0.0
    for off, extra in VIEW_PAIRS:
        bufs, views = [], []
        for i in range(2):                                    # yh and yh2 in buffers of different widths
            buf = ops.h_alloc(B, off + Cout + extra + i, Lout, dev)
            buf[:, :off] = SENTINEL                           # (-77 is a bf16 value)
            buf[:, off + Cout:] = SENTINEL
            bufs.append(buf)
            views.append(buf[:, off:off + Cout])
        assert views[0].stride(0) != views[1].stride(0) or B == 1
        with _Poisoned():
            ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, yh=views[0], yh2=views[1], **kw)
        assert torch.equal(views[0], d1) and torch.equal(views[1], d2)
        for buf, v in zip(bufs, views):
            assert float(v[:, :, Lout:].float().abs().max()) == 0.0
            assert bool((buf[:, :off] == SENTINEL).all()) and bool((buf[:, off + Cout:] == SENTINEL).all())


@pytest.mark.parametrize("case", FIXUP_CASES_H, ids=lambda c: f"{'T' if c[0][0] else 'C'}{c[0][1]}-{c[0][2]}-k{c[0][3]}s{c[0][4]}-{c[1]}-{c[2]}")
def test_views_conv_h3(case):
    """the forced stream-K split over every fixup instantiation of conv_h3"""
    run_views_h3(case[0], 2)
