"""GPU: the smallest problems that reach each instantiation of the stream-K fixup kernel (csrc/conv_fixup.h).
tests/test_kernel_families.py holds the table and pins, on the host, the kernel family, epilogue and fixup form each row takes; here
every row runs.  The fp32 rows run their one op against fp32 torch on the CPU at the tolerance of tests/test_ops_gpu.py, the conv_h3
rows against the float64 convolution of the bf16 operands at the 2e-5 of tests/test_convh_gpu.py.  The module is named to be
collected after the other GPU modules: they cover the same kernels by geometry, and where both fail theirs is the broader finding."""
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref  # noqa: F401  (disables oneDNN: see the bug note in oracle/unet_ref.py)
from test_kernel_families import FIXUP_CASES, FIXUP_CASES_H, fixup_case_id
from test_ops_gpu import TOL, relerr, rnd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", FIXUP_CASES, ids=fixup_case_id)
def test_every_fixup_instantiation_vs_torch(case):
    from phasegen import ops
    (tr, Cin, Cout, k, s, p, Lin, B), op, sched = case[:3]
    x = rnd(51, B, Cin, Lin)
    w = rnd(52, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = F.conv_transpose1d(xr, wr, stride=s, padding=p) if tr else F.conv1d(xr, wr, stride=s, padding=p)
    dy = rnd(53, *yr.shape)
    yr.backward(dy)
    want = {"fwd": yr, "dgrad": xr.grad, "wgrad": wr.grad}[op]
    got = torch.full(want.shape, float("nan"), device="cuda")
    ops.set_conv_schedule(sched)
    try:
        if op == "fwd":
            ops.conv_fwd(x.cuda(), w.cuda(), got, s, p, transposed=tr)
        elif op == "dgrad":
            ops.conv_dgrad(dy.cuda(), w.cuda(), got, s, p, transposed=tr)
        else:
            ops.conv_wgrad(x.cuda(), dy.cuda(), got, s, p, transposed=tr)
    finally:
        ops.set_conv_schedule(0)
    assert relerr(got, want) < TOL


@pytest.mark.parametrize("case", FIXUP_CASES_H, ids=lambda c: f"{'T' if c[0][0] else 'C'}{c[0][1]}-{c[0][2]}-k{c[0][3]}s{c[0][4]}-{c[1]}-{c[2]}")
def test_every_fixup_instantiation_of_conv_h3(case):
    """under the forced stream-K split (schedule 2)"""
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, B = case[0]
    x = rnd(51, B, Cin, Lin)
    w = rnd(52, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1
    want = (F.conv_transpose1d if tr else F.conv1d)(x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double(), stride=s, padding=p)
    xh = ops.h_alloc(B, Cin, Lin, "cuda")
    ops.cast_rows_bf16(x.cuda(), xh)
    wh = ops.shadow_weights(w.cuda(), tr, s)
    y = torch.full(tuple(want.shape), float("nan"), device="cuda")
    ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, transposed=tr, y=y, schedule=2)
    assert relerr(y, want) < 2e-5
