"""GPU: the multi-tile work splits of the conv kernels on small problems.

Every row of FIXUP_CASES, VIEW_CASES, ADDED_CASES and FIXUP_CASES_H has at most a handful of tiles: a workgroup owns one whole tile
or a fragment of one.  What the benchmark and every full-width training step run -- several whole tiles per persistent workgroup,
ranges with whole tiles between a partial head and a partial tail, the hybrid split (whole-tile workgroups and splitting ones in one
launch, the fixup offset by the whole tiles), the contended policy, other oversubscription factors -- was reached only by the
C = 1024 modules, on sampled elements.  SPLIT_CASES / SPLIT_CASES_H (tests/test_kernel_families.py, each row's plan pinned there on
the CPU) reach those regimes on problems of a few tiles through PG_SCHED_SLOTS(n), which plans a call as if the device had n compute
units; the kernels, and what they are handed (gridDim, whole, tiles, slabs), are the ones a full-size layer gets.

Nothing here has a tolerance of its own.  The rows go through the machinery of the small-problem modules:
  values      tests/test_z_conv_values_gpu.py: per element against float64, r_max / r_rms within 4 x the honest CPU stand-in, exact
              zeros, both activated outputs, the dgrad's addend and signed-zero mask, the wgrad with x_act leaky; white and graded
              inputs; fp32, and bf16 / bf16x3 for the families that have those modes; NaN outputs, workspace 0xff
  impulses    the same module: bit for bit
  views       tests/test_z_conv_views_gpu.py: both view layouts and the engine's in-place dgrad, bit-identical to the dense call
  fused Adam  a wgrad with pg_conv_args.adam against the same wgrad followed by ops.adam_step, bit for bit: in the hybrid rows the
              GEMM kernel's epilogue updates the whole tiles and the fixup's the split ones, in one launch
  repeat      a second call on the workspace the first one left (its partial tiles still there): identical bits
and one training step of a small network under the override goes through the comparison of tests/test_fullwidth_gpu.py.

Named to be collected after the other conv modules: where both fail theirs is the broader finding."""
import pytest
import torch

import test_z_conv_values_gpu as values
import test_z_conv_views_gpu as views
from phasegen import detgen
from test_fullwidth_gpu import check_train_step_vs_oracle
from test_kernel_families import (BF16_FAMILIES, CONTENDED, SLOTS, SPLIT_CASES, SPLIT_CASES_H, SPLIT_TABLE, _fields, _opcode, _view_args, family,
                                  fixup_case_id, layers, regimes)
from test_ops_gpu import rnd

pytestmark = pytest.mark.gpu
REGIME = {row: "+".join(declared) for row, declared, _ in SPLIT_TABLE}


def _id(c):
    return f"{REGIME[c]}-{fixup_case_id(c)}"


def _cases(families=None, op=None):
    return [pytest.param(c, id=_id(c)) for c in SPLIT_CASES if (families is None or c[3] in families) and (op is None or c[1] == op)]


def _h_id(row):
    g, epi, form, sched = row
    return f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}-L{g[6]}-B{g[7]}-{epi}-{form}-{sched:#x}"


@pytest.mark.parametrize("case", _cases())
def test_values_fp32(case):
    values.run_values(case, "fp32")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_values_bf16(case):
    values.run_values(case, "bf16")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_values_bf16x3(case):
    values.run_values(case, "bf16x3")


@pytest.mark.parametrize("case", _cases())
def test_impulse_fp32(case):
    values.run_impulse(case, "fp32")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_impulse_bf16(case):
    values.run_impulse(case, "bf16")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_impulse_bf16x3(case):
    values.run_impulse(case, "bf16x3")


@pytest.mark.parametrize("row", SPLIT_CASES_H, ids=_h_id)
def test_values_conv_h3(row):
    values.run_values_h3(row[0], row[3])


@pytest.mark.parametrize("row", SPLIT_CASES_H, ids=_h_id)
def test_impulse_conv_h3(row):
    values.run_impulse_h3(row[0], row[3])


@pytest.mark.parametrize("case", _cases())
def test_views_fp32(case):
    views._run(case, "fp32")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_views_bf16(case):
    views._run(case, "bf16")


@pytest.mark.parametrize("case", _cases(BF16_FAMILIES))
def test_views_bf16x3(case):
    views._run(case, "bf16x3")


@pytest.mark.parametrize("row", SPLIT_CASES_H, ids=_h_id)
def test_views_conv_h3(row):
    views.run_views_h3(row[0], row[3])


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _operands(case):
    """(x, w, dy) of the row on the device: the suite's noise, the weight x 0.1"""
    tr, Cin, Cout, k, s, p, Lin, B = case[0]
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    dev = _dev()
    return rnd(61, B, Cin, Lin).to(dev), (rnd(62, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1).to(dev), rnd(63, B, Cout, Lout).to(dev)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", _cases(op="wgrad"))
def test_fused_adam_is_bit_identical_to_wgrad_then_adam_step(case, prec):
    """conv_wgrad(..., adam=) at step 3 with non-zero moments and a gradient scale: dw as without `adam`, and p / m / v as ops.adam_step
    leaves them from that dw -- every element of dw passes through exactly one epilogue, the GEMM kernel's (whole tiles) or the
    fixup's (split tiles)."""
    from phasegen import ops
    assert case[3] in BF16_FAMILIES                 # (every wgrad family has the bf16 operand mode)
    tr, Cin, Cout, k, s, p, Lin, B = case[0]
    x, w, dy = _operands(case)
    m0, v0 = (rnd(66, *w.shape) * 0.01).to(_dev()), (rnd(67, *w.shape) * 0.01).to(_dev()).square()
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=0.5)
    kw = dict(x_act=ops.ACT_LEAKY, transposed=tr, precision=prec, schedule=case[2])
    dw_plain = ops.conv_wgrad(x, dy, torch.full_like(w, float("nan")), s, p, **kw)
    assert bool(torch.isfinite(dw_plain).all()) and float(dw_plain.abs().max()) > 0
    p1, m1, v1 = w.clone(), m0.clone(), v0.clone()
    ops.adam_step(p1, dw_plain, m1, v1, 3, **hyper)
    p2, m2, v2 = w.clone(), m0.clone(), v0.clone()
    dw_fused = torch.full_like(w, float("nan"))
    with values._Poisoned():
        ops.conv_wgrad(x, dy, dw_fused, s, p, adam=ops.adam_args(p2, m2, v2, 3, **hyper), **kw)
    assert torch.equal(dw_fused, dw_plain)
    for name, got, want, start in (("p", p2, p1, w), ("m", m2, m1, m0), ("v", v2, v1, v0)):
        assert torch.equal(got, want), (case, name, int((got != want).sum()), torch.nonzero(got != want)[:4].tolist())
        assert not torch.equal(got, start), name


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("case", _cases())
def test_a_second_call_on_the_used_workspace_gives_the_same_bits(case, prec):
    """the workspace still holds the first call's partial tiles (and, for a wgrad, its packed operands) when the second is enqueued
    (conv_raw3 is fp32 only: at the other precisions its rows are planned onto conv_raw, under the same slot count)"""
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, B = case[0]
    op, sched = case[1], case[2]
    x, w, dy = _operands(case)
    kw = dict(transposed=tr, precision=prec, schedule=sched)

    def call():
        if op == "fwd":
            return ops.conv_fwd(x, w, torch.full_like(dy, float("nan")), s, p, x_act=ops.ACT_LEAKY, **kw)
        if op == "dgrad":
            return ops.conv_dgrad(dy, w, torch.full_like(x, float("nan")), s, p, **kw)
        return ops.conv_wgrad(x, dy, torch.full_like(w, float("nan")), s, p, x_act=ops.ACT_LEAKY, **kw)

    first, second = call(), call()
    assert bool(torch.isfinite(first).all()) and torch.equal(first, second), case


@pytest.mark.parametrize("row", SPLIT_CASES_H, ids=_h_id)
def test_a_second_resident_forward_on_the_used_workspace_gives_the_same_bits(row):
    """pg_conv_fwd_h twice: the second call finds the first one's partial tiles in the workspace"""
    from phasegen import ops
    geom, epi, form, sched = row
    tr, Cin, Cout, k, s, p, Lin, B = geom
    x, w, _ = _operands((geom,))
    xh = ops.h_alloc(B, Cin, Lin, _dev())
    ops.cast_rows_bf16(x, xh, act=ops.ACT_LEAKY)
    wh = ops.shadow_weights(w, tr, s)
    outs = []
    for _ in range(2):
        y = torch.full((B, Cout, (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1), float("nan"), device=_dev())
        ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, transposed=tr, y=y, schedule=sched)
        outs.append(y)
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0 and torch.equal(outs[0], outs[1]), row


# ---- one network-level check: the layer wiring and the schedule words the engine ORs in, under the override -------------------------
NET = (40, 128, 6)                                  # C = 40: 80-row partial tiles; 6 x (65 .. 14) columns
NET_SCHEDULES = [pytest.param(SLOTS(1), id="slots1"), pytest.param(SLOTS(1) | CONTENDED, id="slots1-contended"),
                 pytest.param(SLOTS(2) | CONTENDED, id="slots2-contended")]
# What the plans of one step must hold, per op, so that a case cannot degenerate into the one-tile and fragment splits
# tests/test_unet_gpu.py already runs (each entry: regimes of which at least one must occur among the op's launches).
#   one slot:             hybrid forwards (D1, U0) and dgrads (U1), hybrid and multi-whole wgrads
#   one slot, contended:  bit 4 turns the hybrid plans into even splits over ranges of 1.5 tiles (a whole tile and half of the next);
#                         the forwards have at most 3 tiles on 2 slots and no tile count that divides, so none is multi-whole;
#                         U0.dgrad runs its 2 tiles in one workgroup, U2 / U1 / U0.wgrad several whole tiles each
#   two slots, contended: every forward and dgrad of this width has at most 3 tiles on 4 slots (2 for conv_raw3) -- grid >= tiles,
#                         nothing to guard; only the wgrads reach multi-tile ranges (U0: 20 tiles on 4 workgroups, U2: whole tiles
#                         between partial ones).  Run for those wgrads' sake, inside the whole step.
NET_GUARD = {
    SLOTS(1): {"fwd": {"hybrid", "multi-whole"}, "dgrad": {"hybrid", "multi-whole"}, "wgrad": {"hybrid", "multi-whole"}},
    SLOTS(1) | CONTENDED: {"fwd": {"contended", "whole-then-partial"}, "dgrad": {"multi-whole"}, "wgrad": {"multi-whole"}},
    SLOTS(2) | CONTENDED: {"wgrad": {"multi-whole"}},
}


@pytest.fixture
def released():
    """the network tests build whole engines (captured graphs, side streams, arenas): drop them before the next module runs"""
    yield
    import gc
    from phasegen import ops
    torch.cuda.synchronize()
    gc.collect()
    ops.release_workspaces()
    torch.cuda.empty_cache()


def _net_regimes(sched):
    """{op: the regimes its launches of one step are in} from pg_conv_describe over the engine's layer geometries at NET"""
    from phasegen import _lib, ops
    C, L, B = NET
    out = {"fwd": set(), "dgrad": set(), "wgrad": set()}
    for name, tr, Cin, Cout, k, s, p, Lin in layers(C, L):
        for op in out:
            if (name, op) == ("D0", "dgrad"):
                continue
            row = ((tr, Cin, Cout, k, s, p, Lin, B), op, sched, None, None, None)
            d = ops.conv_describe(_view_args(_lib, row, None), _opcode(_lib, row))
            auto = _fields(ops.conv_describe(_view_args(_lib, row[:2] + (sched & ~CONTENDED,) + row[3:], None), _opcode(_lib, row)))
            out[op] |= regimes(_fields(d), sched, auto, family(d) == "conv_raw3")
    return out


@pytest.mark.parametrize("sched", NET_SCHEDULES)
def test_train_step_under_the_slot_override_vs_oracle(sched, released):
    """One Trainer.step at C = 40 with the thread's schedule word set: tests/test_fullwidth_gpu.py's comparison with the oracle run
    under the device's sign masks, at its tolerances.  The plans are checked first (NET_GUARD): under the first two words a forward,
    a dgrad and a wgrad launch of the step are each in a multi-tile regime."""
    from phasegen import ops
    reg = _net_regimes(sched)
    for op, any_of in NET_GUARD[sched].items():
        assert reg[op] & any_of, (op, reg)
    if sched & CONTENDED:
        assert {"contended", "head-whole-tail" if sched == SLOTS(2) | CONTENDED else "whole-then-partial"} <= reg["wgrad"], reg
    assert sum(set(g) == {"fwd", "dgrad", "wgrad"} for g in NET_GUARD.values()) == 2
    with ops.conv_options(schedule=sched):
        check_train_step_vs_oracle(*NET, label=f"schedule {sched:#x}")


@pytest.mark.parametrize("sched", [NET_SCHEDULES[0], NET_SCHEDULES[2]])
def test_fused_overlapped_and_serial_adam_agree_under_the_slot_override(sched, released):
    """three steps of the fused, the overlapped and the serial Adam (tests/test_unet_gpu.py) under the override: bit-identical"""
    from phasegen import ops
    from phasegen.trainer import Trainer
    from test_unet_gpu import make_model
    C, L, B = NET
    with ops.conv_options(schedule=sched):
        batches = [torch.from_numpy(detgen.make_batch(B, C, L, seed=40 + i)).cuda() for i in range(3)]
        a, o, b = Trainer(make_model(C)), Trainer(make_model(C), fuse_adam=False), Trainer(make_model(C), overlap_adam=False)
        assert a.fuse_adam and o.overlap_adam and not o.fuse_adam and not b.overlap_adam and not b.fuse_adam
        for x in batches:
            la, lo, lb = a.step(x).clone(), o.step(x).clone(), b.step(x).clone()
            assert torch.equal(la, lb) and torch.equal(lo, lb)
        torch.cuda.synchronize()
    for t in (a, o):
        assert torch.equal(t.engine.arena.flat, b.engine.arena.flat)
        assert torch.equal(t.engine.arena.grad, b.engine.arena.grad)
        assert torch.equal(t.optim.m, b.optim.m) and torch.equal(t.optim.v, b.optim.v)
        assert t.optim.step_count == b.optim.step_count == 3
    assert not torch.equal(b.engine.arena.flat, make_model(C).engine.arena.flat)
