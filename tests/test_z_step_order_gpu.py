"""GPU: the cross-stream ordering of the training step (phasegen/trainer.py) under injected delays.

The overlapped step -- what every data-parallel rank runs, and ``Trainer(fuse_adam=False)`` on one GPU -- enqueues backward on the
caller's stream and each layer's Adam slice on a side stream.  Five single lines of Python make that correct:

    1. a slice starts after its layer's dgrad, the last reader of the old weight          (the event of ``_update_due``)
    2. ... and after its layer's wgrad and bn_bwd, which produce its gradients            (the same event)
    3. ... and after its bucket's collective; with a bf16 payload the widening copy runs inside that wait   (``reducer.wait``)
    4. the next step's forward and backward start after every slice of this step          (the closing ``wait_stream``)
    5. whatever the caller does after ``step()`` returns sees the updated weights          (the same)

The older bit-identity tests (tests/test_unet_gpu.py, tests/test_z_fixup_splits_gpu.py) run the step with natural timing: every
kernel is done before the host has enqueued the next one, so the two streams execute in enqueue order whether or not a dependency
exists.  Here tests/_order.py makes one side LATE by D = max(25 ms, 8 x the unperturbed step, measured in the test) in front of every
launch a rule names, and the result must still have the bits of the serial step (``overlap_adam=False``: one stream, nothing to order),
computed once per shape and unperturbed:

    P0  nothing (the control: the replaced wrappers are transparent)
    P1  late side: every adam_step issued on another stream than the step's               -> 4, 5
    P2  late readers: every conv_dgrad                                                    -> 1
    P3  late producers: every conv_wgrad and bn_bwd                                       -> 2
    P4  late collective (single-rank RCCL group): every all_reduce starts D late on a helper stream   -> 3, and 4 for the wire buffer
    P5  one site: one delayed launch per step, over each of the 8 slices and each of the 7 dgrads in turn

Modes: fused, overlapped, overlapped on a caller's non-default stream, overlapped with collectives (fp32 and bf16 payload).  After
every run the log of the harness is held to the launch counts of a step (8 conv_fwd, 6 bn_fwd, 7 dgrads, 8 wgrads, 6 bn_bwd), to the
streams (every layer's slice on ``_side``; fused: only the six gamma / beta launches, on the step's stream) and to the number of
delayed launches the rule implies.

The harness must catch what it is there to catch.  Two faults are planted from the test, product code untouched; both only make small
tensors hold other values:

    F1  no closing wait: ``Stream.wait_stream(tr._side)`` does nothing.  Caught under P1 at both shapes.
    F2  deaf side stream: ``tr._side.wait_event`` does nothing.  Caught under P2 (the slice overwrites the weight before the delayed
        dgrad has read it) AND under P3 (the slice reads the gradient before the delayed wgrad / bn_bwd has written it).

A delay only reorders streams that the runtime has put on different hardware queues: two streams on one queue run in submission
order, whatever is enqueued.  The first version of this module missed F1 at (16, 64, 3) for that reason -- the trainer's side stream
shared the queue of the step's stream -- so every run first probes the pair (``_order.held_up_by``) and, where a delay on ``_side``
holds the step's stream up, hands the trainer another ``torch.cuda.Stream`` as ``_side`` before its first step.

What F1 and F2 do under P0 is printed, not asserted: a statement about timing (DESIGN.md §4.5 has the record)."""
import contextlib

import pytest
import torch
import torch.distributed as dist

from phasegen import detgen
from _strict import same_bits
import _order
from _order import P0, P1, P2, P3, P4

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64, 3), (40, 48, 2)]           # (C, L, B) of the older bit-identity tests
STEPS = 3
shape_id = "C{0[0]}-L{0[1]}-B{0[2]}".format


def make_model(C):
    from phasegen.model import UNetModel
    return UNetModel(C, 2 * C).load_numpy(detgen.make_params(C, seed=0))


def make_trainer(mode, C):
    from phasegen.trainer import Trainer
    if mode == "serial":
        tr = Trainer(make_model(C), overlap_adam=False)
        assert not tr.overlap_adam and not tr.fuse_adam
    elif mode == "fused":
        tr = Trainer(make_model(C))
        assert tr.fuse_adam
    elif mode in ("overlapped", "caller"):
        tr = Trainer(make_model(C), fuse_adam=False)
    else:
        tr = Trainer(make_model(C), always_reduce=True, grad_compress={"rccl-fp32": None, "rccl-bf16": "bf16"}[mode])
        assert tr.reducer.always and tr.world == 1
    if mode not in ("serial", "fused"):
        assert tr.overlap_adam and not tr.fuse_adam
    return tr


_batches = {}


def batches(shape):
    if shape not in _batches:
        C, L, B = shape
        _batches[shape] = [torch.from_numpy(detgen.make_batch(B, C, L, seed=40 + i)).cuda() for i in range(STEPS)]
    return _batches[shape]


def capture(tr, losses):
    a = tr.engine.arena
    state = {f"losses of step {i}": l for i, l in enumerate(losses)}
    state.update({"arena.flat": a.flat.clone(), "arena.grad": a.grad.clone(), "optim.m": tr.optim.m.clone(), "optim.v": tr.optim.v.clone()})
    state.update({k: v.clone() for k, v in a.buffers.items()})
    state["step_count"] = tr.optim.step_count
    return state


def differing(got, want):
    assert got.keys() == want.keys()
    return [k for k in want if not (same_bits(got[k], want[k]) if torch.is_tensor(want[k]) else got[k] == want[k])]


def assert_same(got, want):
    bad = differing(got, want)
    assert not bad, f"differs from the serial step: {bad}"


_expected = {}


def expected(shape, compress=None):
    """The serial step, run once per shape and payload, unperturbed.  bf16 payload: each rank's bucket is rounded to bf16 before the
    sum and widened back, so with one rank the update sees the bf16 rounding of its own gradient arena."""
    if (shape, compress) not in _expected:
        tr = make_trainer("serial", shape[0])
        losses = []
        for x in batches(shape):
            if compress is None:
                losses.append(tr.step(x).clone())
                continue
            pred = tr.engine.forward(x[:, 0])
            dpred = torch.empty_like(pred)
            tr._loss(pred, x, dpred, tr.losses, tr.mag_weight)
            tr.engine.backward(dpred, lambda name: None)
            g = tr.engine.arena.grad
            g.copy_(g.to(torch.bfloat16).float())
            tr.optim.step(grad_scale=1.0)
            losses.append(tr.losses.clone())
        torch.cuda.synchronize()
        _expected[shape, compress] = capture(tr, losses)
        assert not same_bits(tr.engine.arena.flat, make_model(shape[0]).engine.arena.flat)       # the steps did move the weights
    return _expected[shape, compress]


def run(mode, shape, rule, prepare=None, after=None):
    """Three steps of a fresh trainer under ``rule``.  ``prepare(tr)`` plants a fault before the first step, ``after(tr)`` runs
    straight behind the last ``step()``, before anything synchronises.  Returns (trainer, harness, state)."""
    xs = batches(shape)
    step_ms = _order.measure_step_ms(make_trainer(mode, shape[0]), xs)
    d, passes = _order.delay_for(step_ms)
    tr = make_trainer(mode, shape[0])
    if prepare is not None:
        prepare(tr)
    torch.cuda.synchronize()
    on = torch.cuda.stream(torch.cuda.Stream()) if mode == "caller" else contextlib.nullcontext()
    losses = []
    try:
        with on:
            main = torch.cuda.current_stream()
            assert (main != torch.cuda.default_stream()) == (mode == "caller")
            if tr._side is not None:     # a side stream on the hardware queue of the step's stream cannot be made late or early
                first = tr._side
                tr._side = _order.independent_of(main, first, passes)
                if tr._side is not first:
                    print(f"\n{mode} {shape} {rule}: the trainer's side stream was held up together with the step's stream; replaced")
            with _order.perturbed(rule, main, tr._side, passes) as h:
                for x in xs:
                    h.begin_step()
                    losses.append(tr.step(x).clone())
                if after is not None:
                    after(tr)
    finally:
        torch.cuda.synchronize()
    names = {h.main: "the step's", h.side: "_side"}
    print(f"\n{mode} {shape} {rule}: unperturbed step {step_ms:.2f} ms, D = {d:.1f} ms ({passes} passes); {len(h.fired)} delayed launches "
          f"on {[names.get(s, hex(s)) for s in h.streams_fired_on()]}, {len(h.collectives)} delayed collectives")
    return tr, h, capture(tr, losses)


# ---- every mode x rule row is bit-identical to the serial step --------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("rule", [P0, P1, P2, P3], ids=repr)
@pytest.mark.parametrize("mode", ["fused", "overlapped", "caller"])
def test_step_has_the_bits_of_the_serial_step_under(mode, rule, shape):
    tr, h, got = run(mode, shape, rule)
    _order.check_log(h, tr, STEPS)
    assert_same(got, expected(shape))


SITES = [("adam_step", k) for k in range(8)] + [("conv_dgrad", k) for k in range(7)]


@pytest.mark.parametrize("site", SITES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_one_late_launch_per_step_changes_nothing(site):
    """P5: the orderings per layer -- slice k is the one of BACKWARD_ORDER[k], dgrad k the last reader of that layer's weight"""
    tr, h, got = run("overlapped", SHAPES[0], _order.one_site(*site))
    _order.check_log(h, tr, STEPS)
    assert_same(got, expected(SHAPES[0]))


def test_checkpoint_straight_after_a_step_with_a_late_side_stream_holds_the_updated_state(tmp_path):
    """Ordering 5: ``save_checkpoint`` behind the third ``step()``, no synchronise in between, while every slice is D late."""
    from phasegen.model import UNetModel
    from phasegen.trainer import Trainer
    shape = SHAPES[0]
    path = str(tmp_path / "ckpt_3")
    tr, h, got = run("overlapped", shape, P1, after=lambda t: t.save_checkpoint(path))
    _order.check_log(h, tr, STEPS)
    fresh = Trainer(UNetModel(shape[0], 2 * shape[0]))
    fresh.load_checkpoint(path)
    torch.cuda.synchronize()
    want = expected(shape)
    a = fresh.engine.arena
    for k in detgen.param_order():
        for name, mine, theirs in (("arena.flat", a.flat, want["arena.flat"]), ("optim.m", fresh.optim.m, want["optim.m"]),
                                   ("optim.v", fresh.optim.v, want["optim.v"])):
            assert same_bits(a.view(k, mine), a.view(k, theirs)), f"{name} of {k} in the checkpoint differs from the serial step's"
    for k, v in a.buffers.items():
        assert same_bits(v, want[k]), k
    assert fresh.optim.step_count == want["step_count"] == STEPS
    assert_same(got, want)


def test_enqueue_order_of_one_unperturbed_overlapped_step():
    """The static half, from the log alone: every layer's slice is enqueued after the layer's dgrad (D0: its wgrad), after its wgrad
    and bn_bwd, once, and the slices together are the buckets, which tile the arena."""
    from phasegen.unet import BACKWARD_ORDER
    tr, h, _ = run("overlapped", SHAPES[0], P0)
    assert tr.reducer.buckets.covers_arena()
    bn = _order.bn_layers()
    for step in range(STEPS):
        pos = {(op, k): p for p, op, k, _ in h.step_log(step)}
        slices = _order.slice_layers(h, tr, step)
        assert sorted(name for _, name, _ in slices) == sorted(BACKWARD_ORDER), slices          # every bucket, none twice, nothing else
        assert sorted(_order.slice_span(h, tr, p) for p, _, _ in slices) == sorted(tr.reducer.buckets.spans.values())
        at = {name: p for p, name, _ in slices}
        for i, name in enumerate(BACKWARD_ORDER):
            last_reader = ("conv_dgrad", i) if name != "D0" else ("conv_wgrad", i)
            assert at[name] > pos[last_reader], (name, "slice before the last reader of its weight")
            assert at[name] > pos["conv_wgrad", i], (name, "slice before its wgrad")
            if name in bn:
                assert at[name] > pos["bn_bwd", bn.index(name)], (name, "slice before its bn_bwd")


# ---- planted faults: the harness catches them -------------------------------------------------------------------------------------
def under_p0(fault, shape, prepare):
    _, _, got = run("overlapped", shape, P0, prepare=prepare)
    bad = differing(got, expected(shape))
    print(f"{fault} at {shape} under P0 (natural timing): " + (f"DIFFERS in {bad}" if bad else "passes: the bits of the serial step"))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_planted_fault_no_closing_wait_is_caught_under_a_late_side_stream(shape, monkeypatch):
    """F1.  Without the closing ``wait_stream`` the next forward reads weights, and the next backward overwrites gradients, that the
    late slices have not consumed yet."""
    real = torch.cuda.Stream.wait_stream

    def plant(tr):
        monkeypatch.setattr(torch.cuda.Stream, "wait_stream", lambda self, other: None if other is tr._side else real(self, other))

    under_p0("F1", shape, plant)
    tr, h, got = run("overlapped", shape, P1, prepare=plant)
    _order.check_log(h, tr, STEPS)
    with pytest.raises(AssertionError, match="differs from the serial step"):
        assert_same(got, expected(shape))


class DeafStream(torch.cuda.Stream):
    def wait_event(self, event):
        pass


@pytest.mark.parametrize("rule", [P2, P3], ids=repr)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_planted_fault_deaf_side_stream_is_caught_under_late_readers_and_late_producers(shape, rule):
    """F2.  Caught under P2 and under P3 (module docstring)."""
    def plant(tr):
        tr._side = DeafStream(tr.engine.device)

    if rule is P2:
        under_p0("F2", shape, plant)
    tr, h, got = run("overlapped", shape, rule, prepare=plant)
    _order.check_log(h, tr, STEPS)
    with pytest.raises(AssertionError, match="differs from the serial step"):
        assert_same(got, expected(shape))


# ---- two ranks, one of them late: the worker, the emulation and the assertions of tests/test_dp_two_ranks_gpu.py --------------------
_emulated = {}


@pytest.mark.parametrize("rule", [("P1", 0), ("P2", 1)], ids=lambda r: f"{r[0]}-on-rank-{r[1]}")
def test_two_ranks_skewed_against_each_other_match_the_two_replica_emulation(rule):
    """One rank runs under injected delays (D = max(25 ms, 8 x its unperturbed step) in front of every matching launch), the other
    with natural timing: P1 on rank 0 makes every Adam slice of that rank late (the next step, and the bucket the peer is waiting
    for, must wait for them), P2 on rank 1 every dgrad (its buckets reach the collective late; rank 0's slices must wait for them).
    Same ``emulate(None)`` values and same assertions as test_two_ranks_real_engine_match_the_two_replica_emulation; the cases live
    here so that they are collected behind the older modules, with the rest of this one."""
    import test_dp_two_ranks_gpu as two
    if None not in _emulated:
        _emulated[None] = two.emulate(None)
    two.assert_matches_the_emulation(two.run_ranks(None, rule), _emulated[None])


# ---- overlapped + collectives: a single-rank RCCL group, as tests/test_dp_rccl_gpu.py ----------------------------------------------
@pytest.fixture(scope="module")
def rccl():
    import os
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
@pytest.mark.parametrize("rule", [P0, P1, P2, P3, P4], ids=repr)
@pytest.mark.parametrize("mode", ["rccl-fp32", "rccl-bf16"])
def test_step_with_collectives_has_the_bits_of_the_serial_step_under(rccl, mode, rule, shape):
    tr, h, got = run(mode, shape, rule)
    _order.check_log(h, tr, STEPS)
    assert not tr.reducer.pending
    assert_same(got, expected(shape, "bf16" if mode == "rccl-bf16" else None))
