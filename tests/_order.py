"""Helper of tests/test_z_step_order_gpu.py and tests/test_dp_two_ranks_gpu.py (not collected): the cross-stream ordering of the
training step (phasegen/trainer.py), held under injected delays.

The overlapped step runs backward on the caller's stream and each layer's Adam slice on ``Trainer._side``.  Five orderings make it
correct: a slice starts after (1) its layer's dgrad, the last reader of the old weight, (2) its layer's wgrad and
bn_bwd, the producers of its gradients, (3) its bucket's collective; (4) the next step starts after every slice, (5) so does whatever
the caller does after ``step()``.  At test sizes every kernel is done before the host has enqueued the next one, so two streams
execute in enqueue order whether or not a dependency exists.  ``perturbed(rule, ...)`` makes one side LATE instead:

  * it replaces ``ops.conv_fwd / conv_dgrad / conv_wgrad / bn_fwd / bn_bwd / adam_step`` (unet.py, optim.py and trainer.py look them
    up at call time; ``Trainer`` binds ``ops.loss_fwd_bwd`` at construction, so that one is left alone) by wrappers that append
    (op, occurrence within the step, handle of the current stream) to ``.log``, enqueue a delay on the CURRENT stream when the rule
    matches (the positions in the log go to ``.fired``) and call the original with unchanged arguments;
  * a rule with ``collective=True`` also replaces ``phasegen.trainer.dist.all_reduce``: a helper stream waits for the current one,
    runs the delay, and the real ``all_reduce(..., async_op=True)`` is issued under it -- the work object goes back unchanged, so
    ``Work.wait()`` orders its caller behind a collective that really starts late.

The delay is the one of tests/_strict.py: in-place passes over its 2 GiB buffer, ordinary memory traffic of bounded length; the
number of passes is scaled from ``delay_ms``'s calibration on an idle device (work beside it only makes a delay longer).  Besides
the delays only ``held_up_by`` launches anything: one delay and a 64-float add, to find out whether two streams share a hardware
queue -- they then run in submission order and no delay can reorder them (``independent_of`` picks another stream).  The k-th conv_dgrad / conv_wgrad of a step belongs to BACKWARD_ORDER[k] (D0 has no dgrad), the k-th bn_bwd
to the k-th layer of that order that has a BatchNorm.
"""
import contextlib
import math
import time

import torch

import _strict

OPS = ("conv_fwd", "conv_dgrad", "conv_wgrad", "bn_fwd", "bn_bwd", "adam_step")
PER_STEP = {"conv_fwd": 8, "bn_fwd": 6, "conv_dgrad": 7, "conv_wgrad": 8, "bn_bwd": 6}
FACTOR, FLOOR_MS = 8, 25.0       # one delay D = max(FLOOR_MS, FACTOR x the unperturbed step): a stimulus, not a tolerance


class Rule:
    """``match(op, k, stream handle, harness)`` -> delay in front of this launch; ``fires(overlapped)`` -> delayed launches per step."""

    def __init__(self, name, match=None, fires=lambda overlapped: 0, collective=False):
        self.name, self.match, self.fires, self.collective = name, match, fires, collective

    def __repr__(self):
        return self.name


P0 = Rule("P0")                                                                     # the control: the wrappers are transparent
P1 = Rule("P1", lambda op, k, st, h: op == "adam_step" and st != h.main, lambda overlapped: 8 if overlapped else 0)      # late side
P2 = Rule("P2", lambda op, k, st, h: op == "conv_dgrad", lambda overlapped: PER_STEP["conv_dgrad"])                     # late readers
P3 = Rule("P3", lambda op, k, st, h: op in ("conv_wgrad", "bn_bwd"), lambda overlapped: PER_STEP["conv_wgrad"] + PER_STEP["bn_bwd"])
P4 = Rule("P4", collective=True)                                                    # late collective (8 buckets per step)
RULES = {r.name: r for r in (P0, P1, P2, P3, P4)}


def one_site(op, k):
    """P5: one delayed launch per step, in front of the k-th ``op``"""
    return Rule(f"P5-{op}-{k}", lambda o, i, st, h: o == op and i == k, lambda overlapped: 1)


def bn_layers():
    from phasegen.unet import BACKWARD_ORDER, BN_OF
    return [n for n in BACKWARD_ORDER if n in BN_OF]


def measure_step_ms(tr, batches):
    """wall time of one synchronised, unperturbed step of ``tr`` after a warm-up step (``tr`` is used up by it)"""
    tr.step(batches[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.step(batches[1])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def delay_for(step_ms, factor=FACTOR):
    """(D in ms, passes over the delay buffer that take at least D on an idle device)"""
    d = max(FLOOR_MS, factor * step_ms)
    n, took = _strict.delay_ms(FLOOR_MS)
    return d, max(1, math.ceil(d * n / took))


def held_up_by(stream, other, passes):
    """True when a launch on ``stream`` does not run before a delay enqueued earlier on ``other`` has finished.  The runtime maps
    streams onto a few hardware queues, and two streams that share one execute in submission order: a delay on one of them then
    holds the other up as well, every perturbed run is the serial one and every planted fault passes."""
    if "buf" not in _strict._delay:
        _strict.delay_ms(FLOOR_MS)
    if "probe" not in _strict._delay:
        _strict._delay["probe"] = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    late, early = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(other):
        _strict._passes(_strict._delay["buf"], passes)
        late.record()
    with torch.cuda.stream(stream):
        _strict._delay["probe"].add_(1.0)
        early.record()
    early.synchronize()
    held = late.query()
    torch.cuda.synchronize()
    return held


def independent_of(main, stream, passes, tries=8):
    """``stream``, or a fresh stream of its class, that is not held up together with ``main`` (``held_up_by``)"""
    for _ in range(tries):
        if not held_up_by(main, stream, passes):
            return stream
        stream = type(stream)(stream.device)
    raise AssertionError(f"none of {tries} streams runs beside the step's stream: no delay can reorder anything here")


class Order:
    def __init__(self, rule, main, side, passes):
        self.rule, self.passes = rule, passes
        self.main = main.cuda_stream
        self.side = None if side is None else side.cuda_stream
        self.log = []             # (op, occurrence within the step, stream handle), in enqueue order over all steps
        self.starts = []          # position in the log at which each step begins
        self.fired = []           # positions in the log of the launches that got a delay in front
        self.slices = {}          # position in the log of an adam_step -> (data_ptr of p, numel)
        self.collectives = []     # (step, stream handle the all-reduce was asked for on) of every delayed collective
        self._count = {}

    def begin_step(self):
        self._count = {}
        self.starts.append(len(self.log))

    def step_log(self, i):
        """[(position, op, k, stream handle)] of step i"""
        end = self.starts[i + 1] if i + 1 < len(self.starts) else len(self.log)
        return [(pos,) + self.log[pos] for pos in range(self.starts[i], end)]

    def delay(self):
        _strict._passes(_strict._delay["buf"], self.passes)

    def wrap(self, op, fn):
        def call(*args, **kw):
            k = self._count.get(op, 0)
            self._count[op] = k + 1
            st = torch.cuda.current_stream().cuda_stream
            pos = len(self.log)
            self.log.append((op, k, st))
            if op == "adam_step":
                self.slices[pos] = (args[0].data_ptr(), args[0].numel())
            if self.rule.match is not None and self.rule.match(op, k, st, self):
                self.fired.append(pos)
                self.delay()
            return fn(*args, **kw)
        return call

    def late_all_reduce(self, real, helper):
        def all_reduce(*args, **kw):
            cur = torch.cuda.current_stream()
            helper.wait_stream(cur)
            with torch.cuda.stream(helper):
                self.delay()
                work = real(*args, **kw)
            self.collectives.append((len(self.starts) - 1, cur.cuda_stream))
            return work
        return all_reduce

    def streams_fired_on(self):
        return sorted({self.log[pos][2] for pos in self.fired})


_helper = {}


@contextlib.contextmanager
def perturbed(rule, main, side, passes):
    """Run the body with the six ops replaced (module docstring).  ``main``: the stream the steps run on, ``side``: the trainer's
    ``_side`` (or None), ``passes``: length of one delay (``delay_for``).  Call ``.begin_step()`` in front of every step."""
    from phasegen import ops, trainer
    h = Order(rule, main, side, passes)
    if (rule.match is not None or rule.collective) and "buf" not in _strict._delay:
        _strict.delay_ms(FLOOR_MS)
    if rule.collective:          # one helper stream per process, replaced only when it shares a hardware queue with this run's `main`
        _helper["stream"] = independent_of(main, _helper.get("stream") or torch.cuda.Stream(), passes)
    originals = {op: getattr(ops, op) for op in OPS}
    real = trainer.dist.all_reduce
    for op, fn in originals.items():
        setattr(ops, op, h.wrap(op, fn))
    if rule.collective:
        trainer.dist.all_reduce = h.late_all_reduce(real, _helper["stream"])
    try:
        yield h
    finally:
        trainer.dist.all_reduce = real
        for op, fn in originals.items():
            setattr(ops, op, fn)


def slice_span(h, tr, pos):
    """(start, end) in the arena of the adam_step at position ``pos`` of the log"""
    flat = tr.engine.arena.flat
    ptr, n = h.slices[pos]
    s = (ptr - flat.data_ptr()) // flat.element_size()
    return s, s + n


def slice_layers(h, tr, step):
    """[(position, layer or None, stream handle)] of the adam_step launches of one step: the layer whose bucket the slice is"""
    by_span = {span: name for name, span in tr.reducer.buckets.spans.items()}
    return [(pos, by_span.get(slice_span(h, tr, pos)), st) for pos, op, k, st in h.step_log(step) if op == "adam_step"]


def check_log(h, tr, steps):
    """After a run: the launch counts of every step, the streams everything ran on, and that the rule fired where it claims."""
    from phasegen.unet import BACKWARD_ORDER
    overlapped = tr.overlap_adam and not tr.fuse_adam
    assert len(h.starts) == steps
    for i in range(steps):
        entries = h.step_log(i)
        for op, n in PER_STEP.items():
            got = [e for e in entries if e[1] == op]
            assert [e[2] for e in got] == list(range(n)), (i, op, got)
            assert all(e[3] == h.main for e in got), f"step {i}: a {op} ran on another stream than the step's"
        slices = slice_layers(h, tr, i)
        if overlapped:       # every layer's slice (conv weight + its BatchNorm's gamma / beta) once, in backward order, on the side stream
            assert [name for _, name, _ in slices] == BACKWARD_ORDER, (i, slices)
            assert all(st == h.side and st != h.main for _, _, st in slices), (i, slices, h.side)
        elif tr.fuse_adam:   # only the six gamma / beta launches are left, on the step's stream
            spans = [tr.engine.arena.span(tr.engine.layer_param_keys(n)[1:]) for n in bn_layers()]
            got = [slice_span(h, tr, pos) for pos, _, _ in slices]
            assert got == spans, (i, got, spans)
            assert all(st == h.main for _, _, st in slices), (i, slices)
        else:                # serial: one launch over the arena
            assert len(slices) == 1 and slices[0][2] == h.main and h.slices[slices[0][0]][1] == tr.engine.arena.numel
        here = {e[0] for e in entries}
        fired = [pos for pos in h.fired if pos in here]
        assert len(fired) == h.rule.fires(overlapped), (i, h.rule, [h.log[p] for p in fired])
        for pos in fired:    # a delayed slice sat on the side stream, every other delayed launch on the step's
            op, k, st = h.log[pos]
            assert h.rule.match(op, k, st, h)
            assert st == (h.side if op == "adam_step" else h.main), (i, h.rule, h.log[pos])
        late = [c for c in h.collectives if c[0] == i]
        if h.rule.collective:
            assert len(late) == len(BACKWARD_ORDER) and all(st == h.main for _, st in late), (i, late)
        else:
            assert not late
    assert len(h.fired) == steps * h.rule.fires(overlapped)
