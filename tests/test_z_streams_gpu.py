"""GPU: every entry point of include/phasegen.h that takes a stream, held to the stream contract of the C ABI --

    a call runs asynchronously on the stream passed in, and only there; a call never synchronises.

Every other GPU module but one case runs on the default stream, where a launch (or pg_ola_nt's memset) handed to stream 0 by mistake,
or a blocking copy in a wrapper, gives the same bits.  Here each entry point runs once on a SIDE stream that is still busy with a
delay of at least 200 ms (tests/_strict.py: delayed_stream; the measured length is printed):

    1. the plain call on the default stream warms up (filter bank, ramp, LDS attributes) and forms `expected`;
    2. the float inputs are overwritten with NaN, the outputs hold a sentinel (index inputs, gains and statistics keep their values);
    3. on the side stream: the inputs are restored by copies, then the wrapper runs under strict_workspaces(0xFF) (0x00 for phase_lock);
    4. the moment the wrapper returns the side stream must still be busy, and the wrapper must have taken less than a quarter of the
       delay on the host (measured: 0.01 to 0.3 ms against 370 ms): the call did not wait for the device, at its end or in its middle;
    5. after a synchronise the result has the bits of `expected` and the workspace guards are intact.

The side stream does not block on stream 0 (no torch.cuda.Stream does), so a launch that went to stream 0 runs AT ONCE: before the
copies, on NaN inputs, on poisoned partials or on intermediates nobody has written, or its output is overwritten out of order -- the
bits differ.  The recorder of strict_workspaces also sees the stream handle every library call was given.  Each case first runs the
same call once on the idle side stream, which fills that stream's pool of the caching allocator (a first hipMalloc of a 576 MiB conv
workspace is the allocator's business, not the wrapper's).

Wrappers exempt from step 4 because they legitimately read the device on the host: none.

The last part tests the helper on stand-in kernels made of torch ops: every planted fault must be caught."""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import unet_ref  # noqa: F401  (disables oneDNN: see the bug note in oracle/unet_ref.py)
from phasegen import detgen
from _strict import delayed_stream, delay_ms, same_bits, side_stream, strict_view, strict_workspaces, stream_symbols
import test_z_workspace_gpu as W
from test_z_workspace_gpu import Case, cuda, dev, sent
from test_kernel_families import FIXUP_CASES, FIXUP_CASES_H, VIEW_CASES

pytestmark = pytest.mark.gpu
NAN = float("nan")
REACHED = set()
EXEMPT_FROM_STEP_4 = {}          # case id -> reason (a wrapper that legitimately reads the device on the host); none is expected


def stream_check(case, warm_side=True):
    expected = [t.clone() for t in case.run(case.ins, case.make_outs())]                   # 1
    torch.cuda.synchronize()
    poison = 0x00 if case.lock else 0xFF
    floats = [k for k, v in case.ins.items() if v.is_floating_point() and k not in case.fixed]
    good = {k: case.ins[k].clone() for k in floats}
    if warm_side:
        with torch.cuda.stream(side_stream()), strict_workspaces(poison):
            warm = case.run(case.ins, case.make_outs())
        assert all(same_bits(g, w) for g, w in zip(warm, expected)), f"{case.id}: the idle side stream gives other bits"
    for k in floats:                                                                       # 2
        case.ins[k].fill_(NAN)
    outs = case.make_outs()
    side = delayed_stream()
    try:
        with torch.cuda.stream(side):                                                      # 3
            for k in floats:
                case.ins[k].copy_(good[k], non_blocking=True)
            with strict_workspaces(poison) as s:
                t0 = time.perf_counter()
                got = case.run(case.ins, outs)
                host_ms = (time.perf_counter() - t0) * 1e3
                busy = not side.query()                                                    # 4
        # (leaving strict_workspaces synchronised and checked the guards)                   # 5
    finally:
        torch.cuda.synchronize()
        for k in floats:
            case.ins[k].copy_(good[k])
    print(f"{case.id}: the wrapper returned after {host_ms:.2f} ms on the host; the delay in front of it is {delay_ms()[1]:.0f} ms")
    if case.id not in EXEMPT_FROM_STEP_4:
        assert busy, f"{case.id}: the call waited for the device (the side stream was idle when the wrapper returned)"
        # a wait in the MIDDLE of a call, with launches behind it, leaves the stream busy again: the host time shows it (a warmed-up
        # wrapper returns within a millisecond; one that waited needs what was left of the delay)
        assert host_ms < delay_ms()[1] / 4, f"{case.id}: the call waited for the device ({host_ms:.0f} ms on the host)"
    wrong = {(n, st) for n, st, _ in s.calls if st != side.cuda_stream}
    assert not wrong, f"{case.id}: library calls on another stream than the current one: {wrong}"
    assert len(got) == len(expected)
    for i, (g, w) in enumerate(zip(got, expected)):
        assert same_bits(g, w), f"{case.id}: result {i} differs from the default stream's"
    return s


def reach(case):
    s = stream_check(case)
    if case.symbol is not None:
        assert case.symbol in s.symbols(), (case.symbol, s.symbols())
    REACHED.update(s.symbols())


# ---- one case per entry point: the smallest row of tests/test_z_workspace_gpu.py, and the entry points without a workspace ----------
def _first(rows, op, tr):
    return next(c for c in rows if c[1] == op and c[0][0] == tr)


def stft_case():
    from phasegen import ops
    return Case("stft", {"y": cuda(detgen.normal(51, (2, 496)))}, lambda: {"out": sent(2, 2, 32, 32)},
                lambda i, o: [ops.stft(i["y"], 64, 16, out=o["out"])], symbol="pg_stft")


def stft_crops_case():
    from phasegen import ops
    begin = torch.tensor([0, 700], dtype=torch.int64, device=dev())
    end = torch.tensor([1000, 2000], dtype=torch.int64, device=dev())
    stats = ops.stats_tensor((0.1, 2.0), dev())
    return Case("stft_crops", {"src": cuda(detgen.normal(52, (2000,))), "begin": begin, "end": end, "stats": stats}, lambda: {"out": sent(2, 2, 32, 32)},
                lambda i, o: [ops.stft_crops(i["src"], i["begin"], i["end"], 496, 64, 16, polar=True, stats=i["stats"], out=o["out"])],
                symbol="pg_stft_crops", fixed=("stats",))


def polar_case():
    from phasegen import ops
    return Case("polar", {"d": cuda(detgen.normal(53, (2, 2, 16, 24)))}, lambda: {"out": sent(2, 2, 16, 24)},
                lambda i, o: [ops.polar(i["d"], out=o["out"])], symbol="pg_polar")


def resample_case():
    from phasegen import _lib, ops
    n_out = _lib.load().pg_resample_out_len(1000, 16000, 44100)
    return Case("resample", {"x": cuda(detgen.normal(54, (2, 1000)))}, lambda: {"out": sent(2, n_out)},
                lambda i, o: [ops.resample(i["x"], 44100, 16000, "kaiser_fast", out=o["out"])], symbol="pg_resample")


def spec_clips_case():
    from phasegen import ops
    return Case("spec_clips", {"plane": cuda(detgen.normal(55, (2, 5, 40)))}, lambda: {"out": sent(3, 2, 5, 12)},
                lambda i, o: [ops.spec_clips(i["plane"], 3, 12, 8, 1.3, out=o["out"])], symbol="pg_spec_clips")


def phase_join_case():
    from phasegen import ops
    return Case("phase_join", {"phi": cuda(detgen.uniform(56, (3, 2, 5, 12), -3.0, 3.0))}, lambda: {"out": sent(2, 5, 2 * 8 + 12)},
                lambda i, o: [ops.phase_join(i["phi"], 8, out=o["out"])], symbol="pg_phase_join")


def phase_vocoder_case():
    from phasegen import ops
    ins = {"A": cuda(detgen.uniform(57, (2, 5, 40), -3.0, 3.0)), "M": cuda(detgen.uniform(58, (2, 5, 40), 0.0, 1.0))}
    return Case("phase_vocoder", ins, lambda: {"out": sent(2, 5, 50)},
                lambda i, o: [ops.phase_vocoder(i["A"], 50, 0.7, logmag=i["M"], reset_below=0.5, out=o["out"])], symbol="pg_phase_vocoder")


BN_SHAPE = (3, 4, 6000)          # the three-pass shape of tests/test_z_norm_edges_gpu.py


def _bn_inputs():
    B, Cc, L = BN_SHAPE
    return {"x": cuda(detgen.normal(59, BN_SHAPE) * np.float32(2.0) + np.float32(0.3)), "gamma": cuda(detgen.uniform(60, (Cc,), 0.5, 1.5)),
            "beta": cuda(detgen.normal(61, (Cc,)))}


def bn_fwd_case():
    from phasegen import ops
    B, Cc, L = BN_SHAPE

    def run(i, o):
        ops.bn_fwd(i["x"], o["y"], i["gamma"], i["beta"], o["mean"], o["invstd"], o["rm"], o["rv"], num_batches_tracked=o["nbt"])
        return [o[k] for k in ("y", "mean", "invstd", "rm", "rv", "nbt")]

    return Case("bn_fwd", _bn_inputs(), lambda: {"y": sent(*BN_SHAPE), "mean": sent(Cc), "invstd": sent(Cc), "rm": torch.zeros(Cc, device=dev()),
                                                 "rv": torch.ones(Cc, device=dev()), "nbt": torch.zeros((), dtype=torch.int64, device=dev())},
                run, symbol="pg_bn_fwd")


def bn_bwd_case():
    from phasegen import ops
    B, Cc, L = BN_SHAPE
    ins = _bn_inputs()
    ins["mean"], ins["invstd"] = sent(Cc), sent(Cc)
    ops.bn_fwd(ins["x"], sent(*BN_SHAPE), ins["gamma"], ins["beta"], ins["mean"], ins["invstd"])
    ins["dy"] = cuda(detgen.normal(62, BN_SHAPE))
    del ins["beta"]

    def run(i, o):
        ops.bn_bwd(i["x"], i["dy"], o["dx"], i["gamma"], i["mean"], i["invstd"], o["dgamma"], o["dbeta"])
        return [o["dx"], o["dgamma"], o["dbeta"]]

    return Case("bn_bwd", ins, lambda: {"dx": sent(*BN_SHAPE), "dgamma": sent(Cc), "dbeta": sent(Cc)}, run, symbol="pg_bn_bwd")


def adam_case():
    from phasegen import ops
    n = 100003
    p0, m0, v0 = cuda(detgen.normal(63, (n,))), cuda(detgen.normal(64, (n,)) * np.float32(0.01)), cuda(np.abs(detgen.normal(65, (n,))) * np.float32(1e-4))

    def run(i, o):
        ops.adam_step(o["p"], i["g"], o["m"], o["v"], 3)
        return [o["p"], o["m"], o["v"]]

    return Case("adam_step", {"g": cuda(detgen.normal(66, (n,)))}, lambda: {"p": p0.clone(), "m": m0.clone(), "v": v0.clone()}, run, symbol="pg_adam_step")


def cast_case():
    from phasegen import ops
    return Case("cast_rows_bf16", {"x": cuda(detgen.normal(67, (2, 4, 30)))}, lambda: {"out": ops.h_alloc(2, 4, 30, dev())},
                lambda i, o: [ops.cast_rows_bf16(i["x"], o["out"], act=ops.ACT_LEAKY)], symbol="pg_cast_rows_bf16")


def shadow_case():
    from phasegen import ops
    return Case("shadow_weights", {"w": cuda(detgen.normal(68, (32, 16, 8)))}, dict, lambda i, o: [ops.shadow_weights(i["w"], True, 2)],
                symbol="pg_shadow_weights")


def fill_case():
    from phasegen import ops
    return Case("fill", {}, lambda: {"t": sent(100003)}, lambda i, o: [ops.fill(o["t"], 1.25)], symbol="pg_fill")


def frame_index_case():
    from phasegen import ops
    return Case("stft_frame_index", {}, dict, lambda i, o: [ops.stft_frame_index(496, 64, 16, dev())], symbol="pg_stft_frame_index")


def gl_project_case():
    from phasegen import ops
    ins = {"S": cuda(detgen.normal(69, (2, 2, 17, 33))), "mag": cuda(np.abs(detgen.normal(70, (2, 17, 33))))}

    def run(i, o):
        ops.gl_project(i["S"], i["mag"], o["x"], o["spec"])
        return [o["x"], o["spec"]]

    return Case("gl_project", ins, lambda: {"x": sent(2, 32, 33), "spec": sent(2, 2, 17, 33)}, run, symbol="pg_gl_project")


CASES = {
    "conv1d_fwd": lambda: W.conv_case(_first(FIXUP_CASES, "fwd", False)),
    "conv1d_dgrad": lambda: W.conv_case(_first(FIXUP_CASES, "dgrad", False)),
    "conv1d_wgrad": lambda: W.conv_case(_first(W.PACKED_WGRADS, "wgrad", False)),
    "convt1d_fwd": lambda: W.conv_case(_first(FIXUP_CASES, "fwd", True)),
    "convt1d_dgrad": lambda: W.conv_case(_first(FIXUP_CASES, "dgrad", True)),
    "convt1d_wgrad": lambda: W.conv_case(_first(W.PACKED_WGRADS, "wgrad", True), adam=True),
    "conv_tail_launch": lambda: W.conv_case(next(c for c in VIEW_CASES if c[5] == "tail")),
    "conv_fwd_h": lambda: W.convh_case(FIXUP_CASES_H[0][0], 2),
    "loss_fwd_bwd": lambda: W.loss_case(1, 8, 24),
    "moments_standardize": lambda: W.moments_case(5, False),
    "istft_three_kernels": lambda: W.istft_case(16, 8, 5, 1, 1, True, False),
    "istft_fused_with_seam": lambda: W.istft_case(512, 256, 9, 2, 0, True, False),
    "ola_nt": lambda: W.ola_case(0, True),
    "stitch": lambda: W.stitch_case(W._stitch_shapes()[0], True, True),
    "phase_lock": lambda: W.lock_case(33, 5),
    "wave_compare": lambda: W.wave_case(1, 1),
    "spec_compare": lambda: W.spec_case(1, 1, 1),
    "stft": stft_case, "stft_crops": stft_crops_case, "polar": polar_case, "resample": resample_case, "spec_clips": spec_clips_case,
    "phase_join": phase_join_case, "phase_vocoder": phase_vocoder_case, "bn_fwd": bn_fwd_case, "bn_bwd": bn_bwd_case, "adam_step": adam_case,
    "cast_rows_bf16": cast_case, "shadow_weights": shadow_case, "fill": fill_case, "stft_frame_index": frame_index_case, "gl_project": gl_project_case,
}


@pytest.mark.parametrize("name", list(CASES))
def test_runs_on_the_stream_passed_in_and_does_not_wait(name):
    reach(CASES[name]())


def test_clipnorm_runs_on_the_stream_passed_in_and_does_not_wait():
    """pg_clipnorm_fwd's workspace is an argument of the wrapper: the strict view goes in directly"""
    case = W.clipnorm_case(1, 8, 24, poison=0xFF)
    made = []

    def make_outs():
        made.append(case.make_outs())
        return made[-1]

    s = stream_check(Case("clipnorm_fwd", case.ins, make_outs, case.run, symbol="pg_clipnorm_fwd"))
    for o in made:
        o["guard"].check()
    assert "pg_clipnorm_fwd" in s.symbols()
    REACHED.update(s.symbols())


def test_zz_every_stream_entry_point_was_reached_by_a_passing_case():
    missing = sorted(set(stream_symbols()) - REACHED)
    assert not missing, missing


# ---- the helper catches what it is there to catch (stand-in kernels made of torch ops; every write lands in the helper's own buffers) ----
def _buffer_of(guard):
    (buf, start, need), = guard.held
    return buf, start, need


def test_helper_catches_a_byte_behind_and_a_byte_in_front_of_the_view():
    for where, word in ((lambda start, need: start + need, "behind"), (lambda start, need: start - 1, "in front of")):
        for poison in (0xFF, 0x7F, 0x00):
            guard, view = strict_view(poison, 1000)
            buf, start, need = _buffer_of(guard)
            assert need == 1000 and view.numel() == 1000 and view.data_ptr() % 256 == 0 and start >= 4096 and buf.numel() - start - need >= 64 << 10
            buf[where(start, need)] = poison ^ 0x01
            with pytest.raises(AssertionError, match=word):
                guard.check()
    guard, view = strict_view(0xFF, 1000)
    view.fill_(3)                                             # every byte of the view itself may be written
    guard.check()
    assert bool((guard.contents[0] == 3).all())


def _stand_in_fold(fold, poison, slots=8, written=7):
    """stage 1 writes `written` of `slots` float partials into a strict view, stage 2 folds all `slots`"""
    guard, view = strict_view(poison, 4 * slots)
    part = view.view(torch.float32)
    values = torch.arange(1, written + 1, device=dev(), dtype=torch.float32)
    part[:written] = values
    got = fold(part)
    guard.check()
    return got, fold(values)


def _fmax_fold(t):
    return functools.reduce(torch.fmax, t.unbind())          # fmaxf: a NaN operand is dropped


def test_helper_needs_the_second_poison_for_a_maximum():
    got, want = _stand_in_fold(_fmax_fold, 0xFF)
    assert same_bits(got, want)                               # MISSED under the NaN poison: the reason for 0x7F
    got, want = _stand_in_fold(_fmax_fold, 0x7F)
    assert not same_bits(got, want) and float(got) > 3e38     # caught
    got, want = _stand_in_fold(_fmax_fold, 0x7F, written=8)
    assert same_bits(got, want)                               # (and a fold over written slots only passes)


def test_helper_catches_a_sum_over_an_unwritten_slot():
    got, want = _stand_in_fold(torch.sum, 0xFF)
    assert not same_bits(got, want) and bool(torch.isnan(got))
    got, want = _stand_in_fold(torch.sum, 0xFF, written=8)
    assert same_bits(got, want)


def _two_stage(second_stream=None, sync=None):
    """a stand-in entry point of two stages: tmp = 2 x, then out = tmp + 1 -- the second on `second_stream` (None: the current one);
    sync: torch.cuda.synchronize() between the stages ("middle") or behind them ("end")"""
    def run(i, o):
        torch.mul(i["x"], 2.0, out=o["tmp"])
        if sync == "middle":
            torch.cuda.synchronize()
        with torch.cuda.stream(second_stream or torch.cuda.current_stream()):
            torch.add(o["tmp"], 1.0, out=o["out"])
        if sync == "end":
            torch.cuda.synchronize()
        return [o["out"]]

    return Case("stand-in", {"x": cuda(detgen.normal(71, (1000,)))}, lambda: {"tmp": sent(1000), "out": sent(1000)}, run, needs_ws=False)


def test_helper_catches_a_stage_on_the_default_stream_and_a_synchronise():
    stream_check(_two_stage())                                # a correct stand-in passes
    with pytest.raises(AssertionError, match="differs from the default stream's"):
        stream_check(_two_stage(second_stream=torch.cuda.default_stream()), warm_side=False)
    with pytest.raises(AssertionError, match="the side stream was idle when the wrapper returned"):
        stream_check(_two_stage(sync="end"), warm_side=False)
    with pytest.raises(AssertionError, match="waited for the device"):   # (the stream may be busy again with the second stage: then the host time shows it)
        stream_check(_two_stage(sync="middle"), warm_side=False)
