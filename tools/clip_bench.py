#!/usr/bin/env python3
"""Inference over many clips with per-clip BatchNorm statistics (the reference's semantics, demo.py:33-45): clips/s of
  (a) the loop of batch-of-one forwards (the only way to get these values before stats="clip"), and
  (b) ONE forward over the B clips with stats="clip",
at the full width (C = 1024), 128 and 256 frames, B in {8, 32, 64}, on the fp32 engine and on the bf16-resident one with HIP graphs
off and on -- both legs in the same process on the same inputs --, plus the six pg_clipnorm_fwd launches of one forward alone beside
the six pg_bn_fwd launches at the same shapes and output wiring (time and GB/s of the algorithmic bytes: one read, one or two fp32
writes; 4 rotating buffer sets).  HIP events around every repetition, medians.  Prints a markdown table (DESIGN.md section 4.6
holds a copy); --out writes it to a file as well."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-phasegen_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from phasegen import ops  # noqa: E402
from phasegen.model import UNetModel  # noqa: E402
from phasegen.unet import frame_plan  # noqa: E402


def median_ms(fn, warmup, budget_s, min_reps=5, max_reps=200):
    """Median HIP-event time of fn() in ms: `warmup` calls, then repetitions until `budget_s` seconds of device time are covered."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    while len(times) < min_reps or (sum(times) < budget_s * 1e3 and len(times) < max_reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), len(times)


def forward_rows(C, frames, batches, budget):
    rows = []
    engines = [("fp32", UNetModel(C, 2 * C, precision="fp32").engine, False)]
    bf = UNetModel(C, 2 * C, precision="bf16").engine
    engines += [("bf16-resident", bf, False), ("bf16-resident + graphs", bf, True)]
    for L in frames:
        for B in batches:
            x = torch.randn(B, C, L, device="cuda")
            for label, eng, graphs in engines:
                eng.graphs = graphs

                def loop():
                    for b in range(B):
                        eng.forward(x[b:b + 1], inference=True)

                def batched():
                    eng.forward(x, inference=True, stats="clip")
                t_loop, n_loop = median_ms(loop, 3, budget)            # (3 warm-ups: eager, graph capture, first replay)
                t_clip, n_clip = median_ms(batched, 3, budget)
                eng.graphs = False
                rows.append((label, L, B, t_loop, t_clip, n_loop, n_clip))
                print(f"# {label:24s} L={L} B={B}: loop {t_loop:8.3f} ms ({n_loop} reps), per-clip batched {t_clip:8.3f} ms ({n_clip} reps)", flush=True)
    return rows


def norm_rows(C, frames, batches, budget):
    """The six BatchNorm launches of one forward (fp32-tensor wiring: D1 / D2 store a second activated copy), per-clip and batch."""
    rows = []
    h = 2 * C
    for L in frames:
        L1, L2, L3, _ = frame_plan(L)
        layers = [(L2, True), (L3, True), (L3, False), (L2, False), (L1, False), (L, False)]      # D1 D2 U3 U2 U1 U0
        for B in batches:
            g, be = torch.ones(h, device="cuda"), torch.zeros(h, device="cuda")
            sm, si = torch.empty(h, device="cuda"), torch.empty(h, device="cuda")
            rm, rv = torch.zeros(h, device="cuda"), torch.ones(h, device="cuda")
            nb = torch.zeros((), device="cuda", dtype=torch.long)
            ws = torch.empty(2 * B * h, device="cuda")
            sets = []
            for _ in range(4):
                sets.append([(torch.randn(B, h, l, device="cuda"), torch.empty(B, h, l, device="cuda"),
                              torch.empty(B, h, l, device="cuda") if two else None) for l, two in layers])
            nbytes = sum(4 * B * h * l * (3 if two else 2) for l, two in layers)
            state = {"i": 0}

            def clip():
                state["i"] += 1
                for x, y, y2 in sets[state["i"] % 4]:
                    ops.clipnorm_fwd(x, y, g, be, None, None, rm, rv, y_act=ops.ACT_RELU, y2=y2, y2_act=ops.ACT_LEAKY,
                                     num_batches_tracked=nb, workspace=ws)

            def batch():
                state["i"] += 1
                for x, y, y2 in sets[state["i"] % 4]:
                    ops.bn_fwd(x, y, g, be, sm, si, rm, rv, y_act=ops.ACT_RELU, y2=y2, y2_act=ops.ACT_LEAKY, num_batches_tracked=nb)
            t_clip, _ = median_ms(clip, 8, budget, min_reps=20)
            t_bn, _ = median_ms(batch, 8, budget, min_reps=20)
            rows.append((L, B, t_clip, t_bn, nbytes))
            print(f"# six norm launches L={L} B={B}: clipnorm {t_clip * 1e3:7.1f} us, bn_fwd {t_bn * 1e3:7.1f} us, {nbytes / 1e6:.0f} MB", flush=True)
            del sets
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--budget", type=float, default=0.3, help="seconds of device time per measurement")
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--out", help="also write the markdown tables to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_bench: needs the GPU (nothing here can be measured on a CPU)")
    torch.manual_seed(0)
    lines = []
    if not args.skip_forward:
        lines += ["| engine | frames | B | loop of batch-of-one forwards: ms (clips/s) | one per-clip forward: ms (clips/s) | speed-up |", "|---|---|---|---|---|---|"]
        for label, L, B, t_loop, t_clip, _, _ in forward_rows(args.width, args.frames, args.batches, args.budget):
            lines.append(f"| {label} | {L} | {B} | {t_loop:.2f} ({B / t_loop * 1e3:.0f}) | {t_clip:.2f} ({B / t_clip * 1e3:.0f}) | {t_loop / t_clip:.2f}x |")
        lines.append("")
    lines += ["| frames | B | six `clipnorm` launches: us (GB/s) | six `bn_fwd` launches: us (GB/s) | ratio |", "|---|---|---|---|---|"]
    for L, B, t_clip, t_bn, nbytes in norm_rows(args.width, args.frames, args.batches, args.budget):
        lines.append(f"| {L} | {B} | {t_clip * 1e3:.1f} ({nbytes / t_clip / 1e6:.0f}) | {t_bn * 1e3:.1f} ({nbytes / t_bn / 1e6:.0f}) | {t_clip / t_bn:.2f} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
