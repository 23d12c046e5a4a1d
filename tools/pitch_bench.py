#!/usr/bin/env python3
"""Pitch detection (phasegen.ops.pitch_track, phasegen.track.detect_pitch / autotune), measured in ONE process over alternating rounds
on the 3-minute stereo track of the other track benches:

  * pg_pitch_track at window 1024, lags 16 .. 320, hop 256 on both channels (the complete frames) beside the VALU bound of its
    contract: 3 W tau_max frames n_sig float operations (one subtraction, one multiplication, one addition per sample and lag; the
    contract forbids fusing them) at the device's fp32 vector rate, 157.3 TFLOP/s, and the fraction of that rate reached;
  * pg_varispeed on the plan of a +-0.5 semitone, 5 Hz vibrato in the same process: the other kernel of a pitch correction;
  * the whole ``track.autotune`` (locked vocoder, n_fft 2048 / hop 512) beside ``track.pitch_shift`` with the very curve it found
    passed in, and ``track.detect_pitch`` with ``PitchCurve.correcting`` alone: what the detection, the copy to the host and the host
    curve cost.

HIP events around every repetition; every time is the median over the rounds with min..max.  Prints markdown (DESIGN.md section 4.21
holds a copy); --out writes it to a file as well."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vocoder_bench import fmt, make_audio, time_ms  # noqa: E402  (puts the package and tests/ on the path)

import torch  # noqa: E402

from phasegen import ops, track  # noqa: E402

PEAK_FP32_VECTOR_TFLOPS = 157.3      # 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz: the figure bench.py --full holds the fp32 kernels against


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pitch_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 7:
        sys.exit("pitch_bench: at least 7 rounds")
    n_ch, W, hop, tau_min, tau_max = 2, 1024, 256, 16, 320
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    frames = ops.pitch_frames(a_len, hop, W, tau_max)
    period, apz = torch.empty(n_ch, frames, device="cuda"), torch.empty(n_ch, frames, device="cuda")
    vib = track.PitchCurve.vibrato(args.seconds, 0.5, 5.0)
    plan = vib.plan(a_len, args.sr)
    n_mid = int(round(plan.time_map.out_of_src(a_len, args.sr)))
    mid = make_audio((n_mid + 1) / args.sr, args.sr, n_ch, seed=1)[:, :n_mid]
    pos, scale = torch.from_numpy(plan.pos).cuda(), torch.from_numpy(plan.scale).cuda()
    y = torch.empty(n_ch, a_len, device="cuda")
    runs = {
        "pitch_track": lambda: ops.pitch_track(audio, frames, hop, W, tau_min, tau_max, 0.15, out=(period, apz)),
        "varispeed vibrato": lambda: ops.varispeed(mid, pos, scale, a_len, step=plan.step, out=y),
    }
    kw = dict(phase="vocoder_locked", n_fft=2048, hop_length=512)
    _out, pt, curve = track.autotune(None, audio, return_curve=True, **kw)

    def detect_and_correct():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        track.PitchCurve.correcting(track.detect_pitch(audio, args.sr), retune_ms=50.0)
        return (time.perf_counter() - t0) * 1e3

    whole = {
        "autotune": lambda: track.autotune(None, audio, **kw),
        "pitch_shift(the curve autotune found)": lambda: track.pitch_shift(None, audio, curve, **kw),
    }
    for fn in list(runs.values()) + list(whole.values()):                 # warm-up: tables, workspaces, allocator
        fn()
        fn()
    times = {k: [] for k in list(runs) + list(whole) + ["detect_pitch + correcting (host clock)"]}
    order = list(runs)
    for r in range(args.rounds):
        # every block begins with one call that is not timed (tools/map_bench.py); the order rotates from round to round
        for key in order[r % len(order):] + order[:r % len(order)]:
            runs[key]()
            times[key].append(time_ms(runs[key], inner=5))
        for key, fn in whole.items():
            times[key].append(time_ms(fn))
        times["detect_pitch + correcting (host clock)"].append(detect_and_correct())
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in times.items()) + " ms", flush=True)

    ops_count = 3.0 * W * tau_max * frames * n_ch
    bound_us = ops_count / (PEAK_FP32_VECTOR_TFLOPS * 1e12) * 1e6
    frac = [bound_us / (t * 1e3) for t in times["pitch_track"]]
    rel = [a / b for a, b in zip(times["pitch_track"], times["varispeed vibrato"])]
    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz ({a_len} samples per channel, {frames} frames per channel); window {W}, "
             f"lags {tau_min} .. {tau_max}, hop {hop}; {torch.cuda.get_device_name(0)}; {args.rounds} rounds of 5 calls (whole calls: 1), "
             f"median (min..max); {int(pt.voiced.sum())} of {pt.voiced.shape[0]} frames voiced", "",
             "| kernel | work | time, us | VALU bound at 157.3 TFLOP/s, us | fraction of the vector rate | against pg_varispeed |", "|---|---|---|---|---|---|",
             f"| `pg_pitch_track` | {ops_count / 1e9:.2f} G float operations | {fmt(times['pitch_track'], 1e3, 1)} | {bound_us:.1f} | {fmt(frac, 1.0, 3)} | {fmt(rel, 1.0, 2)} |",
             f"| `pg_varispeed` vibrato | {4 * n_ch * a_len / 1e6:.1f} MB out | {fmt(times['varispeed vibrato'], 1e3, 1)} | | | 1 |",
             "", "| whole call, 2048 / 512, locked vocoder | time, ms | against pitch_shift with the curve passed in |", "|---|---|---|"]
    base = times["pitch_shift(the curve autotune found)"]
    for key in list(whole) + ["detect_pitch + correcting (host clock)"]:
        ratio = [a / b for a, b in zip(times[key], base)]
        lines.append(f"| `{key}` | {fmt(times[key], 1.0, 1)} | {fmt(ratio, 1.0, 2)} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
