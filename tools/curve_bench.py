#!/usr/bin/env python3
"""Pitch curves (phasegen.track.PitchCurve, phasegen.ops.varispeed) beside the uniform pitch shift they generalise, measured in ONE
process over alternating rounds on the 3-minute stereo track of the other track benches:

  * pg_varispeed on the plan of a constant +4 semitone curve beside pg_resample at ``pitch_ratio(4)``'s fraction on the same input
    (the stretched track: both bring it back to the input's length); pg_resample is the yardstick;
  * pg_varispeed on the plan of a +-0.5 semitone, 5 Hz vibrato;
  * with --parent-lib pg_resample of another build of the library (the parent commit's) on the same arguments, outputs compared
    bit for bit: this build's pg_resample keeps its bits, and its time when its median lies within the spread the parent's rounds
    show in the same run;
  * the whole ``track.pitch_shift`` (locked vocoder, n_fft 2048 / hop 512) with the constant curve and with the vibrato beside the
    uniform call at +4 semitones.

HIP events around every repetition; every time is the median over the rounds with min..max.  Prints markdown (DESIGN.md section 4.20
holds a copy); --out writes it to a file as well."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vocoder_bench import fmt, make_audio, time_ms  # noqa: E402  (puts the package and tests/ on the path)
from map_bench import captured, parent_call  # noqa: E402

import torch  # noqa: E402

from phasegen import ops, track  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--semitones", type=float, default=4.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="also time pg_resample of this build of the library (e.g. the parent commit's)")
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("curve_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("curve_bench: at least 5 rounds")
    n_ch, st = 2, args.semitones
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    stretch, ratio = track.pitch_ratio(st)
    curves = {"constant": track.PitchCurve([(0, st), (1, st)]), "vibrato": track.PitchCurve.vibrato(args.seconds, 0.5, 5.0)}
    plans = {k: c.plan(a_len, args.sr) for k, c in curves.items()}
    n_mid = {k: int(round(p.time_map.out_of_src(a_len, args.sr))) for k, p in plans.items()}
    mid = make_audio((max(n_mid.values()) + 1) / args.sr, args.sr, n_ch, seed=1)           # stands for the stretched track
    tables = {k: (torch.from_numpy(p.pos).cuda(), torch.from_numpy(p.scale).cuda()) for k, p in plans.items()}
    y = torch.empty(n_ch, a_len, device="cuda")
    x_const = mid[:, :n_mid["constant"]]
    n_rs = ops._lib.load().pg_resample_out_len(x_const.shape[1], ratio.denominator, ratio.numerator)
    y_rs = torch.empty(n_ch, n_rs, device="cuda")

    runs = {
        "resample": lambda: ops.resample(x_const, ratio.numerator, ratio.denominator, out=y_rs),
        "varispeed constant": lambda: ops.varispeed(x_const, *tables["constant"], a_len, step=plans["constant"].step, out=y),
        "varispeed vibrato": lambda: ops.varispeed(mid[:, :n_mid["vibrato"]], *tables["vibrato"], a_len, step=plans["vibrato"].step, out=y),
    }
    same = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        a = captured("pg_resample", runs["resample"])
        mine = y_rs.clone()
        runs["resample (parent)"] = parent_call(parent, "pg_resample", a)
        y_rs.fill_(-77.0)
        runs["resample (parent)"]()
        same = bool(torch.equal(mine.view(torch.int32), y_rs.view(torch.int32)))
    kw = dict(phase="vocoder_locked", n_fft=2048, hop_length=512)
    whole = {
        f"pitch_shift(+{st:g})": lambda: track.pitch_shift(None, audio, st, **kw),
        f"pitch_shift(constant +{st:g} curve)": lambda: track.pitch_shift(None, audio, curves["constant"], **kw),
        "pitch_shift(vibrato curve)": lambda: track.pitch_shift(None, audio, curves["vibrato"], **kw),
    }
    for fn in list(runs.values()) + list(whole.values()):                 # warm-up: tables, banks, workspaces, allocator
        fn()
        fn()
    times = {k: [] for k in list(runs) + list(whole)}
    order = list(runs)
    for r in range(args.rounds):
        # every block begins with one call that is not timed (tools/map_bench.py); the order rotates from round to round
        for key in order[r % len(order):] + order[:r % len(order)]:
            runs[key]()
            times[key].append(time_ms(runs[key], inner=10))
        for key, fn in whole.items():
            times[key].append(time_ms(fn))
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in times.items()) + " ms", flush=True)

    med = lambda v: sorted(v)[len(v) // 2]
    MB = lambda n: 4 * n / 1e6
    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz ({a_len} samples per channel); +{st:g} semitones = stretch {stretch:.4f}, "
             f"pg_resample by {ratio.denominator} / {ratio.numerator}; {torch.cuda.get_device_name(0)}; {args.rounds} rounds of 10 calls "
             "(whole calls: 1), median (min..max)", "",
             "| kernel | input | output | time, us | against pg_resample |", "|---|---|---|---|---|"]
    for key, n_in, n_out in (("resample", x_const.shape[1], n_rs), ("varispeed constant", n_mid["constant"], a_len), ("varispeed vibrato", n_mid["vibrato"], a_len)):
        rel = [b / a for a, b in zip(times["resample"], times[key])]
        lines.append(f"| `pg_{key.split()[0]}`{' ' + key.split()[1] if ' ' in key else ''} | {MB(n_ch * n_in):.1f} MB | {MB(n_ch * n_out):.1f} MB | {fmt(times[key], 1e3, 1)} | {fmt(rel, 1.0, 2)} |")
    if args.parent_lib:
        p, u = times["resample (parent)"], times["resample"]
        lines.append(f"| `pg_resample` of the other build | | | {fmt(p, 1e3, 1)} | bits {'equal' if same else 'DIFFER'}; this build's median "
                     f"{'within' if med(u) <= max(p) else 'OUTSIDE'} its spread ({med(u) / med(p):.3f} of its median) |")
    lines += ["", "| whole call, 2048 / 512, locked vocoder | time, ms | against the uniform call |", "|---|---|---|"]
    first = next(iter(whole))
    for key in whole:
        rel = [b / a for a, b in zip(times[first], times[key])]
        lines.append(f"| `{key}` | {fmt(times[key], 1.0, 1)} | {fmt(rel, 1.0, 2)} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
