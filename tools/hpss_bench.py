#!/usr/bin/env python3
"""The transient-preserving stretch (phasegen.ops.hpss, phasegen.ops.ola_stretch, phasegen.track transients="ola") measured in ONE
process over alternating rounds, on the track of tools/lock_bench.py (3-minute stereo at n_fft 2048 / hop 512, stretch 1.5):

  * pg_hpss at 17 x 17 on the track's log-magnitude planes (read in place from the polar tensor) and pg_ola_stretch at 256 / 64 on
    the source-grid signal with a ``base``: microseconds, the algorithmic bytes (pg_hpss reads one plane and writes two;
    pg_ola_stretch reads x and base and writes y), bytes per second, and each kernel's bound -- the larger of the bytes over 8 TB/s
    and the operations over the vector rate (pg_hpss: two integer operations per comparator of its two selection networks, 70
    comparators each at 17 inputs, at 78.6 T lane-operations/s; pg_ola_stretch: 4 frames x (multiply, two adds) and a division);
  * the whole ``reconstruct_track(..., phase="vocoder_locked", join="spectral", stretch=1.5)`` with and without transients="ola";
  * the crest of the five bursts of tests/_transient_ref.py's clicky melody on the device at stretch 1.5 and 0.75, without and with
    the option (the float64 figures are in tests/test_transient_host.py).

HIP events around every repetition; every time is the median over the rounds with min..max.  Prints markdown (DESIGN.md section 4.15
holds a copy); --out writes it to a file as well."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vocoder_bench import STATS, fmt, make_audio, time_ms  # noqa: E402  (puts the package and tests/ on the path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _transient_ref  # noqa: E402
from phasegen import ops, track  # noqa: E402

PEAK_BYTES = 8.0e12                       # HBM3E, bytes per second
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9      # CUs x SIMDs x lanes per clock x clock: 78.6 T vector lane-operations per second
COMPARATORS_17 = 70                       # csrc/transient.hip: the pruned selection network of 17 inputs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--stretch", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hpss_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("hpss_bench: at least 5 rounds")
    bins, hop, frames, ov, stretch, n_ch = args.width, args.width // 2, args.frames, args.overlap_frames, args.stretch, 2
    n_fft, spo = 2 * bins, 1.0 / args.stretch
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    pl = track.spectral_plan(a_len, frames, hop, ov, stretch)

    # the kernels alone, on what the pipeline hands them
    begin = torch.arange(n_ch, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(audio.reshape(-1), begin, begin + a_len, pl.n_src, n_fft, hop, polar=True, stats=STATS)
    harm, perc = torch.empty(n_ch, bins, pl.F_src, device="cuda"), torch.empty(n_ch, bins, pl.F_src, device="cuda")
    ops.hpss(pol[:, 0], *track.HPSS_WIN, out=(harm, perc))
    share = float((perc != 0).float().mean())
    p_audio = ops.istft(perc, pol[:, 1], hop, mode=0, normalize=False)
    n_out = hop * (pl.F_out - 1)
    base, y = torch.randn(n_ch, n_out, device="cuda"), torch.empty(n_ch, n_out, device="cuda")
    kw = dict(n_fft=n_fft, hop_length=hop, frames=frames, overlap_frames=ov, stats=STATS, phase="vocoder_locked", join="spectral", stretch=stretch)
    runs = {"hpss": lambda: ops.hpss(pol[:, 0], *track.HPSS_WIN, out=(harm, perc)),
            "ola": lambda: ops.ola_stretch(p_audio, n_out, spo, track.TRANSIENT_WINDOW, track.TRANSIENT_HOP, base=base, out=y),
            "track": lambda: track.reconstruct_track(None, audio, **kw),
            "track+ola": lambda: track.reconstruct_track(None, audio, transients="ola", **kw)}
    inner = {"hpss": 10, "ola": 10, "track": 3, "track+ola": 3}
    for fn in runs.values():                                              # warm-up: workspaces, allocator, tables
        fn()
        fn()
    times = {k: [] for k in runs}
    for r in range(args.rounds):
        for name in runs:
            times[name].append(time_ms(runs[name], inner=inner[name]))
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in times.items()), flush=True)

    x, at = _transient_ref.clicky_melody()
    crest = []
    for s in (1.5, 0.75):
        q = dict(phase="vocoder_locked", join="spectral", stretch=s, normalize=False)
        crest.append((s, _transient_ref.crests(track.reconstruct_track(None, x, **q).cpu().numpy(), at, s),
                      _transient_ref.crests(track.reconstruct_track(None, x, transients="ola", **q).cpu().numpy(), at, s)))

    cells = n_ch * bins * pl.F_src
    hp_bytes, hp_ops = 12.0 * cells, 2.0 * 2 * COMPARATORS_17 * cells
    ol_bytes, ol_ops = 4.0 * (p_audio.numel() + 2 * y.numel()), (4 * 3 + 2) * float(y.numel())
    med = lambda k: float(np.median(times[k])) * 1e-3

    def row(name, key, nbytes, nops):
        t_b, t_o = nbytes / PEAK_BYTES, nops / PEAK_LANE_OPS
        bound, which = (t_b, "bytes") if t_b >= t_o else (t_o, "vector operations")
        return (f"| `{name}` | {nbytes / 1e6:.1f} MB | {nops / 1e9:.2f} G | {fmt(times[key], 1e3, 1)} | {nbytes / med(key) / 1e12:.2f} TB/s | "
                f"{bound * 1e6:.1f} us ({which}) | {100 * bound / med(key):.0f} % |")

    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}, stretch {stretch:g}: F_src {pl.F_src}, F_out {pl.F_out}, "
             f"{cells / 1e6:.1f} M cells, {100 * share:.0f} % of them percussive; {n_out} output samples per channel; "
             f"{torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min..max)", "",
             "| kernel | algorithmic bytes | lane operations | us | bytes per second | bound | share of the bound |", "|---|---|---|---|---|---|---|",
             row(f"pg_hpss {track.HPSS_WIN[0]} x {track.HPSS_WIN[1]}", "hpss", hp_bytes, hp_ops),
             row(f"pg_ola_stretch {track.TRANSIENT_WINDOW} / {track.TRANSIENT_HOP}", "ola", ol_bytes, ol_ops), "",
             "| whole call, phase=\"vocoder_locked\" | ms |", "|---|---|",
             f"| `reconstruct_track(..., stretch={stretch:g})` | {fmt(times['track'], 1.0, 3)} |",
             f"| ... with `transients=\"ola\"` | {fmt(times['track+ola'], 1.0, 3)} |",
             f"| difference | {fmt([b - a for a, b in zip(times['track'], times['track+ola'])], 1.0, 3)} |", "",
             "| clicky melody (6 s, 16 kHz), 2048 / 512, crest of the five bursts (median) | whole plane | split |", "|---|---|---|"]
    lines += [f"| stretch {s:g} | {', '.join(f'{c:.2f}' for c in a)} ({np.median(a):.2f}) | {', '.join(f'{c:.2f}' for c in b)} ({np.median(b):.2f}) |" for s, a, b in crest]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
