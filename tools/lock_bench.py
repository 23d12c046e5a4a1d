#!/usr/bin/env python3
"""Identity phase locking (phasegen.track, phase="vocoder_locked") beside the plain vocoder, measured in ONE process over alternating
rounds on the track of tools/vocoder_bench.py (3-minute stereo at n_fft 2048 / hop 512, stretch 1.5):

  * pg_phase_lock (its three launches together: compose, carry, apply) beside pg_phase_vocoder on the same planes;
  * the whole ``reconstruct_track(join="spectral", stretch=1.5)`` at phase="vocoder_locked" beside phase="vocoder";
  * the four-floor table for both phases: spectrogram consistency (``track.evaluate_stretch``) of the synthetic melody of
    tests/_vocoder_ref.py at stretch 1.5 with the track's own moments, for reset_below in {0, 0.01, 0.05, 0.2}, and for phase="zero".

HIP events around every repetition; every figure is the median over the rounds with min..max.  Prints markdown (DESIGN.md section
4.12 holds a copy); --out writes it to a file as well.  (The split of the kernel time over the three launches is a kernel trace's
business: ``rocprofv3 --kernel-trace --stats -- python tools/lock_bench.py``.)"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vocoder_bench import FLOORS, STATS, fmt, make_audio, time_ms  # noqa: E402  (puts the package and tests/ on the path)

import torch  # noqa: E402

import _vocoder_ref  # noqa: E402
from phasegen import _lib, ops, track  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--stretch", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lock_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("lock_bench: at least 5 rounds")
    bins, hop, frames, ov, n_ch, stretch = args.width, args.width // 2, args.frames, args.overlap_frames, args.channels, args.stretch
    n_fft = 2 * bins
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    pl = track.spectral_plan(a_len, frames, hop, ov, stretch)
    kw = dict(n_fft=n_fft, hop_length=hop, frames=frames, overlap_frames=ov, stats=STATS, sr=args.sr, normalize=False, join="spectral", stretch=stretch)

    # the kernels alone, on the planes the pipeline hands them
    begin = torch.arange(n_ch, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(audio.reshape(-1), begin, begin + a_len, pl.n_src, n_fft, hop, polar=True, stats=STATS)
    out = torch.empty(n_ch, bins, pl.F_out, device="cuda")
    plane_bytes = 4 * (2 * n_ch * bins * pl.F_src + out.numel())
    q = _lib.PhaseLockArgs()
    q.n_ch, q.bins, q.F_out = n_ch, bins, pl.F_out
    ws_bytes = _lib.load().pg_workspace_bytes_phase_lock(ctypes.byref(q))
    floor = track.VOCODER_RESET_BELOW
    runs = {"lock": lambda: ops.phase_lock(pol[:, 1], pl.F_out, 1.0 / stretch, logmag=pol[:, 0], reset_below=floor, out=out),
            "plain": lambda: ops.phase_vocoder(pol[:, 1], pl.F_out, 1.0 / stretch, logmag=pol[:, 0], reset_below=floor, out=out),
            "vocoder_locked": lambda: track.reconstruct_track(None, audio, phase="vocoder_locked", **kw),
            "vocoder": lambda: track.reconstruct_track(None, audio, phase="vocoder", **kw)}
    for fn in runs.values():                                              # warm-up: workspaces, allocator
        fn()
        fn()
    times = {k: [] for k in runs}
    for r in range(args.rounds):
        for name in ("lock", "plain"):
            times[name].append(time_ms(runs[name], inner=10))
        for name in ("vocoder_locked", "vocoder"):
            times[name].append(time_ms(runs[name]))
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in times.items()), flush=True)

    # the floor table on the melody, the track's own moments
    melody = _vocoder_ref.melody()
    table = []
    for fl in FLOORS:
        rep = track.evaluate_stretch(None, melody, 1.5, phases=("vocoder_locked", "vocoder", "zero"), reset_below=fl)
        table.append((fl, rep["metrics"]))
    zero = table[0][1]["zero"]

    ratio = [a / b for a, b in zip(times["lock"], times["plain"])]
    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}, stretch {stretch:g}: F_src {pl.F_src}, F_out {pl.F_out}, "
             f"{n_ch * bins} rows, {-(-pl.F_out // ops.PHASE_LOCK_CHUNK)} chunks of {ops.PHASE_LOCK_CHUNK} frames; "
             f"{torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min..max)", "",
             "| kernel | planes moved once | workspace | us |", "|---|---|---|---|",
             f"| `pg_phase_lock` (compose, carry, apply) | {plane_bytes / 1e6:.1f} MB | {ws_bytes / 1e6:.1f} MB | {fmt(times['lock'], 1e3, 1)} |",
             f"| `pg_phase_vocoder` | {plane_bytes / 1e6:.1f} MB | - | {fmt(times['plain'], 1e3, 1)} |",
             f"| ratio | | | {fmt(ratio, 1.0, 2)} |", "",
             f"| `reconstruct_track(join=\"spectral\", stretch={stretch:g})`, no model | ms |", "|---|---|",
             f"| phase=\"vocoder_locked\" | {fmt(times['vocoder_locked'], 1.0, 2)} |", f"| phase=\"vocoder\" | {fmt(times['vocoder'], 1.0, 2)} |", "",
             "| melody (6 s, 16 kHz) at stretch 1.5, own moments | locked: spectral convergence | LSD dB | plain: spectral convergence | LSD dB |",
             "|---|---|---|---|---|"]
    lines += [f"| reset_below {fl:g} | {m['vocoder_locked']['spectral_convergence']:.4f} | {m['vocoder_locked']['lsd_db']:.3f} | "
              f"{m['vocoder']['spectral_convergence']:.4f} | {m['vocoder']['lsd_db']:.3f} |" for fl, m in table]
    lines += [f"| zero phase | {zero['spectral_convergence']:.4f} | {zero['lsd_db']:.3f} | | |"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
