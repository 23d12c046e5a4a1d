#!/usr/bin/env python3
"""Single-pass spectrogram inversion (phasegen.ops.phase_spsi, phasegen.track phase="spsi") beside identity phase locking, measured in
ONE process over alternating rounds on the track of tools/lock_bench.py (3-minute stereo at n_fft 2048 / hop 512, stretch 1.5):

  * pg_phase_spsi (its three launches together: compose, carry, apply) on the resampled magnitudes beside pg_phase_lock on the
    analysis planes, both writing the same (n_ch, bins, F_out) output;
  * spectrogram consistency (``track.evaluate_stretch``) of the synthetic melody of tests/_vocoder_ref.py at stretch 1.0 and 1.5 with
    the track's own moments for spsi, vocoder_locked, vocoder and zero;
  * Griffin-Lim per clip of the melody (``track.evaluate_track``, waveform join) from noise and from the single-pass inversion at a
    few iteration counts: spectral convergence against the input.

HIP events around every repetition; every time is the median over the rounds with min..max.  Prints markdown (DESIGN.md section 4.13
holds a copy); --out writes it to a file as well."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vocoder_bench import STATS, fmt, make_audio, time_ms  # noqa: E402  (puts the package and tests/ on the path)

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
    ap.add_argument("--gl_iters", default="8,32", help="comma list of Griffin-Lim iteration counts")
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spsi_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("spsi_bench: at least 5 rounds")
    bins, hop, frames, ov, n_ch, stretch = args.width, args.width // 2, args.frames, args.overlap_frames, args.channels, args.stretch
    n_fft = 2 * bins
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    pl = track.spectral_plan(a_len, frames, hop, ov, stretch)

    # the kernels alone, on the planes the pipeline hands them
    begin = torch.arange(n_ch, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(audio.reshape(-1), begin, begin + a_len, pl.n_src, n_fft, hop, polar=True, stats=STATS)
    mag = ops.spec_clips(pol[:, 0], 1, pl.F_out, pl.F_out, 1.0 / stretch)[0]
    out = torch.empty(n_ch, bins, pl.F_out, device="cuda")
    q = _lib.PhaseSpsiArgs()
    q.n_ch, q.bins, q.F = n_ch, bins, pl.F_out
    ws_bytes = _lib.load().pg_workspace_bytes_phase_spsi(ctypes.byref(q))
    floor = track.VOCODER_RESET_BELOW
    runs = {"spsi": lambda: ops.phase_spsi(mag, n_fft, hop, out=out),
            "lock": lambda: ops.phase_lock(pol[:, 1], pl.F_out, 1.0 / stretch, logmag=pol[:, 0], reset_below=floor, out=out)}
    for fn in runs.values():                                              # warm-up: workspaces, allocator
        fn()
        fn()
    times = {k: [] for k in runs}
    for r in range(args.rounds):
        for name in runs:
            times[name].append(time_ms(runs[name], inner=10))
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in times.items()), flush=True)

    melody = _vocoder_ref.melody()
    phases = ("spsi", "vocoder_locked", "vocoder", "zero")
    table = [(s, track.evaluate_stretch(None, melody, s, phases=phases)["metrics"]) for s in (1.0, 1.5)]
    gl = []
    for iters in (int(v) for v in args.gl_iters.split(",")):
        gl.append((iters, {init: track.evaluate_track(None, melody, phases=("griffinlim",), gl_iters=iters, gl_init=init)["metrics"]["griffinlim"]
                           for init in track.GL_INITS}))

    ratio = [a / b for a, b in zip(times["spsi"], times["lock"])]
    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}, stretch {stretch:g}: F_src {pl.F_src}, F_out {pl.F_out}, "
             f"{n_ch * bins} rows, {-(-pl.F_out // ops.PHASE_LOCK_CHUNK)} chunks of {ops.PHASE_LOCK_CHUNK} frames; "
             f"{torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min..max)", "",
             "| kernel | planes read | plane written | workspace | us |", "|---|---|---|---|---|",
             f"| `pg_phase_spsi` (compose, carry, apply) | {4 * mag.numel() / 1e6:.1f} MB | {4 * out.numel() / 1e6:.1f} MB | {ws_bytes / 1e6:.1f} MB | {fmt(times['spsi'], 1e3, 1)} |",
             f"| `pg_phase_lock` (compose, carry, apply) | {8 * n_ch * bins * pl.F_src / 1e6:.1f} MB | {4 * out.numel() / 1e6:.1f} MB | {ws_bytes / 1e6:.1f} MB | {fmt(times['lock'], 1e3, 1)} |",
             f"| ratio | | | | {fmt(ratio, 1.0, 2)} |", "",
             "| melody (6 s, 16 kHz), own moments: spectral convergence (LSD dB) | " + " | ".join(phases) + " |", "|---|" + "---|" * len(phases)]
    lines += [f"| stretch {s:g} | " + " | ".join(f"{m[p]['spectral_convergence']:.4f} ({m[p]['lsd_db']:.2f})" for p in phases) + " |" for s, m in table]
    lines += ["", "| melody, Griffin-Lim per clip against the input: spectral convergence (SI-SDR dB) | from noise | from spsi |", "|---|---|---|"]
    lines += [f"| {iters} iterations | " + " | ".join(f"{m[i]['spectral_convergence']:.4f} ({m[i]['si_sdr_db']:.2f})" for i in track.GL_INITS) + " |"
              for iters, m in gl]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
