#!/usr/bin/env python3
"""The spectral track join (phasegen.track, join="spectral") on one synthetic 3-minute stereo track at n_fft 2048 / hop 512 (128
frames, 32 frames of overlap, batches of 64 clips), measured in ONE process over alternating rounds:

  * pg_spec_clips (the model's input from the whole-track log-magnitude plane) and pg_phase_join (one phase per global frame) alone,
    against the bytes they move: every clip element read once and written once; every clip phase read once, every track phase
    written once.
  * the whole ``reconstruct_track`` at join="waveform" against join="spectral" with a STUB phase source -- an object whose
    ``forward`` hands out precomputed phases, so no weights are needed and the model's time is in neither figure.
  * the overlap energy report: the stub's phases are drawn independently per clip (uniform in (-pi, pi]), a stand-in for predictions
    that disagree.  For both joins: the mean over the overlaps (and channels) of 10 log10(energy of the output inside the overlap /
    energy of the phase="original" output of the same join there), and the same figure over equally long stretches in the MIDDLE of
    the clips, where one clip alone decides: the difference of the two is what the join itself costs.

HIP events around every repetition; every figure is the median over the rounds with min..max.  Prints markdown (DESIGN.md section
4.10 holds a copy); --out writes it to a file as well."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-phasegen_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from phasegen import ops, track  # noqa: E402

STATS = (0.0, 3.0)


def time_ms(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def make_audio(seconds, sr, n_ch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = int(seconds * sr)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    tones = 0.3 * torch.sin(2 * np.pi * 440.0 / sr * t) + 0.2 * torch.sin(2 * np.pi * 1730.0 / sr * t + 0.5)
    return (0.1 * torch.randn(n_ch, n, device="cuda", generator=g) + tones.float()[None]).contiguous()


class StubPhases:
    """Stands in for the model: ``forward`` returns the next rows of a precomputed (n_signals, 2 bins, frames) table, in call order
    (both joins ask for the clips in (clip, channel) order, in batches of clip_batch)."""

    def __init__(self, n_sig, bins, frames, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.table = (torch.rand(n_sig, 2 * bins, frames, device="cuda", generator=g) * 2.0 - 1.0) * float(np.pi)
        self.at = 0

    def forward(self, x, per_clip=False):
        n = x.shape[0]
        out = self.table[self.at:self.at + n]
        self.at = (self.at + n) % self.table.shape[0]
        return out


def fmt(vals, scale=1.0, prec=3):
    return f"{statistics.median(vals) * scale:.{prec}f} ({min(vals) * scale:.{prec}f}..{max(vals) * scale:.{prec}f})"


def band_db(out, orig, starts, length):
    """Mean over the stretches [s, s + length) and channels of 10 log10(energy of out / energy of orig)."""
    vals = []
    for s in starts:
        e = out[:, s:s + length].double().pow(2).sum(1) / orig[:, s:s + length].double().pow(2).sum(1)
        vals.extend((10.0 * torch.log10(e)).tolist())
    return float(np.mean(vals))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--clip_batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spectral_bench: needs the GPU (nothing here can be measured on a CPU)")
    bins, hop, frames, ov, n_ch = args.width, args.width // 2, args.frames, args.overlap_frames, args.channels
    n_fft = 2 * bins
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    pl = track.spectral_plan(a_len, frames, hop, ov)
    T, step, n_clips = track.track_plan(a_len, frames, hop, ov)
    n_sig = n_clips * n_ch
    kw = dict(n_fft=n_fft, hop_length=hop, frames=frames, overlap_frames=ov, stats=STATS, sr=args.sr, clip_batch=args.clip_batch, normalize=False)

    # the kernels alone, on the tensors the pipeline hands them
    begin = torch.arange(n_ch, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(audio.reshape(-1), begin, begin + a_len, pl.n_src, n_fft, hop, polar=True, stats=STATS)
    clips = torch.empty(n_clips, n_ch, bins, frames, device="cuda")
    stub = StubPhases(n_sig, bins, frames, seed=1)
    phi = stub.table.view(n_clips, n_ch, 2 * bins, frames)[:, :, :bins]
    joined = torch.empty(n_ch, bins, pl.F_out, device="cuda")
    sc_bytes = 2 * 4 * clips.numel()
    pj_bytes = 4 * (clips.numel() + joined.numel())
    runs = {"spec_clips": lambda: ops.spec_clips(pol[:, 0], n_clips, frames, pl.sf, 1.0, out=clips),
            "phase_join": lambda: ops.phase_join(phi, pl.sf, out=joined),
            "waveform": lambda: track.reconstruct_track(stub, audio, join="waveform", **kw),
            "spectral": lambda: track.reconstruct_track(stub, audio, join="spectral", **kw)}
    for fn in runs.values():                                              # warm-up: ramps, workspaces, allocator
        fn()
        fn()
    times = {k: [] for k in runs}
    energy = {k: [] for k in ("waveform overlap", "waveform mid-clip", "spectral overlap", "spectral mid-clip")}
    V = ov * hop
    over = [k * step for k in range(1, n_clips) if k * step + V <= a_len]
    assert step >= 2 * V and T == step + V
    mid = [k * step + V + (step - 2 * V) // 2 for k in range(0, n_clips - 1)]    # centred between the clip's two overlaps
    orig = {j: track.reconstruct_track(None, audio, phase="original", join=j, **kw) for j in ("waveform", "spectral")}
    for r in range(args.rounds):
        for name in ("spec_clips", "phase_join"):
            times[name].append(time_ms(runs[name], inner=10))
        for name in ("waveform", "spectral"):
            stub.at = 0
            times[name].append(time_ms(runs[name]))
        stub_r = StubPhases(n_sig, bins, frames, seed=100 + r)           # fresh, independent clip phases every round
        for j in ("waveform", "spectral"):
            stub_r.at = 0
            out = track.reconstruct_track(stub_r, audio, join=j, **kw)
            energy[f"{j} overlap"].append(band_db(out, orig[j], over, V))
            energy[f"{j} mid-clip"].append(band_db(out, orig[j], mid, V))
        del stub_r
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in times.items()) + "; "
              + ", ".join(f"{k} {v[-1]:.2f} dB" for k, v in energy.items()), flush=True)

    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}: {n_clips} clips of {frames} frames, sf {pl.sf}, Vf {pl.Vf}, "
             f"F_out {pl.F_out}, F_src {pl.F_src}; {args.rounds} rounds, median (min..max)", "",
             "| kernel | bytes moved | us | TB/s |", "|---|---|---|---|",
             f"| `pg_spec_clips` (rate 1, {n_sig} clip windows) | {sc_bytes / 1e6:.1f} MB | {fmt(times['spec_clips'], 1e3, 1)} | "
             f"{fmt([sc_bytes / t / 1e9 for t in times['spec_clips']])} |",
             f"| `pg_phase_join` | {pj_bytes / 1e6:.1f} MB | {fmt(times['phase_join'], 1e3, 1)} | {fmt([pj_bytes / t / 1e9 for t in times['phase_join']])} |", "",
             "| `reconstruct_track`, stub phase source | ms |", "|---|---|",
             f"| join=\"waveform\" | {fmt(times['waveform'], 1.0, 2)} |", f"| join=\"spectral\" | {fmt(times['spectral'], 1.0, 2)} |", "",
             f"| energy against phase=\"original\", independent clip phases, {len(over)} overlaps of {V} samples | waveform join dB | spectral join dB |", "|---|---|---|",
             f"| inside the overlaps | {fmt(energy['waveform overlap'], 1.0, 2)} | {fmt(energy['spectral overlap'], 1.0, 2)} |",
             f"| mid-clip stretches of the same length | {fmt(energy['waveform mid-clip'], 1.0, 2)} | {fmt(energy['spectral mid-clip'], 1.0, 2)} |",
             f"| overlap minus mid-clip | {statistics.median(energy['waveform overlap']) - statistics.median(energy['waveform mid-clip']):.2f} | "
             f"{statistics.median(energy['spectral overlap']) - statistics.median(energy['spectral mid-clip']):.2f} |"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
