#!/usr/bin/env python3
"""Whole-track phase reconstruction (phasegen.track.reconstruct_track) on a 300 s track, mono and stereo, given at 44.1 kHz and
at 16 kHz, C = 1024 (n_fft 2048, hop 512, 128 frames, 32 frames of overlap, batches of 64 clips), on the fp32 engine and on the
bf16-resident one: time per stage -- resample, STFT + (x - mean) / std + polar, forward, ISTFT, stitch --, the whole call (which
ends in the host's read of the non-finite count) and seconds of audio per second; plus the stitch launches alone against their
algorithmic bytes (every clip sample read once, every output sample written once, and read and written once more by the
normalising second launch).  Warm-up calls first, HIP events around every repetition, medians.  The audio is seeded noise plus two
tones; the weights are the default initialisation (the time does not depend on their values).  Prints a markdown table (DESIGN.md
section 4.7 holds a copy); --out writes it to a file as well."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-phasegen_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from phasegen import audio as pg_audio  # noqa: E402
from phasegen import ops, preproc, track  # noqa: E402
from phasegen.model import UNetModel  # noqa: E402

STATS = (0.0, 3.0)


def median_ms(fn, warmup, reps, inner=1):
    """Median HIP-event time in ms of ONE fn() call: `warmup` calls, then `reps` event pairs around `inner` back-to-back calls each
    (inner > 1 for launches of a few microseconds, which an event pair alone would not resolve)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times)


def make_audio(seconds, sr, n_ch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = int(seconds * sr)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    tones = 0.3 * torch.sin(2 * np.pi * 440.0 / sr * t) + 0.2 * torch.sin(2 * np.pi * 1730.0 / sr * t + 0.5)
    a = 0.1 * torch.randn(n_ch, n, device="cuda", generator=g) + tones.float()[None]
    return a[0].contiguous() if n_ch == 1 else a.contiguous()


def stages(model, a_src, src_sr, args, reps):
    """Median ms of every stage on the tensors the previous stage left, in pipeline order, and of the whole call."""
    C, hop, frames, ov, cb = args.width, args.width // 2, args.frames, args.overlap_frames, args.clip_batch
    n_fft = 2 * C
    out = {}
    if src_sr != args.sr:
        out["resample"] = median_ms(lambda: preproc.resample(a_src, src_sr, args.sr), 2, reps)
        a = preproc.resample(a_src, src_sr, args.sr)
    else:
        out["resample"] = 0.0
        a = a_src
    a2 = (a[None] if a.dim() == 1 else a).contiguous()
    n_ch, a_len = a2.shape
    T, step, n_clips = track.track_plan(a_len, frames, hop, ov)
    st = torch.tensor(np.repeat(np.arange(n_clips, dtype=np.int64) * step, n_ch), device="cuda")
    rows = torch.tensor(np.tile(np.arange(n_ch, dtype=np.int32), n_clips), device="cuda")
    x = torch.empty(n_clips * n_ch, 2, C, frames, device="cuda")
    pol = torch.empty_like(x)

    def analysis():
        ops.stft(a2, n_fft, hop, out=x, chunk_start=st, chunk_row=rows, chunk_len=T)
        ops.standardize_with_(x, *STATS)
        ops.polar(x, out=pol)
    out["stft"] = median_ms(analysis, 2, reps)
    ph = torch.empty(n_clips * n_ch, C, frames, device="cuda")

    def forward():
        with torch.no_grad():
            for i in range(0, n_clips * n_ch, cb):
                ph[i:i + cb] = model.forward(pol[i:i + cb, 0], per_clip=True)[:, :C]
    out["forward"] = median_ms(forward, 2, reps)
    out["istft"] = median_ms(lambda: pg_audio.synthesize(pol[:, 0], ph, hop, normalize=False), 2, reps)
    clips = pg_audio.synthesize(pol[:, 0], ph, hop, normalize=False).view(n_clips, n_ch, T).transpose(0, 1)
    res = torch.empty(n_ch, a_len, device="cuda")
    out["stitch"] = median_ms(lambda: ops.stitch(clips, step, a_len, normalize=True, out=res, return_status=True), 5, 2 * reps, inner=20)
    out["stitch_raw"] = median_ms(lambda: ops.stitch(clips, step, a_len, out=res), 5, 2 * reps, inner=20)
    out["stitch_bytes"] = 4 * (n_ch * n_clips * T + 3 * n_ch * a_len)
    out["stitch_raw_bytes"] = 4 * (n_ch * n_clips * T + n_ch * a_len)
    out["total"] = median_ms(lambda: track.reconstruct_track(model, a_src, n_fft=n_fft, hop_length=hop, frames=frames, overlap_frames=ov,
                                                             stats=STATS, osr=src_sr if src_sr != args.sr else None, sr=args.sr,
                                                             clip_batch=cb), 1, reps)
    out["clips"], out["seconds"] = n_clips * n_ch, a_len / args.sr
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--clip_batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--osr", type=int, default=44100)
    ap.add_argument("--precisions", nargs="+", default=["fp32", "bf16"], help="fp32, bf16 (= bf16-resident inference), bf16x3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_bench: needs the GPU (nothing here can be measured on a CPU)")
    torch.manual_seed(0)
    lines = ["| engine | channels | input rate | clips | resample ms | STFT + polar ms | forward ms | ISTFT ms | stitch ms | whole call ms | s of audio per s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    stitch_lines = ["| channels | clip samples in, samples out | `pg_stitch` normalised: us (GB/s) | un-normalised, one launch: us (GB/s) |", "|---|---|---|---|"]
    for prec in args.precisions:
        model = UNetModel(args.width, 2 * args.width, gpu_ids=[torch.cuda.current_device()], precision=prec)
        label = "bf16-resident" if prec == "bf16" else prec
        for n_ch in (1, 2):
            for src_sr in (args.osr, args.sr):
                r = stages(model, make_audio(args.seconds, src_sr, n_ch), src_sr, args, args.reps)
                print(f"# {label} {n_ch} ch from {src_sr} Hz: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items() if isinstance(v, float)), flush=True)
                lines.append(f"| {label} | {n_ch} | {src_sr} | {r['clips']} | {r['resample']:.2f} | {r['stft']:.2f} | {r['forward']:.2f} | {r['istft']:.2f} | "
                             f"{r['stitch']:.3f} | {r['total']:.2f} | {r['seconds'] / r['total'] * 1e3:.0f} |")
                if prec == args.precisions[0] and src_sr == args.sr:
                    n_out = int(r["seconds"] * args.sr)
                    stitch_lines.append(f"| {n_ch} | {(r['stitch_raw_bytes'] // 4 - n_ch * n_out)}, {n_ch * n_out} | {r['stitch'] * 1e3:.1f} ({r['stitch_bytes'] / r['stitch'] / 1e6:.0f}) | "
                                        f"{r['stitch_raw'] * 1e3:.1f} ({r['stitch_raw_bytes'] / r['stitch_raw'] / 1e6:.0f}) |")
        del model
        ops.release_workspaces()
        torch.cuda.empty_cache()
    text = "\n".join(lines + [""] + stitch_lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
