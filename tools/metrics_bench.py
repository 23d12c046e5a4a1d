#!/usr/bin/env python3
"""The quality report's device work (phasegen.metrics.compare_audio) on a 300 s stereo track at 16 kHz, n_fft 2048, hop 512:
median HIP-event ms of pg_wave_compare, of the two whole-signal STFTs, of pg_spec_compare (the pass without and the pass with a
gain) and of the whole compare_audio call (which ends in the host's read of the sums), each beside its algorithmic bytes -- 8 B per
sample for pg_wave_compare (x and y read once), 16 B per cell for pg_spec_compare (four floats) -- the TB/s those give and their
share of 8 TB/s.  The same sums composed from torch element-wise and reduction ops on the device are timed in the same process,
alternating with the fused calls repetition by repetition.  Warm-up calls first, medians.  The audio is seeded noise plus two
tones, the estimate a scaled and perturbed copy (the time does not depend on the values).  Prints a markdown table (DESIGN.md
section 4.8 holds a copy); --out writes it to a file as well."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-phasegen_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from phasegen import metrics, ops  # noqa: E402

PEAK_TBS = 8.0


def alternate_ms(fns, warmup, reps, inner=1):
    """Median HIP-event ms of ONE call of each function of ``fns``, the functions taking turns repetition by repetition (helpers as
    in tools/track_bench.py: `inner` back-to-back calls per event pair for launches an event pair alone would not resolve)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) / inner)
    return [statistics.median(t) for t in times]


def make_pair(seconds, sr, n_ch, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = int(seconds * sr)
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    tones = 0.3 * torch.sin(2 * np.pi * 440.0 / sr * t) + 0.2 * torch.sin(2 * np.pi * 1730.0 / sr * t + 0.5)
    x = (0.1 * torch.randn(n_ch, n, device="cuda", generator=g) + tones.float()[None]).contiguous()
    y = (0.8 * x + 0.05 * torch.randn(n_ch, n, device="cuda", generator=g)).contiguous()
    return x, y


def torch_wave(x, y, g):
    """pg_wave_compare's six sums from torch ops (double arithmetic, as the kernel's)."""
    ok = torch.isfinite(x) & torch.isfinite(y)
    xd, yd = torch.where(ok, x, 0).double(), torch.where(ok, y, 0).double()
    d = xd - g * yd
    return torch.stack([(xd * xd).sum(1), (yd * yd).sum(1), (xd * yd).sum(1), (d * d).sum(1), d.abs().amax(1), (~ok).sum(1).double()], 1)


def torch_spec(R, E, g, floor):
    """pg_spec_compare's six sums from torch ops (fp32 element arithmetic, double sums, as the kernel's)."""
    ok = (torch.isfinite(R).all(1) & torch.isfinite(E).all(1))[:, None]
    R, E = torch.where(ok, R, 0), torch.where(ok, E, 0)
    mR = torch.sqrt(R[:, 0] * R[:, 0] + R[:, 1] * R[:, 1])
    mE0 = torch.sqrt(E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1])
    mE = g * mE0
    d = mR - mE
    dl = 10.0 * torch.log10(torch.clamp_min(mR * mR, floor)) - 10.0 * torch.log10(torch.clamp_min(mE * mE, floor))
    lsd = torch.sqrt((dl * dl).sum(1, dtype=torch.float64) / R.shape[2]).sum(1)
    s = lambda a: a.sum((1, 2), dtype=torch.float64)
    return torch.stack([s(mR * mR), s(mE0 * mE0), s(mR * mE0), s(d * d), lsd, (~ok[:, 0]).sum((1, 2)).double()], 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--n_fft", type=int, default=2048)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", help="also write the markdown table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_bench: needs the GPU (nothing here can be measured on a CPU)")
    x, y = make_pair(args.seconds, args.sr, args.channels)
    n_ch, n = x.shape
    R, E = ops.stft(x, args.n_fft, args.hop), ops.stft(y, args.n_fft, args.hop)
    bins, frames = R.shape[2], R.shape[3]
    g = torch.full((n_ch,), 1.2, dtype=torch.float64, device="cuda")
    gm = torch.full((n_ch,), 1.1, dtype=torch.float64, device="cuda")
    wout, sout = torch.empty(n_ch, 6, dtype=torch.float64, device="cuda"), torch.empty(n_ch, 6, dtype=torch.float64, device="cuda")
    # the torch compositions compute what the kernels compute (to the rounding of a differently ordered sum)
    for got, want in ((ops.wave_compare(x, y, gain=g), torch_wave(x, y, g[:, None])),
                      (ops.spec_compare(R, E, gain=gm), torch_spec(R, E, gm.float()[:, None, None], 1e-10))):
        rel = ((got - want).abs() / want.abs().clamp_min(1e-300)).max().item()
        print(f"# fused vs torch composition: worst relative difference {rel:.2e}", flush=True)
        assert rel < 1e-4, (got, want)
    wb, sb = 8 * n_ch * n, 16 * n_ch * bins * frames
    rows = []

    def row(name, ms, nbytes=None, torch_ms=None):
        rate = "" if nbytes is None else f"{nbytes / ms / 1e9:.2f}"
        share = "" if nbytes is None else f"{100 * nbytes / ms / 1e9 / PEAK_TBS:.0f} %"
        rows.append(f"| {name} | {ms:.3f} | {'' if nbytes is None else f'{nbytes / 1e6:.1f}'} | {rate} | {share} | {'' if torch_ms is None else f'{torch_ms:.3f}'} |")
        print("# " + rows[-1], flush=True)

    f, t = alternate_ms([lambda: ops.wave_compare(x, y, out=wout), lambda: torch_wave(x, y, 1.0)], 3, args.reps, inner=10)
    row("`wave_compare`, no gain", f, wb, t)
    f, t = alternate_ms([lambda: ops.wave_compare(x, y, gain=g, out=wout), lambda: torch_wave(x, y, g[:, None])], 3, args.reps, inner=10)
    row("`wave_compare`, gain", f, wb, t)
    Rb, Eb = torch.empty_like(R), torch.empty_like(E)

    def stfts():
        ops.stft(x, args.n_fft, args.hop, out=Rb)
        ops.stft(y, args.n_fft, args.hop, out=Eb)
    row("the two STFTs", alternate_ms([stfts], 3, args.reps)[0])
    del Rb, Eb
    f, t = alternate_ms([lambda: ops.spec_compare(R, E, out=sout), lambda: torch_spec(R, E, 1.0, 1e-10)], 3, args.reps, inner=4)
    row("`spec_compare`, no gain", f, sb, t)
    gf = gm.float()[:, None, None]
    f, t = alternate_ms([lambda: ops.spec_compare(R, E, gain=gm, out=sout), lambda: torch_spec(R, E, gf, 1e-10)], 3, args.reps, inner=4)
    row("`spec_compare`, gain", f, sb, t)
    del R, E
    row("whole `compare_audio`", alternate_ms([lambda: metrics.compare_audio(x, y, args.n_fft, args.hop)], 2, args.reps)[0])
    head = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz: {n_ch} x {n} samples; n_fft {args.n_fft}, hop {args.hop}: {bins} bins x {frames} frames per channel", "",
            "| call | median ms | algorithmic MB | TB/s | of 8 TB/s | torch composition ms |", "|---|---|---|---|---|---|"]
    text = "\n".join(head + rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
