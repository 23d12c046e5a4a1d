#!/usr/bin/env python3
"""dev tool: STFT (+ polar) and ISTFT at the e2e shape (64 signals x 256 frames of 2048 / 512) and the demo shape (1 x 128), event-timed;
`resample` leg: pg_resample on a 300 s track, 44.1 -> 16 kHz and 16 -> 44.1 kHz, both qualities, with scipy.signal.resample_poly on the
host for scale.  Usage: sig_bench.py [stft] [resample]   (no argument: both legs)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-phasegen_amd")); sys.path.insert(0, ROOT)
import torch
from phasegen import ops

def timeit(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3     # us

legs = sys.argv[1:] or ["stft", "resample"]

for nsig, frames, n_fft, hop in () if "stft" not in legs else ((64, 256, 2048, 512), (1, 128, 2048, 512), (64, 256, 1024, 256)):
    n = hop * (frames - 1)
    y = torch.randn(nsig, n, device="cuda") * 0.1
    out = torch.empty(nsig, 2, n_fft // 2, frames, device="cuda")
    a_in, a_out = nsig * n * 4, out.numel() * 4
    t = timeit(lambda: ops.stft(y, n_fft, hop, out=out))
    print(f"[{nsig} x {frames} @ {n_fft}/{hop}] stft        {t:8.1f} us  {(a_in + a_out) / t / 1e6:6.2f} TB/s algorithmic")
    t = timeit(lambda: ops.stft(y, n_fft, hop, polar=True, out=out))
    print(f"[{nsig} x {frames} @ {n_fft}/{hop}] stft+polar  {t:8.1f} us  {(a_in + a_out) / t / 1e6:6.2f} TB/s")
    p2 = torch.empty_like(out)
    t = timeit(lambda: ops.polar(out, p2))
    print(f"[{nsig} x {frames} @ {n_fft}/{hop}] polar       {t:8.1f} us  {2 * a_out / t / 1e6:6.2f} TB/s")
    lm, ph = p2[:, 0].contiguous(), p2[:, 1].contiguous()
    for mode, norm in ((0, True), (0, False), (1, True)):
        t = timeit(lambda: ops.istft(lm, ph, hop, mode=mode, normalize=norm))
        alg = a_out + a_in * (3 if norm else 1)
        print(f"[{nsig} x {frames} @ {n_fft}/{hop}] istft mode {mode} normalize {int(norm)}  {t:8.1f} us  {alg / t / 1e6:6.2f} TB/s algorithmic")
    t = timeit(lambda: ops.istft(lm, ph, hop, mode=0, normalize=True, single_frame=True))
    print(f"[{nsig} x {frames} @ {n_fft}/{hop}] istft three-kernel path (one frame per workgroup)  {t:8.1f} us")

if "resample" in legs:
    import numpy as np
    from scipy.signal import resample_poly
    from phasegen import _lib
    lib = _lib.load()
    for orig, target in ((44100, 16000), (16000, 44100)):
        n_in = 300 * orig
        x = torch.randn(n_in, device="cuda") * 0.1
        xh = x.cpu().numpy()
        for res in ("kaiser_best", "kaiser_fast"):
            taps = lib.pg_resample_taps(target, orig, 0 if res == "kaiser_best" else 1)
            y = ops.resample(x, orig, target, res_type=res)
            t = timeit(lambda: ops.resample(x, orig, target, res_type=res, out=y))
            macs, nbytes = y.numel() * taps, 4 * (n_in + y.numel())
            print(f"[resample 300 s {orig} -> {target} {res}: {n_in} -> {y.numel()} samples, {taps} taps] {t:8.1f} us  "
                  f"{macs / t / 1e3:7.1f} G multiply-adds/s  {nbytes / t / 1e3:7.1f} GB/s")
        t0 = time.perf_counter()
        yh = resample_poly(xh, target // 100, orig // 100)          # scipy's own Kaiser(5.0) filter: for scale, not for parity
        print(f"[resample 300 s {orig} -> {target} scipy.signal.resample_poly on the host, float32, {len(yh)} samples] {(time.perf_counter() - t0) * 1e3:8.1f} ms")
