#!/usr/bin/env python3
"""dev tool: one training batch from raw audio -- 64 crops of 65024 samples at 2048 / 512 and at 1024 / 256, polar = 1, with statistics --
through the fused pg_stft_crops call against the three-launch composition it replaces (chunked pg_stft reading the crops in place,
pg_standardize, pg_polar), event-timed in ONE process, the two alternating round by round; medians, the run-to-run spread (min .. max
over the rounds) and TB/s over the algorithmic bytes (64 x 65024 x 4 B read + 64 x 2 x bins x frames x 4 B written).  The outputs of the
two are compared bit for bit first.  Then an AudioCropLoader epoch's batches per second and, with --train-step, the fp32 training step
of UNetModel(1024, 2048) on one such batch for scale.
Usage: crop_bench.py [--rounds 9] [--reps 20] [--batches 64] [--train-step] [--composition-lib libphasegen.so of another commit]"""
import argparse, ctypes as C, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unet-phasegen_amd")); sys.path.insert(0, ROOT)
import numpy as np
import torch
from phasegen import _lib, ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batches", type=int, default=64, help="batches of the timed loader epoch")
ap.add_argument("--train-step", action="store_true")
ap.add_argument("--composition-lib", default=None, help="run the composition through this build of the library (e.g. the parent commit's)")
a = ap.parse_args()

NSIG, CROP, MEAN, STD = 64, 65024, 0.0123, 1.7
lib = _lib.load()
comp_lib = lib
if a.composition_lib:
    comp_lib = C.CDLL(os.path.abspath(a.composition_lib))
    for name in ("pg_stft", "pg_standardize", "pg_polar"):
        getattr(comp_lib, name).restype, getattr(comp_lib, name).argtypes = _lib.SYMBOLS[name]

def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3     # us

rng = np.random.default_rng(0)
n_tracks, t_len = 8, 10 * CROP
src = torch.randn(n_tracks * t_len, device="cuda") * 0.1
track = rng.integers(0, n_tracks, NSIG)
start = rng.integers(0, t_len - CROP // 2, NSIG)                  # some crops run off the end of their track
begin = torch.from_numpy(track * t_len + start).cuda()
end = torch.from_numpy((track + 1) * t_len).cuda()
rows, st = torch.from_numpy(track.astype(np.int32)).cuda(), torch.from_numpy(start).cuda()
stats = ops.stats_tensor((MEAN, STD), src.device)
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

for n_fft, hop in ((2048, 512), (1024, 256)):
    bins, frames = n_fft // 2, 1 + CROP // hop
    fused_out = torch.empty(NSIG, 2, bins, frames, device="cuda")
    x, p2 = torch.empty_like(fused_out), torch.empty_like(fused_out)
    sa, _ = ops._stft_args(src.view(n_tracks, t_len), n_fft, hop, out=x, chunk_start=st, chunk_row=rows, chunk_len=CROP)
    pa = _lib.PolarArgs()
    pa.n_items, pa.inner, pa.inp, pa.out, pa.use_exp = NSIG, bins * frames, x.data_ptr(), p2.data_ptr(), 1
    def composition():
        _lib.check(comp_lib.pg_stft(C.byref(sa), stream()), "stft")
        _lib.check(comp_lib.pg_standardize(C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(stats.data_ptr()), stream()), "standardize")
        _lib.check(comp_lib.pg_polar(C.byref(pa), stream()), "polar")
    fused = lambda: ops.stft_crops(src, begin, end, CROP, n_fft, hop, polar=True, stats=stats, out=fused_out)
    for _ in range(3): fused(); composition()
    torch.cuda.synchronize()
    same = torch.equal(fused_out, p2)
    tf, tc = [], []
    for _ in range(a.rounds):
        tf.append(window(fused, a.reps)); tc.append(window(composition, a.reps))
    nbytes = NSIG * CROP * 4 + fused_out.numel() * 4
    mf, mc = statistics.median(tf), statistics.median(tc)
    tag = f"[{NSIG} x {CROP} @ {n_fft}/{hop}]"
    print(f"{tag} plan {ops.stft_crops_describe(src, begin, end, CROP, n_fft, hop, polar=True, stats=stats)}; outputs bit-identical: {same}")
    print(f"{tag} fused pg_stft_crops      median {mf:8.1f} us  (min {min(tf):.1f} .. max {max(tf):.1f})  {nbytes / mf / 1e6:6.2f} TB/s algorithmic")
    print(f"{tag} stft+standardize+polar   median {mc:8.1f} us  (min {min(tc):.1f} .. max {max(tc):.1f})  {nbytes / mc / 1e6:6.2f} TB/s algorithmic"
          f"{'  [composition from ' + a.composition_lib + ']' if a.composition_lib else ''}")
    print(f"{tag} fused / composition = {mf / mc:.3f}; not slower within the composition's spread ({max(tc) - min(tc):.1f} us): {mf <= mc + (max(tc) - min(tc))}")

from phasegen.data import AudioCropLoader
tracks = [src[i * t_len:(i + 1) * t_len] for i in range(n_tracks)]
per_epoch = a.batches * NSIG
n_random = max(0, -(-per_epoch // (n_tracks * 10)) - 1)            # 10 aligned chunks per track
loader = AudioCropLoader(tracks, NSIG, t_slice=CROP, n_fft=2048, hop_length=512, n_random=n_random, stats=(MEAN, STD), seed=0)
for _ in loader: pass                                              # warm-up epoch
torch.cuda.synchronize()
import time
t0 = time.perf_counter(); nb = 0
for d in loader: nb += 1
torch.cuda.synchronize()
el = time.perf_counter() - t0
print(f"[loader] epoch of {nb} batches of {NSIG} crops (table build and upload included): {el * 1e3:.1f} ms = {nb / el:.1f} batches/s")

if a.train_step:
    from phasegen.model import UNetModel
    from phasegen.trainer import Trainer
    trainer = Trainer(UNetModel(1024, 2048), lr=1e-3)
    batch = next(iter(loader))[0]
    for _ in range(2): trainer.step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3): trainer.step(batch)
    torch.cuda.synchronize()
    step = (time.perf_counter() - t0) / 3
    print(f"[train] fp32 step of UNetModel(1024, 2048) on one loader batch ({tuple(batch.shape)}): {step * 1e3:.1f} ms = {1 / step:.2f} steps/s; "
          f"the loader yields {nb / el * step:.0f} batches in that time")
