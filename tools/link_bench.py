#!/usr/bin/env python3
"""Channel-linked phase locking (phasegen.ops.phase_lock_linked, phasegen.track link_channels) beside the independent locking it
replaces, measured in ONE process over alternating rounds:

  * pg_phase_lock on the 2 channels of the track of tools/lock_bench.py (3-minute stereo at n_fft 2048 / hop 512, stretch 1.5) beside
    pg_phase_lock_linked on the same channels with the channel mean as the reference (its three launches together: ONE compose and
    carry, apply per channel), both writing the same (n_ch, bins, F_out) output; with --parent-lib also pg_phase_lock of another build
    of the library (the parent commit's) on the same planes, outputs compared bit for bit;
  * the stereo melody of tests/_link_ref.py at n_fft 2048 / hop 512 with its own moments, stretch 1.5 and 0.8, independent and
    linked: per-channel spectral convergence (``track.evaluate_stretch``), spectral convergence of the channel mean against the
    mean's magnitudes (its ``mid_metrics``; for the independent channels the same ``metrics.consistency`` on their untrimmed
    output), and the rms error of the inter-channel phase difference (tests/_link_ref.py: ipd_error on the kernels' outputs).

HIP events around every repetition; every time is the median over the rounds with min..max.  Prints markdown (DESIGN.md section 4.14
holds a copy); --out writes it to a file as well."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vocoder_bench import STATS, fmt, make_audio, time_ms  # noqa: E402  (puts the package and tests/ on the path)

import torch  # noqa: E402

import _link_ref  # noqa: E402
from phasegen import _lib, metrics, ops, track  # noqa: E402


def parent_lock(path, A, M, F_out, spo, floor, out):
    """pg_phase_lock of the library at ``path`` on the planes A, M (n_ch, bins, F_src), views of one polar tensor -> a callable"""
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.pg_workspace_bytes_phase_lock.restype = ctypes.c_int64
    lib.pg_workspace_bytes_phase_lock.argtypes = [ctypes.POINTER(_lib.PhaseLockArgs)]
    lib.pg_phase_lock.restype = ctypes.c_int
    lib.pg_phase_lock.argtypes = [ctypes.POINTER(_lib.PhaseLockArgs), ctypes.c_void_p]
    a = _lib.PhaseLockArgs()
    a.n_ch, a.bins, a.F_src = A.shape
    a.F_out, a.src_per_out, a.reset_below = F_out, spo, floor
    a.A, a.a_stride, a.M, a.m_stride, a.out = A.data_ptr(), A.stride(0), M.data_ptr(), M.stride(0), out.data_ptr()
    need = lib.pg_workspace_bytes_phase_lock(ctypes.byref(a))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    a.workspace, a.workspace_bytes = ws.data_ptr(), need

    def call():
        rc = lib.pg_phase_lock(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and ws is not None, rc
    return call


def quality(x, stretch, n_fft, hop):
    """{"independent" | "linked": (per-channel SC, mid SC, rms IPD error in rad)} of the stereo track x at ``stretch``"""
    kw = dict(n_fft=n_fft, hop_length=hop, phases=("vocoder_locked",))
    linked = track.evaluate_stretch(None, x, stretch, link_channels=True, **kw)
    indep = track.evaluate_stretch(None, x, stretch, **kw)
    an = track._analyse_spectral(x, n_fft, hop, 128, 32, None, None, 16000, "kaiser_best", stretch, True)
    pl, spo, floor = an.plan, 1.0 / stretch, track.VOCODER_RESET_BELOW
    with torch.no_grad():
        mid_mag = ops.spec_clips(an.pol[2:, 0], 1, pl.F_out, pl.F_out, spo)[0]
        an.link = False                                                   # the same analysis, its channels locked independently
        mag, full = track._invert_spectral(an, None, "vocoder_locked", hop, 128, 64, floor)
        mid_indep = metrics.consistency(mid_mag, full.mean(0, keepdim=True), n_fft, hop)["spectral_convergence"]
        ph = {"independent": ops.phase_lock(an.pol[:2, 1], pl.F_out, spo, logmag=an.pol[:2, 0], reset_below=floor),
              "linked": ops.phase_lock_linked(an.pol[:2, 1], an.pol[2, 1], an.pol[2, 0], pl.F_out, spo, reset_below=floor)}
    A, m = an.pol[:2, 1].cpu().numpy(), mag.cpu().numpy()
    ipd = {k: _link_ref.ipd_error(v.cpu().numpy(), A, m, spo) for k, v in ph.items()}
    sc = lambda rep: rep["metrics"]["vocoder_locked"]["spectral_convergence"]
    return {"independent": (sc(indep), mid_indep, ipd["independent"]),
            "linked": (sc(linked), linked["mid_metrics"]["vocoder_locked"]["spectral_convergence"], ipd["linked"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--stretch", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="also time pg_phase_lock of this build of the library (e.g. the parent commit's)")
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("link_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("link_bench: at least 5 rounds")
    bins, hop, frames, ov, stretch, n_ch = args.width, args.width // 2, args.frames, args.overlap_frames, args.stretch, 2
    n_fft, spo, floor = 2 * bins, 1.0 / args.stretch, track.VOCODER_RESET_BELOW
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    pl = track.spectral_plan(a_len, frames, hop, ov, stretch)

    # the kernels alone, on the planes the pipeline hands them: the channels and, as row n_ch, their mean
    rows = torch.cat([audio, audio.mean(0, keepdim=True)])
    begin = torch.arange(n_ch + 1, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(rows.reshape(-1), begin, begin + a_len, pl.n_src, n_fft, hop, polar=True, stats=STATS)
    out = torch.empty(n_ch, bins, pl.F_out, device="cuda")
    runs = {"lock": lambda: ops.phase_lock(pol[:n_ch, 1], pl.F_out, spo, logmag=pol[:n_ch, 0], reset_below=floor, out=out),
            "linked": lambda: ops.phase_lock_linked(pol[:n_ch, 1], pol[n_ch, 1], pol[n_ch, 0], pl.F_out, spo, reset_below=floor, out=out)}
    same = None
    if args.parent_lib:
        runs["lock (parent)"] = parent_lock(args.parent_lib, pol[:n_ch, 1], pol[:n_ch, 0], pl.F_out, spo, floor, out)
        runs["lock"]()
        mine = out.clone()
        runs["lock (parent)"]()
        same = bool(torch.equal(mine.view(torch.int32), out.view(torch.int32)))
    for fn in runs.values():                                              # warm-up: workspaces, allocator
        fn()
        fn()
    times = {k: [] for k in runs}
    for r in range(args.rounds):
        for name in runs:
            times[name].append(time_ms(runs[name], inner=10))
        print(f"# round {r}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in times.items()), flush=True)

    x = _link_ref.stereo_melody()
    table = [(s, quality(x, s, 2048, 512)) for s in (1.5, 0.8)]

    q = _lib.PhaseLockLinkedArgs()
    q.n_ch, q.bins, q.F_out = n_ch, bins, pl.F_out
    ws_linked = _lib.load().pg_workspace_bytes_phase_lock_linked(ctypes.byref(q))
    plane = 4 * bins * pl.F_src / 1e6
    ratio = [a / b for a, b in zip(times["linked"], times["lock"])]
    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}, stretch {stretch:g}: F_src {pl.F_src}, F_out {pl.F_out}, "
             f"{n_ch * bins} rows, {-(-pl.F_out // ops.PHASE_LOCK_CHUNK)} chunks of {ops.PHASE_LOCK_CHUNK} frames; "
             f"{torch.cuda.get_device_name(0)}; {args.rounds} rounds, median (min..max)", "",
             "| kernel | planes read | plane written | workspace | us |", "|---|---|---|---|---|",
             f"| `pg_phase_lock` (compose and carry per channel, apply) | {2 * n_ch * plane:.1f} MB | {4 * out.numel() / 1e6:.1f} MB | {n_ch * ws_linked / 1e6:.1f} MB | {fmt(times['lock'], 1e3, 1)} |",
             f"| `pg_phase_lock_linked` (ONE compose and carry, apply) | {(2 + n_ch) * plane:.1f} MB | {4 * out.numel() / 1e6:.1f} MB | {ws_linked / 1e6:.1f} MB | {fmt(times['linked'], 1e3, 1)} |",
             f"| ratio linked / independent | | | | {fmt(ratio, 1.0, 2)} |"]
    if args.parent_lib:
        lines.append(f"| `pg_phase_lock` of the other build (bits {'equal' if same else 'DIFFER'}) | | | | {fmt(times['lock (parent)'], 1e3, 1)} |")
    lines += ["", "| stereo melody (6 s, 16 kHz), 2048 / 512, own moments | independent: per-channel SC / mid SC / rms IPD error | linked to the mid: the same three |",
              "|---|---|---|"]
    lines += [f"| stretch {s:g} | " + " | ".join(f"{t[k][0]:.4f} / {t[k][1]:.4f} / {t[k][2]:.3g} rad" for k in ("independent", "linked")) + " |" for s, t in table]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
