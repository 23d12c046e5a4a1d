#!/usr/bin/env python3
"""Tempo maps (phasegen.track.TimeMap; the pos= keyword of phasegen.ops.spec_clips, phase_vocoder, phase_lock, phase_lock_linked and
ola_stretch) beside the uniform stretch they generalise, measured in ONE process over alternating rounds:

  * every mapped kernel on the ramp map 1 -> 1.5 (TimeMap.ramp, 64 segments) beside its uniform twin at stretch 1.25, the ramp's
    mean, on the 3-minute stereo track of the other track benches at n_fft 2048 / hop 512: the same planes, outputs of the same
    size;
  * with --parent-lib every uniform twin beside the same entry point of another build of the library (the parent commit's) on the
    same arguments, outputs compared bit for bit: the uniform instantiations keep their bits and their time when this build's median
    lies within the spread the parent's rounds show in the same run;
  * the spectral convergence (``track.evaluate_stretch``) of the synthetic melody of tests/_vocoder_ref.py under the ramp map for
    "vocoder", "vocoder_locked", "spsi" and "zero", beside the uniform figures at stretch 1.0 and 1.5.

HIP events around every repetition; every time is the median over the rounds with min..max.  Prints markdown (DESIGN.md section 4.19
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


def captured(symbol, call):
    """the argument struct the wrapper behind ``call`` hands to ``symbol`` (the call runs once)"""
    lib, box = _lib.load(), {}
    real = getattr(lib, symbol)

    def spy(a, st):
        box["a"] = a._obj
        return real(a, st)
    setattr(lib, symbol, spy)
    try:
        call()
    finally:
        setattr(lib, symbol, real)
    return box["a"]


def parent_call(parent, symbol, a):
    """``symbol`` of the other build on the very arguments this build was given -> a callable"""
    fn = getattr(parent, symbol)
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(type(a)), ctypes.c_void_p]

    def call():
        rc = fn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (symbol, rc)
    return call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1024, help="C (bins): 1024 = the reference's 2048-point FFT")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--overlap_frames", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="also time every uniform twin of this build of the library (e.g. the parent commit's)")
    ap.add_argument("--out", help="also write the markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("map_bench: needs the GPU (nothing here can be measured on a CPU)")
    if args.rounds < 5:
        sys.exit("map_bench: at least 5 rounds")
    bins, hop, frames, ov, n_ch = args.width, args.width // 2, args.frames, args.overlap_frames, 2
    n_fft, r0, r1, floor = 2 * bins, 1.0, 1.5, track.VOCODER_RESET_BELOW
    stretch = (r0 + r1) / 2
    spo = 1.0 / stretch
    audio = make_audio(args.seconds, args.sr, n_ch)
    a_len = audio.shape[1]
    tm = track.TimeMap.ramp(args.seconds, r0, r1, 64)
    pu, pm = track.spectral_plan(a_len, frames, hop, ov, stretch), tm.plan(a_len, frames, hop, ov, args.sr)
    F_out = min(pu.F_out, pm.F_out)                                       # (equal but for the rounding of a_out)
    n_src = max(pu.n_src, pm.n_src)

    # the planes the pipeline hands the kernels: the channels and, as row n_ch, their mean; the percussive audio is noise
    rows = torch.cat([audio, audio.mean(0, keepdim=True)])
    begin = torch.arange(n_ch + 1, dtype=torch.int64, device="cuda") * a_len
    pol = ops.stft_crops(rows.reshape(-1), begin, begin + a_len, n_src, n_fft, hop, polar=True, stats=STATS)
    F_src = pol.shape[-1]
    pos = torch.from_numpy(pm.pos[:F_out].copy()).cuda()
    n_out = hop * (F_out - 1)
    grains = torch.from_numpy(tm.src_of_out(torch.arange(ops.ola_grains(n_out), dtype=torch.float64).numpy() * track.TRANSIENT_HOP, args.sr)).cuda()
    p_audio = 0.1 * torch.randn(n_ch, n_src, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    base = torch.zeros(n_ch, n_out, device="cuda")
    plane_out, wave_out = torch.empty(n_ch, bins, F_out, device="cuda"), torch.empty(n_ch, n_out, device="cuda")
    clip_out = torch.empty(1, n_ch, bins, F_out, device="cuda")
    A, M = pol[:n_ch, 1], pol[:n_ch, 0]
    MB = lambda n: 4 * n / 1e6
    plane, outp = MB(bins * F_src), MB(n_ch * bins * F_out)

    def ola(**g):                                                         # (its table holds one centre per grain, in samples)
        g = dict(pos=grains) if "pos" in g else g
        return ops.ola_stretch(p_audio, n_out, win_len=track.TRANSIENT_WINDOW, hop=track.TRANSIENT_HOP, base=base, out=wave_out, **g)
    # name -> (symbol, call(grid keywords), output, MB read, MB written)
    kernels = {
        "spec_clips": ("pg_spec_clips", lambda **g: ops.spec_clips(M, 1, F_out, F_out, out=clip_out, **g), clip_out, n_ch * plane, outp),
        "phase_vocoder": ("pg_phase_vocoder", lambda **g: ops.phase_vocoder(A, F_out, logmag=M, reset_below=floor, out=plane_out, **g), plane_out,
                          2 * n_ch * plane, outp),
        "phase_lock": ("pg_phase_lock", lambda **g: ops.phase_lock(A, F_out, logmag=M, reset_below=floor, out=plane_out, **g), plane_out,
                       2 * n_ch * plane, outp),
        "phase_lock_linked": ("pg_phase_lock_linked", lambda **g: ops.phase_lock_linked(A, pol[n_ch, 1], pol[n_ch, 0], F_out, reset_below=floor,
                                                                                        out=plane_out, **g), plane_out, (2 + n_ch) * plane, outp),
        "ola_stretch": ("pg_ola_stretch", ola, wave_out, MB(n_ch * n_src) + MB(n_ch * n_out), MB(n_ch * n_out)),
    }
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    runs, same = {}, {}
    for name, (symbol, call, out, _r, _w) in kernels.items():
        runs[name, "uniform"] = lambda call=call: call(src_per_out=spo)
        runs[name, "mapped"] = lambda call=call: call(pos=pos)
        if parent is not None:
            a = captured(symbol, runs[name, "uniform"])
            mine = out.clone()
            runs[name, "parent"] = parent_call(parent, symbol, a)
            out.fill_(-77.0)
            runs[name, "parent"]()
            same[name] = bool(torch.equal(mine.view(torch.int32), out.view(torch.int32)))
    for fn in runs.values():                                              # warm-up: workspaces, allocator, LDS attributes
        fn()
        fn()
    times = {k: [] for k in runs}
    order = list(runs)
    for r in range(args.rounds):
        # Every block begins with one call that is not timed, so that each variant finds the caches as its own previous call left
        # them, whatever ran before it (the planes fit into the last-level cache: without this the variant that follows a call on
        # the same planes gains 2 .. 5 % on the 40 .. 60 us kernels); the order rotates from round to round.
        for key in order[r % len(order):] + order[:r % len(order)]:
            runs[key]()
            times[key].append(time_ms(runs[key], inner=10))
        print(f"# round {r}: " + ", ".join(f"{k[0]}/{k[1]} {v[-1]:.3f}" for k, v in times.items()) + " ms", flush=True)

    med = lambda v: sorted(v)[len(v) // 2]
    lines = [f"{args.seconds:g} s, {n_ch} channels at {args.sr} Hz, n_fft {n_fft}, hop {hop}: F_src {F_src}, F_out {F_out}; uniform stretch {stretch:g} "
             f"beside the ramp {r0:g} -> {r1:g} (64 segments, a_out {pm.a_out} against {pu.a_out}); {torch.cuda.get_device_name(0)}; "
             f"{args.rounds} rounds of 10 calls, median (min..max) in us", "",
             "| kernel | read | written | uniform | mapped | mapped / uniform | uniform, at the median |" + (" uniform of the other build | bits | within its spread |" if parent else ""),
             "|---|---|---|---|---|---|---|" + ("---|---|---|" if parent else "")]
    for name, (symbol, _c, _o, rd, wr) in kernels.items():
        u, m = times[name, "uniform"], times[name, "mapped"]
        ratio = [b / a for a, b in zip(u, m)]
        row = (f"| `{symbol}` / `_map` | {rd:.1f} MB | {wr:.1f} MB | {fmt(u, 1e3, 1)} | {fmt(m, 1e3, 1)} | {fmt(ratio, 1.0, 2)} | "
               f"{(rd + wr) / 1e3 / (med(u) / 1e3):.0f} GB/s |")
        if parent:
            p = times[name, "parent"]
            row += f" {fmt(p, 1e3, 1)} | {'equal' if same[name] else 'DIFFER'} | {'yes' if med(u) <= max(p) else 'NO'} ({med(u) / med(p):.3f} of its median) |"
        lines.append(row)

    x = _vocoder_ref.melody()
    phases = ("vocoder", "vocoder_locked", "spsi", "zero")
    ramp = track.TimeMap.ramp(x.shape[0] / 16000, r0, r1, 64)
    lines += ["", "| synthetic melody (6 s, 16 kHz), 2048 / 512, own moments: spectral convergence | " + " | ".join(phases) + " |", "|---|" + "---|" * len(phases)]
    for label, s in (("uniform 1.0", 1.0), ("uniform 1.5", 1.5), (f"ramp {r0:g} -> {r1:g}", ramp)):
        rep = track.evaluate_stretch(None, x, s, n_fft=2048, hop_length=512, phases=phases)
        lines.append(f"| {label} ({rep['n_out']} samples) | " + " | ".join(f"{rep['metrics'][p]['spectral_convergence']:.4f}" for p in phases) + " |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
