"""GPU: every STFT and ISTFT kernel family of csrc/stft.hip against float64, bin by bin and sample by sample.

References, error scales and the two tiers are those of tests/_signal_ref64.py (derivation there): Tier A, a worst-case bound of the
kernel's operation order that every bin must meet, and Tier B, r_max / r_rms in units of u ||x w||_2 against MARGIN x the same
statistic of an fp32 torch.fft transform of the same input, computed here on the CPU.  tests/test_signal_bounds_host.py shows which
planted faults these comparisons reject.  Every case names the kernel(s) it must reach and checks that against the describe call of
the same arguments; the last test compares the kernels reached by passing cases with the set tests/test_signal_families.py pins.
Shapes are the smallest that reach a branch: ragged and full groups of 4 (8) frames, scalar and 16-byte stores, 4-byte-aligned
samples, outputs and audio, odd hops, chunks with a zero tail, frames that fold twice, a second trip of a persistent workgroup with
a short last XCD chunk (sized from the described grid), the scalar overlap-add, the seams of the fused overlap-add.

Measured on an MI355X: DESIGN.md section 4.2 holds the table.  hop = n_fft is not covered (the fp32 window loses its
relative accuracy at the frame edges and the window-sum-square is not bounded below).

(The file name sorts behind the older test files, like the other test_z_* files: they keep their place in the run.)"""
import collections
import json

import numpy as np
import pytest
import torch

import _signal_ref64 as ref
from phasegen import detgen

gpu = pytest.mark.gpu
GUARD = 12345.0
REACHED = set()                                       # kernel names of the cases that passed
RAN = set()


def describe_fields(entry):
    name, rest = entry.split(",grid=")
    return name, rest.split(",")[0]


def report(case_id, what, **figures):
    print("\nSIGVAL " + json.dumps({"case": case_id, "what": what, **{k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in figures.items()}}))


def offset_view(shape, off, device="cuda"):
    """A dense view of `shape` that begins `off` floats into a 256-byte-aligned buffer, with a guard cell on either side."""
    n = int(np.prod(shape))
    base = torch.full((n + off + 1 + 64,), GUARD, device=device, dtype=torch.float32)
    start = 64 + off                                  # 64 floats = 256 B in front: the view's alignment is `off` floats exactly
    assert base.data_ptr() % 256 == 0
    return base, base[start:start + n].view(*shape)


def guards_intact(base, view):
    n = view.numel()
    start = (view.data_ptr() - base.data_ptr()) // 4
    return bool((base[:start] == GUARD).all()) and bool((base[start + n:] == GUARD).all())


def on_device(y, off=0):
    t = torch.from_numpy(np.ascontiguousarray(y))
    if not off:
        return t.cuda()
    _, v = offset_view(y.shape, off)
    v.copy_(t)
    return v


# ---------------------------------------------------------------------------------------------------------------------------------
# Forward
F = collections.namedtuple("F", "id n_fft hop frames signals single kernel y_off out_off trip2 n_samples polar kinds")


def fcase(id, n_fft, hop, frames, signals=2, single=0, kernel=None, y_off=0, out_off=0, trip2=False, n_samples=None, polar=True,
          kinds=("white", "cosine")):
    if kernel is None:
        kernel = "stft_kernel" if single or n_fft == 4096 else ("stft_w_kernel<{}, 16>" if n_fft == 2048 else "stft_w_kernel<{}, 8>"
                                                                if n_fft == 1024 else "stft_frames_kernel<{}>")
    return F(id, n_fft, hop, frames, signals, single, kernel, y_off, out_off, trip2, n_samples, polar, kinds)


FORWARD_CASES = [
    fcase("r2-4096x3", 4096, 1024, 3, n_samples=3071),
    fcase("r2-64-single", 64, 16, 6, single=1),
    fcase("r2-2048-single", 2048, 512, 5, single=1, out_off=1),
    fcase("r2-32-double-fold", 32, 8, 3, single=1, n_samples=17),
    fcase("r2-4096-double-fold", 4096, 1024, 3, n_samples=2049, signals=1),
    fcase("f4-32-double-fold", 32, 8, 3, n_samples=17),
    fcase("f4-32x5", 32, 8, 5, signals=1),
    fcase("f4-32x8", 32, 8, 8, signals=3),
    fcase("f4-128x5-out+1", 128, 32, 5, out_off=1),
    fcase("f4-128x8-out+1", 128, 32, 8, out_off=1),
    fcase("f4-128x8-hop50", 128, 50, 8),
    fcase("f4-512x5-y+1", 512, 128, 5, y_off=1),
    fcase("f4-512x8", 512, 128, 8, signals=3),
    fcase("f4-512x8-hop50-y+1", 512, 50, 8, y_off=1),
    fcase("f4-32-second-trip", 32, 8, None, signals=3, trip2=True),
    fcase("w8-1024x9", 1024, 256, 9),
    fcase("w8-1024x12-out+1", 1024, 256, 12, out_off=1),
    fcase("w8-1024x16-y+1", 1024, 256, 16, y_off=1, signals=3),
    fcase("w8-1024x9-hop128", 1024, 128, 9),
    fcase("w8-1024x12-hop50", 1024, 50, 12),
    fcase("w8-second-trip", 1024, 256, None, signals=3, trip2=True, kinds=("white",)),
    fcase("w16-2048x9-y+1", 2048, 512, 9, y_off=1),
    fcase("w16-2048x12", 2048, 512, 12, signals=3),
    fcase("w16-2048x16-out+1", 2048, 512, 16, out_off=1),
    fcase("w16-2048x9-hop256", 2048, 256, 9),
    fcase("w16-2048x22-hop50", 2048, 50, 22),
    fcase("w16-second-trip", 2048, 512, None, signals=3, trip2=True, kinds=("white",)),
]
FORWARD_CASES = [c._replace(polar="white" in c.kinds) for c in FORWARD_CASES]


def group_size(case):
    return 8 if case.n_fft in (1024, 2048) and not case.single else 4


def second_trip_frames(case):
    """Frames per signal so that signals x groups lands just above the grid cap (read from the describe string of a call that is
    surely capped), is no multiple of 8, and the last group is ragged."""
    import test_signal_families as fam                # (its describe calls need no device: nothing is dereferenced)
    G = group_size(case)
    cap = int(describe_fields(fam.stft_describe(case.n_fft, case.hop, 256, 64))[1])
    groups = cap // case.signals + 1
    while (case.signals * groups) % 8 == 0:
        groups += 1
    return groups * G - 1


def resolve(case):
    if case.frames is None:
        case = case._replace(frames=second_trip_frames(case))
    if case.n_samples is None:
        case = case._replace(n_samples=case.hop * (case.frames - 1))
    assert 1 + case.n_samples // case.hop == case.frames and case.n_samples > case.n_fft // 2
    return case


def forward_input(case, kind):
    """The input of a resolved case."""
    n = case.n_samples
    if kind == "white":
        return ref.white(700 + case.n_fft % 97 + case.hop, case.signals, n)
    return ref.on_bin_cosine(case.signals, n, case.n_fft, 5 if case.n_fft == 32 else 11)


def check_forward(case, what, got, y, family, polar_of=None):
    """Tiers A and B of `got` (signals, 2, bins, frames) against float64 and the stand-in on the gathered signals y."""
    X = ref.stft64(y, case.n_fft, case.hop)
    sc = ref.forward_scales(y, case.n_fft, case.hop)
    bound = ref.forward_bound(sc, family, case.n_fft)
    if polar_of is not None:
        p = ref.polar_check(got, polar_of, X, bound)
        report(case.id, what, **p)
        assert p["mag"] <= 6e-7 and p["ang"] <= 1.0 and p["excluded"] <= 0.01, (case.id, what, p)
        return
    base = ref.forward_errors(ref.standin_stft(y, case.n_fft, case.hop), X, sc, bound)
    err = ref.forward_errors(got, X, sc, bound)
    kappa = float((sc["l1x"].sum() / sc["l1w"].sum()))
    report(case.id, what, c_A=ref.c_fft(family, case.n_fft) + ref.C_WIN[family] * kappa, a=err["a"], r_max=err["r_max"], r_rms=err["r_rms"],
           ratio_max=err["r_max"] / base["r_max"], ratio_rms=err["r_rms"] / base["r_rms"])
    assert ref.accept(err, base) == (True, ""), (case.id, what, err, base)


def chunk_layout(case):
    """(source rows, starts, rows, gathered): odd starts in two rows; the last chunk runs past the end of its row by a third."""
    n, S = case.n_samples, case.signals
    L = n + 64
    src = ref.white(900 + case.n_fft % 89, 2, L)
    starts = [(3 + 5 * i) % 60 for i in range(S)]
    starts[-1] = L - n + n // 3
    rows = [i % 2 for i in range(S)] if S > 1 else None
    padded = np.concatenate([src, np.zeros((2, n), np.float32)], axis=1)
    gathered = np.stack([padded[rows[i] if rows else 0, s:s + n] for i, s in enumerate(starts)])
    return src, starts, rows, gathered


@gpu
@pytest.mark.parametrize("case", FORWARD_CASES, ids=[c.id for c in FORWARD_CASES])
def test_stft_values(case):
    from phasegen import ops
    case = resolve(case)
    family = ref.family_of(case.n_fft, case.single)
    shape = (case.signals, 2, case.n_fft // 2, case.frames)
    groups = case.signals * -(-case.frames // group_size(case))
    reached = set()

    def described(desc, chunked):
        name, grid = describe_fields(desc)
        assert name == case.kernel.format("true" if chunked else "false"), (case.id, desc)
        if case.trip2:
            assert int(grid) < groups and groups % 8 != 0, (case.id, desc, groups)
        reached.add(name)

    for kind in case.kinds:
        y = forward_input(case, kind)
        yd = on_device(y, case.y_off)
        assert yd.data_ptr() % 8 == (4 if case.y_off else 0)
        described(ops.stft_describe(yd, case.n_fft, case.hop, single_frame=case.single), False)
        plain = ops.stft(yd, case.n_fft, case.hop, single_frame=case.single)
        check_forward(case, f"{kind}", plain.cpu().numpy(), y, family)
        # out= given: a view 4 bytes off 16-byte alignment where the case says so (scalar stores), guard cells on both sides
        base, out = offset_view(shape, case.out_off)
        described(ops.stft_describe(yd, case.n_fft, case.hop, single_frame=case.single, out=out), False)
        ops.stft(yd, case.n_fft, case.hop, single_frame=case.single, out=out)
        assert torch.equal(out, plain) and guards_intact(base, out), (case.id, "out=")
        if kind == "white" and case.polar:
            pol = ops.stft(yd, case.n_fft, case.hop, single_frame=case.single, polar=True)
            check_forward(case, "polar", pol.cpu().numpy(), y, family, polar_of=plain.cpu().numpy())
    # chunked: read in place from two source rows (one row and no chunk_row for a single signal), the last chunk with a zero tail
    src, starts, rows, gathered = chunk_layout(case)
    kw = dict(single_frame=case.single, chunk_len=case.n_samples, chunk_start=torch.tensor(starts, dtype=torch.int64, device="cuda"),
              chunk_row=torch.tensor(rows, dtype=torch.int32, device="cuda") if rows else None)
    srcd = on_device(src)
    described(ops.stft_describe(srcd, case.n_fft, case.hop, **kw), True)
    got = ops.stft(srcd, case.n_fft, case.hop, **kw)
    check_forward(case, "chunked", got.cpu().numpy(), gathered, family)
    if case.polar:
        pol = ops.stft(srcd, case.n_fft, case.hop, polar=True, **kw)
        check_forward(case, "chunked polar", pol.cpu().numpy(), gathered, family, polar_of=got.cpu().numpy())
    REACHED.update(reached)
    RAN.add(case.id)


MEAN, STD = 0.0123, 1.7
CROPS = [("crops-r2", 64, 16, 496, 1, "stft_crops_kernel"), ("crops-f4", 64, 16, 520, 0, "stft_crops_frames_kernel"),
         ("crops-w8", 1024, 256, 2304, 0, "stft_crops_w_kernel<8>"), ("crops-w16", 2048, 512, 4608, 0, "stft_crops_w_kernel<16>")]


@gpu
@pytest.mark.parametrize("id,n_fft,hop,crop_len,single,kernel", CROPS, ids=[c[0] for c in CROPS])
def test_stft_crops_standardised_values(id, n_fft, hop, crop_len, single, kernel):
    """pg_stft_crops with stats: (X - mean) / std against float64.  The epilogue is fp32 (v - mean) / sd with mean and sd rounded
    from double: per part |d| <= (dX + u |mean| + u |v - mean|) / sd + 2 u |z|, i.e. the Tier A bound / sd + u |mean| / sd + 3 u |z|
    (times sqrt 2 for the two parts of the last two terms)."""
    from phasegen import ops
    buf = ref.white(41, 1, 3 * crop_len + 11)[0]
    begin = np.array([0, 3, crop_len + 5, len(buf) - crop_len // 2], np.int64)          # the last one runs past the end: zero tail
    end = np.array([len(buf)] * 4, np.int64)
    gathered = np.zeros((4, crop_len), np.float32)
    for i, b in enumerate(begin):
        gathered[i, :min(crop_len, len(buf) - b)] = buf[b:b + crop_len]
    args = (torch.from_numpy(buf).cuda(), torch.from_numpy(begin).cuda(), torch.from_numpy(end).cuda(), crop_len, n_fft, hop)
    name, _ = describe_fields(ops.stft_crops_describe(*args, stats=(MEAN, STD), single_frame=single))
    assert name == kernel
    got = ops.stft_crops(*args, stats=(MEAN, STD), single_frame=single).cpu().numpy().astype(np.float64)
    family = ref.family_of(n_fft, single)
    X = ref.stft64(gathered, n_fft, hop)
    sc = ref.forward_scales(gathered, n_fft, hop)
    want = (X - MEAN) / STD
    z = np.abs(want[:, 0] + 1j * want[:, 1])
    bound = ref.forward_bound(sc, family, n_fft)[:, None, :] / STD + 2 ** 0.5 * ref.U * (abs(MEAN) / STD + 3 * z)
    d = np.abs((got[:, 0] - want[:, 0]) + 1j * (got[:, 1] - want[:, 1]))
    s32 = (ref.standin_stft(gathered, n_fft, hop) - np.float32(MEAN)) / np.float32(STD)
    assert s32.dtype == np.float32
    ds = np.abs((s32[:, 0] - want[:, 0]) + 1j * (s32[:, 1] - want[:, 1]))
    live = sc["l2"] > 0                                                   # (frames inside the zero tail: Tier A only)
    scale = ref.U * np.where(live, sc["l2"], np.inf)[:, None, :] / STD
    stat = lambda e: (float((e / scale).max()), float(np.sqrt(((e / scale) ** 2).mean(axis=1)).max()))
    (k_max, k_rms), (s_max, s_rms) = stat(d), stat(ds)
    report(id, "standardised", a=float((d / bound).max()), r_max=k_max, r_rms=k_rms, ratio_max=k_max / s_max, ratio_rms=k_rms / s_rms)
    assert np.all(d <= bound) and k_max <= ref.MARGIN * s_max and k_rms <= ref.MARGIN * s_rms


# ---------------------------------------------------------------------------------------------------------------------------------
# Inverse
I = collections.namedtuple("I", "id bins hop frames signals kernels abs_odd kinds")
FUSED8 = ["istft_ola_w_kernel<8>", "istft_seam_kernel"]
FUSED16 = ["istft_ola_w_kernel<16>", "istft_seam_kernel"]


def icase(id, bins, hop, frames, signals=2, kernels=None, abs_odd=False, kinds=("white", "cosine")):
    N = 2 * bins
    if kernels is None:
        if N in (1024, 2048):
            P = 16 if N == 2048 else 8
            kernels = ([f"istft_ola_w_kernel<{P}>"] + (["istft_seam_kernel"] if frames > 8 else [])) if hop * 4 == N else \
                      [f"istft_frames_w_kernel<{P}>", "istft_ola4_kernel"]
        else:
            kernels = ["istft_frames_kernel" if N == 4096 else "istft_frames4_kernel", "istft_ola4_kernel"]
    return I(id, bins, hop, frames, signals, kernels, abs_odd, kinds)


INVERSE_CASES = [
    icase("r2-2048", 2048, 1024, 3),
    icase("f4-16x5", 16, 8, 5, signals=1),
    icase("f4-16x8-abs-odd", 16, 8, 8, abs_odd=True),
    icase("f4-16x5-hop-half", 16, 16, 5),
    icase("f4-16x8-hop-32nd", 16, 1, 8),
    icase("f4-16x5-hop-3q", 16, 24, 5),
    icase("f4-32x6", 32, 16, 6),
    icase("f4-64x8", 64, 32, 8, signals=3),
    icase("f4-64x6-hop50", 64, 50, 6),
    icase("f4-64x8-hop-32nd", 64, 4, 8),
    icase("f4-64x5-hop-3q", 64, 96, 5),
    icase("f4-256x5", 256, 128, 5),
    icase("f4-256x8-abs-odd", 256, 128, 8, abs_odd=True),
    icase("f4-256x5-hop-half", 256, 256, 5),
    icase("f4-256x7-hop50", 256, 50, 7),
    icase("f4-256x8-hop-32nd", 256, 16, 8),
    icase("f4-256x5-hop-3q", 256, 384, 5),
    icase("f4-16-second-trip", 16, 8, 33, signals=64, kinds=("white",)),
    icase("w8-512x7", 512, 256, 7),
    icase("w8-512x9", 512, 256, 9),
    icase("w8-512x16", 512, 256, 16, abs_odd=True),
    icase("w8-512x20", 512, 256, 20, signals=3),
    icase("w8-512x9-hop-half", 512, 512, 9),
    icase("w16-1024x7", 1024, 512, 7),
    icase("w16-1024x9", 1024, 512, 9),
    icase("w16-1024x16", 1024, 512, 16),
    icase("w16-1024x20", 1024, 512, 20, abs_odd=True),
    icase("w16-1024x9-hop-half", 1024, 1024, 9),
    icase("w16-second-trip-seams", 1024, 512, 72, signals=64, kinds=("white",)),
]


def inverse_input(case, kind, mode):
    """(a, b) float32 (signals, bins, frames).  white: normal (re, im) / (|normal|, uniform phase); cosine: the rounded float64 STFT
    of the on-bin cosine (mode 1 only): a spectrum of three bins per frame."""
    shape = (case.signals, case.bins, case.frames)
    if kind == "white":
        if mode == 1:
            return detgen.normal(810 + case.bins % 13, shape), detgen.normal(811 + case.hop % 17, shape)
        return np.abs(detgen.normal(812, shape)), detgen.uniform(813, shape, -3.1415, 3.1415)
    n_fft = 2 * case.bins
    n = case.hop * (case.frames - 1)
    if n <= case.bins:
        return None
    X = ref.stft64(ref.on_bin_cosine(case.signals, n, n_fft, 5 if n_fft == 32 else 11), n_fft, case.hop)
    return X[:, 0].astype(np.float32), X[:, 1].astype(np.float32)


def spectrum_on_device(a, odd):
    """(signals, bins, frames) on the device; odd: with a batch stride of bins x frames + 1 floats (the 16-byte row loads are off)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not odd:
        return t.cuda()
    S, bins, T = a.shape
    flat = torch.zeros(S * (bins * T + 1), device="cuda")
    v = torch.as_strided(flat, (S, bins, T), (bins * T + 1, T, 1))
    v.copy_(t)
    return v


@gpu
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("case", INVERSE_CASES, ids=[c.id for c in INVERSE_CASES])
def test_istft_values(case, mode):
    from phasegen import ops
    N = 2 * case.bins
    length = case.hop * (case.frames - 1)
    reached = set()
    for kind in case.kinds if mode == 1 else ("white",):
        ab = inverse_input(case, kind, mode)
        if ab is None:
            continue
        a, b = ab
        ad, bd = spectrum_on_device(a, case.abs_odd), spectrum_on_device(b, case.abs_odd)
        y64, info = ref.istft64(a, b, case.hop, mode)
        base = ref.inverse_errors(ref.standin_istft(a, b, case.hop, mode), y64, info, ref.inverse_bound(y64, info, ref.family_of(N), N))
        outs, bounds = {}, {}
        unfused = ["istft_frames_w_kernel<16>" if N == 2048 else "istft_frames_w_kernel<8>", "istft_ola4_kernel"] if N in (1024, 2048) else case.kernels
        for path, single, off, want in (("primary", 0, 0, case.kernels), ("audio+1", 0, 1, unfused),
                                        ("single_frame", 1, 0, ["istft_frames_kernel", "istft_ola4_kernel"])):
            family = ref.family_of(N, single)
            guard, out = offset_view((case.signals, length), off)
            (desc,) = ops.istft_describe(ad, bd, case.hop, mode=mode, normalize=False, single_frame=single, out=out)
            names = [describe_fields(e)[0] for e in desc.split("|")]
            assert names == want, (case.id, path, desc)
            if "second-trip" in case.id and path == "primary":
                groups = case.signals * -(-case.frames // (8 if N in (1024, 2048) else 4))
                assert int(describe_fields(desc.split("|")[0])[1]) < groups, (case.id, desc, groups)
            ops.istft(ad, bd, case.hop, mode=mode, normalize=False, single_frame=single, out=out)
            assert guards_intact(guard, out), (case.id, path)
            got = out.cpu().numpy()
            bound = ref.inverse_bound(y64, info, family, N)
            err = ref.inverse_errors(got, y64, info, bound)
            report(case.id, f"mode{mode} {kind} {path}", c_A=ref.c_fft(family, N) + 2 + float(info["C"].max()), a=err["a"], r_max=err["r_max"],
                   r_rms=err["r_rms"], ratio_max=err["r_max"] / base["r_max"], ratio_rms=err["r_rms"] / base["r_rms"])
            assert ref.accept(err, base) == (True, ""), (case.id, path, kind, err, base)
            outs[path], bounds[path] = got.astype(np.float64), bound
            reached.update(names)
            # peak normalisation is one IEEE division by the signal's own fp32 peak
            guard_n, out_n = offset_view((case.signals, length), off)
            (desc,) = ops.istft_describe(ad, bd, case.hop, mode=mode, normalize=True, single_frame=single, out=out_n)
            assert [describe_fields(e)[0] for e in desc.split("|")] == want + ["istft_peak_normalize_kernel"], (case.id, path, desc)
            ops.istft(ad, bd, case.hop, mode=mode, normalize=True, single_frame=single, out=out_n)
            peak = np.abs(got).max(axis=1, keepdims=True)
            assert peak.dtype == np.float32 and np.all(peak > 0)
            gn = out_n.cpu().numpy()
            assert np.array_equal(gn, got / peak) and np.all(np.abs(gn).max(axis=1) == 1.0) and guards_intact(guard_n, out_n), (case.id, path)
            reached.add("istft_peak_normalize_kernel")
        for p in ("audio+1", "single_frame"):                          # the paths that can serve a call agree with each other
            assert np.all(np.abs(outs["primary"] - outs[p]) <= bounds["primary"] + bounds[p]), (case.id, p)
    REACHED.update(reached)
    RAN.add((case.id, mode))


@gpu
@pytest.mark.parametrize("bins,hop,frames,off", [(64, 50, 7, 1), (64, 32, 8, 0), (512, 256, 9, 0)])
def test_a_zero_spectrum_stays_zero(bins, hop, frames, off):
    from phasegen import ops
    z = torch.zeros(2, bins, frames, device="cuda")
    guard, out = offset_view((2, hop * (frames - 1)), off)
    ops.istft(z, z, hop, mode=1, normalize=True, out=out)
    assert bool((out == 0).all()) and guards_intact(guard, out)
    ops.istft(z, z, hop, mode=0, normalize=True, out=out)                # expm1(0) e^{j 0} = 0
    assert bool((out == 0).all())


@gpu
def test_zz_every_signal_kernel_was_reached_by_a_passing_case():
    """Runs last in this module: the kernels named by the cases above that passed are exactly those tests/test_signal_families.py
    finds over its sweep of pg_stft / pg_istft calls (the crops instantiations have their own names and their own test above)."""
    import test_signal_families as fam
    st, ist = fam.sweep()
    want = {k for d in st.values() for k in fam.kernels(d)} | {k for d, _ in ist.values() for k in fam.kernels(d)}
    assert RAN >= {c.id for c in FORWARD_CASES} | {(c.id, m) for c in INVERSE_CASES for m in (0, 1)}, "run the whole module"
    assert REACHED == want, (sorted(want - REACHED), sorted(REACHED - want))
