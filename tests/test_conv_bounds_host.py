"""CPU: does the comparison of tests/_conv_ref64.py have teeth?

(1) the float64 references agree with a direct loop over taps at tiny sizes (every op, both layer kinds, every precision's operands,
    the input activation) and with float64 torch autograd on every row tests/test_z_conv_values_gpu.py runs;
(2) honest convolutions built differently pass: fp32 torch and sequential numpy float32 (forwards and backwards along K, and in
    three K segments added afterwards, as a stream-K fixup adds them) at the fp32 criterion, the same on bf16-rounded operands at
    the bf16 criterion, the emulated split at the bf16x3 criterion -- on every row and input kind of the GPU module;
(3) planted faults -- applied to a stand-in, never to library code -- are rejected, while the older criterion (1e-4 of the tensor's
    max-abs against fp32 torch, as tests/test_ops_gpu.py holds an fp32 result) accepts most of them; the table FAULTS records the
    verdict of both criteria on both inputs, also where the older one already rejects;
(4) on every row whose CONVERR lines carry the [precision] mark, the split's r_rms is at least 10 x sequential fp32's on that row's
    own inputs: the fp32 bound (4 x) rejects an fp32 call that ran the split.  The rows with a GEMM K above 512 are listed by name;
(5) the rows are what the GPU module says they are: every family x op of the fp32 entry points under both work splits with a
    [precision] row each, and the resident forward's rows reach conv_h3 with and without the fixup."""
import numpy as np
import pytest

import _conv_ref64 as ref
import test_z_conv_values_gpu as gpu
from test_kernel_families import BF16_FAMILIES, VIEW_CASES, fixup_case_id

ROWS = list(dict.fromkeys([(c[0], c[1]) for c in gpu.CASES] + [(r[0], "fwd") for r in gpu.H_ROWS]))
BF16_ROWS = list(dict.fromkeys([(c[0], c[1]) for c in gpu.CASES if c[3] in BF16_FAMILIES] + [(r[0], "fwd") for r in gpu.H_ROWS]))


def row_id(row):
    g, op = row
    return f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}p{g[5]}-L{g[6]}-B{g[7]}-{op}"


def x_act_of(op):
    return ref.NONE if op == "dgrad" else ref.LEAKY


# ---- (1) ---------------------------------------------------------------------------------------------------------------------------
def direct(op, geom, x, w, dy):
    """the three ops of a layer written as loops over (sample, channels, tap, frame): (value, mag)"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    xs, ws, dys = ref.shapes(geom)
    out = np.zeros({"fwd": dys, "dgrad": xs, "wgrad": ws}[op])
    mag = np.zeros_like(out)
    Lout = dys[2]
    for b in range(B):
        for c in range(Cin):
            for o in range(Cout):
                for j in range(k):
                    for t in range(Lin if tr else Lout):
                        xi, yi = (t, t * s - p + j) if tr else (t * s - p + j, t)       # frame of x, frame of y
                        if not (0 <= xi < Lin and 0 <= yi < Lout):
                            continue
                        wi = (c, o, j) if tr else (o, c, j)
                        if op == "fwd":
                            term, at = float(x[b, c, xi]) * float(w[wi]), (b, o, yi)
                        elif op == "dgrad":
                            term, at = float(dy[b, o, yi]) * float(w[wi]), (b, c, xi)
                        else:
                            term, at = float(x[b, c, xi]) * float(dy[b, o, yi]), wi
                        out[at] += term
                        mag[at] += abs(term)
    return out, mag


TINY = [(False, 3, 4, 4, 2, 1, 9, 2), (False, 2, 3, 7, 3, 2, 11, 2), (False, 3, 2, 8, 1, 2, 6, 1), (False, 2, 2, 32, 2, 16, 10, 1),
        (False, 2, 3, 5, 2, 2, 8, 2), (True, 3, 4, 5, 2, 1, 4, 2), (True, 2, 3, 8, 2, 1, 3, 2), (True, 2, 3, 7, 3, 2, 5, 1),
        (True, 3, 2, 8, 1, 2, 5, 2), (True, 2, 2, 32, 2, 16, 4, 1), (True, 3, 2, 5, 2, 1, 1, 2)]


@pytest.mark.parametrize("geom", TINY)
def test_references_agree_with_a_direct_loop_over_taps(geom):
    for kind in ("white", "graded"):
        t = ref.make_inputs(geom, kind)
        for op in ("fwd", "dgrad", "wgrad"):
            for prec in ("fp32", "bf16"):
                for x_act in (ref.NONE, ref.LEAKY, ref.RELU):
                    value, mag = ref.conv64(op, geom, t["x"], t["w"], t["dy"], x_act, prec)
                    xa = ref.see(ref.act32(t["x"], x_act), prec)
                    want, wmag = direct(op, geom, xa, ref.see(t["w"], prec), ref.see(t["dy"], prec))
                    assert value.shape == want.shape and value.dtype == np.float64
                    assert np.all(np.abs(value - want) <= 1e-13 * wmag) and np.all(np.abs(mag - wmag) <= 1e-13 * wmag), (geom, kind, op, prec, x_act)
                    assert np.array_equal(mag == 0, wmag == 0)
    assert float(ref.SLOPE32[ref.LEAKY]) == float(np.float32(0.2)) and ref.act32(np.float32([-1.0, 0.0, 2.0]), ref.RELU).tolist() == [0.0, 0.0, 2.0]


def test_bf16_rounding_and_the_split_are_the_library_s():
    import torch
    v = np.concatenate([ref._noise(5, (4096,)), ref._noise(6, (4096,)) * np.float32(2.0 ** -20), np.float32([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -3.0e38])])
    want = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    assert np.array_equal(ref.bf16(v).view(np.uint32), want.view(np.uint32))
    hi, lo = ref.split(v)
    assert np.array_equal(hi, want) and np.array_equal(lo, torch.from_numpy(v - want).to(torch.bfloat16).float().numpy())
    assert np.all(np.abs(v.astype(np.float64) - hi - lo) <= 2.0 ** -17 * np.abs(v))          # 8 + 8 bits and two roundings
    assert np.array_equal(ref.hilo(v).astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_references_agree_with_float64_autograd_on_every_gpu_row(row):
    import torch
    import torch.nn.functional as F
    geom, op = row
    tr, Cin, Cout, k, s, p, Lin, B = geom
    conv = (lambda a, b: F.conv_transpose1d(a, b, stride=s, padding=p)) if tr else (lambda a, b: F.conv1d(a, b, stride=s, padding=p))
    for kind in gpu.KINDS:
        t = gpu.inputs(geom, kind)
        for prec in ("fp32", "bf16"):
            x_act = x_act_of(op)
            value, mag = ref.conv64(op, geom, t["x"], t["w"], t["dy"], x_act, prec)
            xa = torch.from_numpy(ref.see(ref.act32(t["x"], x_act), prec)).double().requires_grad_(True)
            wr = torch.from_numpy(ref.see(t["w"], prec)).double().requires_grad_(True)
            y = conv(xa, wr)
            if op == "fwd":
                want = y.detach().numpy()
            else:
                y.backward(torch.from_numpy(ref.see(t["dy"], prec)).double())
                want = (xa.grad if op == "dgrad" else wr.grad).numpy()
            assert np.all(np.abs(value - want) <= 1e-13 * mag), (row, kind, prec, float((np.abs(value - want) / np.where(mag > 0, mag, 1)).max()))


# ---- (2) ---------------------------------------------------------------------------------------------------------------------------
def segmented(A, Bm, mm=ref.seq32, parts=3, drop=None):
    """K in `parts` segments, each accumulated on its own and added afterwards in order (a stream-K split and its fixup);
    drop = (segment, index of the output elements that miss it) plants a lost segment"""
    K = A.shape[-1]
    cuts = [K * i // parts for i in range(parts + 1)]
    total = None
    for i in range(parts):
        seg = mm(np.ascontiguousarray(A[..., cuts[i]:cuts[i + 1]]), np.ascontiguousarray(Bm[..., cuts[i]:cuts[i + 1], :]))
        if drop is not None and drop[0] == i:
            seg[drop[1]] = 0.0
        total = seg if total is None else total + seg
    return total


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_honest_convolutions_pass(row):
    geom, op = row
    for kind in gpu.KINDS:
        t = gpu.inputs(geom, kind)
        x_act = x_act_of(op)
        for prec in ("fp32",) + (("bf16", "bf16x3") if row in BF16_ROWS else ()):
            value, mag = ref.conv64(op, geom, t["x"], t["w"], t["dy"], x_act, prec)
            A, Bm, shape = ref.gemm(op, geom, t["x"], t["w"], t["dy"], x_act, prec)
            mm = ref.x3 if prec == "bf16x3" else ref.seq32
            plain = mm(A, Bm).reshape(shape)
            base = ref.errors(plain, value, mag)
            others = {"backwards": mm(A, Bm, reverse=True), "segmented": segmented(A, Bm, mm)}
            if prec == "fp32":
                others["torch"] = ref.torch32(op, geom, t["x"], t["w"], t["dy"], x_act)
            assert ref.accept(base, base)
            for name, got in others.items():
                err = ref.errors(got.reshape(shape), value, mag)
                assert ref.accept(err, base), (row, kind, prec, name, err, base)
            if op == "dgrad":                                   # the fused epilogue on a mask source with zeros of both signs
                for mask in (ref.LEAKY, ref.RELU):
                    v2, m2 = ref.dgrad_epilogue64(value, mag, t["add"], t["refz"], mask)
                    b2 = ref.errors(ref.dgrad_epilogue32(plain, t["add"], t["refz"], mask), v2, m2)
                    for name, got in others.items():
                        err = ref.errors(ref.dgrad_epilogue32(got.reshape(shape), t["add"], t["refz"], mask), v2, m2)
                        assert ref.accept(err, b2), (row, kind, prec, name, mask, err, b2)
                    if mask == ref.RELU:
                        assert bool(np.all(m2[t["refz"] <= 0] == 0)) and b2["zeros"]
            if op == "fwd":                                     # the store activations
                for act in (ref.LEAKY, ref.RELU):
                    b2 = ref.errors(ref.act32(plain, act), ref.act64(value, act), mag)
                    for name, got in others.items():
                        assert ref.accept(ref.errors(ref.act32(got.reshape(shape), act), ref.act64(value, act), mag), b2), (row, kind, prec, name, act)


# ---- (3) ---------------------------------------------------------------------------------------------------------------------------
PLANT = (False, 24, 40, 8, 1, 2, 33, 3)             # a Conv1d, k = 8: forward K = 192 (12 slabs of 16), dgrad K = 320; 3 x 30 columns
OLD_TOL = 1e-4                                      # tests/test_ops_gpu.py: TOL, of the tensor's max-abs, against fp32 torch


def low_rows():
    """the output rows of PLANT whose grade (the graded input's power of two on w's row) is at most 2^-6"""
    low = np.flatnonzero(ref.grades(PLANT)["w"] <= -6)
    assert 4 <= low.size <= 20, low
    return low


def _fwd(t):
    return ref.gemm("fwd", PLANT, t["x"], t["w"], None)


def f_demoted(t):
    A, Bm, shape = _fwd(t)
    return ref.x3(A, Bm).reshape(shape)


def f_rounded_rows(t):
    A, Bm, shape = _fwd(t)
    A = A.copy()
    A[0, low_rows()] = ref.bf16(A[0, low_rows()])
    return ref.seq32(A, Bm).reshape(shape)


def f_wrong_tap(t):
    A, Bm, shape = _fwd(t)
    k, o = PLANT[3], int(low_rows()[0])
    taps = A.reshape(A.shape[1], -1, k).copy()
    taps[o, :, :-1] = taps[o, :, 1:]
    return ref.seq32(taps.reshape(A.shape), Bm).reshape(shape)


def f_dropped_slab(t):
    A, Bm, shape = _fwd(t)
    A = A.copy()
    A[0, low_rows(), -16:] = 0.0
    return ref.seq32(A, Bm).reshape(shape)


def f_dropped_segment(t):
    A, Bm, shape = _fwd(t)
    index = (np.full_like(low_rows(), 1), low_rows())                  # sample 1's columns of the low-grade rows: one tile's corner
    return segmented(A, Bm, drop=(1, index)).reshape(shape)


def f_halo(t):
    A, Bm, shape = _fwd(t)
    y = ref.seq32(A, Bm).reshape(shape)
    out = y.copy()
    out[1:, :, 0] += np.float32(2.0 ** -10) * y[:-1, :, -1]
    return out


def f_y2_slope(t):
    A, Bm, shape = _fwd(t)
    return ref.act32(ref.seq32(A, Bm).reshape(shape), ref.LEAKY)       # stored as y2, which asked for ReLU


def f_mask_at_zero(t):
    A, Bm, shape = ref.gemm("dgrad", PLANT, None, t["w"], t["dy"])
    return ref.dgrad_epilogue32(ref.seq32(A, Bm).reshape(shape), t["add"], t["mask_source"], ref.LEAKY, at_zero=1.0)


def want_of(fault, t, zeros_in_ref):
    """(value, mag, honest fp32 stand-in, fp32 torch reference) of the call the fault sits in"""
    t = dict(t, mask_source=t["refz"] if zeros_in_ref else t["ref"])
    if fault is f_mask_at_zero:
        value, mag = ref.conv64("dgrad", PLANT, None, t["w"], t["dy"])
        value, mag = ref.dgrad_epilogue64(value, mag, t["add"], t["mask_source"], ref.LEAKY)
        ep = lambda g: ref.dgrad_epilogue32(g, t["add"], t["mask_source"], ref.LEAKY)
        return t, value, mag, ep(ref.standin("dgrad", PLANT, None, t["w"], t["dy"])), ep(ref.torch32("dgrad", PLANT, None, t["w"], t["dy"]))
    value, mag = ref.conv64("fwd", PLANT, t["x"], t["w"], None)
    honest, torch_ = ref.standin("fwd", PLANT, t["x"], t["w"], None), ref.torch32("fwd", PLANT, t["x"], t["w"], None)
    if fault is f_y2_slope:
        return t, ref.act64(value, ref.RELU), mag, ref.act32(honest, ref.RELU), ref.act32(torch_, ref.RELU)
    return t, value, mag, honest, torch_


def verdicts(fault):
    """{"new white", "new graded", "old white", "old graded"} -> accepted?  The new criterion sees the mask source with zeros of both
    signs; the older tests never put one there (tests/test_z_conv_views_gpu.py asserts ref != 0), so the older criterion sees none."""
    out = {}
    for kind in ("white", "graded"):
        t, value, mag, honest, _ = want_of(fault, gpu.inputs(PLANT, kind), True)
        out["new " + kind] = ref.accept(ref.errors(fault(t), value, mag), ref.errors(honest, value, mag))
        t, _, _, _, torch_ = want_of(fault, gpu.inputs(PLANT, kind), False)
        got = fault(t).astype(np.float64)
        out["old " + kind] = bool(np.abs(got - torch_).max() / np.abs(torch_).max() < OLD_TOL)
    return out


# The faults that name a grade sit at fixed row indices (the rows whose grade is low on the graded input), so they are present on the
# white input too, at full scale: there the older criterion rejects them, and the column to read is "old on graded" -- given the very
# input that has small rows, a max-abs bound still accepts.  (A fault that FOLLOWED the grade -- one that fires only where a channel
# is small -- would not fire on white noise at all, and the older suite, which has no other input, would accept it for that reason.)
A_, R_ = True, False            # accepted / rejected
# fault: (function, new on white, new on graded, old on white -- the suite's own input --, old criterion on the graded input)
FAULTS = {
    "fp32 demoted to the bf16x3 split": (f_demoted, R_, R_, A_, A_),
    "w rounded to bf16 in the output rows of grade <= 2^-6": (f_rounded_rows, R_, R_, R_, A_),
    "tap j + 1 for j in one output row of low grade": (f_wrong_tap, R_, R_, R_, A_),
    "the last K slab dropped in the rows of low grade": (f_dropped_slab, R_, R_, R_, A_),
    "one stream-K segment dropped in a tile corner of low-grade rows": (f_dropped_segment, R_, R_, R_, A_),
    "the neighbouring sample's last column added to the first at 2^-10": (f_halo, R_, R_, R_, R_),
    "mask act'(0) = 1 in place of the slope": (f_mask_at_zero, R_, R_, A_, A_),
    "y2 stored with y's slope (LeakyReLU for ReLU)": (f_y2_slope, R_, R_, R_, R_),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_faults_are_rejected(fault):
    fn, *expected = FAULTS[fault]
    v = verdicts(fn)
    word = lambda ok: "accepts" if ok else "REJECTS"
    print(f"\nFAULT {fault}: new criterion {word(v['new white'])} on white, {word(v['new graded'])} on graded; "
          f"old criterion (1e-4 of max-abs) {word(v['old white'])} on white, {word(v['old graded'])} on graded")
    assert not v["new white"] or not v["new graded"], (fault, v)
    assert [v["new white"], v["new graded"], v["old white"], v["old graded"]] == expected, (fault, v)


def test_the_low_grade_rows_are_invisible_to_a_max_abs_bound():
    """why the older criterion accepts on the graded input: every element of a row of grade <= 2^-6 is below 1e-4 of the tensor's
    maximum there, so the row may hold anything of its own size"""
    t = gpu.inputs(PLANT, "graded")
    value, _ = ref.conv64("fwd", PLANT, t["x"], t["w"], None)
    assert float(np.abs(value[:, low_rows()]).max()) < OLD_TOL * float(np.abs(value).max())


# ---- (4) ---------------------------------------------------------------------------------------------------------------------------
FP32_ROWS = list(dict.fromkeys((c[0], c[1]) for c in gpu.CASES))


def assert_fp32_bound_rejects_the_split(row):
    geom, op = row
    for kind in gpu.KINDS:
        t = gpu.inputs(geom, kind)
        for x_act in ((ref.NONE, ref.LEAKY) if op == "fwd" else (x_act_of(op),)):           # the operands of the GPU module's calls
            value, mag = ref.conv64(op, geom, t["x"], t["w"], t["dy"], x_act)
            A, Bm, shape = ref.gemm(op, geom, t["x"], t["w"], t["dy"], x_act)
            b = ref.errors(ref.seq32(A, Bm).reshape(shape), value, mag)
            c = ref.errors(ref.x3(A, Bm).reshape(shape), value, mag)
            assert c["r_rms"] >= 10.0 * b["r_rms"], (row, kind, x_act, b, c)
            assert not ref.accept(c, b)


def test_precision_rows_separate_fp32_from_the_split_by_10():
    skipped = []
    for row in FP32_ROWS:
        geom, op = row
        if not gpu.precision_row(geom, op):
            skipped.append(f"{row_id(row)} (K = {ref.gemm_k(geom, op)})")
            continue
        assert_fp32_bound_rejects_the_split(row)
    print("\nrows without the precision check (GEMM K above 512; every other check is kept):")
    for s in skipped:
        print("  " + s)
    assert skipped == ["C136-130-k8s2p1-L62-B2-fwd (K = 1088)", "C160-136-k8s1p2-L65-B3-dgrad (K = 1088)", "T250-96-k8s2p6-L129-B2-dgrad (K = 768)"], skipped


def test_split_rows_all_keep_the_precision_mark():
    """the rows of tests/test_z_fixup_splits_gpu.py (SPLIT_CASES: the multi-tile work splits) have GEMM K <= 512, every one: the fp32
    bound of their value tests rejects the bf16x3 split"""
    from test_kernel_families import SPLIT_CASES
    for row in dict.fromkeys((c[0], c[1]) for c in SPLIT_CASES):
        assert gpu.precision_row(*row), row
        assert_fp32_bound_rejects_the_split(row)


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------
def test_the_rows_cover_every_family_op_precision_and_work_split():
    """tests/test_kernel_families.py pins each VIEW_CASES row's plan to the family, epilogue and fixup form the row names; here: the
    rows the value module takes from it hold every family x op of the issue under a split and an unsplit schedule, with a
    [precision] row for each at fp32, and the resident forward's rows at both schedules are conv_h3 with and without a fixup."""
    from phasegen import _lib, ops
    import test_kernel_families as tk
    # the rows the value module adds to VIEW_CASES: their plan is the family, epilogue and fixup form they name, at every precision
    assert gpu.CASES[:len(VIEW_CASES)] == VIEW_CASES and gpu.CASES[len(VIEW_CASES):] == gpu.ADDED_CASES
    for case in gpu.ADDED_CASES:
        geom, op, sched, fam, epi, form = case
        assert case not in VIEW_CASES and fam in BF16_FAMILIES and gpu.precision_row(geom, op)
        for prec in (0, 1, 2):
            d = ops.conv_describe(tk._view_args(_lib, case, None, prec), tk._opcode(_lib, case))
            f = tk._fields(d)
            assert (tk.family(d), tk._epilogue(d), f["fixup"], f["split"]) == (fam, epi, form, "1") and "tail" not in f, (case, prec, d)
    want = {(f, o) for f in ("conv_raw3", "conv_raw(128x256)", "conv_raw(tall 256x128)", "conv_f", "conv_t") for o in ("fwd", "dgrad")}
    want |= {(f, "wgrad") for f in ("conv_g", "conv_g_raw", "conv_g_ps")}
    for split in (True, False):
        have = {(c[3], c[1]) for c in gpu.CASES if (c[5] in ("plain", "wide")) == split and gpu.precision_row(c[0], c[1])}
        assert have >= want, (split, want - have)
    assert {c[3] for c in gpu.CASES if c[3] in BF16_FAMILIES} == set(BF16_FAMILIES)
    assert len({fixup_case_id(c) for c in gpu.CASES}) == len(gpu.CASES)
    for geom, epi, sched in gpu.H_ROWS:
        tr, Cin, Cout, k, s, p, Lin, B = geom
        a = _lib.ConvhArgs()
        a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad, a.transposed = B, Cin, Cout, Lin, k, s, p, int(tr)
        a.Lout = ref.out_len(tr, Lin, k, s, p)
        a.x_pitch = ops.h_pitch(Lin)
        a.x_bs = Cin * a.x_pitch
        a.x = a.w = a.y = 4096
        a.y_bs = Cout * a.Lout
        a.workspace, a.workspace_bytes = 4096, _lib.load().pg_workspace_bytes_conv()
        a.schedule = sched
        d = ops.conv_fwd_h_describe(a)
        fields = dict(kv.split("=", 1) for kv in d.split("|")[1:])
        assert d.startswith("conv_h3_kernel<") and (fields["fixup"] == "none") == (sched == 1) and fields["split"] == ("0" if sched == 1 else "1"), (geom, sched, d)
        assert ref.gemm_k(geom, "fwd") <= ref.PRECISION_K
