"""What the exponent range does to an entry point (include/phasegen.h, "Magnitude range"): the four rules as comparisons of arrays,
and the conditions a case must meet before its rule says anything.  numpy only.

  M1  scale equivariance.  Every operand times an exact power of two, every operand element and every reference output still a
      normal fp32 number (or an exact zero): the outputs are the clean call's outputs times the product of the powers, BIT FOR BIT
      (`check_m1`); an output the formula makes scale-free keeps the clean call's bits (`check_m1_invariant`).  No tolerance.
  M2  gradual underflow.  Operands normal, every reference output below FLT_MIN: |got - ref64| <= B 2^e + R 2^-150 (`check_m2`).
      B 2^e is the bound the family's value module asserts, carried along with the total scale 2^e; R counts the roundings on one
      output's path, each of which moves a denormal result by at most half the denormal spacing, 2^-150.
  M3  denormal operands (`check_m3`).  Two float64 restatements, "kept" (on the values actually stored) and "flushed" (every
      operand element below FLT_MIN replaced by a zero of its sign); the caller names the ONE the header states for the mode and
      every element is held to it within M2's bound.
  M4  overflow (`check_m4`).  S = sum |a b| in float64 along an output's sum.  S < FLT_MAX / 2: finite and within bound.
      |ref64| > FLT_MAX (1 + B): non-finite, with the reference's sign (`nan_ok`: or NaN, the bf16x3 split's inf - inf).
      Between the two: held to neither.

Every checker asserts the condition of its rule from the reference BEFORE it looks at the device's array, prints one RANGE line with
its counts, and raises AssertionError on a violation.  The caps on a case are conditions on the inputs, not measurements: an M2
case has at least half of its outputs non-zero in float64 and above R 2^-150 (`m2_case_ok`), an M4 case at least one output in
the finite zone, one in the overflow zone and at most a quarter in the middle (`m4_case_ok`).  Shared by tests/test_range_host.py
(numpy float32 stand-ins pass every rule, each planted fault fails the rule meant for it, every case of the table meets its
conditions on the float64 reference alone) and tests/test_z_range_gpu.py (the kernels)."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)            # 2^-126, the smallest normal
FLT_MAX = float(np.finfo(np.float32).max)
HALF_DENORM = 2.0 ** -150                             # half the spacing of the fp32 denormals
U = 2.0 ** -24


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def bf16(x):
    """fp32 -> bf16 (round to nearest even, denormals kept) -> fp32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32)


def scaled(a, e):
    """a 2^e in a's own type; asserts that no element was rounded, overflowed or underflowed on the way"""
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    want = np.ldexp(a.astype(np.float64), int(e))
    with np.errstate(over="ignore", under="ignore"):
        out = want.astype(a.dtype)
    assert np.array_equal(out.astype(np.float64), want), f"scaled(.., {e}): not exact"
    return out


def stored(a, e):
    """float32(a 2^e) as a store rounds it (round to nearest even into the denormals): the operand of an M3 case"""
    with np.errstate(under="ignore"):
        return np.ldexp(np.asarray(a, np.float32).astype(np.float64), int(e)).astype(np.float32)


def flushed(a):
    """every element below FLT_MIN replaced by a zero of its sign"""
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < np.float32(FLT_MIN), np.copysign(np.float32(0), a), a).astype(np.float32)


def is_normal_or_zero(a):
    m = np.abs(np.asarray(a, np.float64))
    return (m == 0) | ((m >= FLT_MIN) & (m <= FLT_MAX))


def operands_normal(operands, cast_bf16=False):
    """the operand half of M1's and M2's condition: every element a normal fp32 number or an exact zero (and so its bf16 rounding
    where the mode casts: bf16 has fp32's exponent range, so only a carry past FLT_MAX could leave it)"""
    for a in operands:
        a = np.asarray(a, np.float32)
        if not is_normal_or_zero(a).all():
            return False
        if cast_bf16 and not is_normal_or_zero(bf16(a)).all():
            return False
    return True


def _line(rule, tag, text):
    print(f"RANGE {rule} {tag}: {text}")


# ---- M1 ---------------------------------------------------------------------------------------------------------------------------
def check_m1(got_scaled, got_clean, ref_clean, e, operands=(), cast_bf16=False, out64=False, tag=""):
    """got_scaled == got_clean 2^e, bit for bit (signed zeros included).  Condition: operands normal, ref_clean 2^e normal or zero
    (out64: the outputs are doubles -- the compare kernels' sums -- and normal means a normal double).
    Returns {"n", "zeros", "differ"}."""
    gs, gc = np.asarray(got_scaled), np.asarray(got_clean)
    ref = np.asarray(ref_clean, np.float64)
    assert gs.shape == gc.shape == ref.shape, (tag, gs.shape, gc.shape, ref.shape)
    assert gs.dtype == gc.dtype and gs.dtype.kind == "f", (tag, gs.dtype, gc.dtype)
    assert operands_normal(operands, cast_bf16), f"{tag}: M1's condition, an operand element is not a normal number"
    rs = np.abs(np.ldexp(ref, int(e)))
    normal = ((rs == 0) | ((rs >= np.finfo(np.float64).tiny) & np.isfinite(rs))) if out64 else is_normal_or_zero(rs)
    assert np.isfinite(ref).all() and normal.all(), f"{tag}: M1's condition, a scaled reference output is not a normal number"
    with np.errstate(over="ignore", under="ignore"):
        want = np.ldexp(gc.astype(np.float64), int(e))
    g64 = gs.astype(np.float64)
    differ = ~((g64 == want) & (np.signbit(g64) == np.signbit(want)))
    n = {"n": int(gs.size), "zeros": int((ref == 0).sum()), "differ": int(differ.sum())}
    _line("M1", tag, f"scale 2^{int(e)}, {n['n']} outputs ({n['zeros']} exact zeros), {n['differ']} differ from the clean call's bits times the scale")
    if n["differ"]:
        i = tuple(np.argwhere(differ)[0])
        raise AssertionError(f"{tag}: M1, {n['differ']} of {n['n']} outputs are not the clean call's times 2^{int(e)}, first at {i}: "
                             f"{g64[i]!r} against {want[i]!r}")
    return n


def check_m1_invariant(got_scaled, got_clean, operands=(), cast_bf16=False, tag=""):
    """a scale-free output keeps the clean call's bits"""
    gs, gc = np.asarray(got_scaled), np.asarray(got_clean)
    assert gs.shape == gc.shape and gs.dtype == gc.dtype, (tag, gs.shape, gc.shape)
    assert operands_normal(operands, cast_bf16), f"{tag}: M1's condition, an operand element is not a normal number"
    differ = _bits(gs) != _bits(gc)
    _line("M1", tag, f"scale-free, {gs.size} outputs, {int(differ.sum())} differ from the clean call's bits")
    if differ.any():
        i = tuple(np.argwhere(differ)[0])
        raise AssertionError(f"{tag}: M1 (invariant), {int(differ.sum())} of {gs.size} outputs moved, first at {i}: {gs[i]!r} against {gc[i]!r}")
    return {"n": int(gs.size), "differ": 0}


# ---- M2 ---------------------------------------------------------------------------------------------------------------------------
def m2_case_ok(ref_scaled, R):
    """the cap on an M2 case: every reference output below FLT_MIN, at least half of them non-zero and above R 2^-150"""
    r = np.abs(np.asarray(ref_scaled, np.float64))
    return bool((r < FLT_MIN).all() and 2 * int((r > R * HALF_DENORM).sum()) >= r.size)


def check_m2(got, ref_scaled, bound_scaled, R, operands=(), cast_bf16=False, case_ref=None, tag=""):
    """|got - ref_scaled| <= bound_scaled + R 2^-150 per element; ref_scaled = ref64 2^e and bound_scaled = B 2^e come scaled.
    `case_ref`: the scaled reference the cap is counted on where `ref_scaled` is a ReLU copy of it (half of its elements are zeros by
    construction, not by underflow).
    A flushed zero where |ref_scaled| is above the bound is one of the violations and is counted by name."""
    g = np.asarray(got).astype(np.float64)
    ref, b = np.asarray(ref_scaled, np.float64), np.broadcast_to(np.asarray(bound_scaled, np.float64), np.shape(ref_scaled))
    assert g.shape == ref.shape, (tag, g.shape, ref.shape)
    assert operands_normal(operands, cast_bf16), f"{tag}: M2's condition, an operand element is not a normal number"
    assert (np.abs(ref) < FLT_MIN).all() and m2_case_ok(ref if case_ref is None else case_ref, R), f"{tag}: M2's condition, reference outputs at or above FLT_MIN, or fewer than half above R 2^-150"
    bound = b + R * HALF_DENORM
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(g - ref) <= bound)
    lost = bad & (g == 0)
    _line("M2", tag, f"{g.size} outputs below FLT_MIN, {int((np.abs(ref) > bound).sum())} above their bound (R = {R}); {int(bad.sum())} outside it, "
                     f"{int(lost.sum())} of them flushed to zero; worst |got - ref| / bound {float(np.nanmax(np.abs(g - ref) / bound)):.3f}")
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{tag}: M2, {int(bad.sum())} of {g.size} outputs outside B 2^e + R 2^-150 ({int(lost.sum())} flushed to zero), "
                             f"first at {i}: {g[i]!r} against {ref[i]!r}, bound {bound[i]:.3e}")
    return {"n": int(g.size), "bad": 0}


# ---- M3 ---------------------------------------------------------------------------------------------------------------------------
def check_m3(got, ref_kept, ref_flushed, bound, R, outcome, tag=""):
    """every element within bound + R 2^-150 of the restatement `outcome` names ("kept" or "flushed").  Condition: the two
    restatements are further apart than twice the bound in at least half of the elements the kept one does not make zero (a ReLU mask
    zeroes half of a dgrad's), so that one of them is excluded."""
    assert outcome in ("kept", "flushed"), outcome
    g = np.asarray(got).astype(np.float64)
    rk, rf = np.asarray(ref_kept, np.float64), np.asarray(ref_flushed, np.float64)
    assert g.shape == rk.shape == rf.shape, (tag, g.shape, rk.shape, rf.shape)
    bd = np.broadcast_to(np.asarray(bound, np.float64), g.shape) + R * HALF_DENORM
    apart = np.abs(rk - rf) > 2 * bd
    assert apart.any() and 2 * int(apart.sum()) >= int((rk != 0).sum()), f"{tag}: M3's condition, the kept and the flushed restatement are not apart"
    with np.errstate(invalid="ignore"):
        near_k, near_f = np.abs(g - rk) <= bd, np.abs(g - rf) <= bd
    want = near_k if outcome == "kept" else near_f
    _line("M3", tag, f"{g.size} outputs, {int(apart.sum())} tell the restatements apart; within bound of kept {int(near_k.sum())}, of flushed {int(near_f.sum())}; "
                     f"the header says {outcome}")
    if not want.all():
        i = tuple(np.argwhere(~want)[0])
        raise AssertionError(f"{tag}: M3, {int((~want).sum())} of {g.size} outputs are not the '{outcome}' restatement's "
                             f"(kept matches {int(near_k.sum())}, flushed {int(near_f.sum())}), first at {i}: {g[i]!r}, kept {rk[i]!r}, flushed {rf[i]!r}")
    return {"n": int(g.size), "kept": int(near_k.sum()), "flushed": int(near_f.sum())}


# ---- M4 ---------------------------------------------------------------------------------------------------------------------------
def m4_zones(ref_scaled, S_scaled, B_rel):
    """(finite, overflow, middle) bool arrays: S < FLT_MAX / 2; |ref| > FLT_MAX (1 + B_rel); neither"""
    ref, S = np.asarray(ref_scaled, np.float64), np.asarray(S_scaled, np.float64)
    finite = S < FLT_MAX / 2
    over = np.abs(ref) > FLT_MAX * (1.0 + B_rel)
    assert not (finite & over).any()
    return finite, over, ~finite & ~over


def m4_case_ok(ref_scaled, S_scaled, B_rel):
    finite, over, middle = m4_zones(ref_scaled, S_scaled, B_rel)
    return bool(finite.any() and over.any() and 4 * int(middle.sum()) <= middle.size)


def m4_exponent(ref, S, B_rel, lo=0, hi=260):
    """the total exponent e of an M4 case, from the float64 reference alone: the one in lo..hi with the fewest outputs in the middle
    zone among those that leave at least a quarter of the outputs in each of the other two (ties: the smallest); None if there is none"""
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    best = None
    for e in range(lo, hi + 1):
        with np.errstate(over="ignore"):
            finite, over, middle = m4_zones(np.ldexp(ref, e), np.ldexp(S, e), B_rel)
        if 4 * int(finite.sum()) >= ref.size and 4 * int(over.sum()) >= ref.size and (best is None or int(middle.sum()) < best[0]):
            best = (int(middle.sum()), e)
    return None if best is None else best[1]


def check_m4(got, ref_scaled, S_scaled, bound_scaled, B_rel, nan_ok=False, tag=""):
    """finite zone: finite and within bound_scaled; overflow zone: non-finite with the reference's sign (nan_ok: or NaN)"""
    g = np.asarray(got).astype(np.float64)
    ref = np.asarray(ref_scaled, np.float64)
    assert g.shape == ref.shape, (tag, g.shape, ref.shape)
    assert m4_case_ok(ref, S_scaled, B_rel), f"{tag}: M4's condition, a zone is empty or more than a quarter of the outputs lie in the middle"
    finite, over, middle = m4_zones(ref, S_scaled, B_rel)
    bd = np.broadcast_to(np.asarray(bound_scaled, np.float64), g.shape)
    with np.errstate(invalid="ignore"):
        bad_f = finite & ~(np.isfinite(g) & (np.abs(g - ref) <= bd))
        inf_ok = np.isinf(g) & (np.signbit(g) == np.signbit(ref))
        bad_o = over & ~(inf_ok | (np.isnan(g) if nan_ok else False))
    _line("M4", tag, f"{g.size} outputs: finite zone {int(finite.sum())} ({int(bad_f.sum())} violations), overflow zone {int(over.sum())} "
                     f"({int(bad_o.sum())} violations, {int((over & np.isnan(g)).sum())} NaN), middle {int(middle.sum())}")
    if bad_f.any():
        i = tuple(np.argwhere(bad_f)[0])
        raise AssertionError(f"{tag}: M4, {int(bad_f.sum())} outputs of the finite zone are non-finite or out of bound, first at {i}: {g[i]!r} against {ref[i]!r}")
    if bad_o.any():
        i = tuple(np.argwhere(bad_o)[0])
        raise AssertionError(f"{tag}: M4, {int(bad_o.sum())} outputs of the overflow zone are finite or of the wrong sign, first at {i}: {g[i]!r} against {ref[i]!r}")
    return {"finite": int(finite.sum()), "overflow": int(over.sum()), "middle": int(middle.sum())}


# ---- convolutions: the table of tests/test_z_range_gpu.py, the operands and references of a case -------------------------------------
CONV_M1 = [(40, 40), (-40, -40), (100, -100), (-100, 20)]          # (e_x, e_w); dy takes e_x's place in a dgrad, e_w's in a wgrad
CONV_M2 = (-70, -65)
CONV_M3 = [(-140, 100), (100, -140)]
# ... of the modes that round an operand to bf16: the smallest bf16 denormal is 2^-133, so an operand at 2^-140 rounds to zero whether
# the hardware keeps denormals or not and the case could not tell "kept" from "flushed" (`check_m3` asserts that it can).  There the
# exponent is the largest that still puts every element of the operand below FLT_MIN (`den_exponent`): the elements keep up to seven bits.
def den_exponent(a):
    """the largest e with max |a| 2^e < FLT_MIN"""
    m = float(np.abs(np.asarray(a, np.float64)).max())
    e = int(np.floor(np.log2(FLT_MIN / m)))
    while m * 2.0 ** e >= FLT_MIN:
        e -= 1
    return e


def conv_m3(prec, op, t):
    """the (e_a, e_b) pairs of a row's M3 cases"""
    if prec == "fp32":
        return CONV_M3
    a, b = {"fwd": ("x", "w"), "dgrad": ("dy", "w"), "wgrad": ("x", "dy")}[op]
    return [(den_exponent(t[a]), 100), (100, den_exponent(t[b]))]


def m3_denormal(scales):
    """the operands an M3 pair sends below FLT_MIN"""
    return [k for k, v in scales.items() if v <= -120]
M4_LADDER = (-4, -2, 0, 2, 4)                                      # exponents per channel of the M4 inputs
M4_EX = 60                                                         # e_x of an M4 case; e_w = e - e_x


def conv_scales(op, ex, ew):
    """{operand: exponent} and the output's exponent for a pair (e_a, e_b) of the op's two GEMM operands: fwd (x, w), dgrad (dy, w),
    wgrad (x, dy).  A dgrad's addend has the output's scale; its mask source is scaled with dy's exponent, but never into the denormals (any positive
    scale leaves the mask alone; a denormal one is a comparison with zero, which M3 does not cover)."""
    a, b = {"fwd": ("x", "w"), "dgrad": ("dy", "w"), "wgrad": ("x", "dy")}[op]
    out = {a: ex, b: ew}
    if op == "dgrad":
        out.update(add=ex + ew, ref=max(ex, -100))
    return out, ex + ew


def conv_roundings(K, prec):
    """R of a convolution output whose GEMM is K deep.  Per K index the fp32 path forms one product and adds it (2 roundings; an FMA:
    1), the bf16 path the same on rounded operands, the bf16x3 split three products and three additions (6).  A work split adds
    its partial sums once more: at most one addition per K index again (a partial holds at least one), so + K.  The epilogue adds
    the addend, multiplies by the mask's slope and applies the store activation's slope: 3.  An input activation's slope rounds the
    operand, not a denormal result, and is in B.  R = (2 t + 1) K + 3, t = 3 for bf16x3 and 1 otherwise."""
    t = 3 if prec == "bf16x3" else 1
    return (2 * t + 1) * int(K) + 3


def m4_inputs(geom, make_inputs):
    """the M4 inputs of a row: |noise| with a sign and a power of two from M4_LADDER per channel -- x[b, c, t] carries s_c 2^l_c,
    dy[b, o, t] s_o 2^l_o, w[o, c, j] s_o s_c 2^(l_o + l_c), add like x -- so that every term of one output has ONE sign, in all three ops:
    S = |ref|, every partial sum in any order lies between 0 and the total, and the sign of an overflowed output is a fact about
    the operation and not about the order the kernel adds in.  The ladder spreads the outputs over more binades than the middle
    zone is wide."""
    tr, Cin, Cout = geom[0], geom[1], geom[2]
    t = {k: np.abs(v) for k, v in make_inputs(geom, "white").items()}
    lad = np.array(M4_LADDER)
    f = lambda n, shift: (np.where((np.arange(n) + shift) % 2 == 0, 1.0, -1.0) * np.exp2(lad[(np.arange(n) * 2 + shift) % len(lad)])).astype(np.float32)
    fc, fo = f(Cin, 0), f(Cout, 1)
    t["x"] = t["x"] * fc[None, :, None]
    t["add"] = t["add"] * fc[None, :, None]
    t["dy"] = t["dy"] * fo[None, :, None]
    t["w"] = t["w"] * ((fc[:, None, None] * fo[None, :, None]) if tr else (fo[:, None, None] * fc[None, :, None]))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in t.items()}


def conv_rows(t, geom, op, variant, prec, standin=True, as_split=False):
    """{output name: (value, mag, standin)} of one call of tests/test_z_nonfinite_gpu._conv_variants on the operand set t ("x", "w",
    "dy", "add", "refz"): the float64 value and magnitude of tests/_conv_ref64.py and the honest fp32 stand-in of the precision, with
    the epilogue of the variant applied to all three as tests/test_z_conv_values_gpu.run_values applies it (standin=False: zeros in
    its place, for the cases that take their B from the row's clean call; as_split: the value and magnitude on float32(hi) + float32(lo)
    of every operand, activation applied first -- what the bf16x3 split makes of an operand, which for a denormal one is not the
    operand: lo = bf16(x - hi) has no bits left below 2^-133)"""
    import _conv_ref64 as cref
    name, x_act, mask = variant
    if as_split:
        value, mag = cref.conv64(op, geom, cref.hilo(cref.act32(t["x"], x_act)), cref.hilo(t["w"]), cref.hilo(t["dy"]), cref.NONE, "fp32")
    else:
        value, mag = cref.conv64(op, geom, t["x"], t["w"], t["dy"], x_act, "bf16" if prec == "bf16" else "fp32")
    base = cref.standin(op, geom, t["x"], t["w"], t["dy"], x_act, prec) if standin else np.zeros(value.shape, np.float32)
    return conv_epilogue(t, op, variant, value, mag, base)


def conv_epilogue(t, op, variant, value, mag, base):
    """the variant's epilogue on (value, mag, stand-in) of the op's plain sum: {output name: (value, mag, standin)}"""
    import _conv_ref64 as cref
    name, x_act, mask = variant
    if op == "fwd" and x_act == cref.LEAKY and not name.startswith("y("):         # ("y(leaky x)": the plain y of pg_conv_fwd_h)
        return {"y": (cref.act64(value, cref.LEAKY), mag, cref.act32(base, cref.LEAKY)), "y2": (cref.act64(value, cref.RELU), mag, cref.act32(base, cref.RELU))}
    if op == "dgrad" and mask is not None:
        v2, m2 = cref.dgrad_epilogue64(value, mag, t["add"], t["refz"], mask)
        return {"dx": (v2, m2, cref.dgrad_epilogue32(base, t["add"], t["refz"], mask))}
    return {{"fwd": "y", "dgrad": "dx", "wgrad": "dw"}[op]: (value, mag, base)}


def conv_bound(value, mag, standin):
    """B of a convolution output, per element and relative to nothing: MARGIN x the stand-in's r_max x u x mag -- what
    tests/test_z_conv_values_gpu.check asserts of r_max through tests/_conv_ref64.accept, taken unchanged.  Returns (bound, B_rel)
    with bound = B_rel mag."""
    import _conv_ref64 as cref
    base = cref.errors(standin, value, mag)
    b_rel = cref.MARGIN * base["r_max"] * cref.U
    return b_rel * mag, b_rel


def conv_operands(t, op, scales, how=None):
    """the operand set of a case: t with every operand the op reads times 2^scales[operand] -- exactly (`scaled`), or rounded as a
    store rounds it (`stored`) for the operands `how` names"""
    out = dict(t)
    for k, e in scales.items():
        src = "refz" if k == "ref" else k
        out[src] = (stored if how and k in how else scaled)(t[src], e)
    return out


def conv_k(geom, op):
    """the depth of the op's GEMM with the zeros it multiplies in: fwd Cin k, dgrad Cout k, wgrad B x frames"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    return {"fwd": Cin * k, "dgrad": Cout * k, "wgrad": B * max(Lin, Lout)}[op]


def conv_m2(t, geom, op, variant, prec, rows):
    """the M2 case of a variant from its clean `rows` (conv_rows of t): (T, operands, {name: (ref_scaled, bound_scaled, case_ref)}).
    The two GEMM operands are scaled exactly; a dgrad's addend has the output's scale, 2^-135, where it is a denormal itself: it is
    stored rounded, the reference adds the stored value, and it stays out of the operands the condition calls normal."""
    import _conv_ref64 as cref
    scales, e = conv_scales(op, *CONV_M2)
    add = scales.pop("add", None)
    T = conv_operands(t, op, scales)
    operands = [T["refz" if k == "ref" else k] for k in scales]
    out = {}
    if op == "dgrad" and variant[2] is not None:
        T["add"] = stored(t["add"], add)
        value, mag = cref.conv64(op, geom, t["x"], t["w"], t["dy"], variant[1], "bf16" if prec == "bf16" else "fp32")
        v2, m2 = cref.dgrad_epilogue64(np.ldexp(value, e), np.ldexp(mag, e), T["add"], t["refz"], variant[2])
        _, b_rel = conv_bound(*rows["dx"])
        out["dx"] = (v2, b_rel * m2, np.ldexp(value, e) + T["add"].astype(np.float64))       # (cap: before the mask, whose ReLU form zeroes half)
        return T, operands, out
    for n, (value, mag, base) in rows.items():
        bound, _ = conv_bound(value, mag, base)
        case_ref = None
        if n in ("y", "y2") and op == "fwd" and variant[1] == cref.LEAKY:           # (cap: before the store activation shrinks or zeroes the negatives)
            case_ref = np.ldexp(cref.conv64(op, geom, t["x"], t["w"], t["dy"], variant[1], "bf16" if prec == "bf16" else "fp32")[0], e)
        out[n] = (np.ldexp(value, e), np.ldexp(bound, e), case_ref)
    return T, operands, out


# ---- the M4 case of a conv row (numpy only: shared by the host and the GPU module) ---------------------------------------------------
import functools

M4_VARIANT = {"fwd": ("y", 0, None), "dgrad": ("dx", 0, None), "wgrad": ("dw(leaky x)", 1, None)}        # (name, x_act, mask): the plain sums


@functools.lru_cache(maxsize=None)
def conv_m4_exponent(geom, op, prec):
    """{"t", "value", "mag", "e", "B_worst"} of a row's M4 case, from float64 alone: the inputs of `m4_inputs` and the total exponent
    that leaves the fewest outputs between the zones.  B_worst = MARGIN (3 K + 256) u bounds every B the value module can assert
    here -- a sequential fp32 sum of K same-sign terms is within K u of exact, the split's dropped residuals within 128 u and its
    three sums within 3 K u -- and a larger B only narrows the overflow zone, so the case's condition holds for the real B."""
    import _conv_ref64 as cref
    t = m4_inputs(geom, cref.make_inputs)
    t["refz"] = t["ref"]                                    # (no M4 variant reads the mask source)
    value, mag = cref.conv64(op, geom, t["x"], t["w"], t["dy"], M4_VARIANT[op][1], "bf16" if prec == "bf16" else "fp32")
    b_worst = cref.MARGIN * (3 * conv_k(geom, op) + 256) * cref.U
    return {"t": t, "value": value, "mag": mag, "e": m4_exponent(value, mag, b_worst), "B_worst": b_worst}


@functools.lru_cache(maxsize=None)
def conv_m4_case(geom, op, prec):
    """the operands (x 2^60, the other operand 2^(e - 60)), the scaled reference, S, the bound and B of a row's M4 case"""
    m4 = conv_m4_exponent(geom, op, prec)
    t, e, variant = m4["t"], m4["e"], M4_VARIANT[op]
    name, (value, mag, base) = next(iter(conv_rows(t, geom, op, variant, prec).items()))
    bound, b_rel = conv_bound(value, mag, base)
    assert b_rel <= m4["B_worst"], (b_rel, m4["B_worst"])
    scales, _ = conv_scales(op, M4_EX, e - M4_EX)
    scales = {k: v for k, v in scales.items() if k not in ("add", "ref")}
    return {"T": conv_operands(t, op, scales), "variant": variant, "name": name, "e": e, "ref": np.ldexp(value, e), "S": np.ldexp(mag, e),
            "bound": np.ldexp(bound, e), "B_rel": b_rel}


def conv_variants(op, base):
    """the calls of an op: tests/test_z_nonfinite_gpu._conv_variants (`base`) and, for the operand activation the issue names beside
    LeakyReLU, a plain forward and a wgrad that read ReLU(x)"""
    extra = {"fwd": [("y(relu x)", 2, None)], "dgrad": [], "wgrad": [("dw(relu x)", 2, None)]}[op]
    return list(base) + extra
