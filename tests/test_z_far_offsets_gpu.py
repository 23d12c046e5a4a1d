"""GPU: every 64-bit stride field of include/phasegen.h with row 1 of its tensor placed past 2^31 bytes, 2^32 bytes, 2^31 elements and
2^32 elements from row 0 (tests/_far.py: one 16 GiB arena of sentinel NaNs, stride classes A, A', B, C, D).

Expected value: THE BITS OF THE SAME CALL ON COMPACT STRIDES in the same residue class mod 4 elements, base pointers in the same
residue class mod 16 bytes -- the plan and the vector / scalar path are then the same, and the compact forms are the ones the value
modules (test_z_conv_values_gpu, test_z_signal_values_gpu, test_z_norm_edges_gpu, test_z_pointwise_gpu, ...) hold to float64.  No
tolerance is introduced here.  After every call the whole arena is scanned: every non-sentinel word must lie inside a declared window
of the call, so a store through a truncated index is counted wherever it landed.

The convs GATHER x / dy (and the dgrad's addend and mask source) through buffer descriptors with 31-bit offsets; the host refuses what
does not fit.  Those fields run at the largest accepted extent (compact bits), one element past it (refused, outputs untouched), and
-- the addend and the mask source -- in every class (refused before launch, or compact bits: never other values).

Length classes (the arena zero-filled, random data in windows at the head, around every threshold and in an odd tail): pg_fill,
pg_standardize, pg_moments and pg_wave_compare over 2^31 + 2^19 + 3 elements, pg_adam_step on four arrays whose byte offsets pass 2^32,
pg_polar with input and output of 2^31 + 2^19 floats each, and pg_stft_crops with crops that straddle the thresholds of its flat buffer.

GPU_FIELDS is the table the coverage gate of tests/test_far_offsets_host.py holds against phasegen/_lib.py.  A library call that
returns a hipError_t, or a synchronise that raises, ends the session (pytest.exit): nothing more may start on the device after a fault.

The module is named to be collected behind the value modules: where both fail, theirs is the broader finding."""
import ctypes
import time

import numpy as np
import pytest

import _far
from _far import CLASSES
from test_kernel_families import FIXUP_CASES_H, VIEW_CASES

pytestmark = pytest.mark.gpu
LIMIT = ("limit",)                   # a gathered conv operand: the largest accepted extent and one element past it
WORDS_MAX = 0x1ffffffb               # (0x7ffffff0 - 4) / 4: the largest extent in floats the conv descriptors take

CONV_FWD, CONV_DGRAD, CONV_WGRAD = ("pg_conv1d_fwd", "pg_convt1d_fwd"), ("pg_conv1d_dgrad", "pg_convt1d_dgrad"), ("pg_conv1d_wgrad", "pg_convt1d_wgrad")
GPU_FIELDS = {}
for _s in CONV_FWD:
    GPU_FIELDS.update({(_s, "y_bs"): CLASSES, (_s, "y2_bs"): CLASSES, (_s, "x_bs"): LIMIT})
for _s in CONV_DGRAD:
    GPU_FIELDS.update({(_s, "dx_bs"): CLASSES, (_s, "dy_bs"): LIMIT, (_s, "dx_add_bs"): CLASSES + LIMIT, (_s, "dx_ref_bs"): CLASSES + LIMIT})
for _s in CONV_WGRAD:
    GPU_FIELDS.update({(_s, "x_bs"): LIMIT, (_s, "dy_bs"): LIMIT})
GPU_FIELDS.update({("pg_conv_fwd_h", f): CLASSES for f in ("y_bs", "yh_bs", "yh2_bs")})
GPU_FIELDS[("pg_conv_fwd_h", "x_bs")] = LIMIT
GPU_FIELDS.update({("pg_bn_fwd", f): CLASSES for f in ("x_bs", "y_bs", "y2_bs", "yh_bs", "yh2_bs")})
GPU_FIELDS.update({("pg_bn_bwd", f): CLASSES for f in ("x_bs", "dy_bs", "dx_bs")})
GPU_FIELDS.update({("pg_clipnorm_fwd", f): CLASSES for f in ("x_bs", "y_bs", "y2_bs", "yh_bs", "yh2_bs")})
GPU_FIELDS.update({("pg_cast_rows_bf16", f): CLASSES for f in ("x_bs", "y_bs")})
GPU_FIELDS.update({("pg_istft", f): CLASSES for f in ("a_bs", "b_bs")})
GPU_FIELDS.update({("pg_stft", "src_stride"): CLASSES, ("pg_stft", "src_len"): CLASSES})      # src_len: one long row, chunk_start far
GPU_FIELDS.update({("pg_resample", f): CLASSES for f in ("x_stride", "y_stride")})
GPU_FIELDS.update({("pg_stitch", f): CLASSES for f in ("clip_stride", "track_stride", "out_stride")})
GPU_FIELDS.update({("pg_spec_clips", "p_stride"): CLASSES})
GPU_FIELDS.update({("pg_phase_join", f): CLASSES for f in ("clip_stride", "ch_stride", "row_pitch")})
GPU_FIELDS.update({(s, f): CLASSES for s in ("pg_phase_vocoder", "pg_phase_lock") for f in ("a_stride", "m_stride")})
GPU_FIELDS.update({("pg_phase_lock_linked", "a_stride"): CLASSES, ("pg_phase_spsi", "m_stride"): CLASSES, ("pg_hpss", "m_stride"): CLASSES})
GPU_FIELDS.update({("pg_ola_stretch", f): CLASSES for f in ("x_stride", "y_stride", "base_stride")})
GPU_FIELDS.update({("pg_wave_compare", f): CLASSES for f in ("x_stride", "y_stride")})
GPU_FIELDS.update({("pg_spec_compare", f): CLASSES for f in ("r_stride", "e_stride")})

REACHED = set()                      # (symbol, field, class) of every case that passed
STATS = {}


def dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def rnd(seed, *shape):
    import torch
    from phasegen import detgen
    return torch.from_numpy(detgen.uniform(seed, shape, -1.0, 1.0))


@pytest.fixture(scope="module")
def arena():
    import torch
    free, total = torch.cuda.mem_get_info()
    need = _far.arena_words() * 4 + (8 << 30)
    print(f"\nfar offsets: {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB; arena {_far.arena_words() * 4 / 2**30:.3f} GiB + 8 GiB wanted")
    if free < need:
        pytest.skip(f"far offsets: {free / 2**30:.1f} GiB free, {need / 2**30:.1f} GiB needed")
    t0 = time.time()
    words = torch.empty(_far.arena_words(), dtype=torch.int32, device=dev())
    ar = _far.Arena(words)
    guarded(lambda _: ar.fill(), None)
    assert ar.foreign() == 0
    print(f"far offsets: arena filled and scanned in {time.time() - t0:.2f} s")
    STATS["t0"] = time.time()
    yield ar
    print(f"\nfar offsets: {ar.scans} arena scans; module wall time {time.time() - STATS['t0']:.1f} s")
    ar.words = None
    del words
    torch.cuda.empty_cache()


class Refused(Exception):
    pass


def guarded(fn, lanes):
    """fn(lanes) and a synchronise.  A negative return code (PG_ERR_*: refused before any launch) raises Refused; a hipError_t from the
    library, or a synchronise that raises, ends the session."""
    import torch
    from phasegen import _lib
    codes, check = [], _lib.check

    def spy(rc, what=""):
        codes.append(rc)
        return check(rc, what)

    _lib.check = spy
    try:
        fn(lanes)
    except RuntimeError as e:
        if codes and codes[-1] < 0:
            raise Refused(str(e))
        pytest.exit(f"far offsets: a call failed on the device ({e}); nothing more may start after a fault", returncode=3)
    finally:
        _lib.check = check
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"far offsets: synchronise raised ({e}); nothing more may start after a fault", returncode=3)


def same(a, b):
    return a.shape == b.shape and bool((a == b).all())


def run_case(arena, cls, fn, reached, S=None, what="", refusal=None, same_bits=False):
    """the call on compact strides, then on far ones in the arena: same bits, nothing outside the windows.  refusal: None = the far call
    must run; "must" = it must be refused before launch with the outputs untouched; "may" = refused so, or compact bits.
    same_bits: the header promises the same bits on the 16-byte and the element-by-element path, so class A' (the scalar path) must
    also give the bits of the ALIGNED compact call, class A's."""
    S = _far.strides()[cls] if S is None else S
    compact = _far.Lanes(arena, S, far=False)
    guarded(fn, compact)
    want = compact.results()
    assert want and not all(same(w, i) for w, i in zip(want, compact.initial)), (what, "the compact call wrote nothing")
    far = _far.Lanes(arena, S, far=True)
    try:
        try:
            guarded(fn, far)
        except Refused as e:
            assert refusal in ("must", "may"), (what, cls, str(e))
            assert "exceeds 2 GiB" in str(e), (what, cls, str(e))
            assert arena.foreign() == 0
            assert all(same(r, i) for r, i in zip(far.results(), far.initial)), (what, cls, "a refused call wrote to an output")
        else:
            assert refusal != "must", (what, cls, "accepted")
            got = far.results()
            _far.check_rows(arena, got, want, f"{what} class {cls}")
            if same_bits and cls == "A'":
                aligned = _far.Lanes(arena, _far.strides()["A"], far=False)
                guarded(fn, aligned)
                assert all(same(g, w) for g, w in zip(got, aligned.results())), (what, "the scalar path differs from the 16-byte path")
    finally:
        arena.reset()
    REACHED.update((s, f, cls) for s, f in reached)


# ---- conv ---------------------------------------------------------------------------------------------------------------------------------
def _conv_rows():
    """one row per (op, kernel family, epilogue, schedule) of VIEW_CASES: its smallest geometry, at B = 2 -- but the column-tail rows,
    whose plan needs their columns, as they are (their classes: those in which B - 1 strides still fit the arena).
    tests/test_far_offsets_host.py holds every row's plan to the family and epilogue its id names."""
    best = {}
    for geom, op, sched, fam, epi, form in VIEW_CASES:
        tr, Cin, Cout, k, s, p, Lin, B = geom
        key = (op, fam, epi, sched, geom if form == "tail" else None)
        size = Cin * Lin + Cout * ((Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1)
        if key not in best or size < best[key][0]:
            best[key] = (size, ((tr, Cin, Cout, k, s, p, Lin, B if form == "tail" else 2), op, sched, fam, epi, "tail" if form == "tail" else "any"))
    return [v[1] for v in best.values()]


CONV_ROWS = _conv_rows()


def fits(row, cls):
    """all B rows of a far tensor of this row lie inside the arena in class cls"""
    return (row[0][7] - 1) * _far.strides()[cls] + 8 * _far.LANE < _far.arena_words()      # (a conv call places at most 5 views, a lane each)


def row_classes(rows):
    return [pytest.param(r, c, id=f"{conv_id(r)}-{c}") for r in rows for c in CLASSES if fits(r, c)]


def conv_id(r):
    g = r[0]
    return f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}-L{g[6]}-B{g[7]}-{r[1]}-{r[2]:#x}-{r[3]}-{r[4]}"


def conv_fn(row, far=(), S_of=None, adam=False, add=None):
    """the row's call with the operands named in `far` on far strides (S_of: {name: stride of its own}).  add: None, "views" (addend
    and mask source as tensors of their own) or "inplace" (phasegen/unet.py: the addend IS dx)"""
    (tr, Cin, Cout, k, s, p, Lin, B), op, sched = row[:3]
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    wshape = (Cin, Cout, k) if tr else (Cout, Cin, k)
    x, w, dy = rnd(61, B, Cin, Lin), rnd(62, *wshape) * 0.1, rnd(63, B, Cout, Lout)
    S_of = S_of or {}

    def fd(name):
        return dict(far_dims=(0,) if name in far else (), S=S_of.get(name))

    def fn(L):
        from phasegen import ops
        kw = dict(transposed=tr, precision="fp32", schedule=sched)
        wd = L.dense("w", wshape, data=w)
        if op == "fwd":
            ops.conv_fwd(L.view("x", (B, Cin, Lin), data=x, **fd("x")), wd, L.view("y", (B, Cout, Lout), out=True, **fd("y")), s, p,
                         x_act=ops.ACT_LEAKY, y_act=ops.ACT_LEAKY, y2=L.view("y2", (B, Cout, Lout), out=True, **fd("y2")), y2_act=ops.ACT_RELU, **kw)
        elif op == "dgrad":
            dyv = L.view("dy", (B, Cout, Lout), data=dy, **fd("dy"))
            if add == "inplace":
                dxv = L.view("dx", (B, Cin, Lin), data=rnd(64, B, Cin, Lin), out=True, **fd("dx"))
                ops.conv_dgrad(dyv, wd, dxv, s, p, add=dxv, ref=L.view("ref", (B, Cin, Lin), data=rnd(65, B, Cin, Lin), **fd("ref")), mask=ops.ACT_LEAKY, **kw)
            elif add == "views":
                ops.conv_dgrad(dyv, wd, L.view("dx", (B, Cin, Lin), out=True, **fd("dx")), s, p, add=L.view("add", (B, Cin, Lin), data=rnd(64, B, Cin, Lin), **fd("add")),
                               ref=L.view("ref", (B, Cin, Lin), data=rnd(65, B, Cin, Lin), **fd("ref")), mask=ops.ACT_RELU, **kw)
            else:
                ops.conv_dgrad(dyv, wd, L.view("dx", (B, Cin, Lin), out=True, **fd("dx")), s, p, **kw)
        else:
            xv, dyv = L.view("x", (B, Cin, Lin), data=x, **fd("x")), L.view("dy", (B, Cout, Lout), data=dy, **fd("dy"))
            dw = L.dense("dw", wshape, out=True)
            if adam:
                pw, m, v = L.dense("p", wshape, data=w, out=True), L.dense("m", wshape, data=rnd(66, *wshape) * 0.01, out=True), L.dense("v", wshape, data=rnd(67, *wshape).abs() * 1e-4, out=True)
                ops.conv_wgrad(xv, dyv, dw, s, p, x_act=ops.ACT_LEAKY, adam=ops.adam_args(pw, m, v, 3), **kw)
            else:
                ops.conv_wgrad(xv, dyv, dw, s, p, x_act=ops.ACT_LEAKY, **kw)
    return fn


def _sym(row):
    return "pg_conv" + ("t" if row[0][0] else "") + "1d_" + row[1]


@pytest.mark.parametrize("row,cls", row_classes([r for r in CONV_ROWS if r[1] != "wgrad"]))
def test_conv_outputs_far(arena, row, cls):
    """y and y2 of a forward, dx of a dgrad: stored through 64-bit batch offsets by the GEMM kernels' epilogues and the fixup"""
    names = ("y", "y2") if row[1] == "fwd" else ("dx",)
    run_case(arena, cls, conv_fn(row, far=names), [(_sym(row), n + "_bs") for n in names], what=conv_id(row))


@pytest.mark.parametrize("form", ["views", "inplace"])
@pytest.mark.parametrize("row,cls", row_classes([r for r in CONV_ROWS if r[1] == "dgrad"]))
def test_conv_dgrad_addend_and_mask_source_far(arena, row, cls, form):
    """the skip gradient and the mask source are read through descriptors at 32-bit offsets b * bs + m * L + t: compact bits, or refused
    before launch -- never other values.  (Every class passes 2^31 bytes, so every class is refused: "conv: dx_add / dx_ref exceeds
    2 GiB".)"""
    far = ("add", "ref", "dx") if form == "views" else ("dx", "ref")
    run_case(arena, cls, conv_fn(row, far=far, add=form), [(_sym(row), "dx_add_bs"), (_sym(row), "dx_ref_bs")], what=conv_id(row) + " " + form, refusal="may")


def _limits(row, form=None):
    """{operand read through a descriptor: the largest batch stride the row's call accepts}: x / dy, and with form "views" the dgrad's
    addend and mask source, with "inplace" dx (which IS the addend) and the mask source"""
    (tr, Cin, Cout, k, s, p, Lin, B), op = row[:2]
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    ext = {"x": Cin * Lin, "dy": Cout * Lout, "add": Cin * Lin, "ref": Cin * Lin, "dx": Cin * Lin}
    names = {"fwd": ("x",), "dgrad": ("dy",), "wgrad": ("x", "dy")}[op] + {None: (), "views": ("add", "ref"), "inplace": ("dx", "ref")}[form]
    return {n: (WORDS_MAX - ext[n]) // (B - 1) for n in names}


LIMIT_CASES = ([(r, False, None) for r in CONV_ROWS] + [(r, True, None) for r in CONV_ROWS if r[1] == "wgrad"]
               + [(r, False, f) for r in CONV_ROWS if r[1] == "dgrad" for f in ("views", "inplace")])


@pytest.mark.parametrize("row,adam,form", LIMIT_CASES, ids=lambda v: conv_id(v) if isinstance(v, tuple) else ("adam" if v is True else "plain" if v is False else str(v)))
def test_conv_gathered_operands_at_and_past_the_limit(arena, row, adam, form):
    """x / dy -- and the dgrad's addend and mask source, as views of their own and in the engine's in-place form -- with
    ((B - 1) bs + C L) * 4 = 0x7fffffec bytes at B = 2, the last extent the descriptors take: the offsets of the last sample sit
    just under 2^31, where adding the out-of-range constants of conv_common.h (FAR, OOB) must not wrap back into range and the
    epilogue's (b * bs + off) * 4 must not overflow.  Compact bits; one element more on any of them is refused and leaves the outputs
    untouched."""
    lim = _limits(row, form)
    sym = _sym(row)
    fields = [(sym, {"add": "dx_add_bs", "ref": "dx_ref_bs", "dx": "dx_add_bs"}.get(n, n + "_bs")) for n in lim]
    run_case(arena, "limit", conv_fn(row, far=tuple(lim), S_of=lim, adam=adam, add=form), fields, S=0, what=conv_id(row) + f" {form} at the limit")
    for n in lim:
        past = dict(lim)
        past[n] += 1
        run_case(arena, "limit", conv_fn(row, far=tuple(lim), S_of=past, adam=adam, add=form), [], S=0, what=conv_id(row) + f" {form} {n} past the limit",
                 refusal="must")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("geom", [c[0] for c in FIXUP_CASES_H], ids=lambda g: f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}")
def test_conv_fwd_h_outputs_far(arena, geom, cls):
    import torch
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, _ = geom
    B = 2
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    w = (rnd(52, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1).to(dev())
    xh = ops.h_alloc(B, Cin, Lin, dev())
    ops.cast_rows_bf16(rnd(51, B, Cin, Lin).to(dev()), xh)
    wh = ops.shadow_weights(w, tr, s)
    pitch = ops.h_pitch(Lout)

    def fn(L):
        ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, transposed=tr, y=L.view("y", (B, Cout, Lout), out=True),
                       yh=L.view("yh", (B, Cout, pitch), dtype=torch.bfloat16, out=True), yh_act=ops.ACT_LEAKY,
                       yh2=L.view("yh2", (B, Cout, pitch), dtype=torch.bfloat16, out=True), yh2_act=ops.ACT_RELU, schedule=2)
    run_case(arena, cls, fn, [("pg_conv_fwd_h", f) for f in ("y_bs", "yh_bs", "yh2_bs")], what=f"conv_fwd_h {geom}")


@pytest.mark.parametrize("geom", [c[0] for c in FIXUP_CASES_H], ids=lambda g: f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}")
def test_conv_fwd_h_x_at_and_past_the_limit(arena, geom):
    """bf16 x with ((B - 1) x_bs + Cin x_pitch) * 2 at the last even batch stride below 0x7ffffff0 bytes: compact bits; the next even
    stride is refused.  Every sample carries its PG_H_HEAD zero elements in front and its zero row tails, as ops.h_alloc lays them out."""
    import torch
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, _ = geom
    B = 2
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    w = (rnd(52, *((Cin, Cout, k) if tr else (Cout, Cin, k))) * 0.1).to(dev())
    xh0 = ops.h_alloc(B, Cin, Lin, dev())
    ops.cast_rows_bf16(rnd(51, B, Cin, Lin).to(dev()), xh0)
    wh = ops.shadow_weights(w, tr, s)
    pitch, opitch, head = ops.h_pitch(Lin), ops.h_pitch(Lout), ops.H_HEAD
    rows = torch.cat([torch.zeros(B, head, dtype=torch.bfloat16, device=dev()), xh0.reshape(B, Cin * pitch)], 1)
    top = (0x7ffffff0 - 2) // 2 - Cin * pitch
    top -= top % 2

    def fn_at(x_bs):
        def fn(L):
            v = L.view("xh", (B, head + Cin * pitch), dtype=torch.bfloat16, data=rows, S=x_bs)
            xh = torch.as_strided(v, (B, Cin, pitch), (v.stride(0), pitch, 1), v.storage_offset() + head)
            ops.conv_fwd_h(xh, Lin, wh, tuple(w.shape), s, p, transposed=tr, y=L.view("y", (B, Cout, Lout), far_dims=(), out=True),
                           yh=L.view("yh", (B, Cout, opitch), far_dims=(), dtype=torch.bfloat16, out=True), yh_act=ops.ACT_LEAKY, schedule=2)
        return fn
    run_case(arena, "limit", fn_at(top), [("pg_conv_fwd_h", "x_bs")], S=0, what=f"conv_fwd_h {geom} x at the limit")
    run_case(arena, "limit", fn_at(top + 2), [], S=0, what=f"conv_fwd_h {geom} x past the limit", refusal="must")


# ---- norm, cast ------------------------------------------------------------------------------------------------------------------------
NORM_SHAPE = (2, 3, 44)              # L = 44: the float4 path on aligned strides, with 11 units per row; A' takes the scalar path


def _norm_views(L_, x):
    import torch
    from phasegen import ops
    B, Cc, L = NORM_SHAPE
    pitch = ops.h_pitch(L)
    return dict(x=L_.view("x", NORM_SHAPE, data=x), y=L_.view("y", NORM_SHAPE, out=True), y2=L_.view("y2", NORM_SHAPE, out=True),
                yh=L_.view("yh", (B, Cc, pitch), dtype=torch.bfloat16, out=True), yh2=L_.view("yh2", (B, Cc, pitch), dtype=torch.bfloat16, out=True))


@pytest.mark.parametrize("cls", CLASSES)
def test_bn_fwd_far(arena, cls):
    from phasegen import ops
    B, Cc, L = NORM_SHAPE
    x = rnd(34, B, Cc, L)

    def fn(L_):
        v = _norm_views(L_, x)
        ops.bn_fwd(v["x"], v["y"], L_.dense("gamma", (Cc,), data=rnd(35, Cc) + 2.0), L_.dense("beta", (Cc,), data=rnd(36, Cc)),
                   L_.dense("sm", (Cc,), out=True), L_.dense("si", (Cc,), out=True), y_act=ops.ACT_LEAKY, y2=v["y2"], y2_act=ops.ACT_RELU,
                   yh=v["yh"], yh_act=ops.ACT_LEAKY, yh2=v["yh2"], yh2_act=ops.ACT_RELU)
    run_case(arena, cls, fn, [("pg_bn_fwd", f) for f in ("x_bs", "y_bs", "y2_bs", "yh_bs", "yh2_bs")], what="bn_fwd")


@pytest.mark.parametrize("cls", CLASSES)
def test_clipnorm_fwd_far(arena, cls):
    from phasegen import ops
    B, Cc, L = NORM_SHAPE
    x = rnd(34, B, Cc, L)

    def fn(L_):
        v = _norm_views(L_, x)
        ops.clipnorm_fwd(v["x"], v["y"], L_.dense("gamma", (Cc,), data=rnd(35, Cc) + 2.0), L_.dense("beta", (Cc,), data=rnd(36, Cc)),
                         y_act=ops.ACT_LEAKY, y2=v["y2"], y2_act=ops.ACT_RELU, yh=v["yh"], yh_act=ops.ACT_LEAKY, yh2=v["yh2"], yh2_act=ops.ACT_RELU)
    run_case(arena, cls, fn, [("pg_clipnorm_fwd", f) for f in ("x_bs", "y_bs", "y2_bs", "yh_bs", "yh2_bs")], what="clipnorm_fwd")


@pytest.mark.parametrize("cls", CLASSES)
def test_bn_bwd_far(arena, cls):
    from phasegen import ops
    B, Cc, L = NORM_SHAPE
    x, dy = rnd(34, B, Cc, L), rnd(37, B, Cc, L)

    def fn(L_):
        ops.bn_bwd(L_.view("x", NORM_SHAPE, data=x), L_.view("dy", NORM_SHAPE, data=dy), L_.view("dx", NORM_SHAPE, out=True),
                   L_.dense("gamma", (Cc,), data=rnd(35, Cc) + 2.0), L_.dense("sm", (Cc,), data=rnd(38, Cc) * 0.1), L_.dense("si", (Cc,), data=rnd(39, Cc) * 0.1 + 1.7),
                   L_.dense("dgamma", (Cc,), out=True), L_.dense("dbeta", (Cc,), out=True))
    run_case(arena, cls, fn, [("pg_bn_bwd", f) for f in ("x_bs", "dy_bs", "dx_bs")], what="bn_bwd")


@pytest.mark.parametrize("cls", CLASSES)
def test_cast_rows_bf16_far(arena, cls):
    import torch
    from phasegen import ops
    B, Cc, L = 2, 3, 45
    x = rnd(51, B, Cc, L)

    def fn(L_):
        ops.cast_rows_bf16(L_.view("x", (B, Cc, L), data=x), L_.view("y", (B, Cc, ops.h_pitch(L)), dtype=torch.bfloat16, out=True), act=ops.ACT_LEAKY)
    run_case(arena, cls, fn, [("pg_cast_rows_bf16", f) for f in ("x_bs", "y_bs")], what="cast_rows_bf16")


# ---- stft, istft ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cls", CLASSES)
def test_istft_far(arena, cls, mode):
    from phasegen import ops
    bins, hop, frames, signals = 16, 8, 8, 2
    a = rnd(810, signals, bins, frames).abs() if mode == 0 else rnd(810, signals, bins, frames)
    b = rnd(811, signals, bins, frames) * 3.0

    def fn(L):
        ops.istft(L.view("a", (signals, bins, frames), data=a), L.view("b", (signals, bins, frames), data=b), hop, mode=mode, normalize=True,
                  out=L.dense("audio", (signals, hop * (frames - 1)), out=True))
    run_case(arena, cls, fn, [("pg_istft", "a_bs"), ("pg_istft", "b_bs")], what=f"istft mode {mode}")


@pytest.mark.parametrize("form", ["rows", "one-long-row"])
@pytest.mark.parametrize("cls", CLASSES)
def test_stft_chunked_source_far(arena, cls, form):
    """rows: two source rows src_stride apart, a chunk from each.  one-long-row: ONE row of src_len = S + 200 samples with a chunk at its
    head and one that begins S samples in and runs off the end of the row (the rest reads as zero)."""
    import torch
    from phasegen import _lib, ops
    n_fft, hop, row, chunk = 32, 8, 200, 96
    y = rnd(77, 2, row)

    def fn(L):
        v = L.view("y", (2, row), data=y)
        S = v.stride(0)
        if form == "rows":
            start, rows, src_len, src_stride = [5, 61], [0, 1], row, S
        else:
            start, rows, src_len, src_stride = [5, S + 140], [0, 0], S + row, S + row
        dummy = torch.empty(1, src_len if form == "rows" else 1, device=dev())
        a, out = ops._stft_args(dummy, n_fft, hop, polar=True, out=L.dense("out", (2, 2, n_fft // 2, 1 + chunk // hop), out=True),
                                chunk_start=torch.tensor(start, dtype=torch.int64, device=dev()),
                                chunk_row=torch.tensor(rows, dtype=torch.int32, device=dev()), chunk_len=chunk)
        a.y, a.src_len, a.src_stride = v.data_ptr(), src_len, src_stride
        _lib.check(_lib.load().pg_stft(ctypes.byref(a), ops._stream()), "stft")
    run_case(arena, cls, fn, [("pg_stft", "src_stride" if form == "rows" else "src_len")], what=f"stft {form}")


# ---- track kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_resample_far(arena, cls):
    from phasegen import _lib, ops
    n_in = 301
    n_out = _lib.load().pg_resample_out_len(n_in, 160, 441)
    x = rnd(91, 2, n_in)
    run_case(arena, cls, lambda L: ops.resample(L.view("x", (2, n_in), data=x), 441, 160, out=L.view("y", (2, n_out), out=True)),
             [("pg_resample", "x_stride"), ("pg_resample", "y_stride")], what="resample")


@pytest.mark.parametrize("form", ["clips", "tracks"])
@pytest.mark.parametrize("cls", CLASSES)
def test_stitch_far(arena, cls, form):
    """clips: one track whose two clips lie clip_stride apart.  tracks: two tracks of three clips track_stride apart, rows of out
    out_stride apart."""
    from phasegen import ops
    T, step = 64, 48
    n_tracks, n_clips = (1, 2) if form == "clips" else (2, 3)
    n_out = (n_clips - 1) * step + T - 3
    c = rnd(92, n_tracks, n_clips, T)

    def fn(L):
        clips = L.view("clips", (n_tracks, n_clips, T), far_dims=(1,) if form == "clips" else (0,), data=c)
        out = L.view("out", (n_tracks, n_out), out=True) if form == "tracks" else L.dense("out", (1, n_out), out=True)
        ops.stitch(clips, step, n_out, normalize=True, out=out)
    run_case(arena, cls, fn, [("pg_stitch", "clip_stride")] if form == "clips" else [("pg_stitch", "track_stride"), ("pg_stitch", "out_stride")], what=f"stitch {form}", same_bits=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_spec_clips_far(arena, cls):
    from phasegen import ops
    plane = rnd(93, 2, 5, 44)
    run_case(arena, cls, lambda L: ops.spec_clips(L.view("P", (2, 5, 44), data=plane), 3, 16, 12, src_per_out=0.9, out=L.dense("out", (3, 2, 5, 16), out=True)),
             [("pg_spec_clips", "p_stride")], what="spec_clips", same_bits=True)


@pytest.mark.parametrize("field,shape,far_dim", [("clip_stride", (2, 2, 3, 16), 0), ("ch_stride", (1, 2, 3, 16), 1), ("row_pitch", (1, 1, 2, 16), 2)])
@pytest.mark.parametrize("cls", CLASSES)
def test_phase_join_far(arena, cls, field, shape, far_dim):
    """each of the three strides far on its own (two of them at once would put a row past 2 * 2^32 elements: beyond the arena)"""
    from phasegen import ops
    phi = rnd(94, *shape) * 3.0
    n_clips, n_ch, bins, frames = shape
    run_case(arena, cls, lambda L: ops.phase_join(L.view("phi", shape, far_dims=(far_dim,), data=phi), 12, out=L.dense("out", (n_ch, bins, (n_clips - 1) * 12 + frames), out=True)),
             [("pg_phase_join", field)], what=f"phase_join {field}", same_bits=True)


STRETCH = dict(n_ch=2, bins=5, F_out=40, spo=1 / 1.5)


def _planes():
    from test_z_lock_gpu import f_src_for, planes
    import torch
    F_src = f_src_for(STRETCH["F_out"], STRETCH["spo"])
    A, M = planes(3100, STRETCH["n_ch"], STRETCH["bins"], F_src)
    return torch.from_numpy(A), torch.from_numpy(M), (STRETCH["n_ch"], STRETCH["bins"], F_src), (STRETCH["n_ch"], STRETCH["bins"], STRETCH["F_out"])


@pytest.mark.parametrize("op", ["phase_vocoder", "phase_lock"])
@pytest.mark.parametrize("cls", CLASSES)
def test_vocoder_and_lock_far(arena, cls, op):
    from phasegen import ops
    A, M, shape, oshape = _planes()
    run_case(arena, cls, lambda L: getattr(ops, op)(L.view("A", shape, data=A), STRETCH["F_out"], STRETCH["spo"], logmag=L.view("M", shape, data=M),
                                                    reset_below=0.5, out=L.dense("out", oshape, out=True)),
             [("pg_" + op, "a_stride"), ("pg_" + op, "m_stride")], what=op, same_bits=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_phase_lock_linked_far(arena, cls):
    from phasegen import ops
    A, M, shape, oshape = _planes()
    ref = (1,) + shape[1:]
    run_case(arena, cls, lambda L: ops.phase_lock_linked(L.view("A", shape, data=A), L.dense("Aref", ref, data=A[:1]), L.dense("Mref", ref, data=M[:1]),
                                                         STRETCH["F_out"], STRETCH["spo"], reset_below=0.5, out=L.dense("out", oshape, out=True)),
             [("pg_phase_lock_linked", "a_stride")], what="phase_lock_linked", same_bits=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_phase_spsi_far(arena, cls):
    from phasegen import ops
    A, M, shape, oshape = _planes()
    run_case(arena, cls, lambda L: ops.phase_spsi(L.view("M", shape, data=M), 32, 8, out=L.dense("out", shape, out=True)), [("pg_phase_spsi", "m_stride")], what="phase_spsi", same_bits=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_hpss_far(arena, cls):
    from phasegen import ops
    A, M, shape, oshape = _planes()
    run_case(arena, cls, lambda L: ops.hpss(L.view("M", shape, data=M), 5, 3, out=(L.dense("harm", shape, out=True), L.dense("perc", shape, out=True))),
             [("pg_hpss", "m_stride")], what="hpss", same_bits=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_ola_stretch_far(arena, cls):
    from phasegen import ops
    n_in, n_out = 600, 801
    x, base = rnd(95, 2, n_in), rnd(96, 2, n_out)
    run_case(arena, cls, lambda L: ops.ola_stretch(L.view("x", (2, n_in), data=x), n_out, 0.75, win_len=64, hop=16, base=L.view("base", (2, n_out), data=base),
                                                   out=L.view("y", (2, n_out), out=True)),
             [("pg_ola_stretch", f) for f in ("x_stride", "y_stride", "base_stride")], what="ola_stretch", same_bits=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_wave_compare_far(arena, cls):
    import torch
    from phasegen import ops
    n = 8192 + 37
    x = rnd(41, 2, n)
    y = 0.8 * x + 0.05 * rnd(42, 2, n)
    run_case(arena, cls, lambda L: ops.wave_compare(L.view("x", (2, n), data=x), L.view("y", (2, n), data=y), out=L.dense("out", (2, 6), dtype=torch.float64, out=True)),
             [("pg_wave_compare", "x_stride"), ("pg_wave_compare", "y_stride")], what="wave_compare", same_bits=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_spec_compare_far(arena, cls):
    import torch
    from phasegen import ops
    shape = (2, 2, 9, 37)
    R = rnd(43, *shape)
    E = 0.9 * R + 0.1 * rnd(44, *shape)
    run_case(arena, cls, lambda L: ops.spec_compare(L.view("R", shape, data=R), L.view("E", shape, data=E), gain=1.1, out=L.dense("out", (2, 6), dtype=torch.float64, out=True)),
             [("pg_spec_compare", "r_stride"), ("pg_spec_compare", "e_stride")], what="spec_compare", same_bits=True)


# ---- crops of one flat buffer that straddle the thresholds ------------------------------------------------------------------------------------
def test_stft_crops_straddle_the_thresholds(arena):
    """pg_stft_crops on the arena as its flat training buffer: crops that begin 70 samples in front of 2^31 bytes, 2^32 bytes and 2^31
    elements of src, one near its head, and one that runs off its crop_end 20 samples past 2^31 elements.  Expected: the bits of the same
    crops copied into a small buffer at begins in the same residue class mod 4."""
    import torch
    from phasegen import ops
    n, n_fft, hop = 150, 32, 8
    begins = [66] + [t - 70 for t in (2**29, 2**30, 2**31)]
    crops = [(0, 10**4), (1, 10**4), (2, 10**4), (3, 10**4), (3, 90)]          # (region, crop_end - crop_begin)
    data = rnd(78, len(begins), n).to(dev())

    def call(src, at):
        cb = torch.tensor([at[r] for r, _ in crops], dtype=torch.int64, device=dev())
        ce = torch.tensor([at[r] + e for r, e in crops], dtype=torch.int64, device=dev())
        for r, b in enumerate(at):
            src[b:b + n].copy_(data[r])
        out = []
        guarded(lambda _: out.append(ops.stft_crops(src, cb, ce, n, n_fft, hop, polar=True, stats=(0.1, 1.3))), None)
        return out[0]

    small = torch.empty(256 * len(begins) + 512, dtype=torch.int32, device=dev())
    small.fill_(_far.SENT)
    at_c = [66 + 256 * r for r in range(len(begins))]
    assert all(a % 4 == b % 4 for a, b in zip(at_c, begins))
    want = call(small.view(torch.float32), at_c)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    try:
        for b in begins:
            arena.declare(b, n)
        got = call(arena.words.view(torch.float32), begins)
        assert arena.foreign() == 0
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    finally:
        arena.reset()


# ---- length classes: n past 2^31 elements (pg_fill, pg_standardize), byte offsets past 2^32 (pg_adam_step) ---------------------------------
N_LONG = 2**31 + 2**19 + 3           # 3 mod 4: the scalar tail loop runs past the threshold
N_ADAM = 2**30 + 2**18 + 3
GPU_FIELDS.update({("pg_fill", "arg1"): ("n",), ("pg_standardize", "arg1"): ("n",), ("pg_adam_step", "n"): ("n",), ("pg_wave_compare", "n"): ("n",),
                   ("pg_moments", "n"): ("n",), ("pg_polar", "n_items"): ("n",), ("pg_polar", "inner"): ("n",)})


def length_windows(n):
    """(first element, elements): the head, 264 elements around every threshold below n, and the tail.  Every window begins at a multiple
    of 4 and all but the tail hold whole float4 units; the tail ends with the array's three scalar elements -- so the call on a window
    alone (aligned) takes every element through the same path as the call on the whole array"""
    assert n % 4 == 3
    return [(0, 256)] + [(t - 132, 264) for t in (2**29, 2**30, 2**31) if t + 132 < n - 259] + [(n - 259, 259)]


@pytest.fixture()
def zeroed(arena):
    """the arena zero-filled for a length case, and the sentinel again afterwards"""
    guarded(lambda _: arena.fill(0), None)
    yield arena
    guarded(lambda _: arena.fill(), None)


def count_not(words, lo, hi, value):
    return sum(int((words[a:min(a + (1 << 28), hi)] != value).sum()) for a in range(lo, hi, 1 << 28))


def test_fill_past_2_to_the_31_elements(zeroed):
    import torch
    from phasegen import ops
    words = zeroed.words
    guarded(lambda _: ops.fill(words.view(torch.float32)[:N_LONG], 3.5), None)
    bits = int(np.array([3.5], np.float32).view(np.int32)[0])
    assert count_not(words, 0, N_LONG, bits) == 0 and count_not(words, N_LONG, zeroed.n, 0) == 0
    REACHED.add(("pg_fill", "arg1", "n"))


def test_standardize_past_2_to_the_31_elements(zeroed):
    """in place over 2^31 + 2^19 + 3 elements: the windows hold the bits of the call on the window alone, every other element the one value
    a zero maps to, and nothing behind the array changes"""
    import torch
    from phasegen import ops
    words = zeroed.words
    x = words.view(torch.float32)
    stats = torch.tensor([0.25, 2.0], dtype=torch.float64, device=dev())
    wins = length_windows(N_LONG)
    data = [rnd(300 + i, m).to(dev()) for i, (_, m) in enumerate(wins)]
    want = []
    for d in data + [torch.zeros(4)]:
        c = d.to(dev()).clone()
        assert c.data_ptr() % 16 == 0
        guarded(lambda _: ops.standardize_stats_(c, stats), None)
        want.append(c)
    zero_bits = int(want[-1].view(torch.int32)[0])
    assert bool((want[-1].view(torch.int32) == zero_bits).all())
    for (lo, m), d in zip(wins, data):
        x[lo:lo + m].copy_(d)
    guarded(lambda _: ops.standardize_stats_(x[:N_LONG], stats), None)
    for (lo, m), w in zip(wins, want):
        assert torch.equal(x[lo:lo + m].view(torch.int32), w.view(torch.int32)), (lo, m)
    inside = sum(count_not(words, lo, lo + m, zero_bits) for lo, m in wins)
    assert count_not(words, 0, N_LONG, zero_bits) == inside and count_not(words, N_LONG, zeroed.n, 0) == 0
    REACHED.add(("pg_standardize", "arg1", "n"))


@pytest.mark.parametrize("thin", [False, True], ids=["wide", "thin"])
def test_adam_step_with_byte_offsets_past_2_to_the_32(zeroed, thin):
    """p, g, m, v of 2^30 + 2^18 + 3 elements in the four quarters of the arena: the windows hold the bits of the step on the window
    alone, g is unchanged, and every other word of the arena is still zero (a zero parameter with a zero gradient stays +0.0)"""
    import torch
    from phasegen import ops
    words = zeroed.words
    f = words.view(torch.float32)
    Q = 2**30 + 2**19
    wins = length_windows(N_ADAM)
    kw = dict(lr=1e-3, grad_scale=0.5, thin=thin)
    arrs = [f[k * Q:k * Q + N_ADAM] for k in range(4)]                 # p, g, m, v
    want = []
    for i, (lo, m) in enumerate(wins):
        d = [rnd(400 + i, m).to(dev()), rnd(410 + i, m).to(dev()), (rnd(420 + i, m) * 0.01).to(dev()), (rnd(430 + i, m).abs() * 1e-4).to(dev())]
        for a, t in zip(arrs, d):
            a[lo:lo + m].copy_(t)
        guarded(lambda _: ops.adam_step(d[0], d[1], d[2], d[3], 3, **kw), None)
        want.append(d)
    guarded(lambda _: ops.adam_step(arrs[0], arrs[1], arrs[2], arrs[3], 3, **kw), None)
    inside = 0
    for (lo, m), d in zip(wins, want):
        for k, (a, t) in enumerate(zip(arrs, d)):
            assert torch.equal(a[lo:lo + m].view(torch.int32), t.view(torch.int32)), (lo, m, "pgmv"[k])
            inside += count_not(words, k * Q + lo, k * Q + lo + m, 0)
    assert count_not(words, 0, zeroed.n, 0) == inside
    REACHED.add(("pg_adam_step", "n", "n"))


def test_moments_past_2_to_the_31_elements(zeroed):
    """pg_moments over 2^31 + 2^19 + 3 elements, zero but for the windows, against the float64 closed form: mean = sum(w) / n and
    std^2 = (sum((w - mean)^2) + (n - len(w)) mean^2) / n.  Bounds: those tests/test_signal_gpu.py::test_standardize_matches_numpy
    holds the same two numbers to -- 1e-11 max(1, |mean|) and 1e-11 std."""
    import torch
    from phasegen import ops
    x = zeroed.words.view(torch.float32)
    wins = length_windows(N_LONG)
    data = [rnd(600 + i, m) * 3.0 + 1.5 for i, (_, m) in enumerate(wins)]
    for (lo, m), d in zip(wins, data):
        x[lo:lo + m].copy_(d)
    stats = torch.full((2,), -77.0, dtype=torch.float64, device=dev())
    guarded(lambda _: ops.moments(x[:N_LONG], stats), None)
    got = stats.cpu().numpy()
    w = torch.cat(data).numpy().astype(np.float64)
    mean = w.sum() / N_LONG
    std = np.sqrt((((w - mean) ** 2).sum() + (N_LONG - w.size) * mean * mean) / N_LONG)
    print(f"\nmoments n = 2^31 + 2^19 + 3: mean {got[0]!r} (float64 {mean!r}), std {got[1]!r} (float64 {std!r})")
    assert abs(got[0] - mean) < 1e-11 * max(1.0, abs(mean)) and abs(got[1] - std) < 1e-11 * std
    inside = sum(count_not(zeroed.words, lo, lo + m, 0) for lo, m in wins)
    assert count_not(zeroed.words, 0, zeroed.n, 0) == inside                # the input is untouched, nothing else was written
    REACHED.add(("pg_moments", "n", "n"))


@pytest.mark.parametrize("inner", [8, 3], ids=["float4", "scalar"])
def test_polar_with_element_offsets_past_2_to_the_31(zeroed, inner):
    """pg_polar addresses it * 2 * inner + r: with n_items * inner just above 2^30 + 2^18 the input and the output span 2^31 + 2^19 floats
    each and lie in the two halves of the arena (the issue's n_items * inner = 2^31 + 2^19 + 3 would need two arenas).  Windows of 16
    items at the head, around 2^29, 2^30 and 2^31 elements and at the tail hold the bits of the call on the window alone; every other
    output word is the one value a zero pair maps to; the input is unchanged."""
    import torch
    from phasegen import ops
    f = zeroed.words.view(torch.float32)
    n_items = -(-(2**30 + 2**18 + 3) // inner)
    span, Y0 = n_items * 2 * inner, 2**31 + 2**20
    assert span > 2**31 + 2**19 and Y0 + span <= zeroed.n and Y0 >= span
    firsts = [0] + [t // (2 * inner) - 8 for t in (2**29, 2**30, 2**31)] + [n_items - 16]
    want, zero = [], None
    for i, it in enumerate(firsts):
        d = (rnd(700 + i, 16, 2, 1, inner) * 4.0).to(dev())
        f[it * 2 * inner:(it + 16) * 2 * inner].copy_(d.view(-1))
        out = torch.empty_like(d)
        guarded(lambda _: ops.polar(d, out=out), None)
        want.append(out)
    z = torch.zeros(4, 2, 1, inner, device=dev())
    zo = torch.full_like(z, -77.0)
    guarded(lambda _: ops.polar(z, out=zo), None)
    zero = int(zo.view(torch.int32).view(-1)[0])
    assert bool((zo.view(torch.int32) == zero).all())                       # magnitude and angle of (0, 0): one value
    guarded(lambda _: ops.polar(f[:span].view(n_items, 2, 1, inner), out=f[Y0:Y0 + span].view(n_items, 2, 1, inner)), None)
    words, inside_in, inside_out = zeroed.words, 0, 0
    for it, w in zip(firsts, want):
        lo, hi = it * 2 * inner, (it + 16) * 2 * inner
        assert torch.equal(f[Y0 + lo:Y0 + hi].view(torch.int32), w.view(torch.int32).view(-1)), it
        inside_in += count_not(words, lo, hi, 0)
        inside_out += count_not(words, Y0 + lo, Y0 + hi, zero)
    assert count_not(words, 0, Y0, 0) == inside_in                          # the input, and the gap behind it
    assert count_not(words, Y0, Y0 + span, zero) == inside_out and count_not(words, Y0 + span, zeroed.n, 0) == 0
    REACHED.update({("pg_polar", "n_items", "n"), ("pg_polar", "inner", "n")})


def test_wave_compare_of_one_signal_past_2_to_the_31_elements(zeroed):
    """x and y of 2^31 + 2^19 + 3 samples in the two halves of the arena, zero but for the windows: zeros add exactly nothing to any of the
    six slots, so the float64 sums over the windows are the reference, at the bounds tests/test_compare_gpu.py holds these slots to"""
    import torch
    from phasegen import ops
    from test_compare_gpu import check_wave, wave_ref
    f = zeroed.words.view(torch.float32)
    Y0 = 2**31 + 2**20
    assert Y0 % 4 == 0 and Y0 + N_LONG <= zeroed.n
    wins = length_windows(N_LONG)
    xs = [rnd(500 + i, m) for i, (_, m) in enumerate(wins)]
    ys = [0.8 * x + 0.05 * rnd(520 + i, m) for i, (x, (_, m)) in enumerate(zip(xs, wins))]
    for (lo, m), x, y in zip(wins, xs, ys):
        f[lo:lo + m].copy_(x)
        f[Y0 + lo:Y0 + lo + m].copy_(y)
    out = torch.full((1, 6), -77.0, dtype=torch.float64, device=dev())
    guarded(lambda _: ops.wave_compare(f[:N_LONG], f[Y0:Y0 + N_LONG], gain=1.1, out=out), None)
    check_wave(out, wave_ref(torch.cat(xs)[None].numpy(), torch.cat(ys)[None].numpy(), gain=1.1), "wave_compare n = 2^31 + 2^19 + 3")
    inside = sum(count_not(zeroed.words, b + lo, b + lo + m, 0) for lo, m in wins for b in (0, Y0))
    assert count_not(zeroed.words, 0, zeroed.n, 0) == inside            # the inputs are untouched, nothing else was written
    REACHED.add(("pg_wave_compare", "n", "n"))


# ---- the list is complete ------------------------------------------------------------------------------------------------------------------
def test_zz_every_far_field_was_reached_by_a_passing_case(arena):
    """every (symbol, field) of GPU_FIELDS ran in every class it lists, in a case that passed (a deselected or failed case leaves its
    entry out: run the module whole)"""
    missing = sorted((s, f, c) for (s, f), classes in GPU_FIELDS.items() for c in classes if (s, f, c) not in REACHED)
    assert not missing, missing
