"""CPU: which kernel family does the automatic choice (schedule = 0) reach, for every op x (k, stride) x size class the library serves?

pg_conv_describe / pg_conv_fwd_h_describe are pure functions of the call's arguments, so the whole map is computed without a GPU.  The
test pins the SET of families the automatic choice can reach -- a family nothing reaches is dead weight (round 3 carried three such:
conv_g3, conv_h's 128 x 256 and conv_h2's eight-wave tiles; removed in round 4) -- and prints the table DESIGN.md section 4.1 holds."""
import ctypes
import re

import pytest


def _args(_lib, B, Cin, Cout, Lin, k, s, p, tr, precision=0, schedule=0):
    a = _lib.ConvArgs()
    a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad = B, Cin, Cout, Lin, k, s, p
    a.Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    a.x = a.w = a.y = a.dy = a.dx = a.dw = 4096                      # never dereferenced: describe launches nothing
    a.x_bs = a.dx_bs = Cin * Lin
    a.y_bs = a.dy_bs = Cout * a.Lout
    a.workspace, a.workspace_bytes = 4096, _lib.load().pg_workspace_bytes_conv()
    a.precision, a.schedule = precision, schedule
    return a


# the U-Net's layers at width C (name, transposed, Cin, Cout, k, s, p, frames in at L = 256 / 128)
def layers(C, L):
    from phasegen.unet import frame_plan
    L1, L2, L3, L4 = frame_plan(L)
    return [("D0", False, C, 2 * C, 32, 2, 16, L), ("D1", False, 2 * C, 2 * C, 8, 1, 2, L1), ("D2", False, 2 * C, 2 * C, 8, 2, 1, L2),
            ("D3", False, 2 * C, 4 * C, 4, 2, 1, L3), ("U3", True, 4 * C, 2 * C, 5, 2, 1, L4), ("U2", True, 4 * C, 2 * C, 8, 2, 1, L3),
            ("U1", True, 4 * C, 2 * C, 8, 1, 2, L2), ("U0", True, 4 * C, 2 * C, 32, 2, 16, L1)]


def family(desc):
    name = desc.split("|")[0]
    m = re.match(r"(conv_[a-z0-9_]+)_kernel<(.*)>", name)
    fam = m.group(1)
    if fam == "conv_raw":
        fam += "(tall 256x128)" if m.group(2).split(",")[-1].strip() == "1" else "(128x256)"
    return fam


SIZE_CLASSES = [("bench: batch 64 x 256 frames, C = 1024", 1024, 256, 64), ("configs[1]: batch 32 x 256", 1024, 256, 32),
                ("reference default: batch 16 x 128", 1024, 128, 16), ("demo clip: batch 1 x 128", 1024, 128, 1),
                ("1024-FFT variant: C = 512, batch 64 x 256", 512, 256, 64), ("goldens: C = 16, batch 3 x 24", 16, 24, 3),
                ("many short clips: C = 64, batch 64 x 24", 64, 24, 64)]


def sweep():
    from phasegen import _lib, ops
    ops_ = (("fwd", lambda tr: _lib.OP_CONVT1D_FWD if tr else _lib.OP_CONV1D_FWD), ("dgrad", lambda tr: _lib.OP_CONVT1D_DGRAD if tr else _lib.OP_CONV1D_DGRAD),
            ("wgrad", lambda tr: _lib.OP_CONVT1D_WGRAD if tr else _lib.OP_CONV1D_WGRAD))
    table = {}
    for label, C, L, B in SIZE_CLASSES:
        for name, tr, Cin, Cout, k, s, p, Lin in layers(C, L):
            for prec, pname in ((0, "fp32"), (1, "bf16"), (2, "bf16x3")):
                for opname, opf in ops_:
                    if name == "D0" and opname == "dgrad":
                        continue
                    d = ops.conv_describe(_args(_lib, B, Cin, Cout, Lin, k, s, p, tr, precision=prec), opf(tr))
                    table[(label, pname, name, opname)] = family(d)
    # generic geometry (not one of the network's five (k, s) pairs)
    for opname, opf in ops_:
        d = ops.conv_describe(_args(_lib, 4, 24, 40, 50, 7, 3, 2, False), opf(False))
        table[("generic (k, s) = (7, 3)", "fp32", "-", opname)] = family(d)
    return table


def test_every_family_is_reached_by_some_automatic_choice_and_only_those_exist():
    table = sweep()
    reached = set(table.values())
    assert reached == {"conv_raw3", "conv_raw(128x256)", "conv_raw(tall 256x128)", "conv_g_raw", "conv_g_ps", "conv_f", "conv_t", "conv_g"}, reached
    # who takes what at the bench shape, fp32 (the headline): every F / T layer on one wave per SIMD, wgrads on the per-sample-slab / flat-K kernels
    bench = "bench: batch 64 x 256 frames, C = 1024"
    assert all(table[(bench, "fp32", l, o)] == "conv_raw3" for l in ("D0", "D1", "D2", "D3", "U3", "U2", "U1", "U0") for o in ("fwd", "dgrad") if (l, o) != ("D0", "dgrad"))
    assert {table[(bench, "fp32", l, "wgrad")] for l in ("D0", "U0")} == {"conv_g_raw"} and {table[(bench, "fp32", l, "wgrad")] for l in ("D1", "D2", "D3", "U3", "U2", "U1")} == {"conv_g_ps"}
    # the bf16 operand modes stay on the two-waves-per-SIMD raw kernels; batch 1 takes the tall tile; generic geometry and windows that do not fit: im2col
    assert table[(bench, "bf16", "U0", "fwd")] == "conv_raw(128x256)" and table[("demo clip: batch 1 x 128", "fp32", "D1", "fwd")] == "conv_raw(tall 256x128)"
    assert table[("generic (k, s) = (7, 3)", "fp32", "-", "fwd")] == "conv_f" and table[("many short clips: C = 64, batch 64 x 24", "fp32", "D3", "fwd")] in ("conv_f", "conv_raw(tall 256x128)", "conv_raw3", "conv_raw(128x256)")
    # the table itself (pytest -s prints it; DESIGN.md section 4.1 holds a copy)
    rows = {}
    for (label, prec, layer, op), fam in sorted(table.items()):
        rows.setdefault((label, prec, fam), []).append(f"{layer}.{op}")
    for (label, prec, fam), items in sorted(rows.items()):
        print(f"{label:45s} {prec:7s} {fam:24s} {' '.join(items)}")


def test_the_resident_forward_has_one_family():
    from phasegen import _lib, ops
    a = _lib.ConvhArgs()
    a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad, a.transposed = 64, 1024, 2048, 256, 32, 2, 16, 0
    a.Lout = 129
    a.x_pitch = ops.h_pitch(256)
    a.x_bs = 1024 * a.x_pitch
    a.x = a.w = a.y = 4096
    a.y_bs = 2048 * 129
    a.workspace, a.workspace_bytes = 4096, _lib.load().pg_workspace_bytes_conv()
    assert ops.conv_fwd_h_describe(a).startswith("conv_h3_kernel<32, 2, false>|")
    a.schedule = 64
    buf = ctypes.create_string_buffer(256)
    assert _lib.load().pg_conv_fwd_h_describe(ctypes.byref(a), buf, 256) == _lib.ERR_UNSUPPORTED


def test_fixup_form_follows_segments_per_split_tile():
    """The wide fixup (four workgroups per 32 x 32 block, segments summed four abreast) is taken from 8 segments per split tile on --
    demo.py's single clip: 8-16 tiles over 512 workgroups -- and never at the bench shapes (2-3 segments per split tile): the order in
    which a tile's segments are added is a function of (grid, tiles) alone."""
    from phasegen import _lib, ops

    def fields(d):
        return dict(kv.split("=", 1) for kv in d.split("|")[1:])

    for name, tr, Cin, Cout, k, s, p, Lin in layers(1024, 128):
        f = fields(ops.conv_describe(_args(_lib, 1, Cin, Cout, Lin, k, s, p, tr), _lib.OP_CONVT1D_FWD if tr else _lib.OP_CONV1D_FWD))
        assert f["split"] == "1" and f["fixup"] == "wide" and int(f["grid"]) >= 8 * (int(f["tiles"]) - int(f["whole"])), (name, f)
    seen = set()
    for name, tr, Cin, Cout, k, s, p, Lin in layers(1024, 256):
        for op in ((_lib.OP_CONVT1D_FWD, _lib.OP_CONVT1D_DGRAD, _lib.OP_CONVT1D_WGRAD) if tr else (_lib.OP_CONV1D_FWD, _lib.OP_CONV1D_WGRAD)):
            f = fields(ops.conv_describe(_args(_lib, 64, Cin, Cout, Lin, k, s, p, tr), op))
            seen.add(f["fixup"])
    assert seen <= {"none", "plain"}, seen


def test_column_tail_launch_policy():
    """A conv_raw3 problem whose columns end <= 128 past a full 256-wide tile hands that tail to a second launch of the tall-tile
    kernel where the cost model prices the tail under the extra tile column: the bench shape's 64 x 129 = 8256 columns
    (full tiles: a whole number per CU), the reference's own 16 x 65 = 1040; never where the tail is half a tile (64 x 126 = 8064, 64 x 30),
    never under one-tile-per-workgroup, and PG_SCHED_NO_COLSPLIT turns it off."""
    from phasegen import _lib, ops
    plan = {}
    for name, tr, Cin, Cout, k, s, p, Lin in layers(1024, 256):
        for opn, op in (("fwd", _lib.OP_CONVT1D_FWD if tr else _lib.OP_CONV1D_FWD), ("dgrad", _lib.OP_CONVT1D_DGRAD if tr else _lib.OP_CONV1D_DGRAD)):
            if (name, opn) != ("D0", "dgrad"):
                plan[name + "." + opn] = ops.conv_describe(_args(_lib, 64, Cin, Cout, Lin, k, s, p, tr), op)
    tails = sorted(n for n, d in plan.items() if "|tail=" in d)
    # (D2.fwd / U2.dgrad -- 64 x 61 frames: 120 / 240 full tiles -- would split into unaligned ranges over 256 CUs: left whole)
    assert tails == ["D0.fwd", "D1.dgrad", "U0.dgrad", "U1.fwd"], tails
    for n in tails:
        assert plan[n].startswith("conv_raw3_kernel<") and "|tail=conv_raw_kernel<" in plan[n] and ", 0, 1>,grid=" in plan[n].split("|tail=")[1], plan[n]
    assert "|split=0|" in plan["D0.fwd"] and "|split=0|" in plan["U0.dgrad"]      # 256 / 512 full tiles: whole tiles per workgroup, no fixup
    d0 = ("D0", False, 1024, 2048, 32, 2, 16, 256)
    for sched in (_lib.SCHED_NO_COLSPLIT, _lib.SCHED_TILE_PER_WG, _lib.SCHED_NO_TALL):
        assert "|tail=" not in ops.conv_describe(_args(_lib, 64, *d0[2:4], d0[7], *d0[4:7], False, schedule=sched), _lib.OP_CONV1D_FWD), sched
    ref = ops.conv_describe(_args(_lib, 16, 1024, 2048, 128, 32, 2, 16, False), _lib.OP_CONV1D_FWD)
    assert ref.startswith("conv_raw3_kernel<32, 2, false, false>|grid=256|tiles=32|") and "|tail=conv_raw_kernel<32, 2, false, 0, 1>" in ref, ref
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    assert lib.pg_conv_describe(ctypes.byref(_args(_lib, 64, 1024, 2048, 256, 32, 2, 16, False, schedule=0x60000)), _lib.OP_CONV1D_FWD, buf, 256) == -2


# Small problems that reach every instantiation of the stream-K fixup kernel (csrc/conv_fixup.h): wave tile and wave grid of the
# family's GEMM kernel x epilogue (F, T, T over phase-major rows "Tpm", G) x plain / wide form.
# ((transposed, Cin, Cout, k, s, p, Lin, B), op, schedule, kernel family, epilogue, fixup form)
T_, F_ = True, False
FIXUP_CASES = [
    # im2col: 4 x 2 blocks per wave, 2 x 2 waves
    ((T_, 32, 16, 5, 2, 1, 1, 2), "dgrad", 6, "conv_f", "F", "plain"), ((T_, 32, 16, 8, 2, 1, 3, 3), "dgrad", 6, "conv_f", "F", "wide"),
    ((T_, 32, 16, 5, 2, 1, 1, 2), "fwd", 6, "conv_t", "T", "plain"), ((T_, 32, 16, 8, 2, 1, 3, 3), "fwd", 6, "conv_t", "T", "wide"),
    ((T_, 36, 17, 5, 2, 1, 9, 2), "wgrad", 6, "conv_g", "G", "plain"), ((F_, 36, 72, 4, 2, 1, 61, 5), "wgrad", 6, "conv_g", "G", "wide"),
    # raw-window wgrad: 2 x 4 blocks, 2 x 2 waves
    ((T_, 264, 132, 8, 2, 1, 29, 2), "wgrad", 2, "conv_g_raw", "G", "plain"), ((F_, 36, 72, 4, 2, 1, 61, 5), "wgrad", 2, "conv_g_ps", "G", "wide"),
    # raw 128 x 256: 2 x 4 blocks, 2 x 2 waves
    ((F_, 8, 8, 4, 2, 1, 30, 2), "fwd", 10, "conv_raw(128x256)", "F", "plain"), ((F_, 32, 8, 4, 2, 1, 30, 2), "fwd", 10, "conv_raw(128x256)", "F", "wide"),
    ((F_, 8, 8, 8, 1, 2, 61, 2), "dgrad", 10, "conv_raw(128x256)", "T", "plain"), ((F_, 8, 16, 8, 1, 2, 61, 2), "dgrad", 10, "conv_raw(128x256)", "T", "wide"),
    ((F_, 8, 8, 8, 2, 1, 30, 2), "dgrad", 10, "conv_raw(128x256)", "Tpm", "plain"), ((F_, 8, 32, 8, 2, 1, 30, 2), "dgrad", 10, "conv_raw(128x256)", "Tpm", "wide"),
    # raw tall 256 x 128: 2 x 4 blocks, 4 x 1 waves
    ((F_, 16, 32, 4, 2, 1, 3, 2), "fwd", 2, "conv_raw(tall 256x128)", "F", "plain"), ((F_, 16, 16, 8, 1, 2, 13, 3), "fwd", 2, "conv_raw(tall 256x128)", "F", "wide"),
    ((F_, 16, 8, 8, 1, 2, 13, 3), "dgrad", 2, "conv_raw(tall 256x128)", "T", "plain"), ((F_, 16, 16, 8, 1, 2, 13, 3), "dgrad", 2, "conv_raw(tall 256x128)", "T", "wide"),
    ((F_, 16, 32, 4, 2, 1, 3, 2), "dgrad", 2, "conv_raw(tall 256x128)", "Tpm", "plain"), ((T_, 32, 16, 8, 2, 1, 3, 3), "fwd", 2, "conv_raw(tall 256x128)", "Tpm", "wide"),
    # conv_raw3: 8 x 2 blocks, 1 x 4 waves; plain however many segments a tile has (the first row: 68)
    ((F_, 136, 130, 8, 2, 1, 62, 2), "fwd", 0x4002, "conv_raw3", "F", "plain"), ((F_, 160, 136, 8, 1, 2, 65, 3), "dgrad", 0x4002, "conv_raw3", "T", "plain"),
    ((T_, 48, 125, 5, 2, 1, 30, 6), "fwd", 0x4002, "conv_raw3", "Tpm", "plain"),
    # ... in super-rows of 2 over 3 x 2 tiles: the last super-row is short, and the fixup decodes the tile order itself
    ((F_, 16, 760, 8, 2, 1, 130, 5), "fwd", 0x14002, "conv_raw3", "F", "plain"), ((F_, 380, 32, 8, 2, 1, 130, 5), "dgrad", 0x14002, "conv_raw3", "Tpm", "plain"),
]
# pg_conv_fwd_h (conv_h3: 8 x 2 blocks, 1 x 4 waves; rows of (channel, phase) pairs, never phase-major), schedule 2
FIXUP_CASES_H = [((F_, 16, 16, 8, 1, 2, 13, 3), "F", "plain"), ((F_, 8, 16, 32, 2, 16, 24, 1), "F", "wide"),
                 ((T_, 32, 16, 8, 2, 1, 3, 3), "T", "plain"), ((T_, 32, 16, 8, 1, 2, 10, 3), "T", "wide")]


def fixup_case_id(c):
    g = c[0]
    return f"{'T' if g[0] else 'C'}{g[1]}-{g[2]}-k{g[3]}s{g[4]}-L{g[6]}-B{g[7]}-" + "-".join(str(v) for v in c[1:])


def _fields(d):
    return dict(kv.split("=", 1) for kv in d.split("|")[1:])


def _epilogue(desc):
    """the epilogue a described kernel's fixup runs: G for the wgrads; F / T from the kernel's own form; Tpm for the stride-2 T form of
    the raw-window kernels (conv_raw, conv_raw3), which store phase-major rows"""
    m = re.match(r"conv_([a-z0-9_]+)_kernel<(.*)>", desc.split("|")[0])
    fam, targs = m.group(1), [t.strip() for t in m.group(2).split(",")]
    if fam in ("f", "t", "g"):
        return fam.upper()
    if fam.startswith("g_"):
        return "G"
    if targs[2] != "true":
        return "F"
    return "Tpm" if fam in ("raw", "raw3") and targs[1] == "2" else "T"


def test_every_fixup_instantiation_is_reached_by_a_small_case():
    from phasegen import _lib, ops
    reached = set()
    for geom, op, sched, fam, epi, form in FIXUP_CASES:
        tr, Cin, Cout, k, s, p, Lin, B = geom
        opc = {"fwd": (_lib.OP_CONV1D_FWD, _lib.OP_CONVT1D_FWD), "dgrad": (_lib.OP_CONV1D_DGRAD, _lib.OP_CONVT1D_DGRAD),
               "wgrad": (_lib.OP_CONV1D_WGRAD, _lib.OP_CONVT1D_WGRAD)}[op][tr]
        d = ops.conv_describe(_args(_lib, B, Cin, Cout, Lin, k, s, p, tr, schedule=sched), opc)
        f = _fields(d)
        assert (family(d), _epilogue(d), f["fixup"]) == (fam, epi, form) and "tail" not in f, (geom, op, d)
        reached.add((fam.replace("conv_g_ps", "conv_g_raw"), epi, form))         # (the two raw-window wgrads share a tile geometry)
    # conv_raw3 stays plain however many segments a tile has: one tile in 68 segments, where every other family goes wide (from 8)
    f = _fields(ops.conv_describe(_args(_lib, 2, 136, 130, 62, 8, 2, 1, False, schedule=0x4002), _lib.OP_CONV1D_FWD))
    assert (f["grid"], f["tiles"], f["whole"], f["fixup"]) == ("68", "1", "0", "plain"), f
    # super-rows of 2 over 3 tile rows x 2 tile columns
    for geom, op, sched, *_ in FIXUP_CASES[-2:]:
        tr, Cin, Cout, k, s, p, Lin, B = geom
        f = _fields(ops.conv_describe(_args(_lib, B, Cin, Cout, Lin, k, s, p, tr, schedule=sched), _lib.OP_CONV1D_FWD if op == "fwd" else _lib.OP_CONV1D_DGRAD))
        assert f["tiles"] == "6", f
    for geom, epi, form in FIXUP_CASES_H:
        tr, Cin, Cout, k, s, p, Lin, B = geom
        a = _lib.ConvhArgs()
        a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad, a.transposed = B, Cin, Cout, Lin, k, s, p, int(tr)
        a.Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
        a.x_pitch = ops.h_pitch(Lin)
        a.x_bs = Cin * a.x_pitch
        a.x = a.w = a.y = 4096
        a.y_bs = Cout * a.Lout
        a.workspace, a.workspace_bytes = 4096, _lib.load().pg_workspace_bytes_conv()
        a.schedule = 2
        d = ops.conv_fwd_h_describe(a)
        assert (family(d), _epilogue(d), _fields(d)["fixup"]) == ("conv_h3", epi, form), (geom, d)
        reached.add(("conv_h3", epi, form))
    # 25 instantiations: 2 forms x (im2col F T G, raw 128 x 256 F T Tpm G, raw tall F T Tpm, one wave per SIMD F T) + conv_raw3's plain
    # Tpm; conv_raw3 and conv_h3 share the plain F and T ones, so the table names 27 (family, epilogue, form) triples
    assert len(reached) == 27, sorted(reached)


# ---- the engine's argument patterns (tests/test_z_conv_views_gpu.py runs every row) -----------------------------------------------
# phasegen/unet.py hands the conv entry points channel slices of wider buffers, fuses an activation (and a second output) into the
# forward's store and accumulates the dgrad into its own addend.  VIEW_CASES are the small problems on which the GPU module runs
# those patterns through every kernel family's own epilogue and through every fixup instantiation, in FIXUP_CASES' row format with
# "none" (no tile is split) and "tail" (conv_raw3 over the full 256-wide tiles, the tall tile over the rest) as further forms.


def _one_tile_per_workgroup(case):
    """the same problem with work-split bits 0-1 = 1 (family bits kept: 6 -> 5, 10 -> 9, 2 -> 1, 0x4002 -> 0x4001): the GEMM kernel's
    own epilogue stores every tile"""
    geom, op, sched, fam, epi, _ = case
    return (geom, op, (sched & ~3) | 1, fam, epi, "none")


TAIL = 0x40000 | 0x4000         # conv_raw3 wherever it covers the problem, its column tail always split off
VIEW_CASES = FIXUP_CASES + [_one_tile_per_workgroup(c) for c in FIXUP_CASES] + [
    # column tails.  F: 5 x 63 = 315 columns.  T / Tpm forward and an F dgrad (add / ref through the tail's epilogue): rows of
    # test_ops_gpu._random_geoms_one_wave(32, 20261005) whose plan has a tail.  No Conv1d dgrad of that sweep has one (their columns are
    # B * U <= 256, or the window does not fit), so the two T-form dgrads are the k = 8 layers with the F row's 5 x 63 / 3 x 100 columns
    ((F_, 32, 250, 8, 2, 1, 130, 5), "fwd", TAIL, "conv_raw3", "F", "tail"), ((T_, 250, 96, 8, 2, 6, 129, 2), "dgrad", TAIL, "conv_raw3", "F", "tail"),
    ((T_, 16, 470, 8, 1, 2, 100, 5), "fwd", TAIL, "conv_raw3", "T", "tail"), ((F_, 250, 32, 8, 1, 2, 100, 3), "dgrad", TAIL, "conv_raw3", "T", "tail"),
    ((T_, 32, 250, 32, 2, 25, 129, 5), "fwd", TAIL, "conv_raw3", "Tpm", "tail"), ((F_, 125, 32, 8, 2, 1, 130, 5), "dgrad", TAIL, "conv_raw3", "Tpm", "tail"),
    # packed fp32 wgrads (test_wgrad_packed_gpu.GEOMS[0], [2], [-1]): flat K, per-sample slabs, k = 5's 255-column tiles
    ((F_, 40, 48, 32, 2, 16, 258, 2), "wgrad", 1, "conv_g_raw", "G", "none"), ((F_, 40, 48, 32, 2, 16, 258, 2), "wgrad", 2, "conv_g_raw", "G", "wide"),
    ((F_, 33, 40, 8, 1, 2, 129, 3), "wgrad", 1, "conv_g_ps", "G", "none"), ((F_, 33, 40, 8, 1, 2, 129, 3), "wgrad", 2, "conv_g_ps", "G", "wide"),
    ((T_, 64, 103, 5, 2, 1, 30, 2), "wgrad", 1, "conv_g_ps", "G", "none"), ((T_, 64, 103, 5, 2, 1, 30, 2), "wgrad", 2, "conv_g_ps", "G", "plain"),
    # runtime (k, s) = (7, 3) and its transposed twin (test_ops_gpu.GEOMS): the im2col kernels' S = 0 instantiation
    ((F_, 24, 40, 7, 3, 2, 50, 2), "fwd", 0, "conv_f", "F", "none"), ((F_, 24, 40, 7, 3, 2, 50, 2), "dgrad", 0, "conv_t", "T", "none"),
    ((F_, 24, 40, 7, 3, 2, 50, 2), "wgrad", 0, "conv_g", "G", "none"), ((T_, 24, 40, 7, 3, 2, 17, 2), "fwd", 0, "conv_t", "T", "none"),
    ((T_, 24, 40, 7, 3, 2, 17, 2), "dgrad", 0, "conv_f", "F", "none"), ((T_, 24, 40, 7, 3, 2, 17, 2), "wgrad", 0, "conv_g", "G", "none"),
]
# ---- the raw-window wgrad's instantiations (tests/test_z_wgrad_cover_gpu.py runs every row) ------------------------------------------
# conv_g_raw_kernel / conv_g_ps_kernel<KW, S, BF> exist for the network's five (k, s) pairs x three operand modes.  The tables above
# reach the flat-K kernel of k = 4, k = 5 and (k, s) = (8, 1) at no bf16 mode (and at fp32 only through the packed module's 1e-5
# bound): one geometry each, under one tile per workgroup and under stream-K.  Every row: p > 0 (the first and the last window leave
# the row), 2-3 samples of 29 frames (LP = 29: every other slab runs over a sample end, and padding to 32 would cost 10 %, so the plan
# keeps the flat K axis), one tile, K = 58 / 87.
WGRAD_COVER_CASES = [
    ((F_, 24, 40, 4, 2, 1, 58, 2), "wgrad", 1, "conv_g_raw", "G", "none"), ((F_, 24, 40, 4, 2, 1, 58, 2), "wgrad", 2, "conv_g_raw", "G", "plain"),
    ((T_, 40, 31, 5, 2, 1, 29, 2), "wgrad", 1, "conv_g_raw", "G", "none"), ((T_, 40, 31, 5, 2, 1, 29, 2), "wgrad", 2, "conv_g_raw", "G", "plain"),
    ((F_, 24, 40, 8, 1, 2, 32, 3), "wgrad", 1, "conv_g_raw", "G", "none"), ((F_, 24, 40, 8, 1, 2, 32, 3), "wgrad", 2, "conv_g_raw", "G", "plain"),
]
WGRAD_KS = ((32, 2), (8, 1), (8, 2), (5, 2), (4, 2))
# instantiations no call reaches: pick_family (csrc/conv_igemm.hip) never takes per-sample slabs at k = 32
WGRAD_UNREACHED = {("conv_g_ps", 32, 2, bf) for bf in (0, 1, 2)}


def wgrad_instantiation(desc):
    """(family, KW, S, BF) of a described raw-window wgrad, None for any other kernel"""
    m = re.match(r"(conv_g_raw|conv_g_ps)_kernel<(\d+), (\d+), (\d+)>\|", desc)
    return (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else None


def wgrad_frames(geom):
    """frames per sample of the wgrad's A operand (LP): dy's for a Conv1d, x's for a ConvTranspose1d"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    return Lin if tr else (Lin + 2 * p - k) // s + 1


def test_value_rows_reach_every_raw_window_wgrad_instantiation():
    """The wgrad rows of VIEW_CASES, SPLIT_CASES and WGRAD_COVER_CASES -- each run element by element against float64 at every operand
    mode its family has -- reach 27 of the 30 conv_g_raw / conv_g_ps instantiations; the other three (per-sample slabs at k = 32) no
    plan names at any frame count, so no row can.  On flat-K rows a slab crosses a sample end, every row's windows leave the row on
    both sides, and every (k, s) has a per-sample row whose last slab is padded."""
    from phasegen import _lib, ops
    every = {(fam, k, s, bf) for fam in ("conv_g_raw", "conv_g_ps") for k, s in WGRAD_KS for bf in (0, 1, 2)}
    reached, padded = set(), set()
    for case in VIEW_CASES + SPLIT_CASES + WGRAD_COVER_CASES:
        if case[1] != "wgrad":
            continue
        for prec in (0, 1, 2) if case[3] in BF16_FAMILIES else (0,):
            inst = wgrad_instantiation(ops.conv_describe(_view_args(_lib, case, None, prec), _opcode(_lib, case)))
            if inst:
                reached.add(inst)
                if inst[0] == "conv_g_ps" and wgrad_frames(case[0]) % 16:
                    padded.add(inst[1:3])
    assert reached == every - WGRAD_UNREACHED, sorted(every - reached)
    assert padded == set(WGRAD_KS) - {(32, 2)}, padded
    for L in range(16, 300):                                  # k = 32: the flat K axis whatever the frame count
        for prec in (0, 1, 2):
            d = ops.conv_describe(_args(_lib, 2, 40, 48, 2 * L, 32, 2, 16, False, precision=prec), _lib.OP_CONV1D_WGRAD)
            assert wgrad_frames((False, 40, 48, 32, 2, 16, 2 * L, 2)) == L + 1 and wgrad_instantiation(d)[0] == "conv_g_raw", (L, d)
    assert len(set(WGRAD_COVER_CASES)) == len(WGRAD_COVER_CASES) and not set(WGRAD_COVER_CASES) & set(VIEW_CASES + SPLIT_CASES)
    for case in WGRAD_COVER_CASES:
        geom, op, sched, fam, epi, form = case
        tr, Cin, Cout, k, s, p, Lin, B = geom
        assert max(Cin, Cout) <= 64 and Lin <= 258 and 2 <= B <= 3 and p > 0 and wgrad_frames(geom) % 16 and _gemm_k(geom, op) <= 512, case
        for prec in (0, 1, 2):
            d = ops.conv_describe(_view_args(_lib, case, None, prec), _opcode(_lib, case))
            assert wgrad_instantiation(d) == (fam, k, s, prec) and _epilogue(d) == epi and _fields(d)["fixup"] == form, (case, d)


# families with bf16 / bf16x3 operand modes of their own (conv_raw3 is fp32 only: its problems go to conv_raw at those precisions)
BF16_FAMILIES = ("conv_f", "conv_t", "conv_g", "conv_raw(128x256)", "conv_raw(tall 256x128)", "conv_g_raw", "conv_g_ps")
# (channel offset, further channels behind) of a view inside its buffer: 4 channels in front leave the view 16-byte aligned whatever
# the frame count; 1 in front puts it an odd number of floats into the buffer where the frame count is odd (a base pointer aligned to 4
# bytes only) and keeps the sibling directly in front where it is even
VIEW_PAIRS = ((4, 1), (1, 2))


def view_layout(case, pair):
    """{operand: (channel offset, channels behind, channels, frames, batch stride)} of a row's call under VIEW_PAIRS[pair]: every
    operand a channel slice buf[:, off:off + C] of a (B, off + C + extra, L) buffer of its own width, so that no two batch strides of a
    call are equal; "xb": the forward's / wgrad's x as batch[:, 0] of a (B, 2, C, L) batch."""
    (tr, Cin, Cout, k, s, p, Lin, B), op = case[0], case[1]
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    names = {"fwd": ("x", "y", "y2"), "dgrad": ("dy", "dx", "add", "ref"), "wgrad": ("dy",)}[op]
    off, extra = VIEW_PAIRS[pair]
    out, seen = {}, set()
    if op != "dgrad":
        out["xb"] = (0, 0, Cin, Lin, 2 * Cin * Lin)
        seen.add(2 * Cin * Lin)
    for i, n in enumerate(names):
        C, L = (Cin, Lin) if n in ("x", "dx", "add", "ref") else (Cout, Lout)
        e = extra + i
        while (off + C + e) * L in seen or (off + C + e) * L == C * L:
            e += 1
        seen.add((off + C + e) * L)
        out[n] = (off, e, C, L, (off + C + e) * L)
    return out


def _view_args(_lib, case, pair, precision=0):
    """the row's ConvArgs with the batch strides the GPU module passes (pair None: dense)"""
    tr, Cin, Cout, k, s, p, Lin, B = case[0]
    a = _args(_lib, B, Cin, Cout, Lin, k, s, p, tr, precision=precision, schedule=case[2])
    if case[1] == "fwd":
        a.y2, a.y2_bs, a.y_act, a.y2_act = 4096, a.y_bs, 1, 2
    if case[1] == "dgrad":
        a.dx_add, a.dx_add_bs, a.dx_ref, a.dx_ref_bs, a.dx_mask = 4096, a.dx_bs, 4096, a.dx_bs, 1
    if pair is not None:
        lay = view_layout(case, pair)
        for n, f in (("x", "x_bs"), ("y", "y_bs"), ("y2", "y2_bs"), ("dy", "dy_bs"), ("dx", "dx_bs"), ("add", "dx_add_bs"), ("ref", "dx_ref_bs")):
            if n in lay:
                setattr(a, f, lay[n][4])
        if case[1] == "wgrad":
            a.x_bs = lay["xb"][4]
    return a


def _opcode(_lib, case):
    return {"fwd": (_lib.OP_CONV1D_FWD, _lib.OP_CONVT1D_FWD), "dgrad": (_lib.OP_CONV1D_DGRAD, _lib.OP_CONVT1D_DGRAD),
            "wgrad": (_lib.OP_CONV1D_WGRAD, _lib.OP_CONVT1D_WGRAD)}[case[1]][case[0][0]]


def test_view_cases_plan_is_the_declared_one_and_independent_of_strides():
    """Every VIEW_CASES row's plan names the row's family, epilogue and fixup form ("tail": a conv_raw3 launch plus the tall-tile tail),
    and is the same string for dense operands, for both view layouts of tests/test_z_conv_views_gpu.py and for the forward's x given as
    batch[:, 0]: the GPU module may compare a call on views bit for bit with the call on dense copies.  The rows whose family has bf16
    operand modes keep it (and their epilogue and form) at those precisions."""
    from phasegen import _lib, ops
    assert VIEW_CASES[:len(FIXUP_CASES)] == FIXUP_CASES and len(set(VIEW_CASES)) == len(VIEW_CASES)
    for case in VIEW_CASES + SPLIT_CASES:                    # (SPLIT_CASES: the multi-tile work splits, below)
        geom, op, sched, fam, epi, form = case
        opc = _opcode(_lib, case)
        for prec in (0, 1, 2) if fam in BF16_FAMILIES else (0,):
            dense = ops.conv_describe(_view_args(_lib, case, None, prec), opc)
            f = _fields(dense)
            assert (family(dense), _epilogue(dense)) == (fam, epi), (case, prec, dense)
            if form == "tail":
                assert dense.startswith("conv_raw3_kernel<") and "|tail=conv_raw_kernel<" in dense and ", 0, 1>,grid=" in dense.split("|tail=")[1], (case, dense)
            else:
                assert f["fixup"] == form and "tail" not in f, (case, prec, dense)
            for pair in range(len(VIEW_PAIRS)):
                lay = view_layout(case, pair)
                strides = [v[4] for v in lay.values()]
                assert len(set(strides)) == len(strides) and all(v[4] != v[2] * v[3] for v in lay.values()), (case, lay)
                a = _view_args(_lib, case, pair, prec)
                assert ops.conv_describe(a, opc) == dense, (case, pair, prec)
                if op == "fwd":
                    a.x_bs = lay["xb"][4]
                    assert ops.conv_describe(a, opc) == dense, (case, pair, prec, "batch[:, 0]")
                if op == "dgrad":                           # the in-place form: the addend is the dx view, the mask source dense
                    a.dx_add_bs, a.dx_ref_bs = a.dx_bs, geom[1] * geom[6]
                    assert ops.conv_describe(a, opc) == dense, (case, pair, prec, "in place")
    # what the table holds: every fixup instantiation of the fp32 entry points, every family's own epilogue, three kinds of tail
    assert {(c[3], c[4]) for c in VIEW_CASES if c[5] == "none"} >= {(c[3], c[4]) for c in FIXUP_CASES}
    assert {c[4] for c in VIEW_CASES if c[5] == "tail"} == {"F", "T", "Tpm"}


# ---- the multi-tile work splits on small problems (tests/test_z_fixup_splits_gpu.py runs every row) ----------------------------------
# Every row above has at most a handful of tiles, so a workgroup owns one whole tile or a fragment of one.  PG_SCHED_SLOTS(n) plans a
# call as if the device had n compute units (host side only): the rows below put small problems through the work splits a full-size
# layer takes on 256 CUs.  A plain restatement of make_split / split_lo (csrc/conv_common.h) names the regimes a row's plan is in; it
# is used to CLASSIFY a row, never as an expected value -- the plan itself is pinned field by field from pg_conv_describe.
def SLOTS(n):
    return n << 19


def split_ranges(tiles, nslab, grid, whole):
    """[lo, hi) of every logical workgroup over the (tile, slab) space: the first `whole` own one whole tile each, the others share the
    rest evenly, the first (rest mod workgroups) of them one slab longer"""
    total, wn, gr = tiles * nslab, whole * nslab, grid - whole
    q, r = divmod(total - wn, gr) if gr > 0 else (0, 0)

    def lo(g):
        if g < whole:
            return g * nslab
        g -= whole
        return wn + (g * (q + 1) if g < r else r * (q + 1) + (g - r) * q)

    return [(lo(g), lo(g + 1)) for g in range(grid)]


def regimes(f, sched=0, auto=None, one_wave=False):
    """the regimes of a described plan (f: its fields; sched: the row's schedule word; auto: the fields of the same call without
    PG_SCHED_CONTENDED, for the contended regime; one_wave: conv_raw3 / conv_h3, one workgroup slot per CU instead of two)"""
    tiles, nslab, grid, whole = int(f["tiles"]), int(f["slabs"]), int(f["grid"]), int(f["whole"])
    out = set()
    if tiles % grid == 0 and tiles // grid >= 2 and f["fixup"] == "none":
        out.add("multi-whole")
    if whole >= 2 and grid - whole >= 2 and f["fixup"] != "none":
        out.add("hybrid")
    if f["fixup"] != "none":
        for lo, hi in split_ranges(tiles, nslab, grid, whole)[whole:]:
            head, tail = lo % nslab != 0, hi % nslab != 0
            if hi // nslab - -(-lo // nslab) >= 1:              # a whole tile inside the range
                if head and tail:
                    out.add("head-whole-tail")
                elif tail:
                    out.add("whole-then-partial")
                elif head:
                    out.add("partial-then-whole")
    if sched & 16 and auto is not None and (auto["fixup"] == "none" or int(auto["whole"]) > 0) and f["fixup"] != "none" and whole == 0 and tiles > grid:
        out.add("contended")
    over, slots = ((sched >> 8) & 15) or 4, (sched >> 19) & 31          # (no factor given: the default, 4)
    if slots and tiles > grid and grid == over * slots * (1 if one_wave else 2):
        out.add("oversub")
    return out


IM2COL, STREAMK, NO_TALL, CONTENDED, NO_RAW3, ALL_RAW3, SR2, COLSPLIT = 4, 2, 8, 16, 0x2000, 0x4000, 0x10000, 0x40000


def OVERSUB(f):
    return f << 8


# (row in FIXUP_CASES' format with the slot field inside the schedule word, the regimes the row is here for, its plan after the kernel name)
SPLIT_TABLE = [
    # conv_raw3 (256 x 256 tiles, one workgroup per CU): 2 tile rows (the second partial) x 3 tile columns (the last partial), 7 slabs
    (((F_, 14, 390, 8, 2, 1, 260, 5), "fwd", ALL_RAW3 | SLOTS(1), "conv_raw3", "F", "none"), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none"),
    (((F_, 14, 390, 8, 2, 1, 260, 5), "fwd", ALL_RAW3 | STREAMK | SLOTS(4), "conv_raw3", "F", "plain"), ("head-whole-tail",), "grid=4|tiles=6|slabs=7|split=1|whole=0|fixup=plain"),
    (((T_, 14, 390, 8, 1, 2, 130, 5), "fwd", ALL_RAW3 | SLOTS(1), "conv_raw3", "T", "none"), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none"),
    (((T_, 14, 390, 8, 1, 2, 130, 5), "fwd", ALL_RAW3 | STREAMK | SLOTS(4), "conv_raw3", "T", "plain"), ("head-whole-tail",), "grid=4|tiles=6|slabs=7|split=1|whole=0|fixup=plain"),
    (((F_, 195, 28, 8, 2, 1, 260, 5), "dgrad", ALL_RAW3 | SLOTS(1), "conv_raw3", "Tpm", "none"), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none"),
    (((F_, 195, 28, 8, 2, 1, 260, 5), "dgrad", ALL_RAW3 | STREAMK | SLOTS(4), "conv_raw3", "Tpm", "plain"), ("head-whole-tail",), "grid=4|tiles=6|slabs=7|split=1|whole=0|fixup=plain"),
    # ... in super-rows of 2 over 3 tile rows x 2 tile columns: the last super-row is short
    (((F_, 14, 760, 8, 2, 1, 130, 5), "fwd", SR2 | ALL_RAW3 | SLOTS(1), "conv_raw3", "F", "none"), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none"),
    (((F_, 14, 760, 8, 2, 1, 130, 5), "fwd", SR2 | ALL_RAW3 | STREAMK | SLOTS(4), "conv_raw3", "F", "plain"), ("head-whole-tail",), "grid=4|tiles=6|slabs=7|split=1|whole=0|fixup=plain"),
    (((F_, 380, 28, 8, 2, 1, 130, 5), "dgrad", SR2 | ALL_RAW3 | SLOTS(1), "conv_raw3", "Tpm", "none"), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none"),
    (((F_, 380, 28, 8, 2, 1, 130, 5), "dgrad", SR2 | ALL_RAW3 | STREAMK | SLOTS(4), "conv_raw3", "Tpm", "plain"), ("head-whole-tail",), "grid=4|tiles=6|slabs=7|split=1|whole=0|fixup=plain"),
    # ... 2 x 4 tiles: the default oversubscription factor's grid of 4 x slots through the whole-tile branch (U0.dgrad's bench plan in miniature)
    (((F_, 14, 390, 8, 2, 1, 390, 5), "fwd", ALL_RAW3 | SLOTS(1), "conv_raw3", "F", "none"), ("multi-whole", "oversub"), "grid=4|tiles=8|slabs=7|split=0|whole=0|fixup=none"),
    # ... two whole tiles per workgroup over the full tile columns and the tall tile over the 47 columns behind them: D0.fwd at the bench shape in miniature
    (((F_, 14, 390, 8, 2, 1, 326, 5), "fwd", COLSPLIT | ALL_RAW3 | SLOTS(1), "conv_raw3", "F", "tail"), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none|tail=conv_raw_kernel<8, 2, false, 0, 1>,grid=2"),
    # ... 16 slabs: hybrid (4 whole-tile workgroups, 2 tiles over 4 more), the even split PG_SCHED_CONTENDED takes instead, 3 and 6 tiles per workgroup
    (((F_, 32, 390, 8, 2, 1, 260, 5), "fwd", ALL_RAW3 | SLOTS(4), "conv_raw3", "F", "plain"), ("hybrid",), "grid=8|tiles=6|slabs=16|split=1|whole=4|fixup=plain"),
    (((F_, 32, 390, 8, 2, 1, 260, 5), "fwd", ALL_RAW3 | CONTENDED | SLOTS(4), "conv_raw3", "F", "plain"), ("contended",), "grid=4|tiles=6|slabs=16|split=1|whole=0|fixup=plain"),
    (((F_, 32, 390, 8, 2, 1, 260, 5), "fwd", ALL_RAW3 | OVERSUB(2) | SLOTS(1), "conv_raw3", "F", "none"), ("multi-whole", "oversub"), "grid=2|tiles=6|slabs=16|split=0|whole=0|fixup=none"),
    (((F_, 32, 390, 8, 2, 1, 260, 5), "fwd", ALL_RAW3 | OVERSUB(1) | SLOTS(1), "conv_raw3", "F", "none"), ("multi-whole", "oversub"), "grid=1|tiles=6|slabs=16|split=0|whole=0|fixup=none"),
    (((F_, 390, 32, 8, 1, 2, 130, 5), "dgrad", ALL_RAW3 | SLOTS(4), "conv_raw3", "T", "plain"), ("hybrid",), "grid=8|tiles=6|slabs=16|split=1|whole=4|fixup=plain"),
    # raw 128 x 256 (two workgroups per CU): 2 x 5 tiles, 3 slabs
    (((F_, 12, 136, 4, 2, 1, 380, 6), "fwd", NO_RAW3 | NO_TALL | SLOTS(1), "conv_raw(128x256)", "F", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((F_, 12, 136, 4, 2, 1, 380, 6), "fwd", NO_RAW3 | NO_TALL | STREAMK | SLOTS(2), "conv_raw(128x256)", "F", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    (((T_, 6, 136, 8, 1, 2, 190, 6), "fwd", NO_RAW3 | NO_TALL | SLOTS(1), "conv_raw(128x256)", "T", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((T_, 6, 136, 8, 1, 2, 190, 6), "fwd", NO_RAW3 | NO_TALL | STREAMK | SLOTS(2), "conv_raw(128x256)", "T", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    (((F_, 68, 12, 8, 2, 1, 380, 6), "dgrad", NO_RAW3 | NO_TALL | SLOTS(1), "conv_raw(128x256)", "Tpm", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((F_, 68, 12, 8, 2, 1, 380, 6), "dgrad", NO_RAW3 | NO_TALL | STREAMK | SLOTS(2), "conv_raw(128x256)", "Tpm", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    # ... 32 slabs: hybrid with the plain and with the wide fixup (2 split tiles over 4 / 8 workgroups), contended; 3 x 4 tiles: 3 and 6 per workgroup
    (((F_, 128, 136, 4, 2, 1, 380, 6), "fwd", NO_RAW3 | NO_TALL | SLOTS(2), "conv_raw(128x256)", "F", "plain"), ("hybrid",), "grid=12|tiles=10|slabs=32|split=1|whole=8|fixup=plain"),
    (((F_, 128, 136, 4, 2, 1, 380, 6), "fwd", NO_RAW3 | NO_TALL | SLOTS(4), "conv_raw(128x256)", "F", "wide"), ("hybrid",), "grid=16|tiles=10|slabs=32|split=1|whole=8|fixup=wide"),
    (((F_, 128, 136, 4, 2, 1, 380, 6), "fwd", NO_RAW3 | NO_TALL | CONTENDED | SLOTS(2), "conv_raw(128x256)", "F", "plain"), ("contended",), "grid=4|tiles=10|slabs=32|split=1|whole=0|fixup=plain"),
    (((F_, 32, 264, 4, 2, 1, 300, 6), "fwd", NO_RAW3 | NO_TALL | OVERSUB(2) | SLOTS(1), "conv_raw(128x256)", "F", "none"), ("multi-whole", "oversub"), "grid=4|tiles=12|slabs=8|split=0|whole=0|fixup=none"),
    (((F_, 32, 264, 4, 2, 1, 300, 6), "fwd", NO_RAW3 | NO_TALL | OVERSUB(1) | SLOTS(1), "conv_raw(128x256)", "F", "none"), ("multi-whole", "oversub"), "grid=2|tiles=12|slabs=8|split=0|whole=0|fixup=none"),
    # raw tall 256 x 128: 2 x 5 tiles, 3 slabs
    (((F_, 12, 300, 4, 2, 1, 240, 5), "fwd", NO_RAW3 | SLOTS(1), "conv_raw(tall 256x128)", "F", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((F_, 12, 300, 4, 2, 1, 240, 5), "fwd", NO_RAW3 | STREAMK | SLOTS(2), "conv_raw(tall 256x128)", "F", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    (((F_, 300, 6, 8, 1, 2, 120, 5), "dgrad", NO_RAW3 | SLOTS(1), "conv_raw(tall 256x128)", "T", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((F_, 300, 6, 8, 1, 2, 120, 5), "dgrad", NO_RAW3 | STREAMK | SLOTS(2), "conv_raw(tall 256x128)", "T", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    (((T_, 12, 150, 8, 2, 1, 120, 5), "fwd", NO_RAW3 | SLOTS(1), "conv_raw(tall 256x128)", "Tpm", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((T_, 12, 150, 8, 2, 1, 120, 5), "fwd", NO_RAW3 | STREAMK | SLOTS(2), "conv_raw(tall 256x128)", "Tpm", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    # im2col 256 x 128: 2 x 5 tiles
    (((T_, 300, 12, 4, 2, 1, 120, 5), "dgrad", IM2COL | SLOTS(1), "conv_f", "F", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((T_, 300, 12, 4, 2, 1, 120, 5), "dgrad", IM2COL | STREAMK | SLOTS(2), "conv_f", "F", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    (((F_, 300, 6, 8, 1, 2, 120, 5), "dgrad", IM2COL | SLOTS(1), "conv_t", "T", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=3|split=0|whole=0|fixup=none"),
    (((F_, 300, 6, 8, 1, 2, 120, 5), "dgrad", IM2COL | STREAMK | SLOTS(2), "conv_t", "T", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=3|split=1|whole=0|fixup=plain"),
    (((F_, 75, 300, 8, 2, 1, 40, 4), "wgrad", IM2COL | SLOTS(1), "conv_g", "G", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=5|split=0|whole=0|fixup=none"),
    (((F_, 75, 300, 8, 2, 1, 40, 4), "wgrad", IM2COL | STREAMK | SLOTS(2), "conv_g", "G", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=5|split=1|whole=0|fixup=plain"),
    # raw-window wgrads (128 x 256; k = 5: 255-column tiles): flat K, per-sample slabs; hybrid over 2 x 5 tiles x 16 slabs (plain fixup:
    # 8 whole-tile workgroups, 2 tiles over 4 more) and over 2 x 7 (wide: 12 whole, 2 tiles over 4); K = 256 keeps the fp32 bound 10 x from the split
    (((F_, 138, 136, 8, 2, 1, 40, 4), "wgrad", SLOTS(1), "conv_g_raw", "G", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=5|split=0|whole=0|fixup=none"),
    (((F_, 138, 136, 8, 2, 1, 40, 4), "wgrad", STREAMK | SLOTS(2), "conv_g_raw", "G", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=5|split=1|whole=0|fixup=plain"),
    (((F_, 35, 136, 32, 2, 16, 254, 2), "wgrad", SLOTS(2), "conv_g_raw", "G", "plain"), ("hybrid",), "grid=12|tiles=10|slabs=16|split=1|whole=8|fixup=plain"),
    (((F_, 53, 136, 32, 2, 16, 254, 2), "wgrad", SLOTS(2), "conv_g_raw", "G", "wide"), ("hybrid",), "grid=16|tiles=14|slabs=16|split=1|whole=12|fixup=wide"),
    (((F_, 35, 136, 32, 2, 16, 254, 2), "wgrad", CONTENDED | SLOTS(2), "conv_g_raw", "G", "plain"), ("contended",), "grid=4|tiles=10|slabs=16|split=1|whole=0|fixup=plain"),
    (((F_, 112, 264, 8, 2, 1, 40, 4), "wgrad", OVERSUB(2) | SLOTS(1), "conv_g_raw", "G", "none"), ("multi-whole", "oversub"), "grid=4|tiles=12|slabs=5|split=0|whole=0|fixup=none"),
    (((F_, 112, 264, 8, 2, 1, 40, 4), "wgrad", OVERSUB(1) | SLOTS(1), "conv_g_raw", "G", "none"), ("multi-whole", "oversub"), "grid=2|tiles=12|slabs=5|split=0|whole=0|fixup=none"),
    (((F_, 138, 136, 8, 2, 1, 36, 5), "wgrad", SLOTS(1), "conv_g_ps", "G", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=5|split=0|whole=0|fixup=none"),
    (((F_, 138, 136, 8, 2, 1, 36, 5), "wgrad", STREAMK | SLOTS(2), "conv_g_ps", "G", "plain"), ("head-whole-tail",), "grid=4|tiles=10|slabs=5|split=1|whole=0|fixup=plain"),
    (((T_, 136, 220, 5, 2, 1, 30, 3), "wgrad", SLOTS(1), "conv_g_ps", "G", "none"), ("multi-whole",), "grid=2|tiles=10|slabs=6|split=0|whole=0|fixup=none"),
    (((T_, 136, 220, 5, 2, 1, 30, 3), "wgrad", STREAMK | SLOTS(3), "conv_g_ps", "G", "plain"), ("head-whole-tail",), "grid=6|tiles=10|slabs=6|split=1|whole=0|fixup=plain"),
    (((F_, 138, 136, 8, 2, 1, 252, 2), "wgrad", SLOTS(2), "conv_g_ps", "G", "plain"), ("hybrid",), "grid=12|tiles=10|slabs=16|split=1|whole=8|fixup=plain"),
    (((F_, 212, 136, 8, 2, 1, 252, 2), "wgrad", SLOTS(2), "conv_g_ps", "G", "wide"), ("hybrid",), "grid=16|tiles=14|slabs=16|split=1|whole=12|fixup=wide"),
]
# pg_conv_fwd_h (conv_h3: 256 x 256 tiles, one workgroup per CU; 2 x 3 tiles): FIXUP_CASES_H's format and the schedule word
SPLIT_TABLE_H = [
    (((F_, 28, 390, 8, 1, 2, 130, 5), "F", "none", SLOTS(1)), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none"),
    (((F_, 28, 390, 8, 1, 2, 130, 5), "F", "plain", STREAMK | SLOTS(4)), ("head-whole-tail",), "grid=4|tiles=6|slabs=7|split=1|whole=0|fixup=plain"),
    (((F_, 64, 390, 8, 1, 2, 130, 5), "F", "plain", SLOTS(4)), ("hybrid",), "grid=8|tiles=6|slabs=16|split=1|whole=4|fixup=plain"),
    (((T_, 56, 195, 8, 2, 1, 130, 5), "T", "none", SLOTS(1)), ("multi-whole",), "grid=3|tiles=6|slabs=7|split=0|whole=0|fixup=none"),
    (((T_, 56, 195, 8, 2, 1, 130, 5), "T", "plain", STREAMK | SLOTS(4)), ("head-whole-tail",), "grid=4|tiles=6|slabs=7|split=1|whole=0|fixup=plain"),
    (((T_, 128, 195, 8, 2, 1, 130, 5), "T", "plain", SLOTS(4)), ("hybrid",), "grid=8|tiles=6|slabs=16|split=1|whole=4|fixup=plain"),
]
SPLIT_CASES = [row for row, _, _ in SPLIT_TABLE]
SPLIT_CASES_H = [row for row, _, _ in SPLIT_TABLE_H]
# What the tables leave out, by name:
NOT_REACHED = {
    "head-whole-tail with the wide fixup": "the wide form needs grid >= 8 x split tiles, a range that holds a whole tile needs grid < tiles",
    "conv_raw3 with the wide fixup": "conv_raw3 takes the plain form however many segments a tile has (set_grid)",
    "a mult x slots grid through the uneven split (mult = total slabs / (256 slots) >= 2)": "needs 512 slabs per slot -- 16 tiles per slot at "
    "K = 512, where the value rows lose their [precision] mark; the oversub rows reach mult = 4, 2 and 1 through the whole-tile branch of pick_grid",
}


def _h_args(_lib, ops, geom, sched):
    tr, Cin, Cout, k, s, p, Lin, B = geom
    a = _lib.ConvhArgs()
    a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad, a.transposed = B, Cin, Cout, Lin, k, s, p, int(tr)
    a.Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    a.x_pitch = ops.h_pitch(Lin)
    a.x_bs = Cin * a.x_pitch
    a.x = a.w = a.y = 4096
    a.y_bs = Cout * a.Lout
    a.workspace, a.workspace_bytes = 4096, _lib.load().pg_workspace_bytes_conv()
    a.schedule = sched
    return a


def _gemm_k(geom, op):
    tr, Cin, Cout, k, s, p, Lin, B = geom
    if op == "wgrad":
        return B * (Lin if tr else (Lin + 2 * p - k) // s + 1)
    return (Cin if op == "fwd" else Cout) * (-(-k // s) if tr == (op == "fwd") else k)


def test_split_cases_plans_are_pinned_and_in_their_regime():
    """Every SPLIT_CASES / SPLIT_CASES_H row: family, epilogue, grid, tiles, slabs, split, whole, fixup form and tail launch as the table
    states them, at every precision the family has; the restated ranges put the plan into the regimes the row is there for; the same
    call without the slot field is in none of them (a grid of at least as many workgroups as tiles, as in FIXUP_CASES); and the GEMM K
    stays within 48 .. 512, where the value tests' fp32 bound still rejects the bf16x3 split."""
    from phasegen import _lib, ops
    assert len(set(SPLIT_CASES)) == len(SPLIT_CASES) and not set(SPLIT_CASES) & set(VIEW_CASES)
    assert len({fixup_case_id(c) for c in SPLIT_CASES}) == len(SPLIT_CASES)
    for case, declared, plan in SPLIT_TABLE:
        geom, op, sched, fam, epi, form = case
        assert (sched >> 19) & 31 and 48 <= _gemm_k(geom, op) <= 512, case
        opc = _opcode(_lib, case)
        for prec in (0, 1, 2) if fam in BF16_FAMILIES else (0,):
            d = ops.conv_describe(_view_args(_lib, case, None, prec), opc)
            f = _fields(d)
            assert (family(d), _epilogue(d), d.split("|", 1)[1]) == (fam, epi, plan), (case, prec, d)
            assert ("tail" in f) == (form == "tail") and (form == "tail" or f["fixup"] == form), (case, d)
        auto = _fields(ops.conv_describe(_view_args(_lib, (geom, op, sched & ~CONTENDED) + case[3:], None), opc))
        assert set(declared) <= regimes(f, sched, auto, fam == "conv_raw3"), (case, declared, regimes(f, sched, auto, fam == "conv_raw3"))
        bare = _fields(ops.conv_describe(_view_args(_lib, (geom, op, sched & ~SLOTS(31)) + case[3:], None), opc))
        assert regimes(bare, sched & ~SLOTS(31)) == set() and int(bare["grid"]) >= int(bare["tiles"]), (case, bare)
    for (geom, epi, form, sched), declared, plan in SPLIT_TABLE_H:
        assert (sched >> 19) & 31 and 48 <= _gemm_k(geom, "fwd") <= 512, geom
        d = ops.conv_fwd_h_describe(_h_args(_lib, ops, geom, sched))
        f = _fields(d)
        assert (family(d), _epilogue(d), f["fixup"], d.split("|", 1)[1]) == ("conv_h3", epi, form, plan), (geom, sched, d)
        assert set(declared) <= regimes(f, sched, None, True), (geom, sched, declared)
        assert regimes(_fields(ops.conv_fwd_h_describe(_h_args(_lib, ops, geom, sched & ~SLOTS(31))))) == set()
    # bits above the slot field stay refused; the Python constant is the header's macro
    buf = ctypes.create_string_buffer(256)
    assert _lib.load().pg_conv_describe(ctypes.byref(_args(_lib, 5, 14, 390, 260, 8, 2, 1, False, schedule=1 << 24)), _lib.OP_CONV1D_FWD, buf, 256) == _lib.ERR_SHAPE
    assert _lib.SCHED_SLOTS(31) == SLOTS(31) == 31 << 19 and ops.SCHED_SLOTS(1) == SLOTS(1)
    with pytest.raises(ValueError):
        _lib.SCHED_SLOTS(32)


def test_split_cases_hold_every_regime_for_every_family():
    """Coverage of the tables, as test_every_fixup_instantiation_is_reached_by_a_small_case asserts it for FIXUP_CASES."""
    by = {}
    for (geom, op, sched, fam, epi, form), declared, _ in SPLIT_TABLE:
        for r in declared:
            by.setdefault(r, set()).add((fam, epi, form, sched))
    pairs = {(c[3], c[4]) for c in FIXUP_CASES}
    assert len(pairs) == 14
    # several whole tiles per workgroup, and a range with a whole tile between a partial head and a partial tail: every (family, epilogue)
    assert {(f, e) for f, e, _, _ in by["multi-whole"]} == pairs and {(f, e) for f, e, _, _ in by["head-whole-tail"]} == pairs
    assert {form for _, _, form, _ in by["head-whole-tail"]} == {"plain"}                       # (NOT_REACHED: never wide)
    # conv_raw3: super-rows of 2 over a short last super-row in both regimes, and whole tiles beside the column-tail launch
    for regime in ("multi-whole", "head-whole-tail"):
        assert {e for f, e, _, s in by[regime] if f == "conv_raw3" and s & SR2} == {"F", "Tpm"}
    assert ("conv_raw3", "F", "tail") in {r[:3] for r in by["multi-whole"]}
    # hybrid: conv_raw3 F and T; the 128 x 256 F kernel and both raw-window wgrads under the plain and under the wide fixup
    assert {r[:3] for r in by["hybrid"]} == {("conv_raw3", "F", "plain"), ("conv_raw3", "T", "plain")} | {
        (f, e, form) for f, e in (("conv_raw(128x256)", "F"), ("conv_g_raw", "G"), ("conv_g_ps", "G")) for form in ("plain", "wide")}
    # contended, and oversubscription factors 2 and 1 over more tiles than slots
    three = {"conv_raw3", "conv_raw(128x256)", "conv_g_raw"}
    assert {f for f, _, _, _ in by["contended"]} == three
    assert {(f, (s >> 8) & 15) for f, _, _, s in by["oversub"]} == {(f, o) for f in three for o in (1, 2)} | {("conv_raw3", 0)}      # (0: the default, 4)
    # both fixup forms wherever a family of the table has both (the wide one under the hybrid split)
    for fam in ("conv_raw(128x256)", "conv_g_raw", "conv_g_ps"):
        assert {c[5] for c in SPLIT_CASES if c[3] == fam} >= {"none", "plain", "wide"}
    assert {(epi, r) for (_, epi, _, _), declared, _ in SPLIT_TABLE_H for r in declared} == {
        (e, r) for e in ("F", "T") for r in ("multi-whole", "head-whole-tail", "hybrid")}
    assert len(NOT_REACHED) == 3
