"""The fp32 raw-window wgrad kernels (conv_g_raw / conv_g_ps) read packed operands from the workspace: Q rows with zero halos, P with K
contiguous per row (flat K) or padded per sample, the activation applied.  These tests aim at what the packing removed from the slab
loop: slabs across sample ends at several frame counts, windows that leave the row on both sides (channel 0 with p > 0 included),
odd channel counts and partial column tiles, k = 5's 255-column tiles, the input activation, the fused Adam epilogue and the
stream-K split.  The workspace-size query is checked on the CPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref  # noqa: F401  (disables oneDNN: see the bug note in oracle/unet_ref.py)
from phasegen import detgen

# (transposed, Cin, Cout, k, s, p, Lin, B); LP = frames of the A operand (conv: Lout, convT: Lin) in the comment
GEOMS = [
    (False, 40, 48, 32, 2, 16, 258, 2),     # LP 130, flat K
    (True, 48, 33, 32, 2, 16, 129, 2),      # LP 129, flat K, 33 window channels
    (False, 33, 40, 8, 1, 2, 129, 3),       # LP 126, per-sample slabs
    (False, 16, 40, 8, 1, 2, 132, 2),       # LP 129 at k = 8: flat K (padding would cost 11.6 %)
    (True, 40, 31, 8, 2, 1, 61, 2),         # LP 61
    (False, 24, 40, 8, 2, 1, 52, 3),        # LP 24
    (False, 31, 64, 4, 2, 1, 61, 3),        # LP 30, k = 4
    (True, 64, 103, 5, 2, 1, 30, 2),        # LP 30, k = 5: two column tiles of 51 channels, the second partial
]
IDS = [f"{'t' if g[0] else 'c'}{g[1]}x{g[2]}-k{g[3]}s{g[4]}p{g[5]}-L{g[6]}-B{g[7]}" for g in GEOMS]
# automatic, one tile per workgroup, forced stream-K, flat K forced (bit 7) under stream-K
SCHEDULES = [0, 1, 2, 128 | 2]


def rnd(seed, *shape):
    return torch.from_numpy(detgen.uniform(seed, shape, -1.0, 1.0))


def act_cpu(x, act):
    return F.leaky_relu(x, 0.2) if act == 1 else (F.relu(x) if act == 2 else x)


def reference(geom, act):
    """float64 dW on the CPU, and the same sum over |terms| (the fp32 rounding bound scales with it)"""
    tr, Cin, Cout, k, s, p, Lin, B = geom
    x = rnd(1, B, Cin, Lin)
    w = torch.zeros((Cin, Cout, k) if tr else (Cout, Cin, k), dtype=torch.float64)
    Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    dy = rnd(3, B, Cout, Lout)
    out = []
    for xs, dys in ((act_cpu(x.double(), act), dy.double()), (act_cpu(x.double(), act).abs(), dy.double().abs())):
        wr = w.clone().requires_grad_(True)
        yr = F.conv_transpose1d(xs, wr, stride=s, padding=p) if tr else F.conv1d(xs, wr, stride=s, padding=p)
        yr.backward(dys)
        out.append(wr.grad)
    return x, dy, out[0], out[1]


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", SCHEDULES, ids=["auto", "tile-per-wg", "stream-k", "flat-K/stream-k"])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_wgrad_packed_against_fp64(geom, act, schedule):
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, B = geom
    x, dy, want, mag = reference(geom, act)
    dw = torch.full(want.shape, float("nan"), device="cuda")
    ops.conv_wgrad(x.cuda(), dy.cuda(), dw, s, p, x_act=act, transposed=tr, schedule=schedule)
    err = (dw.cpu().double() - want).abs()
    assert torch.isfinite(dw).all()
    assert bool((err <= 1e-5 * mag + 1e-12).all()), float((err / (mag + 1e-30)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_wgrad_packed_repeatable_and_adam_fused(geom):
    """Same inputs twice (the second call on a workspace full of the first call's packed operands) give the same bits, and the fused
    Adam epilogue equals wgrad followed by pg_adam_step bit for bit, under the forced stream-K split (partial tiles through the fixup)."""
    from phasegen import ops
    tr, Cin, Cout, k, s, p, Lin, B = geom
    x, dy, want, _ = reference(geom, 1)
    xd, dyd = x.cuda(), dy.cuda()
    dw1 = torch.empty(want.shape, device="cuda")
    dw2 = torch.empty(want.shape, device="cuda")
    ops.conv_wgrad(xd, dyd, dw1, s, p, x_act=1, transposed=tr, schedule=2)
    ops.conv_wgrad(xd, dyd, dw2, s, p, x_act=1, transposed=tr, schedule=2)
    assert torch.equal(dw1, dw2)
    w = rnd(7, *want.shape).cuda()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    w_ref, m_ref, v_ref = w.clone(), m.clone(), v.clone()
    ops.adam_step(w_ref, dw1, m_ref, v_ref, 1)
    dw3 = torch.empty_like(dw1)
    ops.conv_wgrad(xd, dyd, dw3, s, p, x_act=1, transposed=tr, schedule=2, adam=ops.adam_args(w, m, v, 1))
    assert torch.equal(dw3, dw1)
    assert torch.equal(w, w_ref) and torch.equal(m, m_ref) and torch.equal(v, v_ref)


def _args(_lib, geom, precision=0, schedule=0):
    tr, Cin, Cout, k, s, p, Lin, B = geom
    a = _lib.ConvArgs()
    a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad = B, Cin, Cout, Lin, k, s, p
    a.Lout = (Lin - 1) * s - 2 * p + k if tr else (Lin + 2 * p - k) // s + 1
    a.x = a.dy = a.dw = 4096                                  # never dereferenced: the size query and the refusal launch nothing
    a.x_bs, a.dy_bs = Cin * Lin, Cout * a.Lout
    a.precision, a.schedule = precision, schedule
    return a


def test_wgrad_workspace_query_and_refusal():
    """CPU: pg_workspace_bytes_wgrad = the stream-K region + the packed operands of the fp32 raw-window kernels (none at bf16 or on the
    im2col kernels); a wgrad handed less returns PG_ERR_WORKSPACE before launching anything."""
    from phasegen import _lib
    lib = _lib.load()
    base = lib.pg_workspace_bytes_conv()
    # U0 at the bench shape: Q = dy (64, 2048, 256) in rows of 320 floats (2 * 128 + 64), P = x (64, 4096, 129) flat: 516 slabs of 16
    u0 = (True, 4096, 2048, 32, 2, 16, 129, 64)
    a = _args(_lib, u0)
    want_q, want_p = 64 * 2048 * 320 * 4, 4096 * 516 * 16 * 4
    assert lib.pg_workspace_bytes_wgrad(ctypes.byref(a), _lib.OP_CONVT1D_WGRAD) == base + want_q + want_p
    # D1 (per-sample slabs): P = dy (64, 2048, 126) padded to 128 frames; Q = x (64, 2048, 129) in rows of 1 * 112 + 24 -> 136 floats
    d1 = (False, 2048, 2048, 8, 1, 2, 129, 64)
    assert lib.pg_workspace_bytes_wgrad(ctypes.byref(_args(_lib, d1)), _lib.OP_CONV1D_WGRAD) == base + 64 * 2048 * 136 * 4 + 64 * 2048 * 128 * 4
    for prec, sched in ((1, 0), (2, 0), (0, 4)):            # bf16 modes, and the im2col kernels (bit 2): nothing packed
        assert lib.pg_workspace_bytes_wgrad(ctypes.byref(_args(_lib, u0, prec, sched)), _lib.OP_CONVT1D_WGRAD) == base
    assert lib.pg_workspace_bytes_wgrad(ctypes.byref(a), _lib.OP_CONV1D_FWD) == _lib.ERR_UNSUPPORTED
    a.workspace, a.workspace_bytes = 4096, base + want_q + want_p - 1
    assert lib.pg_convt1d_wgrad(ctypes.byref(a), None) == _lib.ERR_WORKSPACE
