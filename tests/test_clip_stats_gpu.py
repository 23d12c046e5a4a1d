"""GPU: BatchNorm with per-clip statistics (pg_clipnorm_fwd) and the inference forward built on it (stats="clip").

The reference runs inference one clip at a time with train-mode BatchNorm (demo.py:33-45, train.py:76-83), so a clip is normalised
by its own statistics.  stats="clip" gives that for B clips in one launch sequence.  Bounds are the project's own: 1e-4 relative to
max-abs for the kernel (TOL of test_ops_gpu.py), 2e-5 for forward tensors against the reference (TOL_F of test_unet_gpu.py), 5e-2
for bf16-resident against fp32 (test_e2e_gpu.py).  Everything that must not depend on the batch is compared bit for bit.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import signal_ref, unet_ref
from phasegen import detgen

pytestmark = pytest.mark.gpu
TOL, TOL_F, TOL_H = 1e-4, 2e-5, 5e-2
EPS = 1e-5
# every lane-group width (16 lanes: up to 128 units of one float, or of four where L % 4 == 0; 32 lanes: up to 256; 64 beyond), odd
# and non-multiple-of-4 lengths, 16-byte units (64, 256, 300, 512, 516, 1000, 1024), the longest register-resident rows (1023, 1024)
# and the looping kernel (1027, 1500)
SHAPES = [(1, 16, 3), (3, 48, 29), (5, 40, 61), (4, 24, 62), (3, 16, 64), (2, 24, 65), (3, 40, 126), (64, 40, 129), (3, 8, 255),
          (7, 8, 256), (2, 8, 300), (2, 4, 301), (2, 8, 512), (2, 8, 516), (2, 4, 1000), (2, 4, 1023), (2, 4, 1024), (2, 4, 1027),
          (2, 4, 1500), (1, 1, 1), (2, 3, 2)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def act64(v, act):
    from phasegen import ops
    if act == ops.ACT_LEAKY:
        return torch.where(v > 0, v, 0.2 * v)
    return v.clamp_min(0) if act == ops.ACT_RELU else v


def inputs(B, C, L, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * C + L)
    x = torch.randn(B, C, L, generator=g) * (0.5 + 2 * torch.rand(B, C, 1, generator=g)) + 3 * torch.randn(B, C, 1, generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    return x.cuda(), gamma.cuda(), beta.cuda()


def expected64(x, gamma, beta):
    """float64 per row: mean, biased variance, normalised + affine output."""
    x = x.double()
    mean = x.mean(dim=2, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=2, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * gamma.double()[None, :, None] + beta.double()[None, :, None], mean[..., 0], var[..., 0]


def run(x, gamma, beta, act=0, bf16=True, pitch=None, **kw):
    """One pg_clipnorm_fwd call with fresh outputs: (y, yh or None, save_mean, save_invstd)."""
    from phasegen import ops
    B, C, L = x.shape
    y = torch.full((B, C, L), float("nan"), device="cuda")
    sm, si = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
    yh = None
    if bf16:
        if pitch is None:
            yh = ops.h_alloc(B, C, L, x.device)
        else:
            yh = torch.zeros(B, C, pitch, device="cuda", dtype=torch.bfloat16)
        yh.fill_(-7.0)                                   # sentinel: the row tails must come back untouched
    ops.clipnorm_fwd(x, y, gamma, beta, sm, si, y_act=act, yh=yh, yh_act=act, **kw)
    return y, yh, sm, si


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_float64(shape):
    from phasegen import ops
    B, C, L = shape
    x, gamma, beta = inputs(B, C, L)
    worst = 0.0
    for act in (ops.ACT_NONE, ops.ACT_LEAKY, ops.ACT_RELU):
        y, yh, sm, si = run(x, gamma, beta, act)
        want, mean, var = expected64(x, gamma, beta)
        e = (rel(y, act64(want, act)), rel(sm, mean), rel(si, 1 / torch.sqrt(var + EPS)))
        worst = max(worst, *e)
        assert max(e) < TOL, (shape, act, e)
        # bf16 copy: round-to-nearest-even of the fp32 output of the same call, bit for bit; tails untouched
        assert torch.equal(yh[:, :, :L].view(torch.int16), y.to(torch.bfloat16).view(torch.int16)), (shape, act)
        assert bool((yh[:, :, L:] == -7.0).all())
    print(f"\nclipnorm {shape}: max error vs float64 {worst:.2e} (bound {TOL:g})")


def test_kernel_writes_concat_half_with_second_activated_output():
    """y into the upper half of a (B, 2C', L) buffer (the U-Net's concat), y2 = a second copy with its own activation, for a
    scalar-unit length and a 16-byte-unit one."""
    from phasegen import ops
    for B, C, L in ((3, 24, 61), (3, 24, 128)):
        x, gamma, beta = inputs(B, C, L, seed=1)
        cat = torch.full((B, 2 * C, L), 5.0, device="cuda")
        l2 = torch.empty(B, C, L, device="cuda")
        ops.clipnorm_fwd(x, cat[:, C:], gamma, beta, y_act=ops.ACT_RELU, y2=l2, y2_act=ops.ACT_LEAKY)
        want, _, _ = expected64(x, gamma, beta)
        e = (rel(cat[:, C:], act64(want, ops.ACT_RELU)), rel(l2, act64(want, ops.ACT_LEAKY)))
        print(f"\nclipnorm concat half {(B, C, L)}: {e[0]:.2e} {e[1]:.2e}")
        assert max(e) < TOL and bool((cat[:, :C] == 5.0).all())
        y, _, _, _ = run(x, gamma, beta, ops.ACT_RELU, bf16=False)
        assert torch.equal(cat[:, C:], y)                # where the output lives does not change a bit of it


@pytest.mark.parametrize("shape", [(3, 24, 61), (3, 24, 128)], ids=["scalar-units", "16-byte-units"])
def test_kernel_writes_all_four_outputs_at_once(shape):
    """y, y2, yh and yh2 of ONE call, each with another activation: every output against float64, the bf16 copies the bit-exact
    rounding of the activated fp32 values of the same call (y is stored unactivated, so they can be recomputed from it)."""
    from phasegen import ops
    B, C, L = shape
    x, gamma, beta = inputs(B, C, L, seed=5)
    y, y2 = torch.full((B, C, L), float("nan"), device="cuda"), torch.full((B, C, L), float("nan"), device="cuda")
    yh, yh2 = ops.h_alloc(B, C, L, "cuda").fill_(-7.0), ops.h_alloc(B, C, L, "cuda").fill_(-7.0)
    ops.clipnorm_fwd(x, y, gamma, beta, y_act=ops.ACT_NONE, y2=y2, y2_act=ops.ACT_RELU, yh=yh, yh_act=ops.ACT_LEAKY, yh2=yh2, yh2_act=ops.ACT_RELU)
    want, _, _ = expected64(x, gamma, beta)
    e = (rel(y, want), rel(y2, act64(want, ops.ACT_RELU)), rel(yh[:, :, :L], act64(want, ops.ACT_LEAKY)), rel(yh2[:, :, :L], act64(want, ops.ACT_RELU)))
    print(f"\nclipnorm four outputs {shape}: y {e[0]:.2e} y2 {e[1]:.2e} (bound {TOL:g}); yh {e[2]:.2e} yh2 {e[3]:.2e} (+ one bf16 rounding, 2^-8)")
    assert max(e[:2]) < TOL and max(e[2:]) < TOL + 2.0 ** -8
    yc, y2c = y.cpu(), y2.cpu()
    assert torch.equal(y2c, F.relu(yc))
    assert torch.equal(yh[:, :, :L].cpu().view(torch.int16), F.leaky_relu(yc, 0.2).to(torch.bfloat16).view(torch.int16))
    assert torch.equal(yh2[:, :, :L].cpu().view(torch.int16), y2c.to(torch.bfloat16).view(torch.int16))
    assert yh.shape[2] > L and bool((yh[:, :, L:] == -7.0).all()) and bool((yh2[:, :, L:] == -7.0).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_invariance_is_bitwise(shape):
    B, C, L = shape
    x, gamma, beta = inputs(B, C, L, seed=2)
    y, yh, sm, si = run(x, gamma, beta)
    for b in range(B):
        y1, yh1, sm1, si1 = run(x[b:b + 1], gamma, beta)
        assert torch.equal(y[b:b + 1], y1) and torch.equal(yh[b:b + 1], yh1), (shape, b)
        assert torch.equal(sm[b:b + 1], sm1) and torch.equal(si[b:b + 1], si1), (shape, b)


def test_result_does_not_depend_on_access_width():
    """L % 4 == 0 rows are moved as 16-byte units where every tensor allows it and as scalars otherwise (here: a bf16 pitch that is
    not a multiple of 4, and a misaligned input): the arithmetic order depends on L alone, so the results are bit-identical."""
    B, C, L = 3, 8, 256
    x, gamma, beta = inputs(B, C, L, seed=3)
    y, yh, sm, si = run(x, gamma, beta)
    y_n, yh_n, sm_n, si_n = run(x, gamma, beta, pitch=L + 2)
    assert torch.equal(y, y_n) and torch.equal(yh[:, :, :L], yh_n[:, :, :L]) and torch.equal(sm, sm_n) and torch.equal(si, si_n)
    assert bool((yh_n[:, :, L:] == -7.0).all())
    flat = torch.empty(B * C * L + 1, device="cuda")
    xo = flat[1:].view(B, C, L)                          # 4-byte aligned only
    xo.copy_(x)
    y_o, _, sm_o, _ = run(xo, gamma, beta, bf16=False)
    assert torch.equal(y, y_o) and torch.equal(sm, sm_o)


@pytest.mark.parametrize("shape", [(1, 16, 3), (3, 48, 29), (5, 40, 61), (64, 40, 129), (7, 8, 256), (2, 4, 1500), (3, 5, 1)])
def test_running_buffers_bitwise_and_vs_torch(shape):
    from phasegen import ops
    B, C, L = shape
    x, gamma, beta = inputs(B, C, L, seed=4)
    g = torch.Generator().manual_seed(5)
    rm0, rv0 = torch.randn(C, generator=g).cuda(), (0.5 + torch.rand(C, generator=g)).cuda()
    rm, rv, nb = rm0.clone(), rv0.clone(), torch.full((), 11, device="cuda", dtype=torch.long)
    y = torch.empty_like(x)
    ops.clipnorm_fwd(x, y, gamma, beta, None, None, rm, rv, num_batches_tracked=nb)
    rm1, rv1, nb1 = rm0.clone(), rv0.clone(), torch.full((), 11, device="cuda", dtype=torch.long)
    y1 = torch.empty_like(x[:1])
    for b in range(B):
        ops.clipnorm_fwd(x[b:b + 1], y1, gamma, beta, None, None, rm1, rv1, num_batches_tracked=nb1)
    assert torch.equal(rm, rm1) and torch.equal(rv, rv1)
    assert int(nb) == 11 + B and int(nb1) == 11 + B
    if L > 1:                                            # (torch refuses one value per channel in training mode)
        rmt, rvt = rm0.clone(), rv0.clone()
        for b in range(B):
            F.batch_norm(x[b:b + 1], rmt, rvt, gamma, beta, training=True, momentum=0.1, eps=EPS)
        e = (rel(rm, rmt), rel(rv, rvt))
        print(f"\nclipnorm running buffers {shape}: vs torch {e[0]:.2e} {e[1]:.2e}")
        assert max(e) < TOL
    # only one of the two buffers, and the counter alone
    rm2, nb2 = rm0.clone(), torch.zeros((), device="cuda", dtype=torch.long)
    ops.clipnorm_fwd(x, y, gamma, beta, running_mean=rm2)
    ops.clipnorm_fwd(x, y, gamma, beta, num_batches_tracked=nb2)
    assert torch.equal(rm2, rm) and int(nb2) == B


def clips(C, L):
    """The three one-clip batches of seeds 1, 2, 3 stacked: (3, C, L) network input."""
    return torch.from_numpy(np.concatenate([detgen.make_batch(1, C, L, seed=s)[:, 0] for s in (1, 2, 3)]).copy())


@pytest.mark.parametrize("C,L", [(8, 24), (16, 64)])
def test_per_clip_forward_vs_reference_goldens(C, L, golden_dir):
    """One batched forward with per-clip statistics against the reference's batch-of-one golden (row 0) and against the oracle
    run clip by clip (all rows, all twelve running buffers).  Batch statistics miss these goldens by 0.44 - 0.67."""
    from phasegen.model import UNetModel
    gold = np.load(os.path.join(golden_dir, f"unet_C{C}_L{L}_B1.npz"))
    pn = detgen.make_params(C, seed=0)
    x = clips(C, L)
    eng = UNetModel(C, 2 * C).load_numpy(pn).engine
    out = eng.forward(x.cuda(), inference=True, stats="clip").clone()
    po = unet_ref.to_torch(pn)
    stats = {k: po[k] for k in po if "running" in k or "num_batches" in k}
    with torch.no_grad():
        want = torch.cat([unet_ref.unet_forward(po, x[b:b + 1], stats) for b in range(3)])
    e0, e = rel(out[:1], torch.from_numpy(gold["out"])), rel(out, want)
    print(f"\nper-clip forward C={C} L={L}: row 0 vs golden {e0:.2e}, all rows vs oracle loop {e:.2e} (bound {TOL_F:g})")
    assert e0 < TOL_F and e < TOL_F
    for k in detgen.BN_KEYS:
        for s in (".running_mean", ".running_var"):
            assert rel(eng.arena.buffers[k + s], stats[k + s]) < TOL_F, k + s
        assert int(eng.arena.buffers[k + ".num_batches_tracked"]) == int(stats[k + ".num_batches_tracked"])
    # the plain batched forward is a different function (what the feature is for)
    assert rel(eng.forward(x.cuda(), update_stats=False, inference=True)[:1], torch.from_numpy(gold["out"])) > 0.1


def test_engine_refuses_per_clip_statistics_outside_inference():
    from phasegen.model import UNetModel
    C, L = 8, 24
    eng = UNetModel(C, 2 * C).load_numpy(detgen.make_params(C, seed=0)).engine
    x = clips(C, L).cuda()
    with pytest.raises(ValueError, match="inference"):
        eng.forward(x, stats="clip")
    with pytest.raises(ValueError, match="stats"):
        eng.forward(x, inference=True, stats="sample")
    eng.forward(x)
    eng.forward(x, inference=True, stats="clip")
    assert eng.cur is None
    with pytest.raises(RuntimeError, match="before forward"):
        eng.backward(torch.zeros(3, 2 * C, L, device="cuda"))


def test_model_surface():
    from phasegen.model import UNetModel
    C, L = 16, 64
    m = UNetModel(C, 2 * C).load_numpy(detgen.make_params(C, seed=0))
    x = clips(C, L).cuda()
    with torch.no_grad():
        d0 = m.forward(x)
        got = m.forward(x, per_clip=True)
        d1 = m.forward(x)
        want = m.engine.forward(x, inference=True, stats="clip")
        assert torch.equal(got, want) and torch.equal(d0, d1) and not torch.equal(got, d0)
        assert got.data_ptr() != want.data_ptr()         # a copy, as the default forward returns
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward(x, per_clip=True)
    with pytest.raises(RuntimeError):                    # nothing to differentiate after a per-clip forward
        m.engine.backward(torch.zeros_like(want))
    out = m.forward(x)                                   # training forward + backward still work afterwards
    out.sum().backward()
    with torch.no_grad():
        assert torch.equal(out, d0)


def test_resident_path_per_clip():
    from phasegen.model import UNetModel
    C, B, L = 64, 5, 64
    pn = detgen.make_params(C, seed=0)
    x = torch.from_numpy(np.concatenate([detgen.make_batch(1, C, L, seed=50 + s)[:, 0] for s in range(B)]).copy()).cuda()
    ref = UNetModel(C, 2 * C, precision="fp32").load_numpy(pn).engine.forward(x, update_stats=False, inference=True, stats="clip").clone()
    eng = UNetModel(C, 2 * C, precision="bf16").load_numpy(pn).engine
    assert eng.resident_ok(B, L)
    eager = {s: eng.forward(x, update_stats=False, inference=True, stats=s).clone() for s in ("batch", "clip")}
    e = rel(eager["clip"], ref)
    print(f"\nresident per-clip vs fp32 per-clip: {e:.2e} (bound {TOL_H:g})")
    assert e < TOL_H and bool(torch.isfinite(eager["clip"]).all())
    assert rel(eager["batch"], eager["clip"]) > TOL_H                                # the two modes are far apart
    loop = torch.cat([eng.forward(x[b:b + 1], update_stats=False, inference=True).clone() for b in range(B)])
    print(f"resident per-clip batched vs loop of one-clip resident forwards: {rel(eager['clip'], loop):.2e} (informative)")
    nb = eng.arena.buffers[detgen.BN_KEYS[0] + ".num_batches_tracked"]
    nb0 = int(nb)
    eng.graphs = True
    try:
        for i in range(3):                               # eager, capture + replay, replay -- the modes interleaved at one shape
            for s in ("batch", "clip"):
                got = eng.forward(x, update_stats=(s == "clip"), inference=True, stats=s)
                assert torch.equal(got, eager[s]), (i, s)
        from phasegen import ops
        for key in (("graph", B, L, False, ops.current_schedule(), eng.precision), ("graph", B, L, True, ops.current_schedule(), eng.precision, "clip")):
            assert isinstance(eng.plans[key][0], torch.cuda.CUDAGraph)       # one graph per mode: the mode is part of the key
        assert int(nb) == nb0 + 3 * B                    # replays keep counting: one step per clip
    finally:
        eng.graphs = False


def test_validation_metrics_batched_vs_oracle():
    """The clips, oracle values and bounds of test_next_rows_gpu.py::test_validation_metrics_vs_oracle, forwards batched in chunks
    of two clips (2 + 1) with per-clip statistics."""
    from phasegen.model import UNetModel
    from phasegen.validate import validation_metrics
    C, L, n_fft, hop, n_clips, iters = 16, 24, 32, 8, 3, 4
    n = hop * (L - 1)
    cl = [detgen.make_clip(n, seed=120 + i) for i in range(n_clips)]
    P = np.ascontiguousarray(signal_ref.get_spec_and_angle(np.stack([signal_ref.chunk_and_stft(c, n_fft, hop) for c in cl])), dtype=np.float32)
    pn = detgen.make_params(C, seed=0)
    model = UNetModel(C, 2 * C, precision="fp32").load_numpy(pn)
    got = validation_metrics(model, torch.from_numpy(P).cuda(), hop, n_fft, gl_iters=iters, gl_seed=0, batched=True, clip_batch=2)
    po = unet_ref.to_torch(pn)
    mses, nops, lims = [], [], []
    for c in range(n_clips):
        with torch.no_grad():
            pred = unet_ref.unet_forward(po, torch.from_numpy(P[c:c + 1, 0].copy())).numpy()[0, :C]      # batch of one, train-mode BN
        mag = np.exp(P[c, 0]) - 1
        orig = signal_ref.generate_audio(mag * np.exp(P[c, 1] * 1.j), hop, is_stft=True)
        hyb = signal_ref.generate_audio(mag * np.exp(pred * 1.j), hop, is_stft=True)
        nop = signal_ref.generate_audio(mag.astype(np.complex64), hop, is_stft=True)
        g = torch.Generator(device="cpu")
        g.manual_seed(c)
        init = torch.randn(n, generator=g, dtype=torch.float64).numpy()
        lim, _, _ = signal_ref.griffin_lim(mag, n_fft, hop, iters, init)
        mses.extend(np.sqrt((orig - hyb) ** 2)); nops.extend(np.sqrt((orig - nop) ** 2)); lims.extend(np.sqrt((orig - lim) ** 2))
    want = {"MSE": float(np.mean(mses)), "NOPMSE": float(np.mean(nops)), "LMSE": float(np.mean(lims))}
    print("\nvalidation metrics (batched)", got, want)
    assert abs(got["MSE"] - want["MSE"]) < 1e-5 * want["MSE"]
    assert abs(got["NOPMSE"] - want["NOPMSE"]) < 1e-5 * want["NOPMSE"]
    assert abs(got["LMSE"] - want["LMSE"]) < 1e-4 * want["LMSE"]
    assert want["NOPMSE"] > 0 and want["MSE"] > 0
    assert int(model.engine.arena.buffers[detgen.BN_KEYS[0] + ".num_batches_tracked"]) == n_clips
