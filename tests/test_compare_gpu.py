"""GPU: pg_wave_compare and pg_spec_compare against float64 numpy restatements of their contracts (include/phasegen.h) on the same
fp32 inputs.  Reference and estimate are generated independently (phasegen.detgen), so nothing cancels.

Bounds.  pg_wave_compare forms exact products of two floats and adds at most 7e4 of them in double: slots 0, 1, 3 within 1e-10
relative, slot 2 within 1e-10 * sqrt(sum x^2 * sum y^2) (its terms change sign), slot 4 (a maximum of values formed by the same two
roundings as numpy's) within 1e-15 relative.  pg_spec_compare does its element arithmetic in fp32 -- at most ~10 ulp = 6e-7 on
non-negative terms; x16 margin: slots 0-3 within 1e-5 relative -- and slot 4 / frames, a few ulp of an fp32 log10 of magnitude
<= 100 dB, within 1e-4 dB.  Slot 5 and everything the contract calls bit-identical are compared exactly.
"""
import numpy as np
import pytest
import torch

from phasegen import detgen

pytestmark = pytest.mark.gpu
FLOOR = 1e-10
# (rows, n): the sizes of the issue (1 sample, less than one group of 4, the small track geometry's clip, just under a multiple of 4,
# nine chunks of 8192 with a short last group) on 1-3 rows
WAVE_SHAPES = [(1, 1), (2, 3), (3, 184), (1, 1023), (3, 70001)]
# (n, bins, frames): the issue's cases (one wave, one frame, odd sizes, 16 bin blocks, two frame tiles) plus one of two bin blocks by
# two frame tiles on the 16-byte path
SPEC_SHAPES = [(1, 16, 24), (3, 16, 24), (1, 16, 1), (2, 37, 70), (1, 1024, 5), (2, 16, 261), (2, 70, 264)]


# ---- float64 restatements ---------------------------------------------------------------------------------------------------------
def wave_ref(x, y, gain=None):
    """x, y (rows, n) float32 numpy -> (rows, 6) float64."""
    bad = ~(np.isfinite(x) & np.isfinite(y))
    x64, y64 = np.where(bad, 0.0, x).astype(np.float64), np.where(bad, 0.0, y).astype(np.float64)
    g = np.ones(len(x)) if gain is None else np.broadcast_to(np.asarray(gain, np.float64), (len(x),))
    d = x64 - g[:, None] * y64
    return np.stack([(x64 * x64).sum(1), (y64 * y64).sum(1), (x64 * y64).sum(1), (d * d).sum(1), np.abs(d).max(1), bad.sum(1).astype(np.float64)], 1)


def spec_ref(R, E, gain=None, floor=FLOOR):
    """R, E (n, 2, bins, frames) float32 numpy -> (n, 6) float64, with g_f = float32(gain) and the float32 floor the kernel gets."""
    bad = ~(np.isfinite(R).all(1) & np.isfinite(E).all(1))                            # (n, bins, frames)
    R64, E64 = np.where(bad[:, None], 0.0, R).astype(np.float64), np.where(bad[:, None], 0.0, E).astype(np.float64)
    g = np.ones(len(R)) if gain is None else np.broadcast_to(np.asarray(gain, np.float64), (len(R),)).astype(np.float32).astype(np.float64)
    mR, mE0 = np.sqrt(R64[:, 0] ** 2 + R64[:, 1] ** 2), np.sqrt(E64[:, 0] ** 2 + E64[:, 1] ** 2)
    mE = g[:, None, None] * mE0
    fl = float(np.float32(floor))
    dl = 10.0 * np.log10(np.maximum(mR * mR, fl)) - 10.0 * np.log10(np.maximum(mE * mE, fl))
    lsd = np.sqrt((dl * dl).mean(1)).sum(1)
    s = lambda a: a.sum((1, 2))
    return np.stack([s(mR * mR), s(mE0 * mE0), s(mR * mE0), s((mR - mE) ** 2), lsd, s(bad).astype(np.float64)], 1)


def check_wave(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    for s in (0, 1, 3):
        rel = np.abs(got[:, s] - want[:, s]) / np.maximum(want[:, s], np.finfo(np.float64).tiny)
        print(f"\n{what} slot {s}: worst relative error {rel.max():.3e} (bound 1e-10)")
        assert (rel <= 1e-10).all()
    e2 = np.abs(got[:, 2] - want[:, 2]) / np.maximum(np.sqrt(want[:, 0] * want[:, 1]), np.finfo(np.float64).tiny)
    print(f"{what} slot 2: worst error / sqrt(sum x^2 sum y^2) {e2.max():.3e} (bound 1e-10)")
    assert (e2 <= 1e-10).all()
    e4 = np.abs(got[:, 4] - want[:, 4])
    print(f"{what} slot 4: worst relative error {(e4 / np.maximum(want[:, 4], np.finfo(np.float64).tiny)).max():.3e} (bound 1e-15)")
    assert (e4 <= 1e-15 * want[:, 4]).all()
    assert np.array_equal(got[:, 5], want[:, 5])


def check_spec(got, want, frames, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    for s in (0, 1, 2, 3):
        rel = np.abs(got[:, s] - want[:, s]) / np.maximum(np.abs(want[:, s]), np.finfo(np.float64).tiny)
        print(f"\n{what} slot {s}: worst relative error {rel.max():.3e} (bound 1e-5)")
        assert (rel <= 1e-5).all()
    e4 = np.abs(got[:, 4] - want[:, 4]) / frames
    print(f"{what} slot 4 / frames: worst error {e4.max():.3e} dB of {(want[:, 4] / frames).max():.3f} dB (bound 1e-4 dB)")
    assert (e4 <= 1e-4).all()
    assert np.array_equal(got[:, 5], want[:, 5])


def bits(t):
    return t.cpu().numpy().view(np.int64)


# ---- layouts: dense; rows / signals a multiple of 4 floats apart behind an aligned base (16-byte path wherever the contiguous axis
# allows); the same behind a base pointer offset by one float (scalar path).  Everything outside the rows is NaN: reading it would
# show in slot 5 ---------------------------------------------------------------------------------------------------------------------
def layouts(a):
    """a: numpy (rows, ...) float32 -> dict of device views holding the same values."""
    rows, row = a.shape[0], int(np.prod(a.shape[1:]))
    d = torch.from_numpy(a).cuda()
    stride = (row + 3) // 4 * 4 + 4
    out = {"dense": d}
    for name, off in (("strided", 0), ("offset", 1)):
        flat = torch.full((rows * stride + off,), float("nan"), device="cuda")
        v = flat[off:].view(rows, stride)[:, :row]
        v.copy_(d.reshape(rows, row))
        out[name] = v.view(a.shape) if a.ndim == 2 else v.unflatten(1, a.shape[1:])
        assert out[name].data_ptr() % 16 == 4 * off
    return out


_cache = {}


def wave_case(shape):
    if ("w",) + shape not in _cache:
        from phasegen import ops
        rows, n = shape
        x, y = detgen.normal(5, shape, std=0.7), detgen.normal(6, shape, std=0.5)
        gain = np.array([0.37, -1.25, 2.0])[:rows]
        X, Y = layouts(x), layouts(y)
        got = {k: ops.wave_compare(X[k], Y[k]) for k in X}
        got_g = {k: ops.wave_compare(X[k], Y[k], gain=torch.from_numpy(gain).cuda()) for k in X}
        _cache[("w",) + shape] = (x, y, gain, X, Y, got, got_g, wave_ref(x, y), wave_ref(x, y, gain))
    return _cache[("w",) + shape]


def spec_case(shape):
    if ("s",) + shape not in _cache:
        from phasegen import ops
        n, bins, frames = shape
        R, E = detgen.normal(7, (n, 2, bins, frames), std=3.0), detgen.normal(8, (n, 2, bins, frames), std=2.0)
        gain = np.array([0.81, 1.7, 0.05])[:n]
        X, Y = layouts(R), layouts(E)
        got = {k: ops.spec_compare(X[k], Y[k]) for k in X}
        got_g = {k: ops.spec_compare(X[k], Y[k], gain=torch.from_numpy(gain).cuda()) for k in X}
        _cache[("s",) + shape] = (R, E, gain, X, Y, got, got_g, spec_ref(R, E), spec_ref(R, E, gain))
    return _cache[("s",) + shape]


# ---- pg_wave_compare --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", WAVE_SHAPES)
def test_wave_values_against_float64(shape):
    x, y, gain, X, Y, got, got_g, want, want_g = wave_case(shape)
    assert got["dense"].dtype == torch.float64 and tuple(got["dense"].shape) == (shape[0], 6)
    check_wave(got["dense"], want, f"wave {shape}")
    check_wave(got_g["dense"], want_g, f"wave {shape} with gains")
    assert np.array_equal(bits(got["dense"])[:, :3], bits(got_g["dense"])[:, :3])       # the gain touches slots 3 and 4 only


@pytest.mark.parametrize("shape", WAVE_SHAPES)
def test_wave_paths_and_batching_are_bit_identical(shape):
    from phasegen import ops
    x, y, gain, X, Y, got, got_g, want, want_g = wave_case(shape)
    for k in ("strided", "offset"):                                                     # 16-byte path == scalar path == dense
        assert np.array_equal(bits(got[k]), bits(got["dense"])), k
        assert np.array_equal(bits(got_g[k]), bits(got_g["dense"])), k
    g = torch.from_numpy(gain).cuda()
    for s in range(shape[0]):                                                           # row s alone == row s of the batch
        for k in ("strided", "offset"):
            alone = ops.wave_compare(X[k][s], Y[k][s], gain=g[s:s + 1])
            assert np.array_equal(bits(alone), bits(got_g["dense"][s:s + 1])), (s, k)
    out = torch.zeros(shape[0], 6, dtype=torch.float64, device="cuda")                  # out= and a number as the gain
    assert ops.wave_compare(X["dense"], Y["dense"], gain=0.37, out=out) is out
    assert np.array_equal(bits(out[0]), bits(got_g["dense"][0]))


@pytest.mark.parametrize("shape", WAVE_SHAPES)
def test_wave_identical_inputs_give_exact_zeros(shape):
    from phasegen import ops
    x, y, gain, X, Y, got, got_g, want, want_g = wave_case(shape)
    for k in X:
        r = ops.wave_compare(X[k], X[k].clone()).cpu().numpy()
        assert (r[:, 3] == 0).all() and (r[:, 4] == 0).all() and (r[:, 5] == 0).all(), k
        assert np.array_equal(r[:, 0], r[:, 1]) and np.array_equal(r[:, 0], r[:, 2])


@pytest.mark.parametrize("shape", [(3, 184), (3, 70001)])
def test_wave_non_finite_samples_are_counted_and_zeroed(shape):
    from phasegen import ops
    x, y, gain, X, Y, got, got_g, want, want_g = wave_case(shape)
    rows, n = shape
    yb, xb = y.copy(), x.copy()
    yb[0, n // 3] = np.nan
    yb[rows - 1, n - 1] = np.inf
    yb[rows - 1, 0] = -np.inf
    xb[1, n // 2] = np.nan                                                              # (and one in the reference)
    want = wave_ref(xb, yb, gain)
    assert want[:, 5].tolist() == [1.0, 1.0, 2.0]
    Xb, Yb = layouts(xb), layouts(yb)
    g = torch.from_numpy(gain).cuda()
    first = None
    for k in Xb:
        r = ops.wave_compare(Xb[k], Yb[k], gain=g)
        check_wave(r, want, f"wave {shape} with NaN / inf planted ({k})")
        first = bits(r) if first is None else first
        assert np.array_equal(bits(r), first)
    xz, yz = np.where(np.isfinite(xb) & np.isfinite(yb), xb, 0), np.where(np.isfinite(xb) & np.isfinite(yb), yb, 0)     # zeroed in BOTH inputs
    clean = ops.wave_compare(torch.from_numpy(xz.astype(np.float32)).cuda(), torch.from_numpy(yz.astype(np.float32)).cuda(), gain=g)
    assert np.array_equal(first[:, :5], bits(clean)[:, :5])


# ---- pg_spec_compare --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SPEC_SHAPES)
def test_spec_values_against_float64(shape):
    R, E, gain, X, Y, got, got_g, want, want_g = spec_case(shape)
    assert got["dense"].dtype == torch.float64 and tuple(got["dense"].shape) == (shape[0], 6)
    check_spec(got["dense"], want, shape[2], f"spec {shape}")
    check_spec(got_g["dense"], want_g, shape[2], f"spec {shape} with gains")
    assert np.array_equal(bits(got["dense"])[:, :3], bits(got_g["dense"])[:, :3])       # the gain touches slots 3 and 4 only


@pytest.mark.parametrize("shape", SPEC_SHAPES)
def test_spec_paths_and_batching_are_bit_identical(shape):
    from phasegen import ops
    R, E, gain, X, Y, got, got_g, want, want_g = spec_case(shape)
    for k in ("strided", "offset"):                                                     # strided signals; 16-byte path == scalar path
        assert np.array_equal(bits(got[k]), bits(got["dense"])), k
        assert np.array_equal(bits(got_g[k]), bits(got_g["dense"])), k
    g = torch.from_numpy(gain).cuda()
    for s in range(shape[0]):
        for k in ("strided", "offset"):
            alone = ops.spec_compare(X[k][s:s + 1], Y[k][s:s + 1], gain=g[s:s + 1])
            assert np.array_equal(bits(alone), bits(got_g["dense"][s:s + 1])), (s, k)
    out = torch.zeros(shape[0], 6, dtype=torch.float64, device="cuda")
    assert ops.spec_compare(X["dense"], Y["dense"], gain=0.81, floor=FLOOR, out=out) is out
    assert np.array_equal(bits(out[0]), bits(got_g["dense"][0]))


@pytest.mark.parametrize("shape", SPEC_SHAPES)
def test_spec_identical_inputs_give_exact_zeros(shape):
    from phasegen import ops
    R, E, gain, X, Y, got, got_g, want, want_g = spec_case(shape)
    for k in X:
        r = ops.spec_compare(X[k], X[k].clone()).cpu().numpy()
        assert (r[:, 3] == 0).all() and (r[:, 4] == 0).all() and (r[:, 5] == 0).all(), k
        assert np.array_equal(r[:, 0], r[:, 1]) and np.array_equal(r[:, 0], r[:, 2])


@pytest.mark.parametrize("shape", [(3, 16, 24), (2, 37, 70), (2, 70, 264)])
def test_spec_non_finite_cells_are_counted_and_zeroed(shape):
    from phasegen import ops
    R, E, gain, X, Y, got, got_g, want, want_g = spec_case(shape)
    n, bins, frames = shape
    Eb, Rb = E.copy(), R.copy()
    Eb[0, 0, bins // 2, frames // 3] = np.nan                                           # a real part
    Eb[0, 1, bins // 2, frames // 3] = np.inf                                           # ... and the imaginary part of the SAME cell: one cell
    Eb[n - 1, 1, bins - 1, frames - 1] = -np.inf
    Eb[n - 1, 0, 0, 0] = np.inf
    Rb[1, 1, 3, 5] = np.nan                                                             # (and one in the reference)
    want = spec_ref(Rb, Eb, gain)
    assert want[:, 5].sum() == 4.0 and want[0, 5] >= 1.0
    Xb, Yb = layouts(Rb), layouts(Eb)
    g = torch.from_numpy(gain).cuda()
    first = None
    for k in Xb:
        r = ops.spec_compare(Xb[k], Yb[k], gain=g)
        check_spec(r, want, frames, f"spec {shape} with NaN / inf planted ({k})")
        first = bits(r) if first is None else first
        assert np.array_equal(bits(r), first)
    ok = (np.isfinite(Rb).all(1) & np.isfinite(Eb).all(1))[:, None]
    clean = ops.spec_compare(torch.from_numpy(np.where(ok, Rb, 0).astype(np.float32)).cuda(),
                             torch.from_numpy(np.where(ok, Eb, 0).astype(np.float32)).cuda(), gain=g)
    assert np.array_equal(first[:, :5], bits(clean)[:, :5])


def test_spec_cells_that_are_zero_in_both_inputs_add_nothing_to_the_level_distance():
    """Both levels are the floor's, whatever the gain: zero rows and columns change slots 0-3 by their (zero) terms only and slot 4
    by sqrt of a smaller mean -- restated in float64 -- and an all-zero pair gives six exact zeros."""
    from phasegen import ops
    R, E = detgen.normal(7, (2, 2, 37, 70), std=3.0), detgen.normal(8, (2, 2, 37, 70), std=2.0)
    R[:, :, 5:9], E[:, :, 5:9] = 0.0, 0.0                                               # silent bins
    R[:, :, :, 60:], E[:, :, :, 60:] = 0.0, 0.0                                         # silent frames
    gain = np.array([0.81, 1.7])
    r = ops.spec_compare(torch.from_numpy(R).cuda(), torch.from_numpy(E).cuda(), gain=torch.from_numpy(gain).cuda())
    want = spec_ref(R, E, gain)
    check_spec(r, want, 70, "spec with silent bins and frames")
    live = spec_ref(R[:, :, :, :60], E[:, :, :, :60], gain)
    assert np.allclose(want[:, 4], live[:, 4], rtol=1e-13)                              # the silent frames add exactly nothing
    r60 = ops.spec_compare(torch.from_numpy(np.ascontiguousarray(R[:, :, :, :60])).cuda(),
                           torch.from_numpy(np.ascontiguousarray(E[:, :, :, :60])).cuda(), gain=torch.from_numpy(gain).cuda())
    assert np.array_equal(bits(r)[:, 4], bits(r60)[:, 4])
    z = torch.zeros(2, 2, 37, 70, device="cuda")
    assert (ops.spec_compare(z, z.clone(), gain=3.0).cpu().numpy() == 0).all()


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from phasegen import ops
    x = torch.zeros(2, 100, device="cuda")
    with pytest.raises(ValueError):
        ops.wave_compare(x, x[:, :99])
    with pytest.raises(ValueError):
        ops.wave_compare(x[:, ::2], x[:, ::2])
    with pytest.raises(ValueError):
        ops.wave_compare(x, x, gain=torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.wave_compare(x.double(), x.double())
    R = torch.zeros(2, 2, 16, 24, device="cuda")
    with pytest.raises(ValueError):
        ops.spec_compare(R, R[:, :, :8])
    with pytest.raises(ValueError):
        ops.spec_compare(R[:, :, ::2], R[:, :, ::2])
    with pytest.raises(RuntimeError, match="floor_power"):
        ops.spec_compare(R, R, floor=0.0)
