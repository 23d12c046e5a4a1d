"""GPU: pg_stitch, the crossfaded overlap-add of equal-length clips into tracks, against its arithmetic contract restated in
float64 numpy (include/phasegen.h): for output sample t, k = min(t div step, n_clips-1), j = t - k step; covered twice (k >= 1 and
j < V) -> (a lo + b hi) / (a + b) with a = ramp[V-1-j], b = ramp[j], lo = clip[k-1][j+step], hi = clip[k][j]; else clip[k][j].

Bound: |out - ref| <= 8 * 2^-24 * max|clips|: two products, two sums and one division (at most 2.5 ulp) are about 5 unit roundoffs
of a quotient whose magnitude is at most max|clips| (a convex combination).  Samples covered by one clip are bit-exact.
"""
import numpy as np
import pytest
import torch

from phasegen import detgen

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# (n_tracks, n_clips, T, V, cut): n_out = (n_clips-1) step + T - cut.  16-byte and scalar paths, odd sizes, the largest overlap
# (2 V = T), a last clip cut down to one sample, a single clip, and more than one workgroup
SHAPES = [(1, 5, 184, 64, 37), (2, 4, 184, 92, 0), (1, 7, 184, 8, 183), (1, 9, 23, 11, 3), (1, 1, 184, 64, 100), (2, 40, 4096, 1024, 1000)]


def n_out_of(shape):
    n_tracks, n_clips, T, V, cut = shape
    return (n_clips - 1) * (T - V) + T - cut


def make_clips(shape, seed=3):
    n_tracks, n_clips, T, V, cut = shape
    return detgen.normal(seed, (n_tracks, n_clips, T), std=3.0)


def ref64(clips, step, n_out):
    """-> (float64 (n_tracks, n_out), mask of the samples covered by two clips)."""
    from phasegen import ops
    n_tracks, n_clips, T = clips.shape
    V = T - step
    ramp = ops.stitch_ramp_host(V).astype(np.float64)
    c = clips.astype(np.float64)
    t = np.arange(n_out)
    k = np.minimum(t // step, n_clips - 1)
    j = t - k * step
    hi = c[:, k, j]
    two = (k >= 1) & (j < V)
    out = hi.copy()
    if two.any():
        kk, jj = k[two], j[two]
        a, b = ramp[V - 1 - jj], ramp[jj]
        out[:, two] = (a * c[:, kk - 1, jj + step] + b * c[:, kk, jj]) / (a + b)
    return out, two


_cache = {}


def case(shape):
    """clips (numpy + device), the float64 reference and the dense, aligned, un-normalised result: computed once per shape."""
    if shape not in _cache:
        from phasegen import ops
        n_tracks, n_clips, T, V, cut = shape
        clips = make_clips(shape)
        n_out = n_out_of(shape)
        ref, two = ref64(clips, T - V, n_out)
        d = torch.from_numpy(clips).cuda()
        out = ops.stitch(d, T - V, n_out)
        _cache[shape] = (clips, d, ref, two, out)
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_values_against_float64(shape):
    n_tracks, n_clips, T, V, cut = shape
    clips, d, ref, two, out = case(shape)
    assert tuple(out.shape) == (n_tracks, n_out_of(shape))
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref).max()
    bound = 8 * U * np.abs(clips).max()
    print(f"\nstitch {shape}: max error vs float64 {err:.3e} (bound {bound:.3e}); {int(two.sum())} of {two.size} samples crossfaded")
    assert err <= bound
    assert np.array_equal(got[:, ~two].view(np.int32), ref[:, ~two].astype(np.float32).view(np.int32))     # single cover: copied


def test_2d_input_gives_1d_output():
    from phasegen import ops
    shape = SHAPES[0]
    clips, d, ref, two, out = case(shape)
    o1 = ops.stitch(d[0], 184 - 64, n_out_of(shape))
    assert tuple(o1.shape) == (n_out_of(shape),) and torch.equal(o1, out[0])


def test_no_overlap_concatenates_bit_for_bit():
    from phasegen import ops
    shape = (1, 3, 184, 0, 5)
    clips = make_clips(shape, seed=4)
    n_out = n_out_of(shape)
    out = ops.stitch(torch.from_numpy(clips).cuda(), 184, n_out).cpu().numpy()
    assert np.array_equal(out.reshape(-1).view(np.int32), clips.reshape(-1)[:n_out].view(np.int32))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[5]])
def test_all_ones_clips_give_all_ones(shape):
    from phasegen import ops
    n_tracks, n_clips, T, V, cut = shape
    out = ops.stitch(torch.ones(n_tracks, n_clips, T, device="cuda"), T - V, n_out_of(shape))
    assert bool((out == 1.0).all())


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[5]])
def test_result_does_not_depend_on_access_width(shape):
    """The same clips with clip_stride = T + 1, starting one element into their buffer, and out rows n_out + 3 apart: no 16-byte
    access is possible, the bits are those of the dense aligned call."""
    from phasegen import ops
    n_tracks, n_clips, T, V, cut = shape
    clips, d, ref, two, out = case(shape)
    n_out = n_out_of(shape)
    buf = torch.full((1 + n_tracks * n_clips * (T + 1),), float("nan"), device="cuda")
    view = buf[1:].as_strided((n_tracks, n_clips, T), (n_clips * (T + 1), T + 1, 1))
    view.copy_(d)
    obuf = torch.full((n_tracks, n_out + 3), -7.0, device="cuda")
    o = ops.stitch(view, T - V, n_out, out=obuf[:, :n_out])
    assert o.data_ptr() == obuf.data_ptr()
    assert torch.equal(obuf[:, :n_out].view(torch.int32), out.view(torch.int32))
    assert bool((obuf[:, n_out:] == -7.0).all())                                    # nothing past a row's end is written


def test_normalisation():
    from phasegen import ops
    shape = SHAPES[1]
    n_tracks, n_clips, T, V, cut = shape
    clips, d, ref, two, raw = case(shape)
    n_out = n_out_of(shape)
    raw2, peak, bad = ops.stitch(d, T - V, n_out, return_status=True)
    assert torch.equal(raw2, raw) and int(bad.item()) == 0
    want_peak = raw.abs().max()                                                     # jointly over both tracks
    assert peak.dtype == torch.float32 and torch.equal(peak, want_peak)
    assert float(raw[0].abs().max()) != float(raw[1].abs().max())                   # (the joint peak is not each track's own)
    out, peak_n, bad_n = ops.stitch(d, T - V, n_out, normalize=True, return_status=True)
    assert torch.equal(peak_n, want_peak) and int(bad_n.item()) == 0
    assert float(out.abs().max()) == 1.0
    want = raw.double() / want_peak.double()
    rel = float(((out.double() - want).abs() / want.abs().clamp_min(1e-300)).max())
    print(f"\nstitch normalise: max relative error vs raw / peak {rel:.3e} (bound {2 * U:.3e})")
    assert rel <= 2 * U
    again = ops.stitch(d, T - V, n_out, normalize=True)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))              # run to run
    z, zp, zb = ops.stitch(torch.zeros_like(d), T - V, n_out, normalize=True, return_status=True)
    assert bool((z == 0).all()) and float(zp) == 0.0 and int(zb) == 0


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_non_finite_samples_are_counted_and_kept_out_of_the_peak(shape):
    from phasegen import ops
    n_tracks, n_clips, T, V, cut = shape
    step = T - V
    clips, d, ref, two, raw = case(shape)
    n_out = n_out_of(shape)
    bad_clips = clips.copy()
    bad_clips[0, 1, 3] = np.nan                     # j = 3 < V of clip 1: in the crossfade with clip 0
    bad_clips[n_tracks - 1, 0, 1] = np.inf          # the head of clip 0: covered once
    with np.errstate(invalid="ignore"):
        r64, _ = ref64(bad_clips, step, n_out)
    want_bad = int((~np.isfinite(r64)).sum())
    assert want_bad == 2
    out, peak, bad = ops.stitch(torch.from_numpy(bad_clips).cuda(), step, n_out, return_status=True)
    got = out.cpu().numpy()
    assert int(bad.item()) == want_bad
    assert np.array_equal(np.isfinite(got), np.isfinite(r64))
    assert float(peak) == float(np.abs(got[np.isfinite(got)]).max())
    _, _, clean = ops.stitch(d, step, n_out, return_status=True)
    assert int(clean.item()) == 0


def test_contract_violations_raise_before_the_library_is_called():
    from phasegen import ops
    d = torch.zeros(2, 4, 184, device="cuda")
    with pytest.raises(ValueError):
        ops.stitch(d, 91, 3 * 91 + 184)             # 2 V > T
    with pytest.raises(ValueError):
        ops.stitch(d, 185, 3 * 185 + 1)             # step > T
    with pytest.raises(ValueError):
        ops.stitch(d, 120, 3 * 120)                 # n_out too short: the last clip would be unused
    with pytest.raises(ValueError):
        ops.stitch(d, 120, 3 * 120 + 185)           # n_out beyond the last clip
    with pytest.raises(ValueError):
        ops.stitch(d[:, :, ::2], 60, 3 * 60 + 92)   # samples not contiguous
    with pytest.raises(ValueError):
        ops.stitch(d, 120, 3 * 120 + 184, out=torch.zeros(2, 10, device="cuda"))
    with pytest.raises(ValueError):
        ops.stitch(d.double(), 120, 3 * 120 + 184)
