"""pg_stft_crops against its contract: the bits of stft -> standardize_with_ -> polar on the gathered, zero-padded crops in every
kernel family and store path; no sample outside a crop's own track is read; a row does not depend on its batch; and the values
agree with the oracle (oracle/signal_ref.py) within the tolerances of tests/test_signal_gpu.py.

The source is three detgen.make_clip tracks packed back to back (the second one shorter than a crop); the seven crops are the edge
cases of the memory contract (see ``crops_of``).

(The file name sorts behind every older test file, like the other test_z_* files: the older tests keep their place in the run.)"""
import functools

import numpy as np
import pytest
import torch

from oracle import signal_ref
from phasegen import detgen

gpu = pytest.mark.gpu

MEAN, STD = 0.0123, 1.7
# (n_fft, hop, crop_len, single_frame)
CASES = [(64, 16, 496, 0),          # four-frame kernel, 32 frames: 16-byte stores
         (64, 16, 520, 0),          # four-frame kernel, 33 frames: scalar stores and a partial group
         (64, 16, 496, 1),          # radix-2
         (1024, 256, 6144, 0),      # wave kernel, P = 8, 25 frames
         (2048, 512, 12288, 0),     # wave kernel, P = 16, 25 frames
         (4096, 1024, 8192, 0)]     # radix-2 by size
ROWS_OF_TRACKS_0_AND_2 = (0, 1, 2, 4, 6)


@functools.lru_cache(None)
def source(crop_len):
    """(flat float32 buffer, [(first, one past last) of each track]): tracks of 2 L + 7, L // 2 and L + L // 3 samples."""
    lens = (2 * crop_len + 7, crop_len // 2, crop_len + crop_len // 3)
    tracks = [detgen.make_clip(n, seed=40 + i) for i, n in enumerate(lens)]
    bounds, o = [], 0
    for n in lens:
        bounds.append((o, o + n))
        o += n
    buf = np.concatenate(tracks)
    buf.setflags(write=False)
    return buf, bounds


def crops_of(crop_len):
    """(begin, end) int64 arrays of the seven crops."""
    _, ((b0, e0), (b1, e1), (b2, e2)) = source(crop_len)
    crops = [(b0, e0),                                  # 0: a track's first sample
             (b0 + 3, e0),                              # 1: an odd offset
             (e0 - crop_len // 3, e0),                  # 2: begins in track 0 and would run into track 1
             (b1, e1),                                  # 3: the whole of track 1 (shorter than a crop)
             (e0 - 1, e0),                              # 4: begins at a track's last sample
             (b1 + 4, b1 + 4),                          # 5: end == begin: all zeros
             (e2 - crop_len // 2, e2)]                  # 6: in track 2, runs past the end of the buffer
    return np.array([c[0] for c in crops], np.int64), np.array([c[1] for c in crops], np.int64)


def gather(buf, begin, end, crop_len):
    """The crops as the reference builds them: copied out and zero-padded (preproc_mdb.py:84-88)."""
    out = np.zeros((len(begin), crop_len), np.float32)
    for i, (b, e) in enumerate(zip(begin, end)):
        lim = min(max(e - b, 0), crop_len)
        out[i, :lim] = buf[b:b + lim]
    return out


def composition(gathered, n_fft, hop, single, stats, polar):
    """The three launches the fused call replaces, on device copies of the gathered crops."""
    from phasegen import ops
    x = ops.stft(torch.from_numpy(gathered).cuda(), n_fft, hop, single_frame=single)
    if stats:
        ops.standardize_with_(x, MEAN, STD)
    return ops.polar(x) if polar else x


def run(buf, begin, end, crop_len, n_fft, hop, single, stats, polar):
    from phasegen import ops
    return ops.stft_crops(torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(begin.copy()).cuda(), torch.from_numpy(end.copy()).cuda(),
                          crop_len, n_fft, hop, polar=polar, stats=(MEAN, STD) if stats else None, single_frame=single)


@gpu
@pytest.mark.parametrize("stats,polar", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("n_fft,hop,crop_len,single", CASES)
def test_equals_the_three_launch_composition_bit_for_bit(n_fft, hop, crop_len, single, stats, polar):
    buf, _ = source(crop_len)
    begin, end = crops_of(crop_len)
    got = run(buf, begin, end, crop_len, n_fft, hop, single, stats, polar)
    want = composition(gather(buf, begin, end, crop_len), n_fft, hop, single, stats, polar)
    assert got.shape == want.shape == (7, 2, n_fft // 2, 1 + crop_len // hop)
    assert bool(torch.isfinite(got).all())
    for r in range(7):
        assert torch.equal(got[r], want[r]), (r, float((got[r] - want[r]).abs().max()))
    if not stats and not polar:                                        # and the chunked pg_stft itself, reading track by track
        from phasegen import ops
        b0 = torch.from_numpy(begin[:3]).cuda()
        row0 = torch.from_numpy(buf[:2 * crop_len + 7].copy()).cuda()[None]
        assert torch.equal(got[:3], ops.stft(row0, n_fft, hop, single_frame=single, chunk_start=b0, chunk_len=crop_len))


@gpu
@pytest.mark.parametrize("n_fft,hop,crop_len,single", CASES)
def test_neighbouring_tracks_are_not_read(n_fft, hop, crop_len, single):
    buf, (_, (b1, e1), _) = source(crop_len)
    begin, end = crops_of(crop_len)
    clean = run(buf, begin, end, crop_len, n_fft, hop, single, True, True)
    loud = buf.copy()
    loud[b1:e1] = 1e30                                                 # every sample of track 1
    got = run(loud, begin, end, crop_len, n_fft, hop, single, True, True)
    for r in ROWS_OF_TRACKS_0_AND_2:
        assert torch.equal(got[r], clean[r]), r
    assert not torch.equal(got[3], clean[3])                           # (track 1's own crop did change)


@gpu
@pytest.mark.parametrize("n_fft,hop,crop_len,single", CASES)
def test_a_row_does_not_depend_on_its_batch(n_fft, hop, crop_len, single):
    buf, _ = source(crop_len)
    begin, end = crops_of(crop_len)
    full = run(buf, begin, end, crop_len, n_fft, hop, single, True, True)
    alone = run(buf, begin[3:4], end[3:4], crop_len, n_fft, hop, single, True, True)
    assert torch.equal(alone[0], full[3])
    first = run(buf, begin[[3, 0]], end[[3, 0]], crop_len, n_fft, hop, single, True, True)
    assert torch.equal(first[0], full[3]) and torch.equal(first[1], full[0])


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / max(float(np.max(np.abs(b))), 1e-30))


ORACLE_CASES = [(2048, 512, 12288), (64, 16, 496)]


@functools.lru_cache(None)
def oracle_crop(n_fft, hop, crop_len):
    """One crop with an eighth of zero tail (it begins 7 L / 8 before the end of track 0): (begin, end, standardised [re; im] of the
    oracle in float32, its [log1p|z|; angle], the angle mask of tests/test_signal_gpu.py taken on the standardised values)."""
    buf, ((b0, e0), _, _) = source(crop_len)
    begin, end = np.array([e0 - crop_len + crop_len // 8], np.int64), np.array([e0], np.int64)
    S = signal_ref.chunk_and_stft(gather(buf, begin, end, crop_len)[0], n_fft, hop).astype(np.float32)
    Z = (S - np.float32(MEAN)) / np.float32(STD)                        # the float32 formula of preproc_mdb.py:182
    assert Z.dtype == np.float32
    mag = np.abs(Z[0].astype(np.float64) + 1j * Z[1].astype(np.float64))
    return begin, end, Z, signal_ref.get_spec_and_angle(Z[None])[0], mag > 1e-3 * np.max(np.abs(Z))


@pytest.mark.parametrize("n_fft,hop,crop_len", ORACLE_CASES)
def test_oracle_angle_mask_keeps_at_least_half_of_the_cells(n_fft, hop, crop_len):
    """CPU: the angle comparison below is made where the standardised magnitude is not numerically zero; on detgen.make_clip inputs
    that is far more than half of the cells."""
    big = oracle_crop(n_fft, hop, crop_len)[4]
    assert big.mean() >= 0.5, big.mean()


@gpu
@pytest.mark.parametrize("n_fft,hop,crop_len", ORACLE_CASES)
def test_values_against_the_oracle(n_fft, hop, crop_len):
    buf, _ = source(crop_len)
    begin, end, Z, want, big = oracle_crop(n_fft, hop, crop_len)
    got = run(buf, begin, end, crop_len, n_fft, hop, 0, True, True).cpu().numpy()[0]
    assert got.shape == want.shape
    r = relmax(got[0], want[0])
    d = np.angle(np.exp(1j * (got[1].astype(np.float64) - want[1])))
    print(f"\n{n_fft}/{hop}: log-magnitude relmax {r:.3g}, angle max {np.max(np.abs(d[big])):.3g} rad over {big.mean():.3f} of the cells")
    assert big.mean() >= 0.5
    assert r < 2e-5
    assert np.max(np.abs(d[big])) < 2e-3
    raw = run(buf, begin, end, crop_len, n_fft, hop, 0, True, False).cpu().numpy()[0]          # the standardised [re; im] itself
    assert relmax(raw, Z) < 2e-5
