"""GPU: phasegen.data.AudioCropLoader (fresh crops of raw audio every epoch, one pg_stft_crops launch per batch),
preproc.dataset_stats (the data set's (mean, std) without materialising it) and training from them, in process and through
train.py --audio.

(The file name sorts behind every older test file, like the other test_z_* files: the older tests keep their place in the run.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from phasegen import detgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unet-phasegen_amd")
T_SLICE, N_FFT, HOP, N_RANDOM, BATCH = 184, 32, 8, 2, 4
STATS = (0.0123, 1.7)
KW = dict(t_slice=T_SLICE, n_fft=N_FFT, hop_length=HOP, n_random=N_RANDOM)


def tracks():
    """Three tracks, the second one (2, samples): 4 + 2 x 3 + 3 = 13 aligned chunks, 39 clips per epoch with two random crops each."""
    return [detgen.make_clip(700, seed=60), np.stack([detgen.make_clip(431, seed=61), detgen.make_clip(431, seed=62)]),
            detgen.make_clip(400, seed=63)]


def regions():
    """(samples,) of every channel region, in the order the loader packs them."""
    return [700, 431, 431, 400]


def compose(src, begin, end, stats=STATS):
    """The three-launch composition on the crops (begin, end) of the flat host buffer ``src``, gathered and zero-padded."""
    from phasegen import ops
    g = np.zeros((len(begin), T_SLICE), np.float32)
    for i, (b, e) in enumerate(zip(begin, end)):
        lim = min(max(int(e - b), 0), T_SLICE)
        g[i, :lim] = src[b:b + lim]
    x = ops.stft(torch.from_numpy(g).cuda(), N_FFT, HOP)
    ops.standardize_with_(x, stats[0], stats[1])
    return ops.polar(x)


def test_epochs_follow_the_table_bit_for_bit():
    from phasegen import preproc
    from phasegen.data import AudioCropLoader
    loader = AudioCropLoader(tracks(), BATCH, stats=STATS, seed=7, **KW)
    n = sum(preproc.n_chunks(a_len, T_SLICE, N_RANDOM) for a_len in regions())
    assert n == 39 and loader.num_clips() == n and len(loader) == (n + BATCH - 1) // BATCH == 10
    assert loader.dataset is loader and loader.batch_size == BATCH and loader.stats == STATS
    src = loader.src.cpu().numpy()
    assert src.shape == (sum(regions()),)
    bounds = np.concatenate([[0], np.cumsum(regions())])
    aligned = {int(bounds[r] + s) for r, a_len in enumerate(regions()) for s in range(0, a_len, T_SLICE)}
    tables = []
    for epoch in range(2):
        begin, end = loader.epoch_table(epoch)
        assert begin.dtype == end.dtype == np.int64 and len(begin) == len(end) == n
        tables.append(begin)
        # every crop lies in one region, ends at that region's end and starts where the reference's rule allows
        reg = np.searchsorted(bounds, begin, side="right") - 1
        assert np.array_equal(end, bounds[reg + 1])
        start = begin - bounds[reg]
        a_len = np.asarray(regions())[reg]
        assert np.all((start % T_SLICE == 0) | (start < a_len - T_SLICE // 1.3))
        assert aligned <= set(begin.tolist())                           # the aligned starts are there in every epoch
        want = compose(src, begin, end)
        rows = 0
        for i, (x, label) in enumerate(loader):
            b = min(BATCH, n - i * BATCH)
            assert tuple(x.shape) == (b, 2, N_FFT // 2, 1 + T_SLICE // HOP) and x.dtype == torch.float32 and x.is_cuda
            assert tuple(label.shape) == (b, 1) and label.dtype == torch.float32 and not bool(label.any())
            assert torch.equal(x, want[rows:rows + b]), (epoch, i)
            rows += b
        assert rows == n and i == len(loader) - 1
    assert sorted(tables[0].tolist()) != sorted(tables[1].tolist())     # fresh random starts in epoch 1
    it = loader.__iter__()
    first = it.__next__()                                               # the reference's loader.__iter__().__next__()
    assert torch.equal(first[0], compose(src, *[t[:BATCH] for t in loader.epoch_table(2)]))


def test_same_seed_same_epochs_and_ranks_share_the_table():
    from phasegen.data import AudioCropLoader
    a = AudioCropLoader(tracks(), BATCH, stats=STATS, seed=7, **KW)
    b = AudioCropLoader(tracks(), BATCH, stats=STATS, seed=7, **KW)
    c = AudioCropLoader(tracks(), BATCH, stats=STATS, seed=8, **KW)
    for epoch in range(2):
        for (xa, _), (xb, _) in zip(a, b):
            assert torch.equal(xa, xb)
        assert all(np.array_equal(u, v) for u, v in zip(a.epoch_table(epoch), b.epoch_table(epoch)))
    assert not np.array_equal(a.epoch_table(0)[0], c.epoch_table(0)[0])
    r0 = AudioCropLoader(tracks(), BATCH, stats=STATS, seed=7, rank=0, world=2, **KW)
    r1 = AudioCropLoader(tracks(), BATCH, stats=STATS, seed=7, rank=1, world=2, **KW)
    assert len(r0) == len(r1) == 4                                      # 39 clips: 4 whole global batches of 2 x 4
    full_b, full_e = a.epoch_table(0)                                   # one GPU: the whole shuffled table
    (b0, e0), (b1, e1) = r0.epoch_table(0), r1.epoch_table(0)
    assert len(b0) == len(b1) == 16
    assert np.array_equal(b0, full_b[0:32:2]) and np.array_equal(b1, full_b[1:32:2])            # dealt rank::world from a prefix
    assert np.array_equal(e0, full_e[0:32:2]) and np.array_equal(e1, full_e[1:32:2])
    batches = [x for x, _ in r1]
    assert len(batches) == 4 and all(x.shape[0] == BATCH for x in batches)
    assert torch.equal(torch.cat(batches), compose(r1.src.cpu().numpy(), b1, e1))
    with pytest.raises(ValueError):
        AudioCropLoader([detgen.make_clip(200, seed=1)], 16, stats=STATS, rank=0, world=2, **KW)._usable()


def test_dataset_stats_equal_the_materialised_set():
    """The same chunks either way: build_dataset wants tracks of one channel count, so the two channels go in as tracks of their own."""
    from phasegen import preproc
    from phasegen.data import AudioCropLoader
    t = tracks()
    mono = [t[0], t[1][0], t[1][1], t[2]]
    _, _, (mean, std) = preproc.build_dataset(mono, chunk_seconds=0.0115, rsr=16000, n_fft=N_FFT, hop_length=HOP, n_random=0,
                                              return_stats=True)
    assert int(0.0115 * 16000) == T_SLICE
    for block in (64, 5, 1):
        m, s = preproc.dataset_stats(t, T_SLICE, N_FFT, HOP, block=block)
        print(f"\nblock {block}: mean {m!r} (set {mean!r}, diff {abs(m - mean):.3g}), std {s!r} (set {std!r}, diff {abs(s - std):.3g})")
        assert abs(m - mean) <= 1e-10 * std and abs(s - std) <= 1e-10 * std
    loader = AudioCropLoader(t, BATCH, seed=0, **KW)                   # stats=None: computed from the tracks
    assert abs(loader.stats[0] - mean) <= 1e-10 * std and abs(loader.stats[1] - std) <= 1e-10 * std
    n, m, s = preproc.combine_moments([(3, 1.0, 0.0), (1, 5.0, 0.0)])  # {1, 1, 1, 5}
    assert (n, m) == (4, 2.0) and abs(s - np.sqrt(3.0)) < 1e-15


def test_training_on_the_loader_equals_training_on_the_materialised_batches():
    from phasegen.data import AudioCropLoader, SpectrogramLoader
    from phasegen.model import UNetModel
    from phasegen.trainer import Trainer
    C = N_FFT // 2
    loader = AudioCropLoader(tracks(), 2, stats=STATS, seed=3, **KW)
    begin, end = loader.epoch_table(0)
    data = compose(loader.src.cpu().numpy(), begin, end)
    ref_loader = SpectrogramLoader(data, torch.zeros(data.shape[0], 1, device=data.device), 2, shuffle=False)
    pn = detgen.make_params(C, seed=0)
    got, want = [], []
    for batches, losses in ((loader, got), (ref_loader, want)):
        trainer = Trainer(UNetModel(C, 2 * C).load_numpy(pn), lr=1e-3)
        for step, d in enumerate(batches):
            if step == 2:
                break
            assert tuple(d[0].shape) == (2, 2, C, 24)
            losses.append(trainer.step(d[0]).cpu().numpy().copy())
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g.shape == (3,) and np.all(np.isfinite(g))
        assert np.array_equal(g, w), (g, w)
    assert not np.array_equal(got[0], got[1])


def test_train_py_trains_from_wav_files(tmp_path):
    from scipy.io import wavfile
    rsr = 16000
    for name, n, seed in (("a.wav", 1500, 70), ("b.wav", 900, 71)):
        wavfile.write(str(tmp_path / name), rsr, np.round(detgen.make_clip(n, seed=seed) * 20000.0).astype(np.int16))
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--audio", "a.wav", "b.wav", "--channels", "16", "--n_fft", "32",
                        "--hop", "8", "--chunk", "0.0115", "--n_random", "2", "--batch_size", "2", "--max_steps", "2", "--val_every", "1000",
                        "--ckpt_every", "1000", "--log_dir", "run/"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Epoch 1 done," in r.stdout and "mag loss:" in r.stdout and "ang loss:" in r.stdout
    stats = np.load(tmp_path / "run" / "audio_stats.npy")
    assert stats.dtype == np.float64 and stats.shape == (2,) and np.isfinite(stats).all() and stats[1] > 0
