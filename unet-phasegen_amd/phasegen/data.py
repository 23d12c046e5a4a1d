"""Spectrogram batching of the reference's ``data.py`` (data.py:7-47), device resident.

``get_spec_and_angle`` runs the polar transform on the GPU (pg_polar).  ``get_fft_npy_loader`` keeps the reference's
signature and yield format -- ``[x, label]`` with x (b, 2, bins, frames) float32, label (b, 1) float32, shuffled
every epoch, short last batch kept -- but the whole dataset lives in HBM (288 GB per MI355X) after ONE upload, so a
training step does no host->device copy at all (the reference uploads the batch four times per step,
train.py:42,49,50,57; ``.cuda()`` on what this loader yields is a no-op, so the reference loop runs unchanged).
For data-parallel training rank r of W takes clips r::W of each epoch's permutation (same seed on every rank), after the
permutation has been cut to a whole number of GLOBAL batches (W x batch_size clips): every rank then yields the same number
of full batches per epoch, so the ranks issue the same number of gradient all-reduces (a rank that ran one step more than
its peers would pair its collectives with the next epoch's and hang or silently diverge).

``AudioCropLoader`` has the same surface and yield format but no spectrogram file behind it: it keeps the raw audio in HBM and computes
every batch -- the reference's aligned chunks and fresh random crops each epoch -- with one pg_stft_crops launch.
"""
import os

import numpy as np
import torch

from . import ops


def _device(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError("phasegen.data needs an MI355X (the polar transform and batching run on the device)")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def get_spec_and_angle(data, use_exp=True, device=None, as_numpy=True, chunk=256):
    """data.py:39-47.  ``data``: (N, 2, bins, frames) [re; im] (numpy, memmap or tensor) -> [log1p|z|; angle], float32."""
    dev = _device(device)
    if torch.is_tensor(data) and data.is_cuda:
        out = ops.polar(data.contiguous().float(), use_exp=use_exp)
        return out.cpu().numpy() if as_numpy else out
    n = data.shape[0]
    out = torch.empty(tuple(data.shape), device=dev, dtype=torch.float32)
    for s0 in range(0, n, chunk):                    # stream the (possibly memory-mapped) array through the device
        blk = torch.from_numpy(np.array(data[s0:s0 + chunk], dtype=np.float32)).to(dev)
        ops.polar(blk, out[s0:s0 + chunk], use_exp=use_exp)
    return out.cpu().numpy() if as_numpy else out


class SpectrogramLoader:
    """Iterable with torch DataLoader's surface as the reference uses it (``for i, d in enumerate(loader)``,
    ``loader.__iter__().__next__()``, ``len(loader)``, ``.dataset``, ``.batch_size``)."""

    def __init__(self, data, labels, batch_size, shuffle=True, rank=0, world=1, seed=None):
        self.data, self.labels = data, labels
        self.batch_size, self.shuffle = batch_size, shuffle
        self.rank, self.world = rank, world
        self.dataset = self
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(torch.initial_seed() if seed is None else seed)

    def _usable(self):
        """Clips of an epoch that are dealt out: all of them on one GPU (the short last batch is yielded and dropped by the
        caller, train.py:38-39); with W ranks a whole number of global batches, so that every rank steps equally often."""
        n = self.data.shape[0]
        if self.world == 1:
            return n
        g = self.world * self.batch_size
        if n < g:
            raise ValueError(f"data-parallel loader: {n} clips do not fill one global batch of {self.world} x {self.batch_size}")
        return n // g * g

    def __len__(self):
        n = len(range(self.rank, self._usable(), self.world))
        return (n + self.batch_size - 1) // self.batch_size

    def num_clips(self):
        return self.data.shape[0]

    def __iter__(self):
        n = self.data.shape[0]
        perm = torch.randperm(n, generator=self._gen) if self.shuffle else torch.arange(n)
        perm = perm[:self._usable()][self.rank::self.world].to(self.data.device)
        for s0 in range(0, perm.numel(), self.batch_size):
            idx = perm[s0:s0 + self.batch_size]
            yield [self.data.index_select(0, idx), self.labels.index_select(0, idx)]


def get_fft_npy_loader(paths, labels=None, batch_size=1, norm=True, precon=False, device=None, rank=0, world=1, seed=None):
    """data.py:7-28.  ``norm`` is accepted and ignored exactly as in the reference (it is never read there)."""
    dev = _device(device)
    if not isinstance(paths, list):
        paths = [paths]
    if labels is None:
        labels = [0]
    datas, targets = [], []
    for p, l in zip(paths, labels):                  # zip truncation is reference behaviour (train.py:18-20)
        if os.path.exists(p):                        # missing paths are silently skipped (data.py:17)
            print("{} exists, start loading ...".format(p))
            d = np.load(p, mmap_mode="r")
            if precon:
                d = get_spec_and_angle(d, device=dev, as_numpy=False)
            else:
                d = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
            datas.append(d)
            targets.append(torch.ones(d.shape[0], 1, device=dev) * l)
    assert len(datas) > 0, "datasets should not be an empty iterable"     # what ConcatDataset([]) raises (data.py:26)
    return SpectrogramLoader(torch.cat(datas) if len(datas) > 1 else datas[0],
                             torch.cat(targets) if len(targets) > 1 else targets[0], batch_size, True, rank, world, seed)


class AudioCropLoader:
    """Training batches straight from raw audio, fresh crops every epoch -- no spectrogram file (preproc_mdb.py:66-97,182 and
    data.py:39-47 in ONE launch per batch, pg_stft_crops).

    ``tracks``: mono arrays, (channels, samples) arrays or device tensors at the target rate.  They are packed once into one flat
    device buffer; every channel is a region of its own, and a crop that runs off the end of its region reads zeros (the
    reference's zero-padded tail), never the next region.  Each epoch the table ``preproc.chunk_starts`` would produce for every
    track -- each aligned start followed by its ``n_random`` crops in [0, a_len - t_slice // 1.3), every start taken for every
    channel of the track -- is built on the host from a numpy Generator seeded with (seed, epoch), shuffled, cut to whole global
    batches for ``world`` > 1 exactly as ``SpectrogramLoader`` does, dealt rank::world and uploaded ONCE; a step then makes no
    host-to-device copy.  Yields ``[x, label]`` as ``SpectrogramLoader``: x (b, 2, n_fft/2, frames) = [log1p|z|; angle] of the
    standardised STFT, label (b, 1) zeros; the short last batch is kept on one GPU.
    ``stats``: the data set's (mean, std) (``preproc.dataset_stats`` when None); ``.stats`` holds the pair.
    ``epoch_table(e)``: the (begin, end) index arrays of epoch e in yield order -- what reproducing a run needs."""

    def __init__(self, tracks, batch_size, t_slice=65024, n_fft=2048, hop_length=512, n_random=30, stats=None, rank=0, world=1,
                 seed=None, shuffle=True, device=None):
        from . import preproc
        dev = _device(device)
        self.batch_size, self.shuffle = int(batch_size), shuffle
        self.t_slice, self.n_fft, self.hop_length, self.n_random = int(t_slice), int(n_fft), int(hop_length), int(n_random)
        self.rank, self.world = rank, world
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.dataset = self
        chans = [preproc.as_channels(t, dev) for t in tracks]
        if not chans:
            raise ValueError("AudioCropLoader: no tracks")
        self.src = torch.cat([c.reshape(-1) for c in chans])
        self._tracks, o = [], 0                                          # (first sample of channel 0, channels, samples) per track
        for c in chans:
            self._tracks.append((o, int(c.shape[0]), int(c.shape[1])))
            o += c.numel()
        self._n = sum(n_ch * preproc.n_chunks(a_len, self.t_slice, self.n_random) for _, n_ch, a_len in self._tracks)
        if stats is None:
            stats = preproc.dataset_stats(chans, self.t_slice, self.n_fft, self.hop_length, device=dev)
        self.stats = (float(stats[0]), float(stats[1]))
        self._stats_dev = ops.stats_tensor(self.stats, dev)              # uploaded once
        self._labels = torch.zeros(self.batch_size, 1, device=dev)
        self._epoch = 0

    def num_clips(self):
        return self._n

    def _usable(self):
        """As SpectrogramLoader._usable: everything on one GPU, a whole number of global batches with W ranks."""
        if self.world == 1:
            return self._n
        g = self.world * self.batch_size
        if self._n < g:
            raise ValueError(f"data-parallel loader: {self._n} clips do not fill one global batch of {self.world} x {self.batch_size}")
        return self._n // g * g

    def __len__(self):
        n = len(range(self.rank, self._usable(), self.world))
        return (n + self.batch_size - 1) // self.batch_size

    def full_table(self, epoch):
        """(begin, end) int64 arrays of every crop of ``epoch`` before the cut to whole global batches and the deal to ranks
        (already shuffled): the same on every rank."""
        from . import preproc
        rng = np.random.default_rng((self.seed, int(epoch)))
        begin, end = [], []
        for o, n_ch, a_len in self._tracks:
            starts = np.asarray(preproc.chunk_starts(a_len, self.t_slice, self.n_random, rng), np.int64)
            base = o + a_len * np.arange(n_ch, dtype=np.int64)           # (chunk, channel) order, as preproc.chunk_audio
            begin.append((starts[:, None] + base[None, :]).reshape(-1))
            end.append(np.broadcast_to(base + a_len, (len(starts), n_ch)).reshape(-1))
        begin, end = np.concatenate(begin), np.concatenate(end)
        if self.shuffle:
            perm = rng.permutation(len(begin))
            begin, end = begin[perm], end[perm]
        return begin, end

    def epoch_table(self, epoch):
        """The (begin, end) arrays of THIS rank's crops of ``epoch`` in yield order: batch i is rows [i b, (i + 1) b)."""
        begin, end = self.full_table(epoch)
        sel = slice(self.rank, self._usable(), self.world)
        return np.ascontiguousarray(begin[sel]), np.ascontiguousarray(end[sel])

    def __iter__(self):
        begin, end = self.epoch_table(self._epoch)
        self._epoch += 1
        dev = self.src.device
        begin, end = torch.from_numpy(begin).to(dev), torch.from_numpy(end).to(dev)      # the epoch's only uploads
        for s0 in range(0, begin.numel(), self.batch_size):
            b, e = begin[s0:s0 + self.batch_size], end[s0:s0 + self.batch_size]
            x = ops.stft_crops(self.src, b, e, self.t_slice, self.n_fft, self.hop_length, polar=True, stats=self._stats_dev)
            yield [x, self._labels[:b.numel()]]
