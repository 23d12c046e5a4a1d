"""Feature extraction of preproc_mdb.py on device: wav loading + rate change + chunking + STFT +
global normalisation + shuffled split, producing the on-disk format data.py consumes: (N, 2, n_fft/2, frames) float32
``{genre}_audio_{train,val}.npy``.  That file is no longer the only way to train: ``dataset_stats`` gives the normalisation of the
aligned-chunk set without materialising it, and ``phasegen.data.AudioCropLoader`` (``train.py --audio``) draws the same chunks and
fresh random crops from the raw audio every epoch.  MedleyDB walking and stem mixing (preproc_mdb.py:15-64) stay out of scope; so
do compressed audio formats and augmentations beyond the reference's random crops: the input is wav files (``load_audio``,
``get_mix_chunks``) or already-loaded arrays / device tensors, at the target rate or -- with ``osr`` -- at another one.

  load           preproc_mdb.py:112    the loading half of librosa.load: scipy's wav reader, integer PCM scaled to [-1, 1),
                 channels averaged to mono
  rate change    preproc_mdb.py:112-114 librosa.load(sr=osr) + librosa.resample(osr -> rsr): pg_resample, a Kaiser-windowed sinc
                 with resampy's published kaiser_best / kaiser_fast parameters (parity with resampy's table interpolation is
                 unpinned, include/phasegen.h), on the device
  chunk starts   preproc_mdb.py:66-82  one aligned chunk every t_slice samples plus n_random uniformly random crops in
                 [0, a_len - t_slice // 1.3) after each -- the random starts come from a numpy Generator you pass, so a
                 run is reproducible (the reference uses the global np.random state)
  chunk + STFT   preproc_mdb.py:84-97  zero-padded tail, librosa-convention STFT, DC dropped, [re; im]: ONE pg_stft launch
                 for all chunks of a track, reading the chunks in place (pg_stft_args.chunk_start / chunk_row: no gathered
                 or zero-padded copy of the audio) and writing straight into the dataset array
  normalise      preproc_mdb.py:182    (x - mean) / std over the WHOLE array (re and im together, population std):
                 pg_moments (double accumulators, two-pass) + pg_standardize in place
  split          preproc_mdb.py:174-184 shuffled indices, first n_val clips -> val, rest -> train
  statistics     preproc_mdb.py:182    ``dataset_stats``: the same (mean, std) from blocks of aligned chunks through one reusable
                 buffer (chunked pg_stft + pg_moments per block, combined on the host in float64)
"""
import os

import numpy as np
import torch

from . import ops


def chunk_starts(a_len, t_slice, n_random, rng):
    """Start offsets in the reference's order: aligned start, then its n_random random crops (preproc_mdb.py:73-80)."""
    bnd = a_len - t_slice // 1.3
    starts = []
    for i in range(0, a_len, t_slice):
        starts.append(i)
        for _ in range(n_random):
            starts.append(int(rng.integers(0, bnd)))
    return starts


def n_chunks(a_len, t_slice, n_random):
    """Chunks chunk_starts yields for a track of a_len samples (preproc_mdb.py:73-80)."""
    return len(range(0, a_len, t_slice)) * (1 + n_random)


def load_audio(path, mono=True):
    """The loading half of librosa.load (preproc_mdb.py:112) for wav files, through scipy.io.wavfile: int16 / 32768, int32 / 2^31,
    uint8 (v - 128) / 128, float as is; with ``mono`` the channels are averaged.  -> (float32 array (samples,) -- or
    (channels, samples) for multi-channel files with mono=False --, the file's own sample rate).  No rate change happens here."""
    from scipy.io import wavfile
    sr, d = wavfile.read(path)
    if d.dtype == np.int16:
        a = d.astype(np.float32) / np.float32(32768.0)
    elif d.dtype == np.int32:
        a = d.astype(np.float32) / np.float32(2147483648.0)
    elif d.dtype == np.uint8:
        a = (d.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    elif d.dtype.kind == "f":
        a = d.astype(np.float32)
    else:
        raise ValueError(f"load_audio: unsupported sample type {d.dtype} in {path}")
    if a.ndim == 2:
        a = a.mean(axis=1) if mono else np.ascontiguousarray(a.T)
    return a, int(sr)


def _device_of(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def resample(audio, orig_sr, target_sr, res_type="kaiser_best", device=None):
    """librosa.resample (preproc_mdb.py:114) on the device: host array or device tensor, (samples,) or (channels, samples) ->
    float32 device tensor at ``target_sr`` (ops.resample; equal rates pass through)."""
    if torch.is_tensor(audio):
        a = audio.to(audio.device if device is None and audio.is_cuda else _device_of(device), torch.float32)
    else:
        a = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(_device_of(device))
    return ops.resample(a, orig_sr, target_sr, res_type=res_type)


def chunk_audio(audio, t_slice, n_fft, hop_length, n_random, rng, device=None, out=None):
    """audio: mono float array (or (channels, samples)), on the host or a device tensor (used where it is: no host round
    trip).  -> (n_chunks, channels, 2, n_fft/2, frames) device tensor (``out``, when given, is that tensor: a slice of the
    dataset array)."""
    dev = _device_of(device)
    if torch.is_tensor(audio):
        ad = audio.to(dev, torch.float32)
        ad = (ad[None] if ad.dim() == 1 else ad).contiguous()
    else:
        a = np.asarray(audio, dtype=np.float32)
        if a.ndim == 1:
            a = a[None]
        ad = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_ch, a_len = ad.shape
    starts = chunk_starts(a_len, t_slice, n_random, rng)
    # signal order (chunk, channel): the layout of the dataset array, so the STFT writes it directly
    st = torch.tensor(np.repeat(np.asarray(starts, np.int64), n_ch), device=dev)
    rows = torch.tensor(np.tile(np.arange(n_ch, dtype=np.int32), len(starts)), device=dev)
    bins, frames = n_fft // 2, 1 + t_slice // hop_length
    if out is None:
        out = torch.empty(len(starts), n_ch, 2, bins, frames, device=dev)
    ops.stft(ad, n_fft, hop_length, out=out.view(len(starts) * n_ch, 2, bins, frames), chunk_start=st, chunk_row=rows,
             chunk_len=t_slice)
    return out


def get_mix_chunks(fn, t_slice, n_fft, hop_length, n_random, rsr, osr=44100, rng=None, device=None):
    """preproc_mdb.py:105-116: ``fn`` is a wav path or a tuple of paths (the stems / mixes of one track).  Each file is loaded as
    mono (librosa.load(f, sr=osr): resampled to ``osr`` when its own rate differs), resampled from ``osr`` to ``rsr``, the
    signals are trimmed to the shortest (chunk_audio, preproc_mdb.py:68-69), stacked and chunked.  -> chunk_audio's tensor."""
    if not isinstance(fn, tuple):
        fn = (fn,)
    dev = _device_of(device)
    mix = []
    for f in fn:
        m, sr = load_audio(f, mono=True)
        m = resample(m, sr, osr, device=dev)
        mix.append(resample(m, osr, rsr, device=dev))
    a_len = min(m.shape[-1] for m in mix)
    audio = torch.stack([m[:a_len] for m in mix])
    return chunk_audio(audio, t_slice, n_fft, hop_length, n_random, np.random.default_rng() if rng is None else rng, dev)


def as_channels(audio, device=None):
    """A track as a dense (channels, samples) float32 device tensor: mono arrays gain the channel axis; device tensors stay where
    they are."""
    if torch.is_tensor(audio):
        ad = audio.to(audio.device if device is None and audio.is_cuda else _device_of(device), torch.float32)
    else:
        ad = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(_device_of(device))
    if ad.dim() == 1:
        ad = ad[None]
    if ad.dim() != 2:
        raise ValueError(f"a track is (samples,) or (channels, samples), got {tuple(ad.shape)}")
    return ad.contiguous()


def combine_moments(parts):
    """(n, mean, population std) of the union of disjoint blocks given as (n, mean, std) triples, in float64: the pairwise update of
    Chan, Golub and LeVeque on (n, mean, M2 = n std^2)."""
    n, mean, m2 = 0, 0.0, 0.0
    for nb, mb, sb in parts:
        nb, mb, sb = int(nb), float(mb), float(sb)
        if nb == 0:
            continue
        tot = n + nb
        d = mb - mean
        m2 = m2 + nb * sb * sb + d * d * (n * nb / tot)
        mean = mean + d * (nb / tot)
        n = tot
    if n == 0:
        raise ValueError("combine_moments: no samples")
    return n, mean, float(np.sqrt(m2 / n))


def dataset_stats(tracks, t_slice, n_fft, hop_length, device=None, block=64):
    """The (mean, std) ``build_dataset(..., n_random=0, return_stats=True)`` computes -- over [re; im] of the aligned chunks of every
    track (every channel), population std -- without materialising the set: ``block`` chunks at a time go through one chunked STFT
    into one reusable buffer and pg_moments; the per-block (n, mean, std) are combined on the host in float64
    (``combine_moments``) after ONE read-back.  tracks: mono arrays, (channels, samples) arrays or device tensors at the target rate."""
    dev = _device_of(device)
    bins, frames = n_fft // 2, 1 + t_slice // hop_length
    block = max(1, int(block))
    buf = torch.empty(block, 2, bins, frames, device=dev)
    plan = []                                                            # (track tensor, starts, rows) per block
    for t in tracks:
        ad = as_channels(t, dev)
        n_ch, a_len = ad.shape
        starts = np.repeat(np.arange(0, a_len, t_slice, dtype=np.int64), n_ch)          # (chunk, channel) order, as chunk_audio
        rows = np.tile(np.arange(n_ch, dtype=np.int32), len(starts) // n_ch)
        for s0 in range(0, len(starts), block):
            plan.append((ad, starts[s0:s0 + block], rows[s0:s0 + block]))
    if not plan:
        raise ValueError("dataset_stats: no tracks")
    res = torch.empty(len(plan), 2, dtype=torch.float64, device=dev)
    counts = []
    for i, (ad, st, rw) in enumerate(plan):
        k = len(st)
        ops.stft(ad, n_fft, hop_length, out=buf[:k], chunk_start=torch.from_numpy(st).to(dev), chunk_row=torch.from_numpy(rw).to(dev),
                 chunk_len=t_slice)
        ops.moments(buf[:k], res[i])
        counts.append(k * 2 * bins * frames)
    res = res.cpu().numpy()
    _, mean, std = combine_moments((n, m, s) for n, (m, s) in zip(counts, res))
    return mean, std


def build_dataset(tracks, chunk_seconds=4.064, rsr=16000, n_fft=2048, hop_length=512, n_random=0, n_val=40, seed=0,
                  out_dir=None, genre="Pop", device=None, osr=None, return_stats=False):
    """tracks: list of mono float arrays (or device tensors) at ``rsr`` -- or at ``osr`` when that is given: every track is then
    resampled to ``rsr`` on the device first.  Returns (train, val) float32 numpy arrays; also writes
    ``{out_dir}/{genre}_audio_{train,val}.npy`` when ``out_dir`` is given (preproc_mdb.py:195-196).
    ``return_stats=True``: returns (train, val, (mean, std)) -- the two Python floats of the normalisation, which the reference
    computes and throws away and which new audio needs to be normalised like the training set (phasegen.track) -- and also writes
    them, two float64 values, to ``{out_dir}/{genre}_audio_stats.npy``."""
    rng = np.random.default_rng(seed)
    t_slice = int(chunk_seconds * rsr)
    dev = _device_of(device)
    if osr is not None and osr != rsr:
        tracks = [resample(t, osr, rsr, device=dev) for t in tracks]
    shaped = [(int(np.prod(np.shape(t)[:-1], dtype=np.int64)), np.shape(t)[-1]) for t in tracks]     # (channels, samples) per track
    n_ch = shaped[0][0]
    counts = [n_chunks(a_len, t_slice, n_random) for _, a_len in shaped]
    x = torch.empty(sum(counts), n_ch, 2, n_fft // 2, 1 + t_slice // hop_length, device=dev)    # (N, channels, 2, bins, frames)
    o = 0
    for t, c in zip(tracks, counts):
        chunk_audio(t, t_slice, n_fft, hop_length, n_random, rng, dev, out=x[o:o + c])
        o += c
    if x.shape[1] == 1:
        x = x[:, 0]                                                      # np.squeeze(axis=1), preproc_mdb.py:179-180
    stats = ops.standardize_(x)                                          # numpy .std() is the population std
    x = x.cpu().numpy()
    idx = np.linspace(0, len(x) - 1, len(x), dtype=int)
    rng.shuffle(idx)
    val, train = x[idx][:n_val], x[idx][n_val:]
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, f"{genre}_audio_val.npy"), val)
        np.save(os.path.join(out_dir, f"{genre}_audio_train.npy"), train)
    if return_stats:
        mean, std = (float(v) for v in stats.cpu().numpy())
        if out_dir is not None:
            np.save(os.path.join(out_dir, f"{genre}_audio_stats.npy"), np.array([mean, std], np.float64))
        return train, val, (mean, std)
    return train, val
