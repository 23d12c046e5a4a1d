"""CPU: do the comparisons of tests/_signal_ref64.py have teeth?

(1) the float64 references agree with oracle/signal_ref.py within that oracle's own fp32 roundings and with a direct O(N^2) DFT;
(2) two honest fp32 transforms built differently (torch.fft on fp32 frames; a radix-2 Stockham in numpy float32 with tabulated fp32
    twiddles, the algorithm of fft_lds) pass both tiers on the inputs tests/test_z_signal_values_gpu.py uses;
(3) planted faults -- applied to the stand-in, never to library code -- are rejected, each by the tier named here, while the older
    criterion of tests/test_signal_gpu.py (2e-5 of the tensor maximum on detgen.make_clip) accepts the first three.

What Tier B can see is set by its scale: a fault d in one window coefficient moves every bin of a frame by d |x_n|, that is by
r = d |x_n| / (u ||x w||_2) = 64 / sqrt(3 n_fft / 8) at d = 2^-18 on white noise: 13 at n_fft 64, where the faults are planted, 4.6 at
512 and 2.3 at 2048, where the same fault hides inside the margin of 4 (the stand-in's own r_rms is about 2).  At 2048 the smallest
coefficient fault this comparison rejects is about 2^-15; the older criterion needed 2^-9 there."""
import numpy as np
import pytest

import _signal_ref64 as ref
from oracle import signal_ref
from phasegen import detgen

U = ref.U
stockham = ref.stockham_fft
stockham_inv = lambda x: ref.stockham_fft(x, -1.0)


def inputs(n_fft, hop, frames, signals=2, seed=11):
    n = hop * (frames - 1) + hop // 2
    return {"white": ref.white(seed, signals, n), "cosine": ref.on_bin_cosine(signals, n, n_fft, 5 if n_fft == 32 else 11)}


@pytest.mark.parametrize("n_fft,hop,frames", [(32, 8, 9), (64, 16, 12), (64, 50, 5), (512, 128, 9), (2048, 512, 9), (4096, 1024, 3)])
def test_references_agree_with_the_oracle_and_a_direct_dft(n_fft, hop, frames):
    for name, y in inputs(n_fft, hop, frames).items():
        X = ref.stft64(y, n_fft, hop)
        sc = ref.forward_scales(y, n_fft, hop)
        assert X.shape == (2, 2, n_fft // 2, 1 + y.shape[1] // hop) and X.dtype == np.float64
        assert np.array_equal(ref.stft64(y[0], n_fft, hop), X[0])
        assert np.array_equal(ref.frame_index(y.shape[1], n_fft, hop), signal_ref.frame_indices(y.shape[1], n_fft, hop))
        # the oracle rounds the window (u / 2 relative), the product (u / 2) and its complex64 output (u / 2 of |X| <= l1w per part)
        o = np.stack([signal_ref.chunk_and_stft(y[i], n_fft, hop) for i in range(2)])
        d = np.abs((o[:, 0] - X[:, 0]) + 1j * (o[:, 1] - X[:, 1]))
        assert np.all(d <= 2.0 * U * sc["l1w"][:, None, :]), (name, float((d / (U * sc["l1w"][:, None, :])).max()))
        if n_fft <= 64:
            fr = y.astype(np.float64)[:, ref.frame_index(y.shape[1], n_fft, hop)] * ref.hann64(n_fft)
            D = ref.dft_direct(fr)[:, :, 1:].transpose(0, 2, 1)
            assert np.max(np.abs(D - (X[:, 0] + 1j * X[:, 1]))) <= 1e-13 * sc["l1w"].max()
    # inverse: the oracle works in float64 and rounds its output once
    bins = n_fft // 2
    re, im = detgen.normal(21, (2, bins, frames)), detgen.normal(22, (2, bins, frames))
    y64, info = ref.istft64(re, im, hop)
    assert y64.shape == (2, hop * (frames - 1)) and info["wss"].shape == (hop * (frames - 1),)
    for i in range(2):
        S = np.concatenate([np.zeros((1, frames), np.complex64), (re[i] + 1j * im[i]).astype(np.complex64)], 0)
        assert np.all(np.abs(signal_ref.istft(S, hop) - y64[i]) <= U * np.abs(y64[i]) * (1 + 1e-6) + 1e-300)
    assert np.allclose(info["wss"], signal_ref.window_sumsquare(frames, n_fft, hop)[bins:-bins], rtol=1e-14)
    if n_fft <= 64:                                                     # irfft against the direct inverse sum
        X = np.zeros((2, frames, n_fft), np.complex128)
        X[:, :, 1:bins + 1] = (re + 1j * im).transpose(0, 2, 1)
        X[:, :, bins] = X[:, :, bins].real
        X[:, :, bins + 1:] = np.conj(X[:, :, bins - 1:0:-1])
        k = np.arange(n_fft)
        raw = (X @ np.exp(2j * np.pi * np.outer(k, k) / n_fft)).real / n_fft * ref.hann64(n_fft)
        acc = np.zeros((2, n_fft + hop * (frames - 1)))
        for t in range(frames):
            acc[:, t * hop:t * hop + n_fft] += raw[:, t]
        direct = acc[:, bins:-bins] / info["wss"]
        assert np.max(np.abs(direct - y64)) <= 1e-13 * np.abs(y64).max()


CASES = [(32, 8, 9), (64, 16, 12), (64, 50, 5), (128, 96, 6), (512, 128, 9), (1024, 256, 9), (2048, 512, 9), (4096, 1024, 3)]


@pytest.mark.parametrize("n_fft,hop,frames", CASES)
def test_two_honest_fp32_transforms_pass_both_tiers(n_fft, hop, frames):
    for single in (False, True):
        fam = ref.family_of(n_fft, single)
        for name, y in inputs(n_fft, hop, frames).items():
            X = ref.stft64(y, n_fft, hop)
            sc = ref.forward_scales(y, n_fft, hop)
            bound = ref.forward_bound(sc, fam, n_fft)
            base = ref.forward_errors(ref.standin_stft(y, n_fft, hop), X, sc, bound)
            other = ref.forward_errors(ref.standin_stft(y, n_fft, hop, fft=stockham), X, sc, bound)
            assert ref.accept(base, base) == (True, "") and ref.accept(other, base) == (True, ""), (fam, name, base, other)
        bins = n_fft // 2
        for mode in (1, 0):
            a = detgen.normal(23, (2, bins, frames))
            b = detgen.normal(24, (2, bins, frames))
            if mode == 0:
                a = np.abs(a)
            y64, info = ref.istft64(a, b, hop, mode)
            bound = ref.inverse_bound(y64, info, fam, n_fft)
            base = ref.inverse_errors(ref.standin_istft(a, b, hop, mode), y64, info, bound)
            other = ref.inverse_errors(ref.standin_istft(a, b, hop, mode, fft=stockham_inv), y64, info, bound)
            assert ref.accept(base, base) == (True, "") and ref.accept(other, base) == (True, ""), (fam, mode, base, other)


# ---------------------------------------------------------------------------------------------------------------------------------
N_FFT, HOP, FRAMES = 64, 16, 20                     # where the faults are planted (module docstring)
FRAME, TAP = 7, 29


def old_criterion_accepts(faulty):
    """tests/test_signal_gpu.py's check of a transform `faulty(y) -> (signals, 2, bins, frames)` on its own input."""
    y = np.stack([detgen.make_clip(HOP * (FRAMES - 1), seed=20 + i) for i in range(2)])
    want = np.stack([signal_ref.chunk_and_stft(y[i], N_FFT, HOP) for i in range(2)])
    return float(np.max(np.abs(faulty(y) - want)) / np.max(np.abs(want))) < 2e-5


def forward_verdict(faulty, kind="white"):
    y = inputs(N_FFT, HOP, FRAMES)[kind]
    X = ref.stft64(y, N_FFT, HOP)
    sc = ref.forward_scales(y, N_FFT, HOP)
    bound = ref.forward_bound(sc, "frames", N_FFT)
    base = ref.forward_errors(ref.standin_stft(y, N_FFT, HOP), X, sc, bound)
    return ref.accept(ref.forward_errors(faulty(y), X, sc, bound), base)


def middling_bin(S):
    """A bin of about half the frame's RMS level: 2^-16 of it is 128 u ||x w||_2, far above Tier B's threshold and inside Tier A."""
    mag = np.hypot(S[0, 0, :, FRAME], S[0, 1, :, FRAME])
    return int(np.argmin(np.abs(mag - 0.5 * np.sqrt(np.mean(mag * mag)))))


def scaled_bin(y):
    S = ref.standin_stft(y, N_FFT, HOP)
    S[0, :, middling_bin(S), FRAME] *= np.float32(1.0 + 2.0 ** -16)
    return S


def swapped_pair(y, k=5):
    S = ref.standin_stft(y, N_FFT, HOP)
    M = N_FFT // 2                                                       # rows k - 1 and M - k - 1 hold bins k and M - k
    S[0, :, [k - 1, M - k - 1], FRAME] = S[0, :, [M - k - 1, k - 1], FRAME]
    return S


def window_with(delta, tap=TAP):
    w = ref.window32(N_FFT).copy()
    w[tap] += np.float32(delta)
    return w


def symmetric_window():
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / (N_FFT - 1))).astype(np.float32)


def neighbour_twiddle(x, stage=5, entry=9):
    tw = ref.stockham_twiddles(N_FFT).copy()
    tw[entry] = tw[entry + 1]
    return ref.stockham_fft(x, twiddles={stage: tw})


FORWARD_FAULTS = {
    "one bin of one frame scaled by 1 + 2^-16": (scaled_bin, "B", True),
    "bins k and M - k of one frame exchanged": (swapped_pair, "AB", False),     # (see the note under the table)
    "one window coefficient off by 2^-18": (lambda y: ref.standin_stft(y, N_FFT, HOP, win32=window_with(2.0 ** -18)), "B", True),
    "symmetric instead of periodic Hann": (lambda y: ref.standin_stft(y, N_FFT, HOP, win32=symmetric_window()), "AB", False),
    "one twiddle replaced by its neighbour in one stage": (lambda y: ref.standin_stft(y, N_FFT, HOP, fft=neighbour_twiddle), "AB", False),
}


# The third field: does the older criterion accept the fault on detgen.make_clip?  It accepts the scaled bin and the window
# coefficient.  It does NOT accept an exchanged pair, at any n_fft: two noise bins of make_clip differ by about
# 0.1 sqrt(3 n_fft / 8) (0.5 here, 2.8 at 2048) while 2e-5 of the loudest bin is 1e-4 (3e-3 at 2048).  What the older criterion
# misses about a pair is a mix-up of 1e-3 of one bin into the other, which is the first fault over again.


@pytest.mark.parametrize("fault", list(FORWARD_FAULTS))
def test_planted_forward_faults_are_rejected(fault):
    faulty, tier, old_accepts = FORWARD_FAULTS[fault]
    ok, tiers = forward_verdict(faulty)
    print(f"\n{fault}: rejected by tier {tiers or '-'}")
    assert not ok and tiers == tier, (fault, tiers)
    if fault.startswith("bins k"):                                      # the two bins differ by more than the bound in that frame
        y = inputs(N_FFT, HOP, FRAMES)["white"]
        X = ref.stft64(y, N_FFT, HOP)
        b = ref.forward_bound(ref.forward_scales(y, N_FFT, HOP), "frames", N_FFT)[0, FRAME]
        assert abs((X[0, 0, 4, FRAME] - X[0, 0, 26, FRAME]) + 1j * (X[0, 1, 4, FRAME] - X[0, 1, 26, FRAME])) > 100 * b
    if fault.startswith("one window") or fault.startswith("symmetric"):  # the on-bin cosine sees the window faults too
        assert not forward_verdict(faulty, "cosine")[0]
    assert old_criterion_accepts(faulty) == old_accepts, fault           # the gap of the older criterion, kept on record


def test_a_coefficient_fault_at_2048_needs_2_to_the_minus_15():
    """The detectability scale of the module docstring, at the benchmark's transform length."""
    n_fft, hop = 2048, 512
    y = inputs(n_fft, hop, 9)["white"]
    X = ref.stft64(y, n_fft, hop)
    sc = ref.forward_scales(y, n_fft, hop)
    bound = ref.forward_bound(sc, "w16", n_fft)
    base = ref.forward_errors(ref.standin_stft(y, n_fft, hop), X, sc, bound)
    verdicts = {}
    for e in (-18, -14):
        w = ref.window32(n_fft).copy()
        w[n_fft // 2 + 3] += np.float32(2.0 ** e)
        verdicts[e] = ref.accept(ref.forward_errors(ref.standin_stft(y, n_fft, hop, win32=w), X, sc, bound), base)
    assert verdicts[-18] == (True, "") and verdicts[-14] == (False, "B"), verdicts


def inverse_verdict(faulty):
    bins = N_FFT // 2
    re, im = detgen.normal(25, (2, bins, FRAMES)), detgen.normal(26, (2, bins, FRAMES))
    y64, info = ref.istft64(re, im, HOP)
    bound = ref.inverse_bound(y64, info, "frames", N_FFT)
    raw = ref.standin_frames(re, im)
    base = ref.inverse_errors(ref.standin_ola(raw, HOP), y64, info, bound)
    return ref.accept(ref.inverse_errors(faulty(raw), y64, info, bound), base)


def seam_fault(raw, t=7):
    """Frame 7 (the last of the first group of eight) missing from the hop-long block behind the group boundary."""
    y = ref.standin_ola(raw, HOP).copy()
    w = ref.window32(N_FFT)
    wss = np.zeros(N_FFT + HOP * (FRAMES - 1), np.float32)
    for f in range(FRAMES):
        wss[f * HOP:f * HOP + N_FFT] += w * w
    pos = np.arange(8 * HOP, 9 * HOP)                                   # padded positions; taps pos - t hop of frame t
    y[:, pos - N_FFT // 2] -= (raw[:, t] * w)[:, pos - t * HOP] / wss[pos]
    return y


def interior_wss(wss):
    out = wss.copy()
    out[N_FFT // 2:N_FFT] = wss[N_FFT + 3 * HOP]                        # the first n_fft / 2 kept samples
    return out


INVERSE_FAULTS = {
    "a frame missing from one block at a group boundary": (seam_fault, "AB"),
    "interior window-sum-square at the first n_fft / 2 samples": (lambda raw: ref.standin_ola(raw, HOP, wss32=interior_wss), "AB"),
    "output shifted by one sample": (lambda raw: np.roll(ref.standin_ola(raw, HOP), 1, axis=1), "AB"),
}


@pytest.mark.parametrize("fault", list(INVERSE_FAULTS))
def test_planted_inverse_faults_are_rejected(fault):
    faulty, tier = INVERSE_FAULTS[fault]
    ok, tiers = inverse_verdict(faulty)
    print(f"\n{fault}: rejected by tier {tiers or '-'}")
    assert not ok and tiers == tier, (fault, tiers)


def test_white_noise_keeps_99_percent_of_the_angles():
    """Fused polar is checked where bound / |X| < 1; with the seeds of tests/test_z_signal_values_gpu.py the float64 reference alone
    leaves at most 1 % of the bins of every polar case out."""
    import test_z_signal_values_gpu as cases
    for case in cases.FORWARD_CASES:
        if not case.polar:
            continue
        case = cases.resolve(case)
        y = cases.forward_input(case, "white")
        X = ref.stft64(y, case.n_fft, case.hop)
        bound = ref.forward_bound(ref.forward_scales(y, case.n_fft, case.hop), ref.family_of(case.n_fft, case.single), case.n_fft)
        z = X[:, 0] + 1j * X[:, 1]
        with np.errstate(divide="ignore"):
            excluded = float(np.mean(~(bound[:, None, :] / np.abs(z) < 1.0)))
        assert excluded <= 0.01, (case, excluded)
