"""CPU: which STFT / ISTFT kernels does a call reach, for every (n_fft, hop, frames, signals, chunked, single_frame, alignment)?

pg_stft_describe / pg_istft_describe are pure functions of the call's arguments (sizes, flags, pointer alignment) and of the CU count
(256 without a device, as on an MI355X), so the whole map is computed without a GPU -- as tests/test_kernel_families.py does for the
convolutions.  Every generation of signal kernels has inputs that only it serves, so all of them stay; this test pins which inputs
those are, the set of kernels that exist, and the workspace size callers cache buffers by.  DESIGN.md section 4.2 holds the table."""
import ctypes
import functools
import itertools

N_FFTS = (32, 64, 128, 256, 512, 1024, 2048, 4096)
FRAMES = (2, 7, 8, 9, 256)
SIGNALS = (1, 3, 64)
ALIGNED, UNALIGNED = 4096, 4100          # pointers are never dereferenced: describe launches nothing


def hops(n_fft):
    return (n_fft // 4, n_fft // 2, n_fft // 8, 50)


def stft_describe(n_fft, hop, frames, signals, chunked=0, single=0, ptr=ALIGNED, n_samples=None):
    from phasegen import _lib
    a = _lib.StftArgs()
    a.n_signals, a.n_fft, a.hop, a.n_frames, a.single_frame = signals, n_fft, hop, frames, single
    a.n_samples = hop * (frames - 1) if n_samples is None else n_samples
    a.y, a.out = ptr, ALIGNED
    if chunked:
        a.chunk_start, a.src_len, a.src_stride = ALIGNED, 10 * a.n_samples, 10 * a.n_samples
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().pg_stft_describe(ctypes.byref(a), buf, 256), "stft_describe")
    return buf.value.decode()


def istft_args(bins, hop, frames, signals, single=0, normalize=1, ptr=ALIGNED):
    from phasegen import _lib
    a = _lib.IstftArgs()
    a.n_signals, a.bins, a.n_frames, a.hop, a.mode, a.normalize, a.single_frame = signals, bins, frames, hop, 1, normalize, single
    a.a = a.b = a.workspace = ALIGNED
    a.a_bs = a.b_bs = bins * frames
    a.audio = ptr
    a.workspace_bytes = _lib.load().pg_workspace_bytes_istft(ctypes.byref(a))
    return a


def istft_describe(*args, **kw):
    from phasegen import _lib
    a = istft_args(*args, **kw)
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.load().pg_istft_describe(ctypes.byref(a), buf, 256), "istft_describe")
    return buf.value.decode(), a.workspace_bytes


def kernels(desc):
    return [entry.split(",grid=")[0] for entry in desc.split("|")]


def fields(entry):
    name, rest = entry.split(",grid=")
    grid, block, lds = rest.split(",")
    return name, grid, int(block.split("=")[1]), int(lds.split("=")[1])


@functools.lru_cache(None)
def sweep():
    """{(n_fft, hop, frames, signals, chunked, single, aligned): describe string} of every valid STFT call of the sweep, and
    {(n_fft, hop, frames, signals, single, normalize, aligned): (describe string, workspace bytes)} of every valid ISTFT call."""
    st, ist = {}, {}
    for n_fft in N_FFTS:
        for hop, frames, signals, single, ptr in itertools.product(hops(n_fft), FRAMES, SIGNALS, (0, 1), (ALIGNED, UNALIGNED)):
            if hop * (frames - 1) > n_fft // 2:                          # pg_stft: reflect padding needs n_samples > n_fft / 2
                for chunked in (0, 1):
                    st[(n_fft, hop, frames, signals, chunked, single, ptr == ALIGNED)] = stft_describe(n_fft, hop, frames, signals, chunked, single, ptr)
            if hop <= n_fft:                                             # pg_istft: hop <= n_fft
                for normalize in (0, 1):
                    ist[(n_fft, hop, frames, signals, single, normalize, ptr == ALIGNED)] = istft_describe(n_fft // 2, hop, frames, signals, single, normalize, ptr)
    return st, ist


def test_every_signal_kernel_is_reached_and_only_those_exist():
    st, ist = sweep()
    assert {k for d in st.values() for k in kernels(d)} == {
        "stft_kernel", "stft_frames_kernel<false>", "stft_frames_kernel<true>",
        "stft_w_kernel<false, 16>", "stft_w_kernel<true, 16>", "stft_w_kernel<false, 8>", "stft_w_kernel<true, 8>"}
    assert {k for d, _ in ist.values() for k in kernels(d)} == {
        "istft_frames_kernel", "istft_frames4_kernel", "istft_frames_w_kernel<16>", "istft_frames_w_kernel<8>", "istft_ola_w_kernel<16>",
        "istft_ola_w_kernel<8>", "istft_seam_kernel", "istft_ola4_kernel", "istft_peak_normalize_kernel"}
    # the table (pytest -s prints it; DESIGN.md section 4.2 holds a copy): kernel <- the values of each input over the calls that reach it
    rows = {}
    for (n_fft, hop, frames, signals, chunked, single, aligned), d in st.items():
        rows.setdefault(kernels(d)[0], []).append({"n_fft": n_fft, "single_frame": single, "chunked": chunked})
    for (n_fft, hop, frames, signals, single, normalize, aligned), (d, _) in ist.items():
        for k in kernels(d):
            rows.setdefault(k, []).append({"n_fft": n_fft, "single_frame": single, "hop*4==n_fft": int(hop * 4 == n_fft), "aligned": int(aligned),
                                           "frames": frames, "normalize": normalize})
    for k, calls in rows.items():
        print(f"{k:32s} " + "  ".join(f"{f} {{{','.join(map(str, sorted({c[f] for c in calls})))}}}" for f in calls[0]))


def test_selection_rules_hold_over_the_sweep():
    st, ist = sweep()
    for (n_fft, hop, frames, signals, chunked, single, aligned), d in st.items():
        (k,) = kernels(d)
        key = (n_fft, hop, frames, signals, chunked, single, aligned)
        assert k.startswith("stft_w_kernel<") == (n_fft in (1024, 2048) and not single), key
        assert (k == "stft_kernel") == (n_fft == 4096 or bool(single)), key
        if k != "stft_kernel":
            assert k.split("<")[1].startswith("true" if chunked else "false"), key
            assert k.startswith("stft_w_kernel<") or (k.startswith("stft_frames_kernel<") and n_fft <= 512), key
        if k.startswith("stft_w_kernel<"):
            assert k.endswith(", 16>" if n_fft == 2048 else ", 8>"), key
    for (n_fft, hop, frames, signals, single, normalize, aligned), (d, ws) in ist.items():
        ks = kernels(d)
        key = (n_fft, hop, frames, signals, single, normalize, aligned)
        wave = n_fft in (1024, 2048) and not single
        fused = wave and hop * 4 == n_fft and aligned
        assert ks[0].startswith(("istft_frames_w_kernel<", "istft_ola_w_kernel<")) == wave, key
        assert ks[0].startswith("istft_ola_w_kernel<") == fused, key
        assert (ks[0] == "istft_frames_kernel") == (n_fft == 4096 or bool(single)), key
        assert (ks[0] == "istft_frames4_kernel") == (n_fft <= 512 and not single), key
        if wave:
            assert ks[0].endswith("<16>" if n_fft == 2048 else "<8>"), key
        assert ("istft_seam_kernel" in ks) == (fused and frames > 8), key
        assert ("istft_ola4_kernel" in ks) == (not fused), key
        assert (ks[-1] == "istft_peak_normalize_kernel") == bool(normalize) and ks.count("istft_peak_normalize_kernel") == normalize, key
        assert len(ks) == 1 + (1 if not fused or frames > 8 else 0) + normalize, key
        # the workspace callers cache buffers by: [256 B][peaks per signal: the overlap-add's blocks or two per group of 8 frames, whichever is
        # more, padded to 256 B][frames] -- a function of the sizes alone (not of alignment, single_frame or normalize)
        per = max((hop * (frames - 1) + 1023) // 1024, 2 * ((frames + 7) // 8))
        assert ws == 256 + (signals * per * 4 + 255) // 256 * 256 + signals * frames * n_fft * 4, key


def test_spot_values_at_256_compute_units():
    # STFT: shape -> (kernel, grid, block, dynamic LDS bytes)
    for (signals, frames, n_fft, hop, single), want in {
            (64, 256, 2048, 512, 0): ("stft_w_kernel<false, 16>", "512", 512, 78336),
            (1, 128, 2048, 512, 0): ("stft_w_kernel<false, 16>", "16", 512, 78336),
            (64, 256, 1024, 256, 0): ("stft_w_kernel<false, 8>", "768", 512, 41472),
            (2, 79, 512, 128, 0): ("stft_frames_kernel<false>", "40", 256, 18448),
            (1, 5, 4096, 1024, 0): ("stft_kernel", "5", 256, 81920),
            (3, 128, 2048, 512, 1): ("stft_kernel", str(3 * 128), 256, 40960)}.items():
        assert fields(stft_describe(n_fft, hop, frames, signals, single=single)) == want, (signals, frames, n_fft, hop, single)
    d, ws = istft_describe(1024, 512, 256, 64)
    assert [fields(e) for e in d.split("|")] == [("istft_ola_w_kernel<16>", "512", 512, 78336), ("istft_seam_kernel", "31x64", 256, 0),
                                                 ("istft_peak_normalize_kernel", "128x64", 256, 0)] and ws == 134250752, (d, ws)
    d, ws = istft_describe(512, 256, 7, 2)
    assert [fields(e) for e in d.split("|")] == [("istft_ola_w_kernel<8>", "8", 512, 41472), ("istft_peak_normalize_kernel", "2x2", 256, 0)], d
    assert ws == 57856


def test_describe_makes_the_checks_of_the_call():
    from phasegen import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    a = istft_args(1024, 512, 256, 64)
    assert lib.pg_istft_describe(ctypes.byref(a), buf, 64) == _lib.ERR_NULL                  # buf of at least 128 bytes
    a.workspace_bytes -= 1
    assert lib.pg_istft_describe(ctypes.byref(a), buf, 256) == _lib.ERR_WORKSPACE
    a = istft_args(1024, 512, 256, 64)
    a.audio = None
    assert lib.pg_istft_describe(ctypes.byref(a), buf, 256) == _lib.ERR_NULL
    a = istft_args(1024, 512, 256, 65)
    assert lib.pg_istft_describe(ctypes.byref(a), buf, 256) == _lib.ERR_SHAPE
    s = _lib.StftArgs()
    s.n_signals, s.n_samples, s.n_fft, s.hop, s.n_frames, s.y, s.out = 1, 4096, 8192, 512, 9, ALIGNED, ALIGNED
    assert lib.pg_stft_describe(ctypes.byref(s), buf, 256) == _lib.ERR_UNSUPPORTED
    s.n_fft, s.n_frames = 2048, 8
    assert lib.pg_stft_describe(ctypes.byref(s), buf, 256) == _lib.ERR_SHAPE                 # n_frames != 1 + n_samples / hop
