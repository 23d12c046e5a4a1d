"""CPU: pg_stft_crops on the host side -- the ABI (version, struct size, exports), the argument checks made before any launch, and
the launch plan: the crops call reaches the crops instantiation of the SAME kernel family, with the same grid, block and LDS, as a
chunked pg_stft call of the same sizes, and pg_stft's own plans are what they were before the entry point existed."""
import ctypes

import pytest

ALIGNED = 4096                       # pointers are never dereferenced: describe launches nothing and bad calls fail before a launch
N_FFTS = (64, 512, 1024, 2048, 4096)
SIGNALS = 3

# pg_stft_describe of a chunked call, 3 signals of 6 n_fft samples at hop n_fft / 4 (25 frames), 256 compute units: the strings the
# library printed before pg_stft_crops was added, (n_fft, single_frame) -> plan
PG_STFT_PLANS = {
    (64, 0): "stft_frames_kernel<true>,grid=24,block=256,lds=2312",
    (64, 1): "stft_kernel,grid=75,block=256,lds=1280",
    (512, 0): "stft_frames_kernel<true>,grid=24,block=256,lds=18448",
    (512, 1): "stft_kernel,grid=75,block=256,lds=10240",
    (1024, 0): "stft_w_kernel<true, 8>,grid=16,block=512,lds=41472",
    (1024, 1): "stft_kernel,grid=75,block=256,lds=20480",
    (2048, 0): "stft_w_kernel<true, 16>,grid=16,block=512,lds=78336",
    (2048, 1): "stft_kernel,grid=75,block=256,lds=40960",
    (4096, 0): "stft_kernel,grid=75,block=256,lds=81920",
    (4096, 1): "stft_kernel,grid=75,block=256,lds=81920",
}
# kernel of a pg_stft plan -> the crops instantiation of its family
CROPS_KERNEL = {"stft_kernel": "stft_crops_kernel", "stft_frames_kernel<true>": "stft_crops_frames_kernel",
                "stft_w_kernel<true, 8>": "stft_crops_w_kernel<8>", "stft_w_kernel<true, 16>": "stft_crops_w_kernel<16>"}


def crops_args(n_fft=2048, single=0, signals=SIGNALS):
    from phasegen import _lib
    a = _lib.StftCropsArgs()
    a.n_signals, a.n_fft, a.hop, a.single_frame = signals, n_fft, n_fft // 4, single
    a.n_samples = 6 * n_fft
    a.n_frames = 1 + a.n_samples // a.hop
    a.src = a.out = a.crop_begin = a.crop_end = ALIGNED
    return a


def stft_args(n_fft, single):
    from phasegen import _lib
    a = _lib.StftArgs()
    a.n_signals, a.n_fft, a.hop, a.single_frame = SIGNALS, n_fft, n_fft // 4, single
    a.n_samples = 6 * n_fft
    a.n_frames = 1 + a.n_samples // a.hop
    a.y = a.out = a.chunk_start = ALIGNED
    a.src_len = a.src_stride = 10 * a.n_samples
    return a


def describe(fn, a):
    buf = ctypes.create_string_buffer(256)
    assert fn(ctypes.byref(a), buf, 256) == 0
    return buf.value.decode()


def test_abi_version_struct_size_and_exports():
    from phasegen import _lib
    lib = _lib.load()
    assert lib.pg_version() == 400                                    # a new entry point, not a new ABI
    assert ctypes.sizeof(_lib.StftCropsArgs) == 72                    # 8 int32 + 5 pointers: the header states the number
    assert _lib.StftCropsArgs.src.offset == 32 and _lib.StftCropsArgs.out.offset == 64
    assert ctypes.sizeof(_lib.StftArgs) == 80                         # pg_stft_args did not grow
    for name in ("pg_stft_crops", "pg_stft_crops_describe"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    from phasegen import ops
    assert callable(ops.stft_crops) and callable(ops.stft_crops_describe)


def test_argument_errors_are_reported_without_a_gpu():
    from phasegen import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    for call in (lambda a: lib.pg_stft_crops(ctypes.byref(a), None), lambda a: lib.pg_stft_crops_describe(ctypes.byref(a), buf, 256)):
        for field in ("src", "out", "crop_begin", "crop_end"):
            a = crops_args()
            setattr(a, field, None)
            assert call(a) == _lib.ERR_NULL, field
        a = crops_args()
        a.n_fft = 48
        assert call(a) == _lib.ERR_UNSUPPORTED
        assert b"power of two" in lib.pg_last_error_string()
        for off in (-1, 1):
            a = crops_args()
            a.n_frames += off
            assert call(a) == _lib.ERR_SHAPE, off
        a = crops_args()
        a.n_signals = 0
        assert call(a) == _lib.ERR_SHAPE
        a = crops_args()
        a.n_samples, a.n_frames = a.n_fft // 2, 1 + (a.n_fft // 2) // a.hop         # reflect padding needs n_samples > n_fft / 2
        assert call(a) == _lib.ERR_SHAPE
        a = crops_args()
        a.stats = ALIGNED + 4
        assert call(a) == _lib.ERR_ALIGN
        a = crops_args()
        a.out = ALIGNED + 2
        assert call(a) == _lib.ERR_ALIGN
    assert lib.pg_stft_crops_describe(ctypes.byref(crops_args()), buf, 64) == _lib.ERR_NULL     # buf of at least 128 bytes
    a = crops_args()
    a.stats = ALIGNED + 8                                             # stats are optional and 8-byte aligned: a valid plan
    assert lib.pg_stft_crops_describe(ctypes.byref(a), buf, 256) == 0


@pytest.mark.parametrize("single", (0, 1))
@pytest.mark.parametrize("n_fft", N_FFTS)
def test_crops_call_reaches_the_family_of_the_chunked_call(n_fft, single):
    from phasegen import _lib
    lib = _lib.load()
    want = describe(lib.pg_stft_describe, stft_args(n_fft, single))
    assert want == PG_STFT_PLANS[(n_fft, single)]                     # pg_stft's own plan: unchanged
    kernel, rest = want.split(",grid=")
    got = describe(lib.pg_stft_crops_describe, crops_args(n_fft, single))
    assert got == CROPS_KERNEL[kernel] + ",grid=" + rest              # same family, same grid, block and LDS
    for extra in ("polar", "stats"):                                  # neither the epilogue nor the statistics pick another kernel
        a = crops_args(n_fft, single)
        setattr(a, extra, 1 if extra == "polar" else ALIGNED)
        assert describe(lib.pg_stft_crops_describe, a) == got


def test_plain_stft_plans_are_unchanged():
    """The un-chunked pg_stft calls of tests/test_signal_families.py's spot values, as literals."""
    from phasegen import _lib
    lib = _lib.load()
    for (signals, frames, n_fft, hop, single), want in {
            (64, 256, 2048, 512, 0): "stft_w_kernel<false, 16>,grid=512,block=512,lds=78336",
            (64, 256, 1024, 256, 0): "stft_w_kernel<false, 8>,grid=768,block=512,lds=41472",
            (2, 79, 512, 128, 0): "stft_frames_kernel<false>,grid=40,block=256,lds=18448",
            (1, 5, 4096, 1024, 0): "stft_kernel,grid=5,block=256,lds=81920"}.items():
        a = _lib.StftArgs()
        a.n_signals, a.n_fft, a.hop, a.n_frames, a.single_frame = signals, n_fft, hop, frames, single
        a.n_samples = hop * (frames - 1)
        a.y = a.out = ALIGNED
        assert describe(lib.pg_stft_describe, a) == want
