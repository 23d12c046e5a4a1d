"""Thin host-side wrappers: torch (ROCm) tensors in, one libphasegen C-ABI call out.

PyTorch is plumbing here (device memory + the current HIP stream); every op below is a hand-written gfx950
kernel behind ``include/phasegen.h``.  Activation tensors are (B, channels, frames) views whose frame stride is 1
and channel stride is ``frames``; the batch stride is free, so the two halves of a U-Net concat buffer are passed
as plain slices ``buf[:, :n]`` / ``buf[:, n:]`` without a copy.
"""
import contextlib
import ctypes as C
import functools
import inspect
import threading

import torch

from . import _lib
from ._lib import ACT_LEAKY, ACT_NONE, ACT_RELU, SCHED_CONTENDED, SCHED_SLOTS, SCHED_TILE_PER_WG  # noqa: F401  (re-exported)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_current_device(t, name):
    """Kernels are launched on the CURRENT device's current stream: a tensor that lives on another GPU would make the
    kernel dereference foreign pointers (a GPU memory fault that aborts the process) -- raise instead."""
    if t.device.index != torch.cuda.current_device():
        raise ValueError(f"{name}: tensor is on {t.device} but the current device is cuda:{torch.cuda.current_device()} "
                         "(wrap the call in torch.cuda.device(...))")


class KernelTimer:
    """HIP-event timing of labelled launches on the stream they are launched on (bench.py's roofline leg), plus each
    label's launch plan (pg_conv_describe: the kernel symbol rocprofv3 will report for it)."""

    def __init__(self):
        self.records = {}
        self.plans = {}
        self.bytes = {}          # label -> algorithmic HBM bytes of ONE launch (the HBM-bound kernels: BatchNorm, loss, Adam)

    def summary(self):
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.records.items()}


_timer = None
_cur_label = None


def set_timer(t):
    global _timer
    _timer = t


def _describe(fn, a, what, *op):
    buf = C.create_string_buffer(256)
    _lib.check(fn(C.byref(a), *op, buf, 256), what)
    return buf.value.decode()


def conv_describe(a, op):
    """pg_conv_describe: 'kernel<...>|grid=G|tiles=T|slabs=S|split=0/1|whole=W|fixup=none/plain/wide' for a filled ConvArgs (nothing is launched)."""
    return _describe(_lib.load().pg_conv_describe, a, "conv_describe", op)


def _note_plan(a, op):
    if _timer is not None and _cur_label is not None and _cur_label not in _timer.plans:
        _timer.plans[_cur_label] = conv_describe(a, op)


class timed:
    """``with ops.timed(label[, nbytes])``: one HIP-event pair around the launches inside, on the stream they go to (only while a
    KernelTimer is installed; otherwise free).  ``nbytes``: algorithmic HBM bytes of the launch, for the HBM-side rooflines."""

    def __init__(self, label, nbytes=None):
        self.label = label
        self.nbytes = nbytes

    def __enter__(self):
        global _cur_label
        if _timer is not None:
            _cur_label = self.label
            if self.nbytes is not None:
                _timer.bytes[self.label] = self.nbytes
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        global _cur_label
        if _timer is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _timer.records.setdefault(self.label, []).append((self.a, b))
            _cur_label = None


def _act3(t, name):
    """(ptr, batch_stride) of a (B, C, L) fp32 device view with L-contiguous channels."""
    if t is None:
        return None, 0
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
        raise ValueError(f"{name}: expected a 3-D float32 device tensor, got {tuple(t.shape)} {t.dtype} {t.device}")
    _on_current_device(t, name)
    B, Cc, L = t.shape
    if t.stride(2) != 1 or (Cc > 1 and t.stride(1) != L):
        raise ValueError(f"{name}: frames must be contiguous and channel stride == frames (strides {t.stride()})")
    return t.data_ptr(), (t.stride(0) if B > 1 else Cc * L)


def _dense(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous float32 device tensor")
    _on_current_device(t, name)
    return t.data_ptr()


def _dense_as(t, dtype, name):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous {dtype} device tensor")
    _on_current_device(t, name)
    return t.data_ptr()


def conv_out_len(Lin, k, s, p):
    return (Lin + 2 * p - k) // s + 1


def convt_out_len(Lin, k, s, p):
    return (Lin - 1) * s - 2 * p + k


class _StreamCache:
    """Scratch buffers keyed by (device, stream handle), bounded: at most ``cap`` streams per cache, least recently used evicted.
    A buffer is allocated while its stream is the CURRENT one, so torch's caching allocator ties the block to that stream: an
    evicted (or released) buffer goes back to that stream's pool, and whoever reuses the block is ordered after the stream's
    pending work -- also when a stream handle is recycled after the evicted entry's stream died."""

    def __init__(self, cap=4):
        self.cap = cap
        self.d = {}

    def get(self, device, nbytes_fn, at_least=0):
        device = torch.device(device)
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        buf = self.d.pop(key, None)                     # re-inserted below: dicts keep insertion order -> LRU
        if buf is None or buf.numel() < at_least:
            buf = torch.empty(max(nbytes_fn(), at_least), device=device, dtype=torch.uint8)
        self.d[key] = buf
        while len(self.d) > self.cap:
            self.d.pop(next(iter(self.d)))
        return buf

    def clear(self):
        self.d.clear()


_conv_ws = _StreamCache()
_caches = [_conv_ws]


def _workspace(cache, device, need, what):
    """(ptr, nbytes) of this stream's buffer in ``cache``, at least ``need`` bytes -- the answer of a pg_workspace_bytes_* query,
    where a negative value is an error code (raised as ``what``)."""
    if need < 0:
        _lib.check(int(need), what)
    ws = cache.get(device, lambda: need, need)
    return ws.data_ptr(), ws.numel()


def conv_workspace(device):
    """Scratch for the conv kernels' stream-K schedule (pg_workspace_bytes_conv(), 512 MiB; a wgrad grows it by its packed operands,
    pg_workspace_bytes_wgrad()), one per (device, STREAM):
    launches on one stream are ordered and may share it, launches on different streams may overlap and must not.  At most four
    streams per device hold one at a time (least recently used is dropped); ``release_workspaces()`` drops them all."""
    return _conv_ws.get(device, _lib.load().pg_workspace_bytes_conv)


def release_workspaces():
    """Drop every cached scratch buffer (conv stream-K, loss, ISTFT, overlap-add, moments, stitch, compare): they are re-created on demand."""
    for c in _caches:
        c.clear()


# ---- per-call knobs ---------------------------------------------------------------------------------------------
# The C ABI keeps no state: MFMA operand precision and work-split schedule are fields of pg_conv_args, the FFT schedule
# a field of pg_stft_args / pg_istft_args.  Every op below takes them as keyword arguments; when omitted, the calling
# THREAD's defaults apply (a fresh thread starts at fp32 / automatic), so two threads can drive two streams in different
# precisions.  The engine passes its own precision explicitly.
_PRECISIONS = {"fp32": 0, "f32": 0, "bf16": 1, "bf16x3": 2, 0: 0, 1: 1, 2: 2}


class _Defaults(threading.local):
    precision = 0
    schedule = 0
    stft_single = 0


_tls = _Defaults()


def precision_code(mode):
    if mode not in _PRECISIONS:
        raise ValueError(f"conv precision {mode!r}: expected fp32 / bf16 / bf16x3 (or 0 / 1 / 2)")
    return _PRECISIONS[mode]


def set_conv_precision(mode):
    """This thread's default MFMA operand mode.  0 / "fp32": fp32 operands (the parity path).  1 / "bf16": operands rounded
    to bf16 at fragment load, fp32 accumulate, fp32 tensors and master weights (BASELINE config 5).  2 / "bf16x3": split."""
    _tls.precision = precision_code(mode)


def current_schedule():
    """This thread's default pg_conv_args.schedule word."""
    return _tls.schedule


def set_conv_schedule(mode):
    """This thread's default schedule bits (test hook).  Bits 0-1: 0 automatic, 1 one tile per workgroup, 2 force the stream-K
    split; bit 2 (value 4): im2col kernels instead of the raw-window ones; bit 3 (value 8): never the tall 256 x 128 raw tile;
    bit 7 (value 128): the wgrad keeps the flat-K raw kernel where it would take the per-sample-slab one; bit 13 (value 0x2000):
    never the one-wave-per-SIMD fp32 kernels (conv_raw3.hip), i.e. the two-waves-per-SIMD raw kernels everywhere; bit 14 (0x4000):
    those kernels wherever they cover the problem, also where the automatic choice keeps the older ones (F form of k = 32); bits 15-16:
    their tile order (1 << 15: row-major, 2 << 15 / 3 << 15: super-rows of 2 / 4 tile rows); bit 17 (0x20000): never split the columns past the
    last full 256-wide tile off into a tail launch, bit 18 (0x40000): always, where the geometry allows (the automatic choice prices it);
    bits 19-23 (``SCHED_SLOTS(n)``): plan as if the device had n = 1..31 compute units, so that a small problem takes the work splits of
    a full-size layer (several whole tiles per workgroup, whole tiles between two partial ones, the hybrid split)."""
    if mode < 0 or (mode & ~0xffe0ff) or (mode & 0x60000) == 0x60000 or (mode & 3) == 3 or (mode & 0x70) or (mode & 0x6000) == 0x6000:
        raise ValueError("conv schedule: bad mode")
    _tls.schedule = (_tls.schedule & 0xf00) | mode


def set_conv_oversubscribe(factor):
    """Stream-K grid = factor x resident workgroup slots (1..8).  Use > 1 when other kernels (RCCL collectives) share the chip."""
    if not 1 <= factor <= 8:
        raise ValueError("conv oversubscribe: factor must be 1..8")
    _tls.schedule = (_tls.schedule & ~0xf00) | (factor << 8)


def set_stft_mode(single_frame):
    """0: 4 frames per workgroup through the half-length radix-4 real FFT (default); 1: one frame per workgroup, radix-2."""
    _tls.stft_single = int(bool(single_frame))


@contextlib.contextmanager
def conv_options(precision=None, schedule=None):
    """Scoped thread defaults: ``with ops.conv_options(precision="bf16"): ...``."""
    old = (_tls.precision, _tls.schedule)
    if precision is not None:
        _tls.precision = precision_code(precision)
    if schedule is not None:
        _tls.schedule = schedule
    try:
        yield
    finally:
        _tls.precision, _tls.schedule = old


def _conv_args(transposed, B, Cin, Cout, Lin, k, s, p, device=None, precision=None, schedule=None):
    a = _lib.ConvArgs()
    a.precision = _tls.precision if precision is None else precision_code(precision)
    a.schedule = _tls.schedule if schedule is None else schedule
    a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad = B, Cin, Cout, Lin, k, s, p
    a.Lout = convt_out_len(Lin, k, s, p) if transposed else conv_out_len(Lin, k, s, p)
    if device is not None:
        ws = conv_workspace(device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    return a


def _geom(transposed, w_shape):
    """(Cin, Cout, k) from a weight's shape: Conv1d weights are (Cout, Cin, k), ConvTranspose1d weights (Cin, Cout, k)."""
    a, b, k = w_shape
    return (a, b, k) if transposed else (b, a, k)


def conv_fwd(x, w, y, stride, pad, x_act=ACT_NONE, transposed=False, y_act=ACT_NONE, y2=None, y2_act=ACT_NONE,
             precision=None, schedule=None):
    """y = y_act(conv(x_act(x), w)) (nn.Conv1d, model.py:77) or conv_transpose (model.py:88) -- writes into ``y``;
    optionally a second copy ``y2 = y2_act(conv(...))`` (pre-activated tensors for the consumers)."""
    Cin, Cout, k = _geom(transposed, w.shape)
    B, _, Lin = x.shape
    a = _conv_args(transposed, B, Cin, Cout, Lin, k, stride, pad, x.device, precision, schedule)
    if tuple(x.shape) != (B, Cin, Lin) or tuple(y.shape) != (B, Cout, a.Lout):
        raise ValueError(f"conv_fwd: shapes x{tuple(x.shape)} w{tuple(w.shape)} y{tuple(y.shape)} inconsistent (Lout {a.Lout})")
    a.x, a.x_bs = _act3(x, "x")
    a.y, a.y_bs = _act3(y, "y")
    a.w = _dense(w, "w")
    a.x_act, a.y_act, a.y2_act = x_act, y_act, y2_act
    if y2 is not None:
        if y2.shape != y.shape:
            raise ValueError("conv_fwd: y2 must have y's shape")
        a.y2, a.y2_bs = _act3(y2, "y2")
    lib = _lib.load()
    _note_plan(a, _lib.OP_CONVT1D_FWD if transposed else _lib.OP_CONV1D_FWD)
    fn = lib.pg_convt1d_fwd if transposed else lib.pg_conv1d_fwd
    _lib.check(fn(C.byref(a), _stream()), "convt1d_fwd" if transposed else "conv1d_fwd")
    return y


def conv_dgrad(dy, w, dx, stride, pad, transposed=False, add=None, ref=None, mask=ACT_NONE, precision=None, schedule=None):
    """dx = dgrad(dy, w) [+ add] [* act'(ref)] -- grad wrt the tensor the forward op read."""
    Cin, Cout, k = _geom(transposed, w.shape)
    B, _, Lin = dx.shape
    a = _conv_args(transposed, B, Cin, Cout, Lin, k, stride, pad, dx.device, precision, schedule)
    if tuple(dy.shape) != (B, Cout, a.Lout) or tuple(dx.shape) != (B, Cin, Lin):
        raise ValueError(f"conv_dgrad: shapes dy{tuple(dy.shape)} w{tuple(w.shape)} dx{tuple(dx.shape)} inconsistent")
    a.dy, a.dy_bs = _act3(dy, "dy")
    a.dx, a.dx_bs = _act3(dx, "dx")
    a.w = _dense(w, "w")
    if add is not None:
        if add.shape != dx.shape:
            raise ValueError("conv_dgrad: add must have dx's shape")
        a.dx_add, a.dx_add_bs = _act3(add, "add")
    if ref is not None:
        if ref.shape != dx.shape:
            raise ValueError("conv_dgrad: ref must have dx's shape")
        a.dx_ref, a.dx_ref_bs = _act3(ref, "ref")
        a.dx_mask = mask
    lib = _lib.load()
    _note_plan(a, _lib.OP_CONVT1D_DGRAD if transposed else _lib.OP_CONV1D_DGRAD)
    fn = lib.pg_convt1d_dgrad if transposed else lib.pg_conv1d_dgrad
    _lib.check(fn(C.byref(a), _stream()), "dgrad")
    return dx


def adam_args(p, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """pg_adam_args for ``conv_wgrad(..., adam=)``: the weight ``p`` and its exp_avg / exp_avg_sq, all shaped like dw."""
    a = _lib.AdamArgs()
    a.n = p.numel()
    a.p, a.m, a.v = _dense(p, "p"), _dense(m, "m"), _dense(v, "v")
    a.lr, a.beta1, a.beta2, a.eps, a.grad_scale, a.step = lr, beta1, beta2, eps, grad_scale, step
    return a


def conv_wgrad(x, dy, dw, stride, pad, x_act=ACT_NONE, transposed=False, precision=None, schedule=None, adam=None):
    """dw = wgrad(act(x), dy), overwriting ``dw`` (same layout as the weight).  ``adam`` (from ``adam_args``): the Adam update
    of this weight runs in the kernel's epilogue from the gradient it stores -- bit-identical to ``adam_step`` afterwards; the
    caller must have enqueued every reader of the old weight (the layer's dgrad) before this call."""
    Cin, Cout, k = _geom(transposed, dw.shape)
    B, _, Lin = x.shape
    a = _conv_args(transposed, B, Cin, Cout, Lin, k, stride, pad, x.device, precision, schedule)
    if tuple(x.shape) != (B, Cin, Lin) or tuple(dy.shape) != (B, Cout, a.Lout):
        raise ValueError(f"conv_wgrad: shapes x{tuple(x.shape)} dy{tuple(dy.shape)} dw{tuple(dw.shape)} inconsistent")
    a.x, a.x_bs = _act3(x, "x")
    a.dy, a.dy_bs = _act3(dy, "dy")
    a.dw = _dense(dw, "dw")
    a.x_act = x_act
    if adam is not None:
        if adam.n != dw.numel():
            raise ValueError("conv_wgrad: fused adam tensors must have dw's shape")
        a.adam = C.addressof(adam)
    lib = _lib.load()
    op = _lib.OP_CONVT1D_WGRAD if transposed else _lib.OP_CONV1D_WGRAD
    # the fp32 kernels pack their operands into the workspace behind the stream-K region: grow this stream's buffer to what the call
    # needs (the largest layer's size sticks after the first step)
    need = lib.pg_workspace_bytes_wgrad(C.byref(a), op)
    if need > a.workspace_bytes:
        ws = _conv_ws.get(x.device, lib.pg_workspace_bytes_conv, at_least=need)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _note_plan(a, op)
    fn = lib.pg_convt1d_wgrad if transposed else lib.pg_conv1d_wgrad
    _lib.check(fn(C.byref(a), _stream()), "wgrad")
    return dw


# ---- bf16-resident forward path (BASELINE configs[4]; csrc/conv_h3.hip) ----------------------------------------------------
H_HEAD = 32      # PG_H_HEAD: zero elements the bf16-resident kernels may read in front of a tensor's first row
H_TAIL = 40      # zero tail of every row that covers each layer of the U-Net (pg_conv_fwd_h_supported checks a layer's need)


def h_pitch(L):
    """Row pitch (elements) of a bf16 activation tensor with L frames: 16-byte rows and a zero tail of at least H_TAIL elements
    (the kernels gather row windows as unchecked 16-byte pieces: the convolution's zero padding is read from the tails)."""
    return (L + H_TAIL + 7) // 8 * 8


def h_alloc(B, Cc, L, device):
    """Zero-filled bf16 (B, C, pitch) tensor with H_HEAD zero elements in front of it (a view into a slightly larger buffer):
    producers only ever write frames [0, L), so the zero tails -- and the head -- stay zero."""
    pitch = h_pitch(L)
    flat = torch.zeros(H_HEAD + B * Cc * pitch, device=device, dtype=torch.bfloat16)
    return flat[H_HEAD:].view(B, Cc, pitch)


def _h3(t, L, name):
    """(ptr, batch stride, pitch) of a bf16 (B, C, pitch) device view whose rows are `pitch` apart (pitch = size of dim 2)."""
    if t is None:
        return None, 0, 0
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 3 and t.stride(2) == 1):
        raise ValueError(f"{name}: expected a 3-D bfloat16 device tensor with contiguous rows, got {tuple(t.shape)} {t.dtype}")
    _on_current_device(t, name)
    pitch = t.stride(1) if t.shape[1] > 1 else t.shape[2]
    if pitch < L or (pitch & 1):
        raise ValueError(f"{name}: row pitch {pitch} must be even and >= {L}")
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else t.shape[1] * pitch), pitch


def _convh_args(B, w_shape, Lin, stride, pad, transposed):
    """A ConvhArgs with the layer's geometry filled in (``w_shape`` = shape of the fp32 master weight)."""
    Cin, Cout, k = _geom(transposed, w_shape)
    a = _lib.ConvhArgs()
    a.B, a.Cin, a.Cout, a.Lin, a.k, a.stride, a.pad, a.transposed = B, Cin, Cout, Lin, k, stride, pad, int(transposed)
    a.Lout = convt_out_len(Lin, k, stride, pad) if transposed else conv_out_len(Lin, k, stride, pad)
    return a


def conv_fwd_h_supported(B, w_shape, Lin, stride, pad, transposed):
    """True if the bf16-resident kernels cover this layer at this batch / frame count (pg_conv_fwd_h_supported; host only)."""
    a = _convh_args(B, w_shape, Lin, stride, pad, transposed)
    a.x_pitch = h_pitch(Lin)
    a.x_bs = a.Cin * a.x_pitch
    return bool(_lib.load().pg_conv_fwd_h_supported(C.byref(a)))


def shadow_weights(w, transposed, stride, out=None):
    """bf16 shadow of a conv weight in the bf16-resident kernels' GEMM layout (pg_shadow_weights)."""
    Cin, Cout, k = _geom(transposed, w.shape)
    n = _lib.load().pg_shadow_elems(Cin, Cout, k, stride, int(transposed))
    if out is None or out.numel() != n:
        out = torch.empty(n, device=w.device, dtype=torch.bfloat16)
    _lib.check(_lib.load().pg_shadow_weights(_dense(w, "w"), C.c_void_p(out.data_ptr()), Cin, Cout, k, stride, int(transposed), _stream()),
               "shadow_weights")
    return out


def cast_rows_bf16(x, out, act=ACT_NONE):
    """fp32 (B, C, L) -> bf16 (B, C, pitch) rows, activation applied, tails zeroed."""
    a = _lib.CastArgs()
    a.B, a.C, a.L = x.shape
    a.act = act
    a.x, a.x_bs = _act3(x, "x")
    a.y, a.y_bs, a.pitch = _h3(out, x.shape[2], "out")
    _lib.check(_lib.load().pg_cast_rows_bf16(C.byref(a), _stream()), "cast_rows_bf16")
    return out


def conv_fwd_h(xh, Lin, wh, w_shape, stride, pad, transposed=False, y=None, yh=None, yh_act=ACT_NONE, yh2=None, yh2_act=ACT_NONE,
               schedule=None):
    """bf16-resident forward conv (pg_conv_fwd_h): xh bf16 (B, Cin, pitch) holding Lin frames, wh the layer's bf16 shadow
    (``w_shape`` = shape of the fp32 master weight).  Outputs: fp32 y (B, Cout, Lout) and / or bf16 yh / yh2 (stored activated)."""
    B = xh.shape[0]
    a = _convh_args(B, w_shape, Lin, stride, pad, transposed)
    Cin, Cout, k = a.Cin, a.Cout, a.k
    a.schedule = _tls.schedule if schedule is None else schedule
    if xh.shape[1] != Cin:
        raise ValueError(f"conv_fwd_h: x has {xh.shape[1]} channels, weight expects {Cin}")
    a.x, a.x_bs, a.x_pitch = _h3(xh, Lin + 1, "xh")
    # v0.3 layout contract: the kernels gather the window of row (0, 0) from up to PG_H_HEAD elements IN FRONT of the tensor (the
    # convolution's left padding is read, not synthesised).  The C side only sees a pointer; here the storage is visible: a tensor
    # that starts closer than H_HEAD elements to the beginning of its allocation (plain torch.zeros(B, C, pitch) instead of
    # ops.h_alloc) would make the kernel read in front of the allocation -- foreign bytes as padding, or a GPU memory fault.
    if xh.storage_offset() < H_HEAD:
        raise ValueError(f"conv_fwd_h: xh starts {xh.storage_offset()} elements into its allocation; the bf16-resident kernels read "
                         f"{H_HEAD} zero elements in front of it -- allocate activations with ops.h_alloc (or pass a channel slice)")
    if wh.dtype != torch.bfloat16 or wh.numel() != _lib.load().pg_shadow_elems(Cin, Cout, k, stride, int(transposed)):
        raise ValueError("conv_fwd_h: wh must be the bf16 shadow of the layer's weight (ops.shadow_weights)")
    _on_current_device(wh, "wh")
    a.w = wh.data_ptr()
    if y is not None:
        if tuple(y.shape) != (B, Cout, a.Lout):
            raise ValueError(f"conv_fwd_h: y{tuple(y.shape)} should be {(B, Cout, a.Lout)}")
        a.y, a.y_bs = _act3(y, "y")
    if yh is not None:
        a.yh, a.yh_bs, a.yh_pitch = _h3(yh, a.Lout, "yh")
        a.yh_act = yh_act
    if yh2 is not None:
        a.yh2, a.yh2_bs, a.yh2_pitch = _h3(yh2, a.Lout, "yh2")
        a.yh2_act = yh2_act
    ws = conv_workspace(xh.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if _timer is not None and _cur_label is not None and _cur_label not in _timer.plans:
        _timer.plans[_cur_label] = conv_fwd_h_describe(a)
    _lib.check(_lib.load().pg_conv_fwd_h(C.byref(a), _stream()), "conv_fwd_h")
    return a.Lout


def conv_fwd_h_describe(a):
    """pg_conv_fwd_h_describe: 'conv_h3_kernel<...>|grid=G|tiles=T|slabs=S|split=0/1|whole=W|fixup=none/plain/wide' for a filled ConvhArgs."""
    return _describe(_lib.load().pg_conv_fwd_h_describe, a, "conv_fwd_h_describe")


def _norm_outputs(a, L, y, y_act, y2, y2_act, yh, yh_act, yh2, yh2_act):
    """Bind the outputs of a normalisation forward into a BnArgs / ClipNormArgs (same field names): fp32 y / y2 (B, C, L) and bf16
    yh / yh2 (B, C, pitch), each optional and stored with its own activation."""
    a.y_act, a.y2_act = y_act, y2_act
    if y is not None:                       # (a tensor that is not given costs no call: these wrappers are on the launch-bound path)
        a.y, a.y_bs = _act3(y, "y")
    if y2 is not None:
        a.y2, a.y2_bs = _act3(y2, "y2")
    if yh is not None:
        a.yh, a.yh_bs, a.yh_pitch, a.yh_act = *_h3(yh, L, "yh"), yh_act
    if yh2 is not None:
        a.yh2, a.yh2_bs, a.yh2_pitch, a.yh2_act = *_h3(yh2, L, "yh2"), yh2_act


def bn_fwd(x, y, gamma, beta, save_mean, save_invstd, running_mean=None, running_var=None, eps=1e-5, momentum=0.1,
           y_act=ACT_NONE, y2=None, y2_act=ACT_NONE, yh=None, yh_act=ACT_NONE, yh2=None, yh2_act=ACT_NONE, num_batches_tracked=None):
    """Train-mode BatchNorm forward (model.py:81,83).  ``num_batches_tracked``: the layer's int64 counter (0-d device tensor),
    incremented by the kernel itself -- no extra launch."""
    a = _lib.BnArgs()
    a.B, a.C, a.L = x.shape
    a.eps, a.momentum = eps, momentum
    a.x, a.x_bs = _act3(x, "x")
    _norm_outputs(a, x.shape[2], y, y_act, y2, y2_act, yh, yh_act, yh2, yh2_act)
    a.gamma, a.beta = _dense(gamma, "gamma"), _dense(beta, "beta")
    a.save_mean, a.save_invstd = _dense(save_mean, "save_mean"), _dense(save_invstd, "save_invstd")
    if running_mean is not None:
        a.running_mean, a.running_var = _dense(running_mean, "running_mean"), _dense(running_var, "running_var")
    if num_batches_tracked is not None:
        a.num_batches_tracked = _dense_as(num_batches_tracked, torch.int64, "num_batches_tracked")
    _lib.check(_lib.load().pg_bn_fwd(C.byref(a), _stream()), "bn_fwd")
    return y


def clipnorm_fwd(x, y, gamma, beta, save_mean=None, save_invstd=None, running_mean=None, running_var=None, eps=1e-5, momentum=0.1,
                 y_act=ACT_NONE, y2=None, y2_act=ACT_NONE, yh=None, yh_act=ACT_NONE, yh2=None, yh2_act=ACT_NONE, num_batches_tracked=None,
                 workspace=None):
    """BatchNorm forward with PER-CLIP statistics (pg_clipnorm_fwd): every row (b, c) of x (B, C, L) is normalised by its own mean
    and biased variance -- what B batch-of-one ``bn_fwd`` calls compute (the reference's inference, demo.py:33-45), in one launch.
    Outputs as in ``bn_fwd``; ``save_mean`` / ``save_invstd`` are optional and (B, C).  The running buffers (C) take one momentum
    step per clip in clip order, ``num_batches_tracked`` grows by B.  ``workspace``: float32 scratch of at least 2 * B * C elements
    for the running-buffer chain (allocated here when missing; pass a persistent one to capture the call in a graph)."""
    a = _lib.ClipNormArgs()
    a.B, a.C, a.L = B, Cc, L = x.shape
    a.eps, a.momentum = eps, momentum
    a.x, a.x_bs = _act3(x, "x")
    for name, t in (("y", y), ("y2", y2)):
        if t is not None and tuple(t.shape) != (B, Cc, L):
            raise ValueError(f"clipnorm_fwd: {name}{tuple(t.shape)} should be {(B, Cc, L)}")
    for name, t in (("yh", yh), ("yh2", yh2)):
        if t is not None and tuple(t.shape[:2]) != (B, Cc):
            raise ValueError(f"clipnorm_fwd: {name}{tuple(t.shape)} should be ({B}, {Cc}, pitch)")
    _norm_outputs(a, L, y, y_act, y2, y2_act, yh, yh_act, yh2, yh2_act)
    for name, t, n in (("gamma", gamma, Cc), ("beta", beta, Cc), ("save_mean", save_mean, B * Cc), ("save_invstd", save_invstd, B * Cc),
                       ("running_mean", running_mean, Cc), ("running_var", running_var, Cc)):
        if t is not None and t.numel() != n:
            raise ValueError(f"clipnorm_fwd: {name} has {t.numel()} elements, expected {n}")
    a.gamma, a.beta = _dense(gamma, "gamma"), _dense(beta, "beta")
    if save_mean is not None:
        a.save_mean = _dense(save_mean, "save_mean")
    if save_invstd is not None:
        a.save_invstd = _dense(save_invstd, "save_invstd")
    if running_mean is not None:
        a.running_mean = _dense(running_mean, "running_mean")
    if running_var is not None:
        a.running_var = _dense(running_var, "running_var")
    if num_batches_tracked is not None:
        a.num_batches_tracked = _dense_as(num_batches_tracked, torch.int64, "num_batches_tracked")
    if running_mean is not None or running_var is not None:
        if workspace is None:
            workspace = torch.empty(2 * B * Cc, device=x.device, dtype=torch.float32)
        a.workspace, a.workspace_bytes = _dense(workspace, "workspace"), 4 * workspace.numel()
    _lib.check(_lib.load().pg_clipnorm_fwd(C.byref(a), _stream()), "clipnorm_fwd")
    return y


def bn_bwd(x, dy, dx, gamma, save_mean, save_invstd, dgamma, dbeta):
    a = _lib.BnArgs()
    a.B, a.C, a.L = x.shape
    a.x, a.x_bs = _act3(x, "x")
    a.dy, a.dy_bs = _act3(dy, "dy")
    a.dx, a.dx_bs = _act3(dx, "dx")
    a.gamma = _dense(gamma, "gamma")
    a.save_mean, a.save_invstd = _dense(save_mean, "save_mean"), _dense(save_invstd, "save_invstd")
    a.dgamma, a.dbeta = _dense(dgamma, "dgamma"), _dense(dbeta, "dbeta")
    _lib.check(_lib.load().pg_bn_bwd(C.byref(a), _stream()), "bn_bwd")
    return dx


_loss_ws = _StreamCache()
_caches.append(_loss_ws)


def loss_fwd_bwd(pred, batch, dpred=None, losses=None, mag_weight=0.2):
    """train.py:45-60 fused with its gradient.  Returns the 3-float device tensor [loss, ang, mag]."""
    B, C2, L = pred.shape
    Cc = C2 // 2
    if tuple(batch.shape) != (B, 2, Cc, L):
        raise ValueError(f"loss: batch {tuple(batch.shape)} does not match pred {tuple(pred.shape)}")
    a = _lib.LossArgs()
    a.B, a.C, a.L, a.mag_weight = B, Cc, L, mag_weight
    a.pred, a.batch = _dense(pred, "pred"), _dense(batch, "batch")
    if dpred is not None:
        a.dpred = _dense(dpred, "dpred")
    if losses is None:
        losses = torch.empty(3, device=pred.device, dtype=torch.float32)
    a.losses = _dense(losses, "losses")
    lib = _lib.load()
    a.workspace, a.workspace_bytes = _workspace(_loss_ws, pred.device, lib.pg_workspace_bytes_loss(C.byref(a)), "workspace_bytes_loss")
    _lib.check(lib.pg_loss_fwd_bwd(C.byref(a), _stream()), "loss_fwd_bwd")
    return losses


def adam_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, thin=False):
    a = _lib.AdamArgs()
    a.thin = int(bool(thin))
    a.n = p.numel()
    a.p, a.g, a.m, a.v = _dense(p, "p"), _dense(g, "g"), _dense(m, "m"), _dense(v, "v")
    a.lr, a.beta1, a.beta2, a.eps, a.grad_scale, a.step = lr, beta1, beta2, eps, grad_scale, step
    _lib.check(_lib.load().pg_adam_step(C.byref(a), _stream()), "adam_step")


def fill(t, value):
    _lib.check(_lib.load().pg_fill(C.c_void_p(_dense(t, "t")), t.numel(), value, _stream()), "fill")
    return t


def _stft_args(y, n_fft, hop, polar=False, out=None, single_frame=None, chunk_start=None, chunk_row=None, chunk_len=None):
    """The pg_stft_args of one ops.stft call and the tensor it fills."""
    if y.dim() == 1:
        y = y[None]
    a = _lib.StftArgs()
    if chunk_start is None:
        n_sig, n_samp = y.shape
    else:
        if chunk_start.dtype != torch.int64 or (chunk_row is not None and chunk_row.dtype != torch.int32):
            raise TypeError("chunk_start must be int64 and chunk_row int32")
        n_sig, n_samp = chunk_start.numel(), int(chunk_len)
        if chunk_row is not None and chunk_row.numel() != n_sig:
            raise ValueError("chunk_row needs one entry per chunk")
        a.chunk_start = _dense_as(chunk_start, torch.int64, "chunk_start")
        a.chunk_row = _dense_as(chunk_row, torch.int32, "chunk_row") if chunk_row is not None else None
        a.src_len, a.src_stride = y.shape[1], y.shape[1]
    nf = 1 + n_samp // hop
    if out is None:
        out = torch.empty(n_sig, 2, n_fft // 2, nf, device=y.device, dtype=torch.float32)
    elif tuple(out.shape) != (n_sig, 2, n_fft // 2, nf):
        raise ValueError(f"stft: out must be {(n_sig, 2, n_fft // 2, nf)}, got {tuple(out.shape)}")
    a.n_signals, a.n_samples, a.n_fft, a.hop, a.n_frames, a.polar = n_sig, n_samp, n_fft, hop, nf, int(polar)
    a.single_frame = _tls.stft_single if single_frame is None else int(bool(single_frame))
    a.y, a.out = _dense(y, "y"), _dense(out, "out")
    return a, out


def stft(y, n_fft, hop, polar=False, out=None, single_frame=None, chunk_start=None, chunk_row=None, chunk_len=None):
    """(n_signals, n_samples) -> (n_signals, 2, n_fft/2, 1 + n_samples // hop); preproc_mdb.py:84-97 (+ data.py:39-47).

    Chunked source (preproc_mdb.py:66-97): with ``chunk_start`` (int64 device tensor) signal s is the ``chunk_len`` samples of
    row ``chunk_row[s]`` (int32 device tensor; default row 0) of y (rows, samples) that begin at chunk_start[s]; samples past
    the end of the row read as zero -- no gathered or zero-padded copy of the audio is made."""
    a, out = _stft_args(y, n_fft, hop, polar, out, single_frame, chunk_start, chunk_row, chunk_len)
    _lib.check(_lib.load().pg_stft(C.byref(a), _stream()), "stft")
    return out


def stft_describe(*args, **kw):
    """pg_stft_describe for the arguments of ``stft``: 'kernel<...>,grid=G,block=T,lds=B' of the launch the call would make."""
    return _describe(_lib.load().pg_stft_describe, _stft_args(*args, **kw)[0], "stft_describe")


def stats_tensor(stats, device):
    """The two-double device tensor {mean, std} pg_stft_crops / pg_standardize read, from a ``(mean, std)`` pair of Python floats (one
    upload: callers that run many batches build it once) or from such a tensor (returned as it is).  std must be finite and > 0."""
    if torch.is_tensor(stats):
        if stats.dtype != torch.float64 or stats.numel() != 2 or not stats.is_cuda or not stats.is_contiguous():
            raise TypeError("stats must be a dense device tensor of two float64 values {mean, std}")
        return stats
    mean, std = (float(v) for v in stats)
    if not (mean == mean and abs(mean) != float("inf")) or not (0.0 < std < float("inf")):
        raise ValueError(f"stats: mean must be finite and std finite and positive, got ({mean}, {std})")
    return torch.tensor([mean, std], dtype=torch.float64).to(device)


def _stft_crops_args(src, crop_begin, crop_end, crop_len, n_fft, hop, polar=False, stats=None, out=None, single_frame=None):
    """The pg_stft_crops_args of one ops.stft_crops call, the tensor it fills and the tensors the struct points to."""
    if src.dim() != 1:
        raise ValueError("stft_crops: src is ONE flat buffer (1-D)")
    for t, name in ((crop_begin, "crop_begin"), (crop_end, "crop_end")):
        if t.dtype != torch.int64 or t.dim() != 1 or t.device != src.device:
            raise TypeError(f"stft_crops: {name} must be a 1-D int64 tensor on src's device")
    n_sig, n_samp = crop_begin.numel(), int(crop_len)
    if crop_end.numel() != n_sig:
        raise ValueError("stft_crops: crop_begin and crop_end need one entry per crop each")
    if stats is not None:
        stats = stats_tensor(stats, src.device)
    nf = 1 + n_samp // hop
    if out is None:
        out = torch.empty(n_sig, 2, n_fft // 2, nf, device=src.device, dtype=torch.float32)
    elif tuple(out.shape) != (n_sig, 2, n_fft // 2, nf):
        raise ValueError(f"stft_crops: out must be {(n_sig, 2, n_fft // 2, nf)}, got {tuple(out.shape)}")
    a = _lib.StftCropsArgs()
    a.n_signals, a.n_samples, a.n_fft, a.hop, a.n_frames, a.polar = n_sig, n_samp, n_fft, hop, nf, int(polar)
    a.single_frame = _tls.stft_single if single_frame is None else int(bool(single_frame))
    a.src, a.out = _dense(src, "src"), _dense(out, "out")
    a.crop_begin, a.crop_end = _dense_as(crop_begin, torch.int64, "crop_begin"), _dense_as(crop_end, torch.int64, "crop_end")
    a.stats = stats.data_ptr() if stats is not None else None
    return a, out, stats


def stft_crops(src, crop_begin, crop_end, crop_len, n_fft, hop, polar=False, stats=None, out=None, single_frame=None):
    """One launch from raw audio to a training batch: crop s is the ``crop_len`` samples of the flat device buffer ``src`` from
    crop_begin[s], read up to crop_end[s] (the end of its track) and zero beyond -> (n_crops, 2, n_fft/2, 1 + crop_len // hop), the
    bits of ``stft`` on the gathered crops, then ``standardize_with_`` (``stats``: a two-double device tensor or a (mean, std) pair
    of Python floats; the pair is uploaded on every call, so loops pass ``stats_tensor(...)``), then ``polar``.
    The caller guarantees 0 <= crop_begin and crop_end <= src.numel(): the device arrays are not checked."""
    a, out, _keep = _stft_crops_args(src, crop_begin, crop_end, crop_len, n_fft, hop, polar, stats, out, single_frame)
    _lib.check(_lib.load().pg_stft_crops(C.byref(a), _stream()), "stft_crops")
    return out


def stft_crops_describe(*args, **kw):
    """pg_stft_crops_describe for the arguments of ``stft_crops``."""
    a, _out, _keep = _stft_crops_args(*args, **kw)
    return _describe(_lib.load().pg_stft_crops_describe, a, "stft_crops_describe")


def _out(out, want, device, who, rows=False):
    """The ``out=`` argument of a wrapper: None -> a new float32 tensor shaped ``want``, else ``out`` itself, which must be shaped
    ``want``.  ``rows``: the wrapper takes a row stride, so ``out`` must be a float32 device tensor with contiguous rows (the other
    wrappers hand it to ``_dense``, which checks the rest)."""
    if out is None:
        return torch.empty(want, device=device, dtype=torch.float32)
    if rows:
        if not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == want and (want[-1] == 1 or out.stride(-1) == 1)):
            raise ValueError(f"{who}: out must be a float32 device tensor of shape {want} with contiguous rows")
        _on_current_device(out, "out")
    elif tuple(out.shape) != want:
        raise ValueError(f"{who}: out must be {want}, got {tuple(out.shape)}")
    return out


_RES_TYPES = {"kaiser_best": _lib.RS_KAISER_BEST, "kaiser_fast": _lib.RS_KAISER_FAST,
              _lib.RS_KAISER_BEST: _lib.RS_KAISER_BEST, _lib.RS_KAISER_FAST: _lib.RS_KAISER_FAST}
_resample_banks = {}     # (U, D, quality, device) -> device copy of pg_resample_bank's output (read-only; at most 226 KB each)


def resample_bank_host(up, down, quality=_lib.RS_KAISER_BEST):
    """pg_resample_bank: the (taps, U) float32 polyphase filter bank of up / down, built on the host in double (no GPU needed)."""
    import numpy as np
    lib = _lib.load()
    n = lib.pg_resample_bank_elems(up, down, quality)
    if n < 0:
        _lib.check(int(n), "resample_bank_elems")
    bank = np.empty(n, np.float32)
    _lib.check(lib.pg_resample_bank(bank.ctypes.data_as(C.c_void_p), up, down, quality), "resample_bank")
    return bank.reshape(lib.pg_resample_taps(up, down, quality), -1)


def _resample_bank(up, down, quality, device):
    import math
    g = math.gcd(up, down)
    key = (up // g, down // g, quality, torch.device(device))
    bank = _resample_banks.get(key)
    if bank is None:
        bank = _resample_banks[key] = torch.from_numpy(resample_bank_host(up, down, quality)).to(device)
    return bank


def resample(x, orig_sr, target_sr, res_type="kaiser_best", out=None):
    """librosa.resample(x, orig_sr, target_sr) of preproc_mdb.py:114 on device: x (n,) or (n_signals, n) float32 whose rows are
    contiguous (the row stride is free) -> (..., ceil(n * target_sr / orig_sr)).  Kaiser-windowed sinc with resampy's published
    ``kaiser_best`` / ``kaiser_fast`` parameters (include/phasegen.h; parity with resampy's table interpolation is unpinned).
    The filter bank is built once per (reduced ratio, quality, device).  Equal rates return ``x`` itself, as librosa does."""
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if res_type not in _RES_TYPES:
        raise ValueError(f"resample: res_type must be 'kaiser_best' or 'kaiser_fast', got {res_type!r}")
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() in (1, 2)):
        raise ValueError(f"resample: expected a 1-D or 2-D float32 device tensor, got {tuple(x.shape)} {x.dtype} {x.device}")
    if orig_sr == target_sr and orig_sr > 0:
        return x
    _on_current_device(x, "x")
    lib = _lib.load()
    x2 = x[None] if x.dim() == 1 else x
    n_sig, n_in = x2.shape
    if n_in > 1 and x2.stride(1) != 1:
        raise ValueError(f"resample: samples must be contiguous (strides {x.stride()})")
    n_out = lib.pg_resample_out_len(n_in, target_sr, orig_sr)
    if n_out < 0:
        _lib.check(int(n_out), "resample_out_len")
    want = (n_out,) if x.dim() == 1 else (n_sig, n_out)
    out = _out(out, want, x.device, "resample", rows=True)
    o2 = out[None] if out.dim() == 1 else out
    quality = _RES_TYPES[res_type]
    a = _lib.ResampleArgs()
    a.n_signals, a.up, a.down, a.quality, a.n_in, a.n_out = n_sig, target_sr, orig_sr, quality, n_in, n_out
    a.x, a.x_stride = x2.data_ptr(), (x2.stride(0) if n_sig > 1 else n_in)
    a.y, a.y_stride = o2.data_ptr(), (o2.stride(0) if n_sig > 1 else n_out)
    a.bank = _resample_bank(target_sr, orig_sr, quality, x.device).data_ptr()
    _lib.check(lib.pg_resample(C.byref(a), _stream()), "resample")
    return out


# resampy's published (zeros, beta, rolloff) per quality: the parameters of pg_resample's filter (csrc/pg_kaiser.h)
VARISPEED_FILTERS = {_lib.RS_KAISER_BEST: (64, 14.769656459379492, 0.9475937167399596), _lib.RS_KAISER_FAST: (16, 8.555504641634386, 0.85)}
_varispeed_tables = {}   # (device, quality, per_zero) -> device copy of pg_varispeed_table's output (read-only; at most 256 KB each)


def varispeed_table_host(zeros, per_zero, beta, rolloff):
    """pg_varispeed_table: the (zeros * per_zero + 1, 2) float32 table of pairs (h_i, h_{i+1} - h_i) of the Kaiser-windowed sinc,
    ``per_zero`` samples per zero crossing, built on the host in double (no GPU needed)."""
    import numpy as np
    lib = _lib.load()
    zeros, per_zero = int(zeros), int(per_zero)
    n = lib.pg_varispeed_table_elems(zeros, per_zero)
    if n < 0:
        _lib.check(int(n), "varispeed_table_elems")
    table = np.empty(n, np.float32)
    _lib.check(lib.pg_varispeed_table(table.ctypes.data_as(C.c_void_p), zeros, per_zero, float(beta), float(rolloff)), "varispeed_table")
    return table.reshape(-1, 2)


def _varispeed_table(quality, per_zero, device):
    key = (torch.device(device), quality, per_zero)
    table = _varispeed_tables.get(key)
    if table is None:
        zeros, beta, rolloff = VARISPEED_FILTERS[quality]
        table = _varispeed_tables[key] = torch.from_numpy(varispeed_table_host(zeros, per_zero, beta, rolloff)).to(device)
    return table


def varispeed_blocks(n_out, step):
    """nb = ceil(n_out / step): the blocks of ``varispeed``; ``pos`` holds nb + 1 entries and ``scale`` nb."""
    return -(-int(n_out) // int(step))


def varispeed(x, pos, scale, n_out, step=64, res_type="kaiser_best", per_zero=512, table=None, out=None):
    """Band-limited resampling along a table of source positions (pg_varispeed): x (n,) or (n_signals, n) float32 on the device whose
    rows are contiguous (the row stride is free) -> (..., n_out).  Output t of block j = t // step reads the source at
    pos[j] + (t - j step) (pos[j + 1] - pos[j]) / step samples through the Kaiser-windowed sinc of ``resample`` narrowed to
    scale[j] in [0.25, 1] of the band (1: the filter as it is; below 1 for a block that is read faster than one sample per output).
    ``pos``: 1-D float64 device tensor of nb + 1 entries, ``scale``: 1-D float32 device tensor of nb entries, nb =
    ``varispeed_blocks(n_out, step)``; ``step`` a power of two up to 4096.  ``res_type`` picks resampy's (zeros, beta, rolloff), as in
    ``resample``; the filter is tabulated ``per_zero`` times per zero crossing (a power of two up to 512) and interpolated linearly,
    the table built once per (device, res_type, per_zero).  ``table``: (device table from ``varispeed_table_host``, zeros, per_zero)
    in place of the cached one."""
    who = "varispeed"
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (1, 2)):
        raise ValueError(f"{who}: expected a 1-D or 2-D float32 device tensor")
    _on_current_device(x, "x")
    x2 = x[None] if x.dim() == 1 else x
    n_sig, n_in = x2.shape
    n_out, step = int(n_out), int(step)
    if n_sig < 1 or n_in < 1 or n_out < 1:
        raise ValueError(f"{who}: empty input {tuple(x.shape)} or n_out {n_out}")
    if n_in > 1 and x2.stride(1) != 1:
        raise ValueError(f"{who}: samples must be contiguous (strides {x.stride()})")
    if not (1 <= step <= _lib.VARISPEED_MAX_STEP and step & (step - 1) == 0):
        raise ValueError(f"{who}: step must be a power of two within [1, {_lib.VARISPEED_MAX_STEP}], got {step}")
    if table is None:
        if res_type not in _RES_TYPES:
            raise ValueError(f"{who}: res_type must be 'kaiser_best' or 'kaiser_fast', got {res_type!r}")
        quality, per_zero = _RES_TYPES[res_type], int(per_zero)
        zeros = VARISPEED_FILTERS[quality][0]
        if not (1 <= per_zero <= _lib.VARISPEED_MAX_PER_ZERO and per_zero & (per_zero - 1) == 0):
            raise ValueError(f"{who}: per_zero must be a power of two within [1, {_lib.VARISPEED_MAX_PER_ZERO}], got {per_zero}")
        tab = _varispeed_table(quality, per_zero, x.device)
    else:
        try:
            tab, zeros, per_zero = table
            zeros, per_zero = int(zeros), int(per_zero)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: table must be (device tensor, zeros, per_zero)")
        if not (1 <= zeros <= _lib.VARISPEED_MAX_ZEROS and 1 <= per_zero <= _lib.VARISPEED_MAX_PER_ZERO and per_zero & (per_zero - 1) == 0):
            raise ValueError(f"{who}: table needs zeros within [1, {_lib.VARISPEED_MAX_ZEROS}] and per_zero a power of two within "
                             f"[1, {_lib.VARISPEED_MAX_PER_ZERO}], got {zeros} and {per_zero}")
        if not (torch.is_tensor(tab) and tab.is_cuda and tab.dtype == torch.float32 and tab.numel() == 2 * (zeros * per_zero + 1)):
            raise ValueError(f"{who}: table must be a float32 device tensor of 2 * (zeros * per_zero + 1) = {2 * (zeros * per_zero + 1)} entries")
    tab_ptr = _dense(tab, "table")
    nb = varispeed_blocks(n_out, step)
    if not (torch.is_tensor(pos) and pos.is_cuda and pos.dtype == torch.float64 and pos.dim() == 1):
        raise ValueError(f"{who}: pos must be a 1-D float64 device tensor")
    if pos.shape[0] != nb + 1:
        raise ValueError(f"{who}: pos must hold {nb + 1} entries (ceil(n_out / step) + 1), got {pos.shape[0]}")
    if not (torch.is_tensor(scale) and scale.is_cuda and scale.dtype == torch.float32 and scale.dim() == 1):
        raise ValueError(f"{who}: scale must be a 1-D float32 device tensor")
    if scale.shape[0] != nb:
        raise ValueError(f"{who}: scale must hold {nb} entries (ceil(n_out / step)), got {scale.shape[0]}")
    pos_ptr, scale_ptr = _dense_as(pos, torch.float64, "pos"), _dense_as(scale, torch.float32, "scale")
    want = (n_out,) if x.dim() == 1 else (n_sig, n_out)
    out = _out(out, want, x.device, who, rows=True)
    o2 = out[None] if out.dim() == 1 else out
    x_stride, y_stride = (x2.stride(0) if n_sig > 1 else n_in), (o2.stride(0) if n_sig > 1 else n_out)
    if x_stride < n_in or y_stride < n_out:
        raise ValueError(f"{who}: rows overlap in memory (strides {x.stride()} and {out.stride()})")
    _int32_sizes(who, n_in=n_in, n_out=n_out, x_stride=x_stride, y_stride=y_stride)
    a = _lib.VarispeedArgs()
    a.n_sig, a.n_in, a.n_out, a.step, a.zeros, a.per_zero = n_sig, n_in, n_out, step, zeros, per_zero
    a.x_stride, a.y_stride = x_stride, y_stride
    a.pos, a.scale, a.table, a.x, a.y = pos_ptr, scale_ptr, tab_ptr, x2.data_ptr(), o2.data_ptr()
    _lib.check(_lib.load().pg_varispeed(C.byref(a), _stream()), who)
    return out


def pitch_frames(n_in, hop=256, window=1024, tau_max=320):
    """the complete frames of ``pitch_track`` in a row of ``n_in`` samples: max(1, 1 + (n_in - window - tau_max) // hop)"""
    return max(1, 1 + (int(n_in) - int(window) - int(tau_max)) // int(hop))


def pitch_track(x, frames=None, hop=256, window=1024, tau_min=16, tau_max=320, threshold=0.15, out=None):
    """The fundamental period of every frame of every row, YIN (pg_pitch_track): x (n,) or (n_signals, n) float32 on the device whose
    rows are contiguous (the row stride is free) -> (period, ap), each (..., frames) float32.  Frame f holds the ``window + tau_max``
    samples from f * hop on (zeros past the row's end); ``period[f]`` is the lag in [tau_min, tau_max - 1] picked by the absolute
    ``threshold`` on the cumulative-mean-normalised difference, refined by a parabola (in samples: f0 = sr / period), ``ap[f]`` the
    normalised difference there: a frame is voiced where ``ap < threshold`` (the caller's decision; both are NaN for a frame that
    holds a non-finite sample).  ``frames=None``: the complete frames, ``pitch_frames(n, hop, window, tau_max)``.  ``window`` within
    [4, 2048], 2 <= tau_min < tau_max <= 1024.  ``out=(period, ap)``: views that are written in place.  Runs on the current stream
    and never synchronises."""
    who = "pitch_track"
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (1, 2)):
        raise ValueError(f"{who}: expected a 1-D or 2-D float32 device tensor")
    _on_current_device(x, "x")
    x2 = x[None] if x.dim() == 1 else x
    n_sig, n_in = x2.shape
    hop, window, tau_min, tau_max, threshold = int(hop), int(window), int(tau_min), int(tau_max), float(threshold)
    if n_sig < 1 or n_in < 1:
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")
    if n_in > 1 and x2.stride(1) != 1:
        raise ValueError(f"{who}: samples must be contiguous (strides {x.stride()})")
    if hop < 1:
        raise ValueError(f"{who}: hop must be positive, got {hop}")
    if not _lib.PITCH_MIN_WINDOW <= window <= _lib.PITCH_MAX_WINDOW:
        raise ValueError(f"{who}: window must be within [{_lib.PITCH_MIN_WINDOW}, {_lib.PITCH_MAX_WINDOW}], got {window}")
    if not _lib.PITCH_MIN_TAU <= tau_min < tau_max <= _lib.PITCH_MAX_TAU:
        raise ValueError(f"{who}: lags must satisfy {_lib.PITCH_MIN_TAU} <= tau_min < tau_max <= {_lib.PITCH_MAX_TAU}, got {tau_min} and {tau_max}")
    frames = pitch_frames(n_in, hop, window, tau_max) if frames is None else int(frames)
    if frames < 1:
        raise ValueError(f"{who}: frames must be positive, got {frames}")
    want = (frames,) if x.dim() == 1 else (n_sig, frames)
    if out is None:
        period, ap = _out(None, want, x.device, who), _out(None, want, x.device, who)
    else:
        try:
            period, ap = out
        except (TypeError, ValueError):
            raise ValueError(f"{who}: out must be (period, ap)")
        if not (torch.is_tensor(period) and torch.is_tensor(ap)):
            raise ValueError(f"{who}: out must be (period, ap)")
        period, ap = _out(period, want, x.device, who, rows=True), _out(ap, want, x.device, who, rows=True)
    p2, a2 = (period[None], ap[None]) if x.dim() == 1 else (period, ap)
    x_stride = x2.stride(0) if n_sig > 1 else n_in
    o_stride = p2.stride(0) if n_sig > 1 else frames
    if n_sig > 1 and a2.stride(0) != o_stride:
        raise ValueError(f"{who}: period and ap must have the same row stride (strides {period.stride()} and {ap.stride()})")
    if x_stride < n_in or o_stride < frames:
        raise ValueError(f"{who}: rows overlap in memory (strides {x.stride()} and {period.stride()})")
    _int32_sizes(who, n_in=n_in, frames=frames, hop=hop, x_stride=x_stride, out_stride=o_stride)
    a = _lib.PitchTrackArgs()
    a.n_sig, a.n_in, a.frames, a.hop, a.window, a.tau_min, a.tau_max = n_sig, n_in, frames, hop, window, tau_min, tau_max
    a.x_stride, a.out_stride, a.threshold = x_stride, o_stride, threshold
    a.x, a.period, a.ap = x2.data_ptr(), p2.data_ptr(), a2.data_ptr()
    _lib.check(_lib.load().pg_pitch_track(C.byref(a), _stream()), who)
    return period, ap


_stitch_ramps = {}       # (V, device) -> device copy of pg_stitch_ramp's output (read-only)
_stitch_ws = _StreamCache()
_caches.append(_stitch_ws)


def stitch_ramp_host(overlap):
    """pg_stitch_ramp: the crossfade ramp float32(sin^2(pi (j + 0.5) / (2 V))), j < V, built on the host in double (no GPU needed)."""
    import numpy as np
    ramp = np.empty(max(int(overlap), 0), np.float32)
    _lib.check(_lib.load().pg_stitch_ramp(ramp.ctypes.data_as(C.c_void_p) if ramp.size else None, int(overlap)), "stitch_ramp")
    return ramp


def _stitch_ramp(V, device):
    key = (V, torch.device(device))
    ramp = _stitch_ramps.get(key)
    if ramp is None:
        ramp = _stitch_ramps[key] = torch.from_numpy(stitch_ramp_host(V)).to(device)
    return ramp


def stitch(clips, step, n_out, normalize=False, out=None, return_status=False):
    """Crossfaded overlap-add of equal-length clips into tracks (pg_stitch): clips (n_clips, T) or (n_tracks, n_clips, T) float32
    on the device, samples contiguous, outer strides free; clip k begins at output sample k * step and shares V = T - step samples
    (0 <= 2 V <= T) with the next one under a sin^2 ramp; (n_clips - 1) * step < n_out <= (n_clips - 1) * step + T.  -> (n_out,)
    or (n_tracks, n_out).  ``normalize``: divide by the peak of the finite samples of ALL tracks (utils.py:42 for whole tracks).
    ``return_status``: also the (peak, n_nonfinite) device tensors (float32 / int32, 0-d)."""
    if not (torch.is_tensor(clips) and clips.is_cuda and clips.dtype == torch.float32 and clips.dim() in (2, 3)):
        raise ValueError("stitch: clips must be a 2-D or 3-D float32 device tensor")
    _on_current_device(clips, "clips")
    c3 = clips[None] if clips.dim() == 2 else clips
    n_tracks, n_clips, T = c3.shape
    step, n_out = int(step), int(n_out)
    if n_tracks < 1 or n_clips < 1 or T < 1:
        raise ValueError(f"stitch: empty clips {tuple(clips.shape)}")
    if not 1 <= step <= T or 2 * (T - step) > T:
        raise ValueError(f"stitch: step {step} with clips of {T} samples (need 1 <= step <= T and an overlap T - step of at most T / 2)")
    if not (n_clips - 1) * step < n_out <= (n_clips - 1) * step + T:
        raise ValueError(f"stitch: n_out {n_out} outside ({(n_clips - 1) * step}, {(n_clips - 1) * step + T}]")
    if T > 1 and c3.stride(2) != 1:
        raise ValueError(f"stitch: samples must be contiguous (strides {clips.stride()})")
    clip_stride = c3.stride(1) if n_clips > 1 else T
    track_stride = c3.stride(0) if n_tracks > 1 else n_clips * max(clip_stride, T)
    if clip_stride < T or track_stride < 0:
        raise ValueError(f"stitch: clips overlap in memory (strides {clips.stride()})")
    want = (n_out,) if clips.dim() == 2 else (n_tracks, n_out)
    out = _out(out, want, clips.device, "stitch", rows=True)
    o2 = out[None] if out.dim() == 1 else out
    out_stride = o2.stride(0) if n_tracks > 1 else n_out
    if out_stride < n_out:
        raise ValueError(f"stitch: rows of out overlap (strides {out.stride()})")
    lib = _lib.load()
    a = _lib.StitchArgs()
    a.n_tracks, a.n_clips, a.clip_len, a.step, a.n_out = n_tracks, n_clips, T, step, n_out
    a.clips, a.clip_stride, a.track_stride = c3.data_ptr(), clip_stride, track_stride
    a.out, a.out_stride = o2.data_ptr(), out_stride
    if T > step:
        a.ramp = _stitch_ramp(T - step, clips.device).data_ptr()
    a.normalize = int(bool(normalize))
    status = None
    if normalize or return_status:
        a.workspace, a.workspace_bytes = _workspace(_stitch_ws, clips.device, lib.pg_workspace_bytes_stitch(C.byref(a)), "workspace_bytes_stitch")
    if return_status:
        status = (torch.empty((), device=clips.device, dtype=torch.float32), torch.empty((), device=clips.device, dtype=torch.int32))
        a.peak, a.n_nonfinite = status[0].data_ptr(), status[1].data_ptr()
    _lib.check(lib.pg_stitch(C.byref(a), _stream()), "stitch")
    return (out, status[0], status[1]) if return_status else out


def _pos_keyword(fn):
    """Decorator of the five stretch wrappers: ``fn`` takes ``pos=None`` as its last parameter, by keyword.  ``inspect.signature``
    of the result reports the parameter list callers have always seen, without it (as phasegen.track's ``_keyword_options`` does for
    the track functions), and ``fn.options`` lists the keyword."""
    sig = inspect.signature(fn)
    assert list(sig.parameters)[-1] == "pos"

    @functools.wraps(fn)
    def call(*args, pos=None, **kw):
        return fn(*args, pos=pos, **kw)
    call.__signature__ = sig.replace(parameters=[p for p in sig.parameters.values() if p.name != "pos"])
    call.options = {"pos": None}
    return call


def _pos_table(pos, n, who, src_per_out, what):
    """``pos`` of a mapped call: a 1-D float64 device tensor of exactly ``n`` entries (``what``), dense; a ``src_per_out`` other than
    the default beside it is a contradiction."""
    if src_per_out != 1.0:
        raise ValueError(f"{who}: pos and src_per_out {src_per_out} are two time grids: pass one")
    if not (torch.is_tensor(pos) and pos.is_cuda and pos.dtype == torch.float64 and pos.dim() == 1):
        raise ValueError(f"{who}: pos must be a 1-D float64 device tensor")
    if pos.shape[0] != n:
        raise ValueError(f"{who}: pos must hold {n} entries ({what}), got {pos.shape[0]}")
    return _dense_as(pos, torch.float64, "pos")


def _int32_sizes(who, **sizes):
    """the mapped entry points take int32 sizes"""
    for name, v in sizes.items():
        if v > 0x7fffffff:
            raise ValueError(f"{who}: {name} = {v} does not fit the int32 sizes of a mapped call")


def _ch_rows(stride, F_src, bins, n_ch, who, name):
    """a channel stride in elements as the count of rows a mapped call takes"""
    if n_ch == 1:
        return bins
    if stride % F_src:
        raise ValueError(f"{who}: channels of {name} must be a whole number of rows apart for a mapped call (stride {stride}, rows of {F_src})")
    return stride // F_src


@_pos_keyword
def spec_clips(plane, n_clips, frames, sf, src_per_out=1.0, out=None, pos=None):
    """Clip windows of a spectrogram plane, optionally resampled along time (pg_spec_clips): plane (n_ch, bins, F_src) float32 on the
    device, frames contiguous, rows F_src apart, the channel stride free (``pol[:, 0]`` of a (n_ch, 2, bins, F) polar tensor is read in
    place) -> (n_clips, n_ch, bins, frames), dense.  Frame f of clip k is the plane at position (k * sf + f) * src_per_out, linearly
    interpolated between its two neighbours and clamped at the last frame; src_per_out == 1.0 copies.  n_clips = 1, frames = F_out
    resamples the whole plane.  ``pos`` (pg_spec_clips_map): a float64 device tensor of (n_clips - 1) * sf + frames source-frame
    positions, one per global output frame, in place of the line g * src_per_out (NaN and negatives count as 0)."""
    who = "spec_clips"
    p_stride = _vocoder_plane(plane, "plane", who=who)
    n_ch, bins, F_src = plane.shape
    n_clips, frames, sf, src_per_out = int(n_clips), int(frames), int(sf), float(src_per_out)
    if min(n_clips, frames, sf) < 1:
        raise ValueError(f"{who}: sizes must be positive (plane {tuple(plane.shape)}, n_clips {n_clips}, frames {frames}, sf {sf})")
    if not 0.0 < src_per_out < float("inf"):
        raise ValueError(f"{who}: src_per_out must be finite and positive, got {src_per_out}")
    if pos is None:
        name, a = who, _lib.SpecClipsArgs()
        a.src_per_out, a.p_stride = src_per_out, p_stride
    else:
        name, a = "spec_clips_map", _lib.SpecClipsMapArgs()
        a.pos = _pos_table(pos, (n_clips - 1) * sf + frames, who, src_per_out, "(n_clips - 1) * sf + frames")
        _int32_sizes(who, F_src=F_src, n_clips=n_clips, frames=frames, sf=sf)
        a.p_ch_rows = _ch_rows(p_stride, F_src, bins, n_ch, who, "plane")
    out = _out(out, (n_clips, n_ch, bins, frames), plane.device, who)
    a.n_clips, a.n_ch, a.bins, a.frames, a.sf, a.F_src = n_clips, n_ch, bins, frames, sf, F_src
    a.P, a.out = plane.data_ptr(), _dense(out, "out")
    _lib.check(getattr(_lib.load(), "pg_" + name)(C.byref(a), _stream()), name)
    return out


def phase_join(phi, sf, ramp=None, out=None):
    """One phase per global frame from the phases of overlapped clips (pg_phase_join): phi (n_clips, n_ch, bins, frames) float32 on
    the device, frames contiguous, the other three strides free (``y.view(n_clips, n_ch, 2 * bins, frames)[:, :, :bins]`` of a model
    output is read in place); clip k begins at global frame k * sf and shares Vf = frames - sf frames (1 <= Vf, 2 * Vf <= frames)
    with the next one -> (n_ch, bins, (n_clips - 1) * sf + frames).  A shared frame gets the circular mean of its two phases under
    the sin^2 ramp of ``stitch`` (``ramp``: Vf device floats to use instead), every other frame its clip's phase bit for bit."""
    if not (torch.is_tensor(phi) and phi.is_cuda and phi.dtype == torch.float32 and phi.dim() == 4):
        raise ValueError("phase_join: phi must be a 4-D float32 device tensor (n_clips, n_ch, bins, frames)")
    _on_current_device(phi, "phi")
    n_clips, n_ch, bins, frames = phi.shape
    sf = int(sf)
    Vf = frames - sf
    if min(n_clips, n_ch, bins, frames) < 1:
        raise ValueError(f"phase_join: empty phi {tuple(phi.shape)}")
    if sf < 1 or Vf < 1 or 2 * Vf > frames:
        raise ValueError(f"phase_join: sf {sf} with clips of {frames} frames (need 1 <= frames - sf and 2 * (frames - sf) <= frames)")
    if frames > 1 and phi.stride(3) != 1:
        raise ValueError(f"phase_join: frames must be contiguous (strides {phi.stride()})")
    row_pitch = phi.stride(2) if bins > 1 else frames
    plane = (bins - 1) * row_pitch + frames
    ch_stride = phi.stride(1) if n_ch > 1 else plane
    clip_stride = phi.stride(0) if n_clips > 1 else n_ch * max(ch_stride, plane)
    if row_pitch < frames or ch_stride < plane or clip_stride < plane:
        raise ValueError(f"phase_join: rows overlap in memory (strides {phi.stride()})")
    F_out = (n_clips - 1) * sf + frames
    out = _out(out, (n_ch, bins, F_out), phi.device, "phase_join")
    if ramp is None:
        ramp = _stitch_ramp(Vf, phi.device)
    elif tuple(ramp.shape) != (Vf,):
        raise ValueError(f"phase_join: ramp must hold Vf = {Vf} floats, got {tuple(ramp.shape)}")
    a = _lib.PhaseJoinArgs()
    a.n_clips, a.n_ch, a.bins, a.frames, a.sf = n_clips, n_ch, bins, frames, sf
    a.phi, a.clip_stride, a.ch_stride, a.row_pitch = phi.data_ptr(), clip_stride, ch_stride, row_pitch
    a.out, a.ramp = _dense(out, "out"), _dense(ramp, "ramp")
    _lib.check(_lib.load().pg_phase_join(C.byref(a), _stream()), "phase_join")
    return out


def _vocoder_plane(t, name, shape=None, who="phase_vocoder"):
    """(n_ch, bins, F_src) float32 on the device, frames contiguous, rows F_src apart, the channel stride free -> that stride.
    ``who``: the caller the messages name."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
        raise ValueError(f"{who}: {name} must be a 3-D float32 device tensor (n_ch, bins, F_src)")
    _on_current_device(t, name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be shaped like angle, {tuple(shape)}, got {tuple(t.shape)}")
    n_ch, bins, F_src = t.shape
    if min(n_ch, bins, F_src) < 1:
        raise ValueError(f"{who}: empty {name} {tuple(t.shape)}")
    if (F_src > 1 and t.stride(2) != 1) or (bins > 1 and t.stride(1) != F_src):
        raise ValueError(f"{who}: frames of {name} must be contiguous and rows F_src apart (strides {t.stride()})")
    stride = t.stride(0) if n_ch > 1 else bins * F_src
    if stride < bins * F_src:
        raise ValueError(f"{who}: channels of {name} overlap in memory (strides {t.stride()})")
    return stride


def _stretch_args(a, who, angle, F_out, src_per_out, pos, logmag, reset_below, out, refs=None):
    """Checks the arguments ``phase_vocoder``, ``phase_lock`` and ``phase_lock_linked`` share and fills everything but the workspace
    of ``a``, one of their six structs: with ``pos`` (F_out source-frame positions) a mapped one, which takes the table and channel
    strides in rows, else a uniform one, which takes ``src_per_out`` and strides in elements.  ``refs``: (ref_angle, ref_logmag) of
    a linked call.  The scalars are range-checked first, ``src_per_out`` too when ``pos`` is given; then a ``pos`` beside a
    ``src_per_out`` other than 1.0 is refused.  -> ``out``, allocated when None."""
    a_stride = _vocoder_plane(angle, "angle", who=who)
    n_ch, bins, F_src = angle.shape
    if refs is not None:
        refs = [t[None] if torch.is_tensor(t) and t.dim() == 2 else t for t in refs]
        for t, name in zip(refs, ("ref_angle", "ref_logmag")):
            _vocoder_plane(t, name, who=who)
            if tuple(t.shape) != (1, bins, F_src):
                raise ValueError(f"{who}: {name} must be (bins, F_src) or (1, bins, F_src) = {(1, bins, F_src)}, got {tuple(t.shape)}")
        a.Aref, a.Mref = refs[0].data_ptr(), refs[1].data_ptr()
    F_out, src_per_out, reset_below = int(F_out), float(src_per_out), float(reset_below)
    if F_out < 1:
        raise ValueError(f"{who}: F_out must be positive, got {F_out}")
    if not 0.0 < src_per_out < float("inf"):
        raise ValueError(f"{who}: src_per_out must be finite and positive, got {src_per_out}")
    if not 0.0 <= reset_below < float("inf"):
        raise ValueError(f"{who}: reset_below must be finite and not negative, got {reset_below}")
    mapped = pos is not None
    if mapped:
        a.pos = _pos_table(pos, F_out, who, src_per_out, "F_out")
        _int32_sizes(who, F_src=F_src, F_out=F_out)
    else:
        a.src_per_out = src_per_out
    if logmag is not None:
        m_stride = _vocoder_plane(logmag, "logmag", angle.shape, who=who)
        if mapped:
            a.m_ch_rows = _ch_rows(m_stride, F_src, bins, n_ch, who, "logmag")
        else:
            a.m_stride = m_stride
        a.M = logmag.data_ptr()
    out = _out(out, (n_ch, bins, F_out), angle.device, who)
    a.n_ch, a.bins, a.F_src, a.F_out, a.reset_below = n_ch, bins, F_src, F_out, reset_below
    if mapped:
        a.a_ch_rows = _ch_rows(a_stride, F_src, bins, n_ch, who, "angle")
    else:
        a.a_stride = a_stride
    a.A, a.out = angle.data_ptr(), _dense(out, "out")
    return out


PHASE_LOCK_CHUNK = 32          # output frames per chunk of pg_phase_lock's scan (csrc/lock.hip: LK_CHUNK)
_lock_ws = _StreamCache()
_caches.append(_lock_ws)


def _lock_call(name, a, device):
    """pg_<name>, one of the five entry points of csrc/lock.hip, on the workspace its own query asks for."""
    lib, query = _lib.load(), "workspace_bytes_" + name
    a.workspace, a.workspace_bytes = _workspace(_lock_ws, device, getattr(lib, "pg_" + query)(C.byref(a)), query)
    _lib.check(getattr(lib, "pg_" + name)(C.byref(a), _stream()), name)


@_pos_keyword
def phase_vocoder(angle, F_out, src_per_out=1.0, logmag=None, reset_below=0.0, out=None, pos=None):
    """The phase-vocoder phase of a time-stretched spectrogram (pg_phase_vocoder): angle (n_ch, bins, F_src) float32 on the device,
    frames contiguous, rows F_src apart, the channel stride free (``pol[:, 1]`` of a (n_ch, 2, bins, F) polar tensor is read in place)
    -> (n_ch, bins, F_out), dense, in [-pi, pi].  Output frame g sits at source position g * src_per_out (src_per_out = 1 / stretch);
    every bin's phase advances from frame to frame by the wrapped difference of the two analysis phases around that position, summed
    exactly on a 2^32 grid of the turn.  ``logmag`` (same shape, ``pol[:, 0]``) and ``reset_below``: a frame whose log-magnitude is
    below the floor takes the analysis phase itself (the transient / silence reset); without either nothing resets after frame 0.
    src_per_out == 1.0 returns the analysis phase (to 2 pi / 2^33 and one rounding).  ``pos`` (pg_phase_vocoder_map): a float64
    device tensor of F_out source-frame positions in place of the line g * src_per_out (NaN and negatives count as 0; the positions
    need not grow)."""
    name, a = ("phase_vocoder", _lib.PhaseVocoderArgs()) if pos is None else ("phase_vocoder_map", _lib.PhaseVocoderMapArgs())
    out = _stretch_args(a, "phase_vocoder", angle, F_out, src_per_out, pos, logmag, reset_below, out)
    _lib.check(getattr(_lib.load(), "pg_" + name)(C.byref(a), _stream()), name)
    return out


@_pos_keyword
def phase_lock(angle, F_out, src_per_out=1.0, logmag=None, reset_below=0.0, out=None, pos=None):
    """The phase-vocoder phase with identity phase locking (pg_phase_lock): ``angle`` and ``logmag`` (required) as in
    ``phase_vocoder``, (n_ch, bins <= 4096, F_src) float32 on the device, read in place from a polar tensor -> (n_ch, bins, F_out),
    dense, in [-pi, pi].  In every output frame the peaks of the log-magnitude (larger than the two bins below, not smaller than the
    two above) advance by their own measured phase advance and every other bin takes the rotation of its nearest peak, so the
    analysis' phase relations inside a sinusoid's lobe survive; a peak below ``reset_below`` resets its whole region to the analysis
    phase.  Exact on a 2^32 grid of the turn, like ``phase_vocoder``; src_per_out == 1.0 returns the analysis phase.  ``pos``
    (pg_phase_lock_map): F_out source-frame positions, as in ``phase_vocoder``."""
    if logmag is None:
        raise ValueError("phase_lock: logmag is required (the peaks are those of the log-magnitude)")
    name, a = ("phase_lock", _lib.PhaseLockArgs()) if pos is None else ("phase_lock_map", _lib.PhaseLockMapArgs())
    out = _stretch_args(a, "phase_lock", angle, F_out, src_per_out, pos, logmag, reset_below, out)
    _lock_call(name, a, angle.device)
    return out


@_pos_keyword
def phase_lock_linked(angle, ref_angle, ref_logmag, F_out, src_per_out=1.0, reset_below=0.0, out=None, pos=None):
    """``phase_lock`` with the channels linked (pg_phase_lock_linked): ``angle`` (n_ch, bins <= 4096, F_src) as in ``phase_lock``, read
    in place from a polar tensor; ``ref_angle`` and ``ref_logmag``: the planes of ONE reference channel (the channel mean, in
    phasegen.track), (bins, F_src) or (1, bins, F_src), dense -> (n_ch, bins, F_out), dense, in [-pi, pi].  The peaks, the regions
    and the rotation are those ``phase_lock(ref_angle, ..., logmag=ref_logmag)`` forms, once, and every channel adds its own
    analysis phase to that one rotation: the phase difference between any two channels is the analysis' own in every cell, so the
    stereo image and the mono sum survive the stretch.  A channel equal to the reference gets ``phase_lock``'s bits;
    src_per_out == 1.0 returns the analysis phase.  ``pos`` (pg_phase_lock_linked_map): F_out source-frame positions, as in
    ``phase_vocoder``."""
    name, a = ("phase_lock_linked", _lib.PhaseLockLinkedArgs()) if pos is None else ("phase_lock_linked_map", _lib.PhaseLockLinkedMapArgs())
    out = _stretch_args(a, "phase_lock_linked", angle, F_out, src_per_out, pos, None, reset_below, out, refs=(ref_angle, ref_logmag))
    _lock_call(name, a, angle.device)
    return out


def phase_spsi(logmag, n_fft, hop, bin0=1, out=None):
    """A phase from the magnitudes alone, in one pass (pg_phase_spsi; single-pass spectrogram inversion, Beauregard et al. 2015):
    ``logmag`` (n_ch, bins <= 4096, F) float32 on the device, on the OUTPUT frame grid, frames contiguous, rows F apart, the channel
    stride free (``pol[:, 0]`` of a (n_ch, 2, bins, F) polar tensor is read in place) -> (n_ch, bins, F), dense, in [-pi, pi].  The
    peaks of every frame (``phase_lock``'s) advance by their parabola-interpolated frequency, (bin + offset) * hop / n_fft of a turn
    per frame, every other bin follows its nearest peak, and odd FFT bins get the half turn of the centred Hann framing; ``bin0`` is
    the FFT bin of row 0 (1: the DC row is dropped).  Exact on a 2^32 grid of the turn.  No analysis phase, no weights, no
    iteration: the model-free estimate a predicted phase has to beat, and a start for Griffin-Lim."""
    m_stride = _vocoder_plane(logmag, "logmag", who="phase_spsi")
    n_ch, bins, F = logmag.shape
    n_fft, hop, bin0 = int(n_fft), int(hop), int(bin0)
    if not 1 <= hop <= n_fft:
        raise ValueError(f"phase_spsi: need 1 <= hop <= n_fft, got hop {hop} and n_fft {n_fft}")
    if not 0 <= bin0 <= 65536:
        raise ValueError(f"phase_spsi: bin0 must be within [0, 65536], got {bin0}")
    out = _out(out, (n_ch, bins, F), logmag.device, "phase_spsi")
    a = _lib.PhaseSpsiArgs()
    a.n_ch, a.bins, a.F, a.n_fft, a.hop, a.bin0 = n_ch, bins, F, n_fft, hop, bin0
    a.M, a.m_stride = logmag.data_ptr(), m_stride
    a.out = _dense(out, "out")
    _lock_call("phase_spsi", a, logmag.device)
    return out


def hpss(logmag, win_t=17, win_f=17, out=None):
    """Harmonic / percussive split of a log-magnitude plane by median filtering (pg_hpss; Fitzgerald 2010 with binary masks):
    ``logmag`` (n_ch, bins, F) float32 on the device, frames contiguous, rows F apart, the channel stride free (``pol[:, 0]`` of a
    polar tensor is read in place) -> (harm, perc), (n_ch, bins, F) each, dense.  A cell goes to ``harm`` when the median of the
    ``win_t`` frames around it in its row is at least the median of the ``win_f`` bins around it in its frame (IEEE total order on the
    bits, edges replicated), else to ``perc``; the other plane holds +0.0 there, so every cell lands in exactly one plane bit for
    bit.  Windows are odd and at most 31.  ``out``: a (harm, perc) pair of dense tensors to fill."""
    who = "hpss"
    m_stride = _vocoder_plane(logmag, "logmag", who=who)
    n_ch, bins, F = logmag.shape
    win_t, win_f = int(win_t), int(win_f)
    for w, name in ((win_t, "win_t"), (win_f, "win_f")):
        if not (1 <= w <= _lib.HPSS_MAX_WIN and w % 2 == 1):
            raise ValueError(f"{who}: {name} must be odd and within 1 .. {_lib.HPSS_MAX_WIN}, got {w}")
    if out is not None and not (isinstance(out, (tuple, list)) and len(out) == 2):
        raise ValueError(f"{who}: out must be a (harm, perc) pair")
    harm = _out(None if out is None else out[0], (n_ch, bins, F), logmag.device, who)
    perc = _out(None if out is None else out[1], (n_ch, bins, F), logmag.device, who)
    a = _lib.HpssArgs()
    a.n_ch, a.bins, a.F, a.win_t, a.win_f = n_ch, bins, F, win_t, win_f
    a.M, a.m_stride = logmag.data_ptr(), m_stride
    a.harm, a.perc = _dense(harm, "harm"), _dense(perc, "perc")
    _lib.check(_lib.load().pg_hpss(C.byref(a), _stream()), who)
    return harm, perc


_ola_windows = {}        # (device, win_len) -> device copy of pg_ola_window's output (read-only)


def ola_window_host(win_len):
    """pg_ola_window: the periodic Hann window float32(0.5 - 0.5 cos(2 pi j / win_len)), built on the host in double (no GPU needed)."""
    import numpy as np
    win = np.empty(max(int(win_len), 0), np.float32)
    _lib.check(_lib.load().pg_ola_window(win.ctypes.data_as(C.c_void_p) if win.size else None, int(win_len)), "ola_window")
    return win


def _ola_window(win_len, device):
    key = (torch.device(device), win_len)
    win = _ola_windows.get(key)
    if win is None:
        win = _ola_windows[key] = torch.from_numpy(ola_window_host(win_len)).to(device)
    return win


def _ola_rows(t, name, who):
    """(n,) or (n_sig, n) float32 on the device, samples contiguous, the row stride free -> the 2-D view"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() in (1, 2)):
        raise ValueError(f"{who}: {name} must be a 1-D or 2-D float32 device tensor")
    _on_current_device(t, name)
    t2 = t[None] if t.dim() == 1 else t
    if min(t2.shape) < 1:
        raise ValueError(f"{who}: empty {name} {tuple(t.shape)}")
    if (t2.shape[1] > 1 and t2.stride(1) != 1) or (t2.shape[0] > 1 and t2.stride(0) < t2.shape[1]):
        raise ValueError(f"{who}: samples of {name} must be contiguous and rows must not overlap (strides {t.stride()})")
    return t2


def ola_grains(n_out, win_len=256, hop=64):
    """How many grains cover the ``n_out`` output samples of ``ola_stretch``: the entries of its ``pos`` table."""
    return (int(n_out) + int(win_len) // 2) // int(hop) + 1


@_pos_keyword
def ola_stretch(x, n_out, src_per_out=1.0, win_len=256, hop=64, base=None, out=None, pos=None):
    """Time-domain overlap-add at a time ratio (pg_ola_stretch): x (n_in,) or (n_sig, n_in) float32 on the device, samples
    contiguous, the row stride free -> (..., n_out).  Output frame g, ``win_len`` samples of a periodic Hann window around output
    sample g * hop, is the input around sample rint(g * hop * src_per_out) (src_per_out = 1 / stretch), weighted, and every output
    sample is the weighted sum over the frames that cover it divided by the sum of their weights: the frames are moved, not
    stretched, so a click stays a click.  src_per_out == 1.0 returns x to a few ulps.  ``base`` (shaped like the result, rows free):
    added to the result in the same launch.  The window table is built once per (device, win_len).  ``pos`` (pg_ola_stretch_map): a
    float64 device tensor of ``ola_grains(n_out, win_len, hop)`` source centres in samples, one per grain, in place of the line
    g * hop * src_per_out (a NaN centre is outside the signal)."""
    who = "ola_stretch"
    x2 = _ola_rows(x, "x", who)
    n_sig, n_in = x2.shape
    n_out, src_per_out, win_len, hop = int(n_out), float(src_per_out), int(win_len), int(hop)
    if n_out < 1:
        raise ValueError(f"{who}: n_out must be positive, got {n_out}")
    if not 0.0 < src_per_out < float("inf"):
        raise ValueError(f"{who}: src_per_out must be finite and positive, got {src_per_out}")
    if not (2 <= win_len <= 4096 and win_len % 2 == 0):
        raise ValueError(f"{who}: win_len must be even and within 2 .. 4096, got {win_len}")
    if not 1 <= hop <= win_len // 2:
        raise ValueError(f"{who}: hop must be within 1 .. win_len / 2 = {win_len // 2}, got {hop}")
    want = (n_out,) if x.dim() == 1 else (n_sig, n_out)
    b2 = None
    if base is not None:
        if not torch.is_tensor(base) or tuple(base.shape) != want:
            raise ValueError(f"{who}: base must be shaped like the result, {want}")
        b2 = _ola_rows(base, "base", who)
    out = _out(out, want, x.device, who, rows=True)
    o2 = out[None] if out.dim() == 1 else out
    if n_sig > 1 and o2.stride(0) < n_out:
        raise ValueError(f"{who}: rows of out overlap (strides {out.stride()})")
    # (the stride of a single row is its length)
    x_stride, y_stride = (x2.stride(0), o2.stride(0)) if n_sig > 1 else (n_in, n_out)
    base_stride = 0 if b2 is None else b2.stride(0) if n_sig > 1 else n_out
    if pos is None:
        name, a = who, _lib.OlaStretchArgs()
        a.src_per_out = src_per_out
    else:
        name, a = "ola_stretch_map", _lib.OlaStretchMapArgs()
        a.pos = _pos_table(pos, ola_grains(n_out, win_len, hop), who, src_per_out, "ola_grains(n_out, win_len, hop)")
        _int32_sizes(who, n_in=n_in, n_out=n_out, x_stride=x_stride, base_stride=base_stride, y_stride=y_stride)
    a.n_sig, a.win_len, a.hop, a.n_in, a.n_out = n_sig, win_len, hop, n_in, n_out
    a.x, a.x_stride = x2.data_ptr(), x_stride
    if b2 is not None:
        a.base, a.base_stride = b2.data_ptr(), base_stride
    a.y, a.y_stride = o2.data_ptr(), y_stride
    a.win = _ola_window(win_len, x.device).data_ptr()
    _lib.check(getattr(_lib.load(), "pg_" + name)(C.byref(a), _stream()), name)
    return out


_formant_bases = {}      # (device, bins, order) -> device copy of pg_formant_basis's output (read-only; at most 1 MiB each)


def formant_basis_host(bins, order):
    """pg_formant_basis: the cosine table T[q][k] = cos(pi q (k + 1/2) / bins), (order, bins) row-major, followed by the ``order``
    liftered weights s[q], as ONE float32 array of order * bins + order entries, built on the host in double (no GPU needed)."""
    import numpy as np
    bins, order = int(bins), int(order)
    n = _lib.load().pg_formant_basis_elems(bins, order)
    _lib.check(min(n, 0), "formant_basis_elems")
    basis = np.empty(n, np.float32)
    _lib.check(_lib.load().pg_formant_basis(basis.ctypes.data_as(C.c_void_p), bins, order), "formant_basis")
    return basis


def _formant_basis(bins, order, device):
    key = (torch.device(device), bins, order)
    basis = _formant_bases.get(key)
    if basis is None:
        basis = _formant_bases[key] = torch.from_numpy(formant_basis_host(bins, order)).to(device)
    return basis


def formant_shift(logmag, ratio, order=64, hold=16, iters=2, eps=0.01, return_env=False, out=None):
    """The spectral envelope of every frame of a log-magnitude plane, re-imposed at ``ratio`` times each bin's frequency
    (pg_formant_shift): ``logmag`` (n_ch, bins, F) float32 on the device, cells within [0, 80], frames contiguous, rows F apart, the
    channel stride a whole number of rows (``pol[:, 0]`` of a polar tensor is read in place) -> (n_ch, bins, F), dense.  Per frame:
    a peak hold over ``hold`` bins on either side, a liftered cosine smoothing of ``order`` coefficients, ``iters`` repetitions of
    "smooth the maximum of the held frame and the envelope"; then out = log1p(expm1(x) a / b) with a, b = expm1 of the envelope at
    bin (k + 1) ratio - 1 and at bin k, plus ``eps``.  ratio == 1.0 returns the plane's bits; a zero cell stays +0.0.
    ``ratio`` > 1 reads the envelope higher up, i.e. moves the formants DOWN by that factor.  ``return_env``: -> (out, env), the
    envelope itself (n_ch, bins, F).  ``out``: a dense tensor to fill.  The table is built once per (device, bins, order)."""
    who = "formant_shift"
    if not (torch.is_tensor(logmag) and logmag.is_cuda and logmag.dtype == torch.float32 and logmag.dim() == 3):
        raise ValueError(f"{who}: logmag must be a 3-D float32 device tensor (n_ch, bins, F)")
    stride = _vocoder_plane(logmag, "logmag", who=who)
    n_ch, bins, F = logmag.shape
    ratio, order, hold, iters, eps = float(ratio), int(order), int(hold), int(iters), float(eps)
    if bins > _lib.FORMANT_MAX_BINS:
        raise ValueError(f"{who}: at most {_lib.FORMANT_MAX_BINS} bins, got {bins}")
    if stride % F != 0:
        raise ValueError(f"{who}: the channel stride of logmag must be a whole number of rows of {F} frames (strides {logmag.stride()})")
    if not 1 <= order <= min(bins, _lib.FORMANT_MAX_ORDER):
        raise ValueError(f"{who}: order must be within 1 .. min(bins, {_lib.FORMANT_MAX_ORDER}) = {min(bins, _lib.FORMANT_MAX_ORDER)}, got {order}")
    if not 0 <= hold <= _lib.FORMANT_MAX_HOLD:
        raise ValueError(f"{who}: hold must be within 0 .. {_lib.FORMANT_MAX_HOLD}, got {hold}")
    if not 0 <= iters <= _lib.FORMANT_MAX_ITERS:
        raise ValueError(f"{who}: iters must be within 0 .. {_lib.FORMANT_MAX_ITERS}, got {iters}")
    if not 0.25 <= ratio <= 4.0:
        raise ValueError(f"{who}: ratio must be within [0.25, 4], got {ratio}")
    if not 0.0 < eps < float("inf"):
        raise ValueError(f"{who}: eps must be finite and positive, got {eps}")
    if stride // F >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"{who}: more than 2^31 - 1 frames or rows between channels")
    out = _out(out, (n_ch, bins, F), logmag.device, who)
    a = _lib.FormantArgs()
    a.n_ch, a.bins, a.F, a.m_ch_rows = n_ch, bins, F, stride // F
    a.order, a.hold, a.iters, a.ratio, a.eps = order, hold, iters, ratio, eps
    a.M, a.basis = logmag.data_ptr(), _formant_basis(bins, order, logmag.device).data_ptr()
    a.out = _dense(out, "out")
    env = None
    if return_env:
        env = torch.empty((n_ch, bins, F), device=logmag.device, dtype=torch.float32)
        a.env = env.data_ptr()
    _lib.check(_lib.load().pg_formant_shift(C.byref(a), _stream()), who)
    return (out, env) if return_env else out


def formant_envelope(logmag, order=64, hold=16, iters=2, out=None):
    """The envelope alone (pg_formant_shift with ``env`` only): ``logmag`` as in ``formant_shift`` -> (n_ch, bins, F), dense."""
    who = "formant_envelope"
    stride = _vocoder_plane(logmag, "logmag", who=who)
    n_ch, bins, F = logmag.shape
    order, hold, iters = int(order), int(hold), int(iters)
    if bins > _lib.FORMANT_MAX_BINS or stride % F != 0 or not 1 <= order <= min(bins, _lib.FORMANT_MAX_ORDER) \
            or not 0 <= hold <= _lib.FORMANT_MAX_HOLD or not 0 <= iters <= _lib.FORMANT_MAX_ITERS or stride // F >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"{who}: arguments outside formant_shift's limits (bins {bins}, order {order}, hold {hold}, iters {iters}, strides {logmag.stride()})")
    out = _out(out, (n_ch, bins, F), logmag.device, who)
    a = _lib.FormantArgs()
    a.n_ch, a.bins, a.F, a.m_ch_rows = n_ch, bins, F, stride // F
    a.order, a.hold, a.iters, a.ratio, a.eps = order, hold, iters, 1.0, 0.01
    a.M, a.basis = logmag.data_ptr(), _formant_basis(bins, order, logmag.device).data_ptr()
    a.env = _dense(out, "out")
    _lib.check(_lib.load().pg_formant_shift(C.byref(a), _stream()), who)
    return out


_compare_ws = _StreamCache()
_caches.append(_compare_ws)


def _compare_gain(gain, n_sig, device, name):
    """None, a number, or a float64 device tensor of 1 or n_sig entries -> n_sig contiguous device doubles (or None)."""
    if gain is None:
        return None
    if not torch.is_tensor(gain):
        return torch.full((n_sig,), float(gain), dtype=torch.float64, device=device)
    if not (gain.is_cuda and gain.dtype == torch.float64 and gain.numel() in (1, n_sig)):
        raise ValueError(f"{name}: gain must be a number or a float64 device tensor of 1 or {n_sig} entries")
    _on_current_device(gain, "gain")
    return gain.reshape(-1).expand(n_sig).contiguous()


def _compare_out(out, n_sig, device, name):
    if out is None:
        return torch.empty(n_sig, 6, dtype=torch.float64, device=device)
    if not (out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (n_sig, 6) and out.is_contiguous()):
        raise ValueError(f"{name}: out must be a contiguous float64 device tensor of shape {(n_sig, 6)}")
    _on_current_device(out, "out")
    return out


def wave_compare(x, y, gain=None, out=None):
    """pg_wave_compare: x (reference) and y (estimate), (n,) or (n_signals, n) float32 device tensors of equal shape whose rows are
    contiguous (the row strides are free) -> (n_signals, 6) float64 device tensor, per row
    [sum x^2, sum y^2, sum x y, sum (x - g y)^2, max |x - g y|, number of non-finite samples] (such samples count as 0 in both).
    ``gain``: None (1.0), a number, or a float64 device tensor of one entry or one per row -- nothing is read back to the host."""
    for name, t in (("x", x), ("y", y)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() in (1, 2)):
            raise ValueError(f"wave_compare: {name} must be a 1-D or 2-D float32 device tensor")
        _on_current_device(t, name)
    if x.shape != y.shape:
        raise ValueError(f"wave_compare: shapes differ: x{tuple(x.shape)} y{tuple(y.shape)}")
    x2, y2 = (x[None], y[None]) if x.dim() == 1 else (x, y)
    n_sig, n = x2.shape
    if n_sig < 1 or n < 1:
        raise ValueError(f"wave_compare: empty input {tuple(x.shape)}")
    if n > 1 and (x2.stride(1) != 1 or y2.stride(1) != 1):
        raise ValueError("wave_compare: samples must be contiguous")
    a = _lib.WaveCompareArgs()
    a.n_signals, a.n = n_sig, n
    a.x, a.x_stride = x2.data_ptr(), (x2.stride(0) if n_sig > 1 else n)
    a.y, a.y_stride = y2.data_ptr(), (y2.stride(0) if n_sig > 1 else n)
    if a.x_stride < n or a.y_stride < n:
        raise ValueError("wave_compare: rows overlap in memory")
    g = _compare_gain(gain, n_sig, x.device, "wave_compare")
    if g is not None:
        a.gain = g.data_ptr()
    out = _compare_out(out, n_sig, x.device, "wave_compare")
    a.out = out.data_ptr()
    lib = _lib.load()
    a.workspace, a.workspace_bytes = _workspace(_compare_ws, x.device, lib.pg_workspace_bytes_wave_compare(C.byref(a)), "workspace_bytes_wave_compare")
    _lib.check(lib.pg_wave_compare(C.byref(a), _stream()), "wave_compare")
    return out


def spec_compare(R, E, gain=None, floor=1e-10, out=None):
    """pg_spec_compare: R (reference) and E (estimate) in ``stft``'s layout, (n_signals, 2, bins, frames) float32 device tensors
    (each signal dense, the signal stride free) -> (n_signals, 6) float64 device tensor, per signal [sum mR^2, sum mE0^2,
    sum mR mE0, sum (mR - g mE0)^2, sum over frames of the rms over bins of the level difference in dB, number of non-finite cells]
    with levels 10 log10(max(m^2, floor)).  ``gain`` as in ``wave_compare``."""
    for name, t in (("R", R), ("E", E)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 2):
            raise ValueError(f"spec_compare: {name} must be a float32 device tensor (n_signals, 2, bins, frames)")
        _on_current_device(t, name)
        if t.numel() == 0:
            raise ValueError(f"spec_compare: empty input {tuple(t.shape)}")
        if not t[0].is_contiguous():
            raise ValueError(f"spec_compare: every signal of {name} must be dense (strides {t.stride()})")
    if R.shape != E.shape:
        raise ValueError(f"spec_compare: shapes differ: R{tuple(R.shape)} E{tuple(E.shape)}")
    n_sig, _, bins, frames = R.shape
    a = _lib.SpecCompareArgs()
    a.n_signals, a.bins, a.frames, a.floor_power = n_sig, bins, frames, float(floor)
    a.R, a.r_stride = R.data_ptr(), (R.stride(0) if n_sig > 1 else 2 * bins * frames)
    a.E, a.e_stride = E.data_ptr(), (E.stride(0) if n_sig > 1 else 2 * bins * frames)
    if a.r_stride < 2 * bins * frames or a.e_stride < 2 * bins * frames:
        raise ValueError("spec_compare: signals overlap in memory")
    g = _compare_gain(gain, n_sig, R.device, "spec_compare")
    if g is not None:
        a.gain = g.data_ptr()
    out = _compare_out(out, n_sig, R.device, "spec_compare")
    a.out = out.data_ptr()
    lib = _lib.load()
    a.workspace, a.workspace_bytes = _workspace(_compare_ws, R.device, lib.pg_workspace_bytes_spec_compare(C.byref(a)), "workspace_bytes_spec_compare")
    _lib.check(lib.pg_spec_compare(C.byref(a), _stream()), "spec_compare")
    return out


_moments_ws = _StreamCache()
_caches.append(_moments_ws)


def moments(x, stats=None):
    """pg_moments: (mean, population std) of a dense float32 tensor, reduced in double, into the two-double device tensor ``stats``
    (allocated when None; a row of a larger float64 tensor lets a loop collect many results and read them back once)."""
    lib = _lib.load()
    ws = _moments_ws.get(x.device, lib.pg_workspace_bytes_moments)
    if stats is None:
        stats = torch.empty(2, dtype=torch.float64, device=x.device)
    elif not (stats.is_cuda and stats.dtype == torch.float64 and stats.numel() == 2 and stats.is_contiguous()):
        raise TypeError("moments: stats must be a dense device tensor of two float64 values")
    a = _lib.MomentsArgs()
    a.n, a.x, a.stats = x.numel(), _dense(x, "x"), stats.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.pg_moments(C.byref(a), _stream()), "moments")
    return stats


def standardize_(x):
    """preproc_mdb.py:182 in place on a dense float32 tensor: x = (x - x.mean()) / x.std() over the WHOLE array (population
    std, moments reduced in double).  Returns the (mean, std) device tensor (2 doubles)."""
    lib = _lib.load()
    stats = moments(x)
    _lib.check(lib.pg_standardize(C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(stats.data_ptr()), _stream()), "standardize")
    return stats


def standardize_stats_(x, stats):
    """``standardize_`` with the moments of ANOTHER reduction: x = (x - mean) / std in place with the two-double device tensor
    ``stats`` = {mean, std} (``moments`` of a part of x, say), the same pg_standardize launch.  Returns ``stats``."""
    if not (torch.is_tensor(stats) and stats.is_cuda and stats.dtype == torch.float64 and stats.numel() == 2 and stats.is_contiguous()):
        raise TypeError("standardize_stats_: stats must be a dense device tensor of two float64 values")
    _lib.check(_lib.load().pg_standardize(C.c_void_p(_dense(x, "x")), x.numel(), C.c_void_p(stats.data_ptr()), _stream()), "standardize")
    return stats


def standardize_with_(x, mean, std):
    """``standardize_`` with statistics the caller supplies -- a training set's (mean, std) applied to new audio: x = (x - mean)
    / std in place, the same pg_standardize launch (float32 arithmetic on float32(mean), float32(std)).  Returns the two-double
    device tensor it passed."""
    stats = torch.tensor([float(mean), float(std)], dtype=torch.float64).to(x.device)
    _lib.check(_lib.load().pg_standardize(C.c_void_p(_dense(x, "x")), x.numel(), C.c_void_p(stats.data_ptr()), _stream()), "standardize")
    return stats


def stft_frame_index(n_samples, n_fft, hop, device="cuda"):
    nf = 1 + n_samples // hop
    idx = torch.empty(nf, n_fft, device=device, dtype=torch.int32)
    _lib.check(_lib.load().pg_stft_frame_index(n_samples, n_fft, hop, nf, C.c_void_p(idx.data_ptr()), _stream()), "stft_frame_index")
    return idx


def polar(d, out=None, use_exp=True):
    """data.py:39-47: (N, 2, bins, frames) [re; im] -> [log1p|z| (or |z|); angle]."""
    if out is None:
        out = torch.empty_like(d)
    a = _lib.PolarArgs()
    a.n_items, a.inner = d.shape[0], d[0, 0].numel()
    a.inp, a.out = _dense(d, "d"), _dense(out, "out")
    a.use_exp = int(bool(use_exp))
    _lib.check(_lib.load().pg_polar(C.byref(a), _stream()), "polar")
    return out


_istft_ws = _StreamCache()
_caches.append(_istft_ws)


def _istft_calls(a_t, b_t, audio, hop, mode, normalize, single_frame):
    """The pg_istft_args of ops.istft's calls, one per 64 signals, each with its workspace attached (yielded one at a time: the
    workspace is the stream's cached buffer)."""
    n, bins, nf = a_t.shape
    for s0 in range(0, n, 64):
        s1 = min(n, s0 + 64)
        a = _lib.IstftArgs()
        a.n_signals, a.bins, a.n_frames, a.hop, a.mode, a.normalize = s1 - s0, bins, nf, hop, mode, int(normalize)
        a.single_frame = _tls.stft_single if single_frame is None else int(bool(single_frame))
        a.a, a.a_bs = _act3(a_t[s0:s1], "a")
        a.b, a.b_bs = _act3(b_t[s0:s1], "b")
        a.audio = audio[s0:s1].data_ptr()
        a.workspace, a.workspace_bytes = _workspace(_istft_ws, a_t.device, _lib.load().pg_workspace_bytes_istft(C.byref(a)), "workspace_bytes_istft")
        yield a


def _istft_audio(a_t, hop, out):
    n, bins, nf = a_t.shape
    if out is None:
        return torch.empty(n, hop * (nf - 1), device=a_t.device, dtype=torch.float32)
    if tuple(out.shape) != (n, hop * (nf - 1)):
        raise ValueError(f"istft: out must be {(n, hop * (nf - 1))}, got {tuple(out.shape)}")
    _dense(out, "out")
    return out


def istft(a_t, b_t, hop, mode=0, normalize=True, single_frame=None, out=None):
    """(n, bins, frames) x2 -> (n, hop*(frames-1)).  mode 0: (logmag, phase) per demo.py:39; mode 1: (re, im).
    utils.py:34-42: zero DC row, librosa.istft, peak normalisation.  ``out``: a dense (n, hop*(frames-1)) float32 tensor or view to
    fill (a view that is not 16-byte aligned takes the three-kernel path at every size: pg_istft's selection rule)."""
    audio = _istft_audio(a_t, hop, out)
    for a in _istft_calls(a_t, b_t, audio, hop, mode, normalize, single_frame):
        _lib.check(_lib.load().pg_istft(C.byref(a), _stream()), "istft")
    return audio


def istft_describe(a_t, b_t, hop, mode=0, normalize=True, single_frame=None, out=None):
    """pg_istft_describe for the arguments of ``istft``: one string per call (64 signals each), its launches joined by '|'."""
    audio = _istft_audio(a_t, hop, out)
    return [_describe(_lib.load().pg_istft_describe, a, "istft_describe")
            for a in _istft_calls(a_t, b_t, audio, hop, mode, normalize, single_frame)]


def gl_project(S, mag, x, spec_out=None):
    """utils.py:122-124: new_spec = mag * exp(1j * angle(S)) -> GEMM operand x (2*bins-2, frames) (+ [re; im] copy).
    Batched: S (n, 2, bins, frames), mag (n, bins, frames), x (n, 2*bins-2, frames), spec_out (n, 2, bins, frames)."""
    a = _lib.GlArgs()
    if mag.dim() == 3:
        a.n, a.bins, a.frames = mag.shape
        if tuple(S.shape) != (a.n, 2, a.bins, a.frames) or tuple(x.shape) != (a.n, 2 * a.bins - 2, a.frames):
            raise ValueError("gl_project: batched shapes inconsistent")
    else:
        a.bins, a.frames = mag.shape
    a.S, a.mag, a.x = _dense(S, "S"), _dense(mag, "mag"), _dense(x, "x")
    if spec_out is not None:
        if spec_out.shape != S.shape:
            raise ValueError("gl_project: spec_out must have S's shape")
        a.spec_out = _dense(spec_out, "spec_out")
    _lib.check(_lib.load().pg_gl_project(C.byref(a), _stream()), "gl_project")


_ola_ws = _StreamCache()
_caches.append(_ola_ws)


def ola_nt(frames_nt, hop, audio, normalize=False):
    """Overlap-add of (n_fft, frames)-major windowed frames (any even n_fft) into ``audio`` (hop * (frames - 1),); batched:
    frames (n, n_fft, frames) -> audio (n, hop * (frames - 1)), n <= 64, each clip normalised by its own peak."""
    a = _lib.OlaArgs()
    if frames_nt.dim() == 3:
        a.n, a.n_fft, a.frames = frames_nt.shape
        if tuple(audio.shape) != (a.n, hop * (a.frames - 1)):
            raise ValueError("ola_nt: audio must be (n, hop * (frames - 1))")
    else:
        a.n_fft, a.frames = frames_nt.shape
    a.hop, a.normalize = hop, int(normalize)
    a.fr, a.audio = _dense(frames_nt, "frames"), _dense(audio, "audio")
    ws = _ola_ws.get(audio.device, lambda: 256)
    a.workspace, a.workspace_bytes = ws.data_ptr(), 256
    _lib.check(_lib.load().pg_ola_nt(C.byref(a), _stream()), "ola_nt")
    return audio
