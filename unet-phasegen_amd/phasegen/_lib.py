"""ctypes binding of libphasegen.so (the C ABI declared in include/phasegen.h).

The library is the product: there is no CPU or eager-PyTorch fallback.  If the shared object is missing or a
symbol cannot be resolved, importing the ops raises; if a call returns non-zero, ``check`` raises RuntimeError
with ``pg_last_error_string()`` (the reference's error convention is Python exceptions).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libphasegen.so")
ABI_VERSION = 400     # include/phasegen.h PG_VERSION these struct layouts were written against (argument structs grow between minor versions)

ACT_NONE, ACT_LEAKY, ACT_RELU = 0, 1, 2
PREC_FP32, PREC_BF16, PREC_BF16X3 = 0, 1, 2           # pg_conv_args.precision
OK, ERR_NULL, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3, -4, -5   # return codes (PG_ERR_*)
OP_CONV1D_FWD, OP_CONV1D_DGRAD, OP_CONV1D_WGRAD, OP_CONVT1D_FWD, OP_CONVT1D_DGRAD, OP_CONVT1D_WGRAD = range(6)   # pg_conv_describe
SCHED_AUTO, SCHED_TILE_PER_WG, SCHED_FORCE_STREAMK, SCHED_NO_RAW, SCHED_NO_TALL, SCHED_CONTENDED = 0, 1, 2, 4, 8, 16   # pg_conv_args.schedule bits
SCHED_NO_PS = 128      # wgrad: keep the flat-K raw kernel (no per-sample slabs)
SCHED_NO_RAW3 = 0x2000  # fp32 F / T: never the one-wave-per-SIMD kernels (conv_raw3.hip)
SCHED_ALL_RAW3 = 0x4000  # ... those kernels wherever they cover the problem (also the F form of k = 32, which auto leaves on the older ones)
SCHED_NO_COLSPLIT = 0x20000  # fp32 F / T on conv_raw3: keep the columns past the last full 256-wide tile in the same launch (no tail launch)
SCHED_COLSPLIT = 0x40000     # ... or always hand them to the tail launch where the geometry allows (tests; the automatic choice prices the tail)


def SCHED_SLOTS(n):
    """PG_SCHED_SLOTS(n), schedule bits 19-23: plan the call as if the device had n = 1..31 compute units (0: the device's own count)"""
    if not 0 <= n <= 31:
        raise ValueError("SCHED_SLOTS: n must be 0..31")
    return n << 19


RS_KAISER_BEST, RS_KAISER_FAST = 0, 1     # pg_resample_args.quality (PG_RS_*)
# (pg_convh_args.schedule bits 5-6 selected tile families that ABI 0.4 removed; bit 12, the surviving conv_h3 family, is a no-op)

c_float_p = C.c_void_p  # device pointers travel as integers


class ConvArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("Lin", C.c_int32), ("Lout", C.c_int32),
                ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
                ("x", C.c_void_p), ("x_bs", C.c_int64), ("x_act", C.c_int32), ("precision", C.c_int32),
                ("w", C.c_void_p),
                ("y", C.c_void_p), ("y_bs", C.c_int64),
                ("dy", C.c_void_p), ("dy_bs", C.c_int64),
                ("dx", C.c_void_p), ("dx_bs", C.c_int64),
                ("dx_add", C.c_void_p), ("dx_add_bs", C.c_int64),
                ("dx_ref", C.c_void_p), ("dx_ref_bs", C.c_int64),
                ("dx_mask", C.c_int32), ("schedule", C.c_int32),
                ("dw", C.c_void_p), ("y_act", C.c_int32), ("y2_act", C.c_int32), ("y2", C.c_void_p), ("y2_bs", C.c_int64),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("adam", C.c_void_p)]        # const pg_adam_args*: optimiser step fused into the wgrad epilogue (or NULL)


class BnArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("eps", C.c_float), ("momentum", C.c_float),
                ("x", C.c_void_p), ("x_bs", C.c_int64), ("y", C.c_void_p), ("y_bs", C.c_int64),
                ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("save_mean", C.c_void_p), ("save_invstd", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("dy", C.c_void_p), ("dy_bs", C.c_int64), ("dx", C.c_void_p), ("dx_bs", C.c_int64),
                ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("y_act", C.c_int32), ("y2_act", C.c_int32), ("y2", C.c_void_p), ("y2_bs", C.c_int64),
                ("yh", C.c_void_p), ("yh_bs", C.c_int64), ("yh_pitch", C.c_int32), ("yh_act", C.c_int32),
                ("yh2", C.c_void_p), ("yh2_bs", C.c_int64), ("yh2_pitch", C.c_int32), ("yh2_act", C.c_int32),
                ("num_batches_tracked", C.c_void_p)]


class ClipNormArgs(C.Structure):
    """pg_clipnorm_args: BatchNorm forward with per-clip statistics (include/phasegen.h)."""
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("eps", C.c_float), ("momentum", C.c_float), ("_pad0", C.c_int32),
                ("x", C.c_void_p), ("x_bs", C.c_int64), ("y", C.c_void_p), ("y_bs", C.c_int64), ("y2", C.c_void_p), ("y2_bs", C.c_int64),
                ("y_act", C.c_int32), ("y2_act", C.c_int32),
                ("yh", C.c_void_p), ("yh_bs", C.c_int64), ("yh_pitch", C.c_int32), ("yh_act", C.c_int32),
                ("yh2", C.c_void_p), ("yh2_bs", C.c_int64), ("yh2_pitch", C.c_int32), ("yh2_act", C.c_int32),
                ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("save_mean", C.c_void_p), ("save_invstd", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("num_batches_tracked", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class ConvhArgs(C.Structure):
    """pg_convh_args: bf16-resident forward conv / transposed conv (include/phasegen.h)."""
    _fields_ = [("B", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("Lin", C.c_int32), ("Lout", C.c_int32),
                ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("transposed", C.c_int32), ("schedule", C.c_int32),
                ("x", C.c_void_p), ("x_bs", C.c_int64), ("x_pitch", C.c_int32), ("_pad0", C.c_int32),
                ("w", C.c_void_p), ("y", C.c_void_p), ("y_bs", C.c_int64),
                ("yh", C.c_void_p), ("yh_bs", C.c_int64), ("yh_pitch", C.c_int32), ("yh_act", C.c_int32),
                ("yh2", C.c_void_p), ("yh2_bs", C.c_int64), ("yh2_pitch", C.c_int32), ("yh2_act", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class CastArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("pitch", C.c_int32), ("act", C.c_int32), ("_pad0", C.c_int32),
                ("x", C.c_void_p), ("x_bs", C.c_int64), ("y", C.c_void_p), ("y_bs", C.c_int64)]


class LossArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("mag_weight", C.c_float),
                ("pred", C.c_void_p), ("batch", C.c_void_p), ("dpred", C.c_void_p), ("losses", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class AdamArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("grad_scale", C.c_double), ("step", C.c_int32), ("thin", C.c_int32)]


class StftArgs(C.Structure):
    _fields_ = [("n_signals", C.c_int32), ("n_samples", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32),
                ("n_frames", C.c_int32), ("polar", C.c_int32), ("single_frame", C.c_int32), ("_pad0", C.c_int32),
                ("y", C.c_void_p), ("out", C.c_void_p),
                ("chunk_start", C.c_void_p), ("chunk_row", C.c_void_p), ("src_len", C.c_int64), ("src_stride", C.c_int64)]


class StftCropsArgs(C.Structure):
    """pg_stft_crops_args: STFT of crops of one flat buffer, fused with standardisation and polar (include/phasegen.h)."""
    _fields_ = [("n_signals", C.c_int32), ("n_samples", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32),
                ("n_frames", C.c_int32), ("polar", C.c_int32), ("single_frame", C.c_int32), ("_pad0", C.c_int32),
                ("src", C.c_void_p), ("crop_begin", C.c_void_p), ("crop_end", C.c_void_p), ("stats", C.c_void_p),
                ("out", C.c_void_p)]


class MomentsArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("x", C.c_void_p), ("stats", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


class PolarArgs(C.Structure):
    _fields_ = [("n_items", C.c_int64), ("inner", C.c_int64), ("inp", C.c_void_p), ("out", C.c_void_p),
                ("use_exp", C.c_int32), ("_pad0", C.c_int32)]


class IstftArgs(C.Structure):
    _fields_ = [("n_signals", C.c_int32), ("bins", C.c_int32), ("n_frames", C.c_int32), ("hop", C.c_int32),
                ("mode", C.c_int32), ("normalize", C.c_int32), ("single_frame", C.c_int32), ("_pad0", C.c_int32),
                ("a", C.c_void_p), ("a_bs", C.c_int64), ("b", C.c_void_p), ("b_bs", C.c_int64),
                ("audio", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class GlArgs(C.Structure):
    _fields_ = [("bins", C.c_int32), ("frames", C.c_int32), ("S", C.c_void_p), ("mag", C.c_void_p), ("x", C.c_void_p),
                ("spec_out", C.c_void_p), ("n", C.c_int32), ("_pad0", C.c_int32)]


class OlaArgs(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("frames", C.c_int32), ("hop", C.c_int32), ("normalize", C.c_int32),
                ("fr", C.c_void_p), ("audio", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("n", C.c_int32), ("_pad0", C.c_int32)]


class ResampleArgs(C.Structure):
    """pg_resample_args: sample-rate conversion by up / down (include/phasegen.h)."""
    _fields_ = [("n_signals", C.c_int32), ("up", C.c_int32), ("down", C.c_int32), ("quality", C.c_int32),
                ("n_in", C.c_int64), ("n_out", C.c_int64),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("y", C.c_void_p), ("y_stride", C.c_int64),
                ("bank", C.c_void_p)]


class StitchArgs(C.Structure):
    """pg_stitch_args: crossfaded overlap-add of equal-length clips into tracks (include/phasegen.h)."""
    _fields_ = [("n_tracks", C.c_int32), ("n_clips", C.c_int32), ("clip_len", C.c_int32), ("step", C.c_int32),
                ("n_out", C.c_int64),
                ("clips", C.c_void_p), ("clip_stride", C.c_int64), ("track_stride", C.c_int64),
                ("out", C.c_void_p), ("out_stride", C.c_int64),
                ("ramp", C.c_void_p), ("normalize", C.c_int32), ("_pad0", C.c_int32),
                ("peak", C.c_void_p), ("n_nonfinite", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class SpecClipsArgs(C.Structure):
    """pg_spec_clips_args: clip windows of a spectrogram plane, optionally resampled along time (include/phasegen.h)."""
    _fields_ = [("n_clips", C.c_int32), ("n_ch", C.c_int32), ("bins", C.c_int32), ("frames", C.c_int32),
                ("sf", C.c_int32), ("_pad0", C.c_int32), ("F_src", C.c_int64), ("src_per_out", C.c_double),
                ("P", C.c_void_p), ("p_stride", C.c_int64), ("out", C.c_void_p)]


class PhaseJoinArgs(C.Structure):
    """pg_phase_join_args: one phase per global frame from the phases of overlapped clips (include/phasegen.h)."""
    _fields_ = [("n_clips", C.c_int32), ("n_ch", C.c_int32), ("bins", C.c_int32), ("frames", C.c_int32),
                ("sf", C.c_int32), ("_pad0", C.c_int32),
                ("phi", C.c_void_p), ("clip_stride", C.c_int64), ("ch_stride", C.c_int64), ("row_pitch", C.c_int64),
                ("out", C.c_void_p), ("ramp", C.c_void_p)]


class PhaseVocoderArgs(C.Structure):
    """pg_phase_vocoder_args: the phase-vocoder phase of a time-stretched spectrogram (include/phasegen.h)."""
    _fields_ = [("n_ch", C.c_int32), ("bins", C.c_int32), ("F_src", C.c_int64), ("F_out", C.c_int64),
                ("src_per_out", C.c_double), ("reset_below", C.c_float), ("_pad0", C.c_int32),
                ("A", C.c_void_p), ("a_stride", C.c_int64), ("M", C.c_void_p), ("m_stride", C.c_int64), ("out", C.c_void_p)]


class PhaseLockArgs(C.Structure):
    """pg_phase_lock_args: the phase-vocoder phase with identity phase locking (include/phasegen.h)."""
    _fields_ = PhaseVocoderArgs._fields_ + [("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class PhaseLockLinkedArgs(C.Structure):
    """pg_phase_lock_linked_args: identity phase locking with ONE rotation, the reference plane's, for all channels (include/phasegen.h)."""
    _fields_ = [("n_ch", C.c_int32), ("bins", C.c_int32), ("F_src", C.c_int64), ("F_out", C.c_int64),
                ("src_per_out", C.c_double), ("reset_below", C.c_float), ("_pad0", C.c_int32),
                ("A", C.c_void_p), ("a_stride", C.c_int64), ("Aref", C.c_void_p), ("Mref", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class PhaseSpsiArgs(C.Structure):
    """pg_phase_spsi_args: a phase from the magnitudes alone, single-pass spectrogram inversion (include/phasegen.h)."""
    _fields_ = [("n_ch", C.c_int32), ("bins", C.c_int32), ("F", C.c_int64), ("n_fft", C.c_int32), ("hop", C.c_int32),
                ("bin0", C.c_int32), ("_pad0", C.c_int32), ("M", C.c_void_p), ("m_stride", C.c_int64), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


HPSS_MAX_WIN = 31     # PG_HPSS_MAX_WIN


class HpssArgs(C.Structure):
    """pg_hpss_args: harmonic / percussive split of a log-magnitude plane by median filtering (include/phasegen.h)."""
    _fields_ = [("n_ch", C.c_int32), ("bins", C.c_int32), ("F", C.c_int64), ("win_t", C.c_int32), ("win_f", C.c_int32),
                ("M", C.c_void_p), ("m_stride", C.c_int64), ("harm", C.c_void_p), ("perc", C.c_void_p)]


class OlaStretchArgs(C.Structure):
    """pg_ola_stretch_args: time-domain overlap-add of a short window at a time ratio (include/phasegen.h)."""
    _fields_ = [("n_sig", C.c_int32), ("win_len", C.c_int32), ("hop", C.c_int32), ("_pad0", C.c_int32),
                ("n_in", C.c_int64), ("n_out", C.c_int64), ("src_per_out", C.c_double),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("win", C.c_void_p),
                ("base", C.c_void_p), ("base_stride", C.c_int64), ("y", C.c_void_p), ("y_stride", C.c_int64)]


FORMANT_MAX_BINS, FORMANT_MAX_ORDER, FORMANT_MAX_HOLD, FORMANT_MAX_ITERS = 4096, 64, 64, 16     # pg_formant_shift's limits


class FormantArgs(C.Structure):
    """pg_formant_args: the spectral envelope of a log-magnitude plane, optionally re-imposed at a frequency ratio (include/phasegen.h).
    No 64-bit field: every size is an int32 and the channel stride is a count of rows."""
    _fields_ = [("n_ch", C.c_int32), ("bins", C.c_int32), ("F", C.c_int32), ("m_ch_rows", C.c_int32),
                ("order", C.c_int32), ("hold", C.c_int32), ("iters", C.c_int32), ("_pad0", C.c_int32),
                ("ratio", C.c_double), ("eps", C.c_float), ("_pad1", C.c_float),
                ("M", C.c_void_p), ("basis", C.c_void_p), ("env", C.c_void_p), ("out", C.c_void_p)]


class SpecClipsMapArgs(C.Structure):
    """pg_spec_clips_map_args: pg_spec_clips over a table of source-frame positions (include/phasegen.h).  No 64-bit integer field:
    every size is an int32 and the channel stride is a count of rows."""
    _fields_ = [("n_clips", C.c_int32), ("n_ch", C.c_int32), ("bins", C.c_int32), ("frames", C.c_int32),
                ("sf", C.c_int32), ("F_src", C.c_int32), ("p_ch_rows", C.c_int32), ("_pad0", C.c_int32),
                ("pos", C.c_void_p), ("P", C.c_void_p), ("out", C.c_void_p)]


class PhaseVocoderMapArgs(C.Structure):
    """pg_phase_vocoder_map_args: pg_phase_vocoder over a table of source-frame positions (include/phasegen.h)."""
    _fields_ = [("n_ch", C.c_int32), ("bins", C.c_int32), ("F_src", C.c_int32), ("F_out", C.c_int32),
                ("reset_below", C.c_float), ("a_ch_rows", C.c_int32), ("m_ch_rows", C.c_int32), ("_pad0", C.c_int32),
                ("pos", C.c_void_p), ("A", C.c_void_p), ("M", C.c_void_p), ("out", C.c_void_p)]


class PhaseLockMapArgs(C.Structure):
    """pg_phase_lock_map_args: pg_phase_lock over a table of source-frame positions (include/phasegen.h)."""
    _fields_ = PhaseVocoderMapArgs._fields_ + [("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class PhaseLockLinkedMapArgs(C.Structure):
    """pg_phase_lock_linked_map_args: pg_phase_lock_linked over a table of source-frame positions (include/phasegen.h)."""
    _fields_ = [("n_ch", C.c_int32), ("bins", C.c_int32), ("F_src", C.c_int32), ("F_out", C.c_int32),
                ("reset_below", C.c_float), ("a_ch_rows", C.c_int32), ("_pad0", C.c_int32), ("_pad1", C.c_int32),
                ("pos", C.c_void_p), ("A", C.c_void_p), ("Aref", C.c_void_p), ("Mref", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class OlaStretchMapArgs(C.Structure):
    """pg_ola_stretch_map_args: pg_ola_stretch with one source centre per grain (include/phasegen.h)."""
    _fields_ = [("n_sig", C.c_int32), ("win_len", C.c_int32), ("hop", C.c_int32), ("n_in", C.c_int32),
                ("n_out", C.c_int32), ("x_stride", C.c_int32), ("base_stride", C.c_int32), ("y_stride", C.c_int32),
                ("pos", C.c_void_p), ("x", C.c_void_p), ("win", C.c_void_p), ("base", C.c_void_p), ("y", C.c_void_p)]


VARISPEED_MAX_ZEROS, VARISPEED_MAX_PER_ZERO, VARISPEED_MAX_STEP = 64, 512, 4096     # pg_varispeed's limits


class VarispeedArgs(C.Structure):
    """pg_varispeed_args: band-limited resampling along a table of source positions and bandwidths (include/phasegen.h).  No 64-bit
    integer field: every size is an int32 and the row strides are counts of samples."""
    _fields_ = [("n_sig", C.c_int32), ("n_in", C.c_int32), ("n_out", C.c_int32), ("step", C.c_int32),
                ("zeros", C.c_int32), ("per_zero", C.c_int32), ("x_stride", C.c_int32), ("y_stride", C.c_int32),
                ("pos", C.c_void_p), ("scale", C.c_void_p), ("table", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p)]


PITCH_MIN_WINDOW, PITCH_MAX_WINDOW, PITCH_MIN_TAU, PITCH_MAX_TAU = 4, 2048, 2, 1024     # pg_pitch_track's limits


class PitchTrackArgs(C.Structure):
    """pg_pitch_track_args: YIN per frame -- the period and the aperiodicity of every frame of every row (include/phasegen.h).  No
    64-bit integer field and no workspace: every size is an int32 and the strides are counts of elements."""
    _fields_ = [("n_sig", C.c_int32), ("n_in", C.c_int32), ("frames", C.c_int32), ("hop", C.c_int32),
                ("window", C.c_int32), ("tau_min", C.c_int32), ("tau_max", C.c_int32),
                ("x_stride", C.c_int32), ("out_stride", C.c_int32), ("threshold", C.c_float),
                ("x", C.c_void_p), ("period", C.c_void_p), ("ap", C.c_void_p)]


class WaveCompareArgs(C.Structure):
    """pg_wave_compare_args: six sums per signal of a reference / estimate pair of waveforms (include/phasegen.h)."""
    _fields_ = [("n_signals", C.c_int32), ("_pad0", C.c_int32), ("n", C.c_int64),
                ("x", C.c_void_p), ("x_stride", C.c_int64), ("y", C.c_void_p), ("y_stride", C.c_int64),
                ("gain", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class SpecCompareArgs(C.Structure):
    """pg_spec_compare_args: six sums per signal of a reference / estimate pair of spectrograms (include/phasegen.h)."""
    _fields_ = [("n_signals", C.c_int32), ("bins", C.c_int32), ("frames", C.c_int32), ("floor_power", C.c_float),
                ("R", C.c_void_p), ("r_stride", C.c_int64), ("E", C.c_void_p), ("e_stride", C.c_int64),
                ("gain", C.c_void_p), ("out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


# every symbol include/phasegen.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "pg_conv1d_fwd": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "pg_conv1d_dgrad": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "pg_conv1d_wgrad": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "pg_convt1d_fwd": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "pg_convt1d_dgrad": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "pg_convt1d_wgrad": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "pg_conv_describe": (C.c_int, [C.POINTER(ConvArgs), C.c_int32, C.c_char_p, C.c_int32]),
    "pg_conv_fwd_h": (C.c_int, [C.POINTER(ConvhArgs), C.c_void_p]),
    "pg_conv_fwd_h_supported": (C.c_int, [C.POINTER(ConvhArgs)]),
    "pg_workspace_bytes_moments": (C.c_int64, []),
    "pg_moments": (C.c_int, [C.POINTER(MomentsArgs), C.c_void_p]),
    "pg_standardize": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "pg_shadow_elems": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "pg_shadow_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "pg_cast_rows_bf16": (C.c_int, [C.POINTER(CastArgs), C.c_void_p]),
    "pg_workspace_bytes_conv": (C.c_int64, []),
    "pg_workspace_bytes_wgrad": (C.c_int64, [C.POINTER(ConvArgs), C.c_int32]),
    "pg_bn_fwd": (C.c_int, [C.POINTER(BnArgs), C.c_void_p]),
    "pg_bn_bwd": (C.c_int, [C.POINTER(BnArgs), C.c_void_p]),
    "pg_workspace_bytes_clipnorm": (C.c_int64, [C.POINTER(ClipNormArgs)]),
    "pg_clipnorm_fwd": (C.c_int, [C.POINTER(ClipNormArgs), C.c_void_p]),
    "pg_workspace_bytes_loss": (C.c_int64, [C.POINTER(LossArgs)]),
    "pg_loss_fwd_bwd": (C.c_int, [C.POINTER(LossArgs), C.c_void_p]),
    "pg_adam_step": (C.c_int, [C.POINTER(AdamArgs), C.c_void_p]),
    "pg_stft": (C.c_int, [C.POINTER(StftArgs), C.c_void_p]),
    "pg_stft_describe": (C.c_int, [C.POINTER(StftArgs), C.c_char_p, C.c_int32]),
    "pg_stft_crops": (C.c_int, [C.POINTER(StftCropsArgs), C.c_void_p]),
    "pg_stft_crops_describe": (C.c_int, [C.POINTER(StftCropsArgs), C.c_char_p, C.c_int32]),
    "pg_stft_frame_index": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "pg_polar": (C.c_int, [C.POINTER(PolarArgs), C.c_void_p]),
    "pg_workspace_bytes_istft": (C.c_int64, [C.POINTER(IstftArgs)]),
    "pg_istft": (C.c_int, [C.POINTER(IstftArgs), C.c_void_p]),
    "pg_istft_describe": (C.c_int, [C.POINTER(IstftArgs), C.c_char_p, C.c_int32]),
    "pg_gl_project": (C.c_int, [C.POINTER(GlArgs), C.c_void_p]),
    "pg_ola_nt": (C.c_int, [C.POINTER(OlaArgs), C.c_void_p]),
    "pg_resample_out_len": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "pg_resample_taps": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "pg_resample_bank_elems": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "pg_resample_bank": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "pg_resample": (C.c_int, [C.POINTER(ResampleArgs), C.c_void_p]),
    "pg_stitch_ramp": (C.c_int, [C.c_void_p, C.c_int32]),
    "pg_workspace_bytes_stitch": (C.c_int64, [C.POINTER(StitchArgs)]),
    "pg_stitch": (C.c_int, [C.POINTER(StitchArgs), C.c_void_p]),
    "pg_spec_clips": (C.c_int, [C.POINTER(SpecClipsArgs), C.c_void_p]),
    "pg_phase_join": (C.c_int, [C.POINTER(PhaseJoinArgs), C.c_void_p]),
    "pg_phase_vocoder": (C.c_int, [C.POINTER(PhaseVocoderArgs), C.c_void_p]),
    "pg_workspace_bytes_phase_lock": (C.c_int64, [C.POINTER(PhaseLockArgs)]),
    "pg_phase_lock": (C.c_int, [C.POINTER(PhaseLockArgs), C.c_void_p]),
    "pg_workspace_bytes_phase_lock_linked": (C.c_int64, [C.POINTER(PhaseLockLinkedArgs)]),
    "pg_phase_lock_linked": (C.c_int, [C.POINTER(PhaseLockLinkedArgs), C.c_void_p]),
    "pg_workspace_bytes_phase_spsi": (C.c_int64, [C.POINTER(PhaseSpsiArgs)]),
    "pg_phase_spsi": (C.c_int, [C.POINTER(PhaseSpsiArgs), C.c_void_p]),
    "pg_hpss": (C.c_int, [C.POINTER(HpssArgs), C.c_void_p]),
    "pg_ola_stretch": (C.c_int, [C.POINTER(OlaStretchArgs), C.c_void_p]),
    "pg_ola_window": (C.c_int, [C.c_void_p, C.c_int32]),
    "pg_formant_shift": (C.c_int, [C.POINTER(FormantArgs), C.c_void_p]),
    "pg_formant_basis_elems": (C.c_int64, [C.c_int32, C.c_int32]),
    "pg_formant_basis": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "pg_spec_clips_map": (C.c_int, [C.POINTER(SpecClipsMapArgs), C.c_void_p]),
    "pg_phase_vocoder_map": (C.c_int, [C.POINTER(PhaseVocoderMapArgs), C.c_void_p]),
    "pg_workspace_bytes_phase_lock_map": (C.c_int64, [C.POINTER(PhaseLockMapArgs)]),
    "pg_phase_lock_map": (C.c_int, [C.POINTER(PhaseLockMapArgs), C.c_void_p]),
    "pg_workspace_bytes_phase_lock_linked_map": (C.c_int64, [C.POINTER(PhaseLockLinkedMapArgs)]),
    "pg_phase_lock_linked_map": (C.c_int, [C.POINTER(PhaseLockLinkedMapArgs), C.c_void_p]),
    "pg_ola_stretch_map": (C.c_int, [C.POINTER(OlaStretchMapArgs), C.c_void_p]),
    "pg_varispeed_table_elems": (C.c_int64, [C.c_int32, C.c_int32]),
    "pg_varispeed_table": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double]),
    "pg_varispeed": (C.c_int, [C.POINTER(VarispeedArgs), C.c_void_p]),
    "pg_pitch_track": (C.c_int, [C.POINTER(PitchTrackArgs), C.c_void_p]),
    "pg_workspace_bytes_wave_compare": (C.c_int64, [C.POINTER(WaveCompareArgs)]),
    "pg_wave_compare": (C.c_int, [C.POINTER(WaveCompareArgs), C.c_void_p]),
    "pg_workspace_bytes_spec_compare": (C.c_int64, [C.POINTER(SpecCompareArgs)]),
    "pg_spec_compare": (C.c_int, [C.POINTER(SpecCompareArgs), C.c_void_p]),
    "pg_fill": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "pg_conv_fwd_h_describe": (C.c_int, [C.POINTER(ConvhArgs), C.c_char_p, C.c_int32]),
    "pg_version": (C.c_int, []),
    "pg_last_error_string": (C.c_char_p, []),
}

_lib = None


def load():
    """Load libphasegen.so and bind every declared symbol.  Raises if anything is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `make -C unet-phasegen_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback for the phasegen hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.pg_version() // 100 != ABI_VERSION // 100:
        raise RuntimeError(f"{LIB_PATH} is ABI {lib.pg_version()}, this binding was written against {ABI_VERSION}: rebuild the library "
                           "(`make -C unet-phasegen_amd/csrc`)")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().pg_last_error_string()
        raise RuntimeError(f"libphasegen {what} failed: {msg.decode() if msg else rc}")
