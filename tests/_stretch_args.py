"""The bad-argument table of the stretched-plane calls, pg_phase_vocoder and pg_phase_lock: both validate through one host checker
(csrc/pg_track.h: pg_stretch_check), so ONE table of bad inputs runs through both entry points (tests/test_vocoder_host.py,
tests/test_lock_host.py).  Every case is refused before any launch; the pointers are fake and never dereferenced.  What is not
common stays with its own test: M == NULL (optional in the one, required in the other), 4097 bins and the workspace."""
import ctypes

ENTRIES = {"pg_phase_vocoder": "PhaseVocoderArgs", "pg_phase_lock": "PhaseLockArgs"}


def args(_lib, entry):
    """2 channels of 5 bins, 19 source frames -> 25 output frames."""
    a = getattr(_lib, ENTRIES[entry])()
    a.n_ch, a.bins, a.F_src, a.F_out, a.src_per_out, a.reset_below = 2, 5, 19, 25, 0.75, 0.05
    a.A = a.M = a.out = 4096
    a.a_stride = a.m_stride = 5 * 19
    if entry == "pg_phase_lock":
        a.workspace, a.workspace_bytes = 4096, 1 << 20
    return a


def _set(**fields):
    def change(a):
        for k, v in fields.items():
            setattr(a, k, v)
    return change


def table(_lib):
    """(label, change(args), expected code, a word of the message) per bad input."""
    t = []
    t += [(f"{f} NULL", _set(**{f: None}), _lib.ERR_NULL, b"required") for f in ("A", "out")]
    t += [(f"{f} = {bad}", _set(**{f: bad}), _lib.ERR_SHAPE, b"non-positive") for f in ("n_ch", "bins", "F_src", "F_out") for bad in (0, -3)]
    t += [(f"src_per_out = {bad}", _set(src_per_out=bad), _lib.ERR_SHAPE, b"src_per_out")
          for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan"))]
    t += [(f"reset_below = {bad}", _set(reset_below=bad), _lib.ERR_SHAPE, b"reset_below")
          for bad in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan"))]
    t += [(f"{f} short", _set(**{f: 5 * 19 - 1}), _lib.ERR_SHAPE, f.encode()) for f in ("a_stride", "m_stride")]
    t += [(f"{f} + {off}", _set(**{f: 4096 + off}), _lib.ERR_ALIGN, b"misaligned") for f in ("A", "M", "out") for off in (1, 2, 3)]
    t += [("2^62 elements", _set(n_ch=1 << 30, bins=4096, F_out=1 << 62, a_stride=4096 * 19, m_stride=4096 * 19), _lib.ERR_SHAPE, b"2^62")]
    return t


def run(_lib, entry):
    """Runs the table through `entry`, asserts each case's code, message word and `entry`'s own prefix -> {label: code}."""
    lib = _lib.load()
    f = getattr(lib, entry)
    assert f(None, None) == _lib.ERR_NULL
    got = {}
    for label, change, code, word in table(_lib):
        a = args(_lib, entry)
        change(a)
        got[label] = f(ctypes.byref(a), None)
        msg = lib.pg_last_error_string()
        assert got[label] == code and word in msg and msg.startswith(entry[3:].encode() + b": "), (entry, label, got[label], msg)
    return got


def run_both(_lib):
    """The table through both entry points: each reports what the table says, and the two report the same code for the same input."""
    v, k = run(_lib, "pg_phase_vocoder"), run(_lib, "pg_phase_lock")
    assert len(v) == len(table(_lib)) == 2 + 8 + 5 + 5 + 2 + 9 + 1 and v == k, {c: (v[c], k[c]) for c in v if v[c] != k[c]}
    return v
