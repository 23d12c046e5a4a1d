"""The bad-argument table of the stretched-plane calls: pg_phase_vocoder, pg_phase_lock and pg_phase_lock_linked, each with its mapped
twin.  All six validate through one host checker (csrc/pg_track.h: pg_stretch_check), so ONE table of bad inputs runs through all six
entry points (tests/test_vocoder_host.py, tests/test_lock_host.py).  A case names its field abstractly -- "stride A" is a_stride in a
uniform struct and a_ch_rows in a mapped one, "M" is Mref in a linked one -- and ``concrete`` turns it into the entry's own field.
Every case is refused before any launch; the pointers are fake and never dereferenced.  What is not common stays with its own test:
M == NULL (optional in the one, required in the others), 4097 bins and the workspace."""
import ctypes

# entry point -> (struct, mapped, linked)
ENTRIES = {"pg_phase_vocoder": ("PhaseVocoderArgs", False, False), "pg_phase_vocoder_map": ("PhaseVocoderMapArgs", True, False),
           "pg_phase_lock": ("PhaseLockArgs", False, False), "pg_phase_lock_map": ("PhaseLockMapArgs", True, False),
           "pg_phase_lock_linked": ("PhaseLockLinkedArgs", False, True), "pg_phase_lock_linked_map": ("PhaseLockLinkedMapArgs", True, True)}
TWINS = [(e, e + "_map") for e in ("pg_phase_vocoder", "pg_phase_lock", "pg_phase_lock_linked")]
BINS, F_SRC = 5, 19
SHORT = "one element (uniform) or one row (mapped) short of a plane"


def concrete(entry, field, value=None):
    """the abstract ``field`` of a case as ``entry``'s struct names it (None: the struct has no such field) and its value"""
    _cls, mapped, linked = ENTRIES[entry]
    if field in ("stride A", "stride M"):
        if linked and field == "stride M":
            return None, None
        name = field[-1].lower() + ("_ch_rows" if mapped else "_stride")
        return name, ((BINS - 1 if mapped else BINS * F_SRC - 1) if value is SHORT else value)
    if field == "M" and linked:
        return "Mref", value
    return field, value


def args(_lib, entry):
    """2 channels of 5 bins, 19 source frames -> 25 output frames."""
    cls, mapped, linked = ENTRIES[entry]
    a = getattr(_lib, cls)()
    a.n_ch, a.bins, a.F_src, a.F_out, a.reset_below = 2, BINS, F_SRC, 25, 0.05
    a.A = a.out = 4096
    for f in (("Aref", "Mref") if linked else ("M",)) + (("pos",) if mapped else ()):
        setattr(a, f, 4096)
    for f in ("stride A", "stride M"):
        name, _ = concrete(entry, f)
        if name:
            setattr(a, name, BINS if mapped else BINS * F_SRC)
    if not mapped:
        a.src_per_out = 0.75
    if "lock" in entry:
        a.workspace, a.workspace_bytes = 4096, 1 << 20
    return a


def table(_lib):
    """(label, {abstract field: value}, expected code, a word of the message or the abstract field the message names, who runs it)
    per bad input.  who: None (all six), "uniform", "mapped", or "own M" (the entries whose M has a stride of its own)."""
    t = []
    t += [(f"{f} NULL", {f: None}, _lib.ERR_NULL, b"required", None) for f in ("A", "out")]
    t += [(f"{f} = {bad}", {f: bad}, _lib.ERR_SHAPE, b"non-positive", None) for f in ("n_ch", "bins", "F_src", "F_out") for bad in (0, -3)]
    t += [(f"src_per_out = {bad}", dict(src_per_out=bad), _lib.ERR_SHAPE, b"src_per_out", "uniform")
          for bad in (0.0, -0.5, float("inf"), float("-inf"), float("nan"))]
    t += [(f"reset_below = {bad}", dict(reset_below=bad), _lib.ERR_SHAPE, b"reset_below", None)
          for bad in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan"))]
    t += [(f"{f} short", {f: SHORT}, _lib.ERR_SHAPE, f, who) for f, who in (("stride A", None), ("stride M", "own M"))]
    t += [(f"{f} + {off}", {f: 4096 + off}, _lib.ERR_ALIGN, b"misaligned", None) for f in ("A", "M", "out") for off in (1, 2, 3)]
    t += [("2^62 elements", {"n_ch": 1 << 30, "bins": 4096, "F_out": 1 << 62, "stride A": 4096 * F_SRC, "stride M": 4096 * F_SRC},
           _lib.ERR_SHAPE, b"2^62", "uniform")]
    t += [("pos NULL", dict(pos=None), _lib.ERR_NULL, b"pos required", "mapped")]
    t += [(f"pos + {off}", dict(pos=4096 + off), _lib.ERR_ALIGN, b"misaligned", "mapped") for off in (1, 2, 4, 7)]
    return t


def runs(entry, who):
    _cls, mapped, linked = ENTRIES[entry]
    return {None: True, "uniform": not mapped, "mapped": mapped, "own M": not linked}[who]


def run(_lib, entry):
    """Runs `entry`'s share of the table through it, asserts each case's code, message word and `entry`'s own prefix -> {label: code}."""
    lib = _lib.load()
    f = getattr(lib, entry)
    assert f(None, None) == _lib.ERR_NULL
    got = {}
    for label, change, code, word, who in table(_lib):
        if not runs(entry, who):
            continue
        a = args(_lib, entry)
        for field, value in change.items():
            name, value = concrete(entry, field, value)
            if name:
                setattr(a, name, value)
        if isinstance(word, str):
            word = concrete(entry, word)[0].encode()
        got[label] = f(ctypes.byref(a), None)
        msg = lib.pg_last_error_string()
        assert got[label] == code and word in msg and msg.startswith(entry[3:].encode() + b": "), (entry, label, got[label], msg)
    return got


def run_all(_lib):
    """The table through all six entry points: each reports what the table says, every uniform / mapped pair reports the same code
    for every case the two share, and so do the three uniform entry points among themselves."""
    got = {entry: run(_lib, entry) for entry in ENTRIES}
    assert len(table(_lib)) == 2 + 8 + 5 + 5 + 2 + 9 + 1 + 1 + 4
    uniform, mapped = 2 + 8 + 5 + 5 + 2 + 9 + 1, 2 + 8 + 5 + 2 + 9 + 1 + 4
    assert {e: len(g) for e, g in got.items()} == {"pg_phase_vocoder": uniform, "pg_phase_lock": uniform, "pg_phase_lock_linked": uniform - 1,
                                                   "pg_phase_vocoder_map": mapped, "pg_phase_lock_map": mapped, "pg_phase_lock_linked_map": mapped - 1}
    for u, m in TWINS:
        shared = set(got[u]) & set(got[m])
        assert len(shared) == len(got[u]) - 6 and all(got[u][c] == got[m][c] for c in shared), (u, m)
    v, k, n = got["pg_phase_vocoder"], got["pg_phase_lock"], got["pg_phase_lock_linked"]
    assert v == k and all(n[c] == v[c] for c in n), {c: (v[c], k[c], n.get(c)) for c in v if not v[c] == k[c] == n.get(c, v[c])}
    return v
