"""numpy restatement of pg_phase_lock's contract (include/phasegen.h) word for word, for the phase-locking tests (no GPU, no phasegen
import): a plain Python loop over the output frames, uint32 wrap-around sums, IEEE fp32 comparisons.  The device must reproduce it
BIT FOR BIT.

  peak_map     one frame's magnitudes (bins,) -> P (bins,) int64: the peak every bin belongs to
  phase_lock   A, M (..., bins, F_src) float32 -> (..., bins, F_out) float32; with return_rotation also T (..., bins, F_out) uint32
"""
import numpy as np

from _vocoder_ref import angle_of, positions, q

REACH = 2                                                                   # PG_LOCK_REACH


def peaks(m):
    """(bins,) float32 -> bool (bins,): b is a peak iff m[b] is not NaN and, for d = 1 .. REACH, (b - d < 0 or m[b] > m[b-d]) and
    (b + d >= bins or m[b] >= m[b+d])."""
    m = np.asarray(m, np.float32)
    ok = ~np.isnan(m)
    with np.errstate(invalid="ignore"):
        for d in range(1, REACH + 1):
            below, above = np.ones(m.shape[0], bool), np.ones(m.shape[0], bool)
            below[d:] = m[d:] > m[:-d]                                      # (b - d < 0: nothing to compare with)
            above[:-d] = m[:-d] >= m[d:]                                    # (b + d >= bins: likewise)
            ok &= below & above
    return ok


def peak_map(m):
    """P(b): the peak nearest to b in |b - p|, a tie going to the lower peak; without any peak P(b) = b."""
    pk = np.flatnonzero(peaks(m)).astype(np.int64)
    b = np.arange(np.asarray(m).shape[0], dtype=np.int64)
    if pk.size == 0:
        return b
    j = np.searchsorted(pk, b)                                              # the first peak at or above b
    lower, upper = pk[np.maximum(j - 1, 0)], pk[np.minimum(j, pk.size - 1)]
    return np.where(np.abs(b - lower) <= np.abs(upper - b), lower, upper)   # (no peak on one side: both are the same peak)


def phase_lock(A, F_out, src_per_out, M, reset_below=0.0, return_rotation=False):
    A, M = np.asarray(A, np.float32), np.asarray(M, np.float32)
    assert A.shape == M.shape and A.ndim >= 2
    lead, (bins, F_src) = A.shape[:-2], A.shape[-2:]
    A2, M2 = A.reshape(-1, bins, F_src), M.reshape(-1, bins, F_src)
    i0, i1 = positions(F_out, src_per_out, F_src)
    qA = q(A2)
    floor = np.float32(reset_below)
    out = np.empty((A2.shape[0], bins, F_out), np.float32)
    rot = np.empty((A2.shape[0], bins, F_out), np.uint32)
    for c in range(A2.shape[0]):
        T = np.zeros(bins, np.uint32)                                       # T_0 = 0
        for g in range(F_out):
            a = qA[c, :, i0[g]]
            if g >= 1:
                m = M2[c, :, i0[g]]
                P = peak_map(m)
                e = qA[c, :, i1[g - 1]] - a                                 # uint32 - uint32 wraps
                with np.errstate(invalid="ignore"):
                    reset = m[P] < floor                                    # (False for a NaN)
                T = np.where(reset, np.uint32(0), T[P] + e[P])
            rot[c, :, g] = T
            out[c, :, g] = angle_of(T + a)
    out, rot = out.reshape(lead + (bins, F_out)), rot.reshape(lead + (bins, F_out))
    return (out, rot) if return_rotation else out
