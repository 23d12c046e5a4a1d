"""GPU: the five stretch wrappers of phasegen.ops (spec_clips, phase_vocoder, phase_lock, phase_lock_linked, ola_stretch) validate a
uniform call and a mapped one (``pos=``) through the same code: every bad argument that does not concern ``pos`` itself raises a
ValueError with the SAME message either way -- a wrong dtype, a CPU tensor, a plane of the wrong rank, rows that are not F_src apart,
overlapping channels, an output length of 0, reset_below -1 and NaN, src_per_out 0 and inf (with ``pos`` given too: the range is
checked before the two grids are refused) -- and one good call of each, uniform and mapped, returns.  Planes are (2, 5, 19) -> 25
frames; the overlap-add signal is (2, 40) -> 7 samples with win_len 8 and hop 2.  Ten tiny launches in all."""
import numpy as np
import pytest
import torch

from test_z_map_gpu import dev, planes, uniform

pytestmark = pytest.mark.gpu
N_CH, BINS, F_SRC, F_OUT = 2, 5, 19, 25
N_IN, N_OUT, WIN, HOP = 40, 7, 8, 2
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def calls():
    """name -> (call(first=good plane or signal, n=good output length, **keywords), the good first argument, the good table)"""
    from phasegen import ops
    A, M = (dev(v) for v in planes(31, N_CH, BINS, F_SRC))
    Ar, Mr = (dev(v[0]) for v in planes(32, 1, BINS, F_SRC))
    x = dev(np.random.RandomState(33).standard_normal((N_CH, N_IN)).astype(np.float32))
    pos = dev(uniform(F_OUT, 0.7))
    grains = dev(uniform(ops.ola_grains(N_OUT, WIN, HOP), 1.4))
    assert grains.shape[0] == 6
    return {
        "spec_clips": (lambda p=M, n=F_OUT, **kw: ops.spec_clips(p, 1, n, F_OUT, **kw), M, pos),
        "phase_vocoder": (lambda p=A, n=F_OUT, **kw: ops.phase_vocoder(p, n, **{"logmag": M, **kw}), A, pos),
        "phase_lock": (lambda p=A, n=F_OUT, **kw: ops.phase_lock(p, n, **{"logmag": M, **kw}), A, pos),
        "phase_lock_linked": (lambda p=A, n=F_OUT, **kw: ops.phase_lock_linked(p, Ar, Mr, n, **kw), A, pos),
        "ola_stretch": (lambda p=x, n=N_OUT, **kw: ops.ola_stretch(p, n, win_len=WIN, hop=HOP, **kw), x, grains),
    }


def bad_arguments(name, good):
    """label -> (positional arguments, keywords) of a call that has to be refused"""
    if name == "ola_stretch":
        bad = {"3-D": good[None], "samples not contiguous": good[:, ::2], "overlapping rows": torch.as_strided(good, (N_CH, N_IN // 2 + 1), (N_IN // 2, 1))}
    else:
        bad = {"2-D": good[0], "4-D": good[None], "rows not F_src apart": good[:, :, :-1],
               "overlapping channels": torch.as_strided(good, (N_CH, BINS, F_SRC), (F_SRC, F_SRC, 1))}
    bad.update({"float64": good.double(), "on the CPU": good.cpu()})
    cases = {label: ((t,), {}) for label, t in bad.items()}
    cases["no output"] = ((good, 0), {})
    cases.update({f"src_per_out {v}": ((), dict(src_per_out=v)) for v in (0.0, INF)})
    if name.startswith("phase_"):
        cases.update({f"reset_below {v}": ((), dict(reset_below=v)) for v in (-1.0, NAN)})
    return cases


@pytest.mark.parametrize("name", ["spec_clips", "phase_vocoder", "phase_lock", "phase_lock_linked", "ola_stretch"])
def test_a_bad_argument_is_refused_in_the_same_words_with_and_without_pos(calls, name):
    call, good, table = calls[name]
    cases = bad_arguments(name, good)
    assert len(cases) == {"spec_clips": 9, "ola_stretch": 8}.get(name, 11)
    for label, (args, kw) in cases.items():
        with pytest.raises(ValueError) as without:
            call(*args, **kw)
        with pytest.raises(ValueError) as with_pos:
            call(*args, pos=table, **kw)
        assert str(without.value) == str(with_pos.value) and str(without.value).startswith(name + ": "), (name, label, str(with_pos.value))
    want = (N_CH, N_OUT) if name == "ola_stretch" else (1, N_CH, BINS, F_OUT) if name == "spec_clips" else (N_CH, BINS, F_OUT)
    for grid in (dict(src_per_out=0.7), dict(pos=table)):
        out = call(**grid)
        assert tuple(out.shape) == want and bool(torch.isfinite(out).all()), (name, grid)
