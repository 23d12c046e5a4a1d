"""GPU: value rows for the raw-window wgrad instantiations that no other table reaches.

tests/test_kernel_families.py lists which conv_g_raw_kernel / conv_g_ps_kernel<KW, S, BF> the rows of the value modules run
(test_value_rows_reach_every_raw_window_wgrad_instantiation) and holds WGRAD_COVER_CASES, the rows added for the rest: the flat-K
kernel of k = 4, k = 5 and (k, s) = (8, 1) at the bf16 operand modes -- and at fp32 under the float64 criterion.  They run here exactly
as the rows of tests/test_z_conv_values_gpu.py do: every element against float64 within 4 x the honest stand-in of the same precision
(tests/_conv_ref64.py), one-hot inputs bit for bit, NaN outputs and a poisoned workspace."""
import pytest

from test_kernel_families import WGRAD_COVER_CASES, fixup_case_id
from test_z_conv_values_gpu import run_impulse, run_values

pytestmark = pytest.mark.gpu
PRECISIONS = ("fp32", "bf16", "bf16x3")


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", WGRAD_COVER_CASES, ids=fixup_case_id)
def test_values(case, prec):
    run_values(case, prec)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", WGRAD_COVER_CASES, ids=fixup_case_id)
def test_impulse(case, prec):
    run_impulse(case, prec)
