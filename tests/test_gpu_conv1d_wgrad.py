"""Element-wise float64 parity, bit-for-bit conditions and refusals of the grouped Conv1d weight-gradient launch (csrc/conv1d_wgrad.hip) on
the MI355X: each case of tests/gpu_conv1d_wgrad_check.py as a pytest test."""
import pytest

import gpu_conv1d_wgrad_check as kc


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.CASES, ids=[c.__name__ for c in kc.CASES])
def test_conv1d_wgrad_case(case):
    results = case()
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
