"""Kernel-level pins of the per-channel column sums (colreduce, BatchNorm statistics, the Conformer convolution module's statistics)
on the MI355X: each case of tests/gpu_colsum_check.py as a pytest test."""
import pytest

import gpu_colsum_check as kc


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.CASES, ids=[c.__name__ for c in kc.CASES])
def test_colsum_case(case):
    results = case()
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
