"""Kernel-level pins of the row-wise and element-wise kernels between the GEMMs (LayerNorm with residual / dropout / hscale, the ln_act
family, activation + dropout, positional encoding, GLU, the element-wise BatchNorm kernels, adds and casts) on the MI355X: each case of
tests/gpu_row_kernel_check.py as a pytest test."""
import pytest

import gpu_row_kernel_check as kc


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.CASES, ids=[c.__name__ for c in kc.CASES])
def test_row_kernel_case(case):
    results = case()
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
