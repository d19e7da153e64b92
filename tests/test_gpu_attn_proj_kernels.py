"""Element-wise float64 parity, and bit-for-bit equality with the separate launches, of the fused attention backward that carries the
out-projection's data gradient (attn_proj_bwd) on the MI355X: each case of tests/gpu_attn_proj_kernel_check.py as a pytest test."""
import pytest

import gpu_attn_proj_kernel_check as kc


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.CASES, ids=[c.__name__ for c in kc.CASES])
def test_attn_proj_kernel_case(case):
    results = case()
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
