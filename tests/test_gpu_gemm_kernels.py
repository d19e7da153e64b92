"""Float64 and bit-exact parity of the GEMM families (skinny, generic, fast, LDS-DMA, 8-wave) on the MI355X, each case held to the route
it was written for: each family of tests/gpu_gemm_kernel_check.py as a pytest test."""
import pytest

import gpu_gemm_kernel_check as kc


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.CASES, ids=[c.__name__ for c in kc.CASES])
def test_gemm_kernel_case(case):
    results = case()
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
