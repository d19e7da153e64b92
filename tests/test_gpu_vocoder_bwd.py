"""HiFi-GAN generator backward on the MI355X: each case of tests/gpu_vocoder_bwd_check.py as a pytest test."""
import pytest

import gpu_vocoder_bwd_check as vc


@pytest.mark.gpu
@pytest.mark.parametrize("case", vc.CASES, ids=[c.__name__ for c in vc.CASES])
def test_vocoder_bwd_case(case):
    results = case()
    for ok, msg in results:
        print(("ok   " if ok else "FAIL ") + msg)
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
