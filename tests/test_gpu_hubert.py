"""The HuBERT-Soft content encoder on the MI355X (map-free attention, front-end layer 0, unit log-probs, the model, encode / encode_batch):
each case of tests/gpu_hubert_check.py as a pytest test."""
import pytest

import gpu_hubert_check as kc


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.CASES, ids=[c.__name__ for c in kc.CASES])
def test_hubert_case(case):
    results = case()
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
