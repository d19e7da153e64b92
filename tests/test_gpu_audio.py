"""Waveform conditioning on the MI355X: each case of tests/gpu_audio_check.py as a pytest test."""
import pytest

import gpu_audio_check as gc


@pytest.mark.gpu
@pytest.mark.parametrize("case", gc.CASES, ids=[c.__name__ for c in gc.CASES])
def test_audio_case(case):
    results = case()
    for ok, msg in results:
        print(("ok   " if ok else "FAIL ") + msg)
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
