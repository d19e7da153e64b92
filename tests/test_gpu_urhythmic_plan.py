"""The stretch plan on the MI355X: each case of tests/gpu_urhythmic_plan_check.py as a pytest test."""
import pytest

import gpu_urhythmic_plan_check as gc


@pytest.mark.gpu
@pytest.mark.parametrize("case", gc.CASES, ids=[c.__name__ for c in gc.CASES])
def test_urhythmic_plan_case(case):
    results = case()
    for ok, msg in results:
        print(("ok   " if ok else "FAIL ") + msg)
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
