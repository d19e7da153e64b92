"""The one-launch refresh of the derived weight copies on the MI355X: each case of tests/gpu_derived_refresh_check.py as a pytest
test."""
import pytest

import gpu_derived_refresh_check as dc


@pytest.mark.gpu
@pytest.mark.parametrize("case", dc.CASES, ids=[c.__name__ for c in dc.CASES])
def test_derived_refresh_case(case):
    results = case()
    bad = [msg for ok, msg in results if not ok]
    assert not bad, "\n".join(bad)
