"""Host-side pins of tests/conv1d_wgrad_ref.py (no GPU): the float64 restatement of the Conv1d weight gradient equals torch.autograd of
F.conv1d, and each of the four planted errors breaks the comparison rule of the GPU cases on every case's own inputs."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv1d_wgrad_ref as C  # noqa: E402
import step_kernels_ref as R  # noqa: E402

F32, F64 = torch.float32, torch.float64
IDS = [C.name_of(c) for c in C.CASES]


def _autograd(dy, x, ks):
    w = torch.zeros(dy.shape[2], x.shape[2], ks, dtype=F64, requires_grad=True)
    y = F.conv1d(x.to(F64).transpose(1, 2), w, padding=(ks - 1) // 2)
    y.backward(dy.to(F64).transpose(1, 2))
    return w.grad


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
@pytest.mark.parametrize("regime", ["normal", "exact"])
def test_restatement_equals_autograd_of_conv1d(case, regime):
    dy, x, pre = C.inputs(case, regime)
    want = _autograd(dy, x, case[4])
    got = C.wgrad(dy, x, case[4], F64)
    if regime == "exact":
        assert torch.equal(got, want)
        assert R.bits_equal(C.wgrad(dy, x, case[4], F32, pre), C.wgrad(dy, x, case[4], F64, pre).to(F32))      # float32 is exact there too
    else:
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-12 * scale
    assert torch.equal(C.wgrad(dy, x, case[4], F64, pre), pre.to(F64) + got)


def test_exact_regime_rejects_what_is_not_exact():
    dy, x, pre = C.inputs(C.CASES[4], "exact")
    assert C.exact_ok(dy, x, pre)
    assert not C.exact_ok(dy.float() + 0.5, x, pre)
    assert not C.exact_ok(dy.float() * 4096, x.float() * 4096, pre)


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
@pytest.mark.parametrize("regime", ["normal", "exact"])
@pytest.mark.parametrize("plant", C.PLANTS)
def test_every_plant_breaks_the_rule(case, regime, plant):
    dy, x, pre = C.inputs(case, regime)
    ks = case[4]
    ref64, yard = C.wgrad(dy, x, ks, F64, pre), C.wgrad(dy, x, ks, F32, pre)
    assert R.compare(yard, ref64, yard, F32)[0]
    bad = C.wgrad(dy, x, ks, F32, pre, plant=plant)
    ok, ratio, d, msg = R.compare(bad, ref64, yard, F32)
    assert not ok, f"plant {plant} passes the rule on {C.name_of(case)} ({regime}): {msg}"
    # ... and by orders of magnitude: the edge rows carry EDGE times the rest
    err = float((bad.to(F64) - ref64).abs().max())
    assert err > 100 * (R.MARGIN * d + float(R.ulp_out(ref64, F32).max())), (plant, err, d)
