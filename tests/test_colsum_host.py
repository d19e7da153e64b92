"""CPU side of the column-sum pins: tests/colsum_ref.py agrees with plain float64 torch sums and with F.batch_norm's running
statistics, the premise of the exact regime holds on every case's own tensors, and each of five planted errors is rejected by the
regime that is there to catch it."""
import pytest
import torch
import torch.nn.functional as F

import colsum_ref as CS
import step_kernels_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EPS, MOM = 1e-5, 0.1


def test_ordered_restatement_is_a_sum():
    """The float32 restatement of the documented order adds every present row exactly once: it equals the plain float64 sum on
    integer inputs, for both stage-1 layouts, ragged chunks and absent rows."""
    for (rows, D, step, chunking) in ((257, 24, 4, CS.colreduce_chunks), (4097, 8, 4, CS.colreduce_chunks), (300, 16, 32, CS.bn_vec_chunks),
                                      (4100, 8, 32, CS.bn_vec_chunks)):
        x = CS.ints(rows, D, seed=rows)
        chunks, rpc = chunking(rows)
        assert chunks <= CS.WS_CHUNKS and chunks * rpc >= rows > (chunks - 1) * rpc
        assert torch.equal(CS.ordered_colsum(x, chunks, rpc, step).to(F64), x.to(F64).sum(0))
    m = CS.MASKED
    rows = m["B"] * m["Tn"]
    keep = CS.present(rows, m["Tn"], m["vlens"])
    assert int(keep.sum()) == CS.n_present(rows, m["Tn"], m["vlens"]) == 28
    x = CS.ints(rows, 8, seed=1)
    for step in (4, 32):
        assert torch.equal(CS.ordered_colsum(x, 1, 64, step, keep).to(F64), x[keep].to(F64).sum(0))
    assert CS.colreduce_chunks(4097) == (64, 65) and CS.bn_vec_chunks(4100) == (43, 96) and CS.colreduce_chunks(1) == (1, 1)


@pytest.mark.parametrize("mode", CS.COLREDUCE_MODES)
def test_colreduce_terms_vs_plain_torch(mode):
    """The addends of every mode, summed in float64, are the formulas of csrc/norm.hip's mode table written with plain torch."""
    rows, D = 65, 24
    inp = CS.colreduce_inputs(mode, rows, D, F32, exact=False)
    t0, t1 = CS.colreduce_terms(mode, inp, F64)
    dy, x, mean, rstd = (None if inp[k] is None else inp[k].to(F64) for k in ("dy", "x", "mean", "rstd"))
    want = {0: lambda: (dy.sum(0), None),
            1: lambda: (dy.sum(0), torch.einsum("rc,rc,r->c", dy, x - mean[:, None], rstd)),
            2: lambda: (dy.sum(0), (dy * (x - mean) * rstd).sum(0)),
            3: lambda: (((x - mean) ** 2).sum(0), None),
            4: lambda: ((dy * x).sum(0), None),
            5: lambda: (dy.sum(0), dy.t() @ mean),
            6: lambda: (x.sum(0), (x * x).sum(0))}[mode]()
    assert torch.allclose(CS.colsum(t0), want[0], rtol=1e-12, atol=1e-12)
    assert (t1 is None) == (want[1] is None) == (mode not in CS.HAS_DOT)
    if t1 is not None:
        assert torch.allclose(CS.colsum(t1), want[1], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("rows", [2, 65])
def test_bn_restatement_vs_batch_norm(rows):
    """bn_stats64 and bn_finalize (from the mean and E[x^2]) give F.batch_norm's running statistics and 1 / sqrt(var + eps) in float64."""
    C = 24
    x, rm0, rv0 = R.randn(rows, C, seed=rows).to(F64), R.randn(C, seed=1).to(F64), R.randn(C, seed=2).abs().to(F64) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    F.batch_norm(x, rm, rv, None, None, True, MOM, EPS)
    mean, rstd, grm, grv = CS.bn_stats64(x, EPS, MOM, rm0, rv0)
    want_rstd = 1.0 / torch.sqrt(x.var(0, unbiased=False) + EPS)
    for got, want in ((mean, x.mean(0)), (rstd, want_rstd), (grm, rm), (grv, rv)):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    rstd2, grm2, grv2 = CS.bn_finalize(x.mean(0), (x * x).mean(0), rows, EPS, MOM, rm0, rv0, F64, True)
    for got, want in ((rstd2, want_rstd), (grm2, rm), (grv2, rv)):
        assert torch.allclose(got, want, rtol=1e-9, atol=1e-9)
    y = CS.bn_stats_yard(x, EPS, MOM, rm0, rv0)
    for got, want in zip(y, (mean, rstd, grm, grv)):
        assert torch.allclose(got.to(F64), want, rtol=1e-4, atol=1e-5)
    # one row: the n > 1 branch leaves the (zero) variance as it is
    _, _, _, rv1 = CS.bn_stats64(x[:1], EPS, MOM, rm0, rv0)
    assert torch.allclose(rv1, (1 - MOM) * rv0) and torch.allclose(CS.bn_stats_yard(x[:1], EPS, MOM, rm0, rv0)[3].to(F64), rv1, rtol=1e-6)


def test_convmod_restatements():
    """z = a for the exact inputs of the convolution module (GLU, depthwise conv by torch in float32), and the backward statistics are
    autograd's gradients of beta and gamma through swish(xhat * gamma + beta)."""
    for (B, T, C, ks, _) in CS.CONVMOD_SHAPES[:2]:
        y2, w, b, a = CS.convmod_exact_inputs(B, T, C, ks, seed=3)
        z = F.conv1d(F.glu(y2.float(), dim=-1).transpose(1, 2), w, b, padding=(ks - 1) // 2, groups=C).transpose(1, 2)
        assert torch.equal(z, a.float())
    rows, C = 37, 8
    da, z = R.randn(rows, C, seed=1).to(F64), R.randn(rows, C, seed=2).to(F64)
    mean, rstd = R.randn(C, seed=3).to(F64), R.randn(C, seed=4).abs().to(F64) + 0.5
    gamma, beta = (R.randn(C, seed=s).to(F64).requires_grad_(True) for s in (5, 6))
    pre = (z - mean) * rstd * gamma + beta
    ((pre * torch.sigmoid(pre)) * da).sum().backward()
    sdy, sdyx = CS.convmod_bwd_stats(da, z, mean, rstd, gamma.detach(), beta.detach(), F64)
    assert torch.allclose(sdy, beta.grad, rtol=1e-12, atol=1e-12) and torch.allclose(sdyx, gamma.grad, rtol=1e-12, atol=1e-12)


def _exact_term_sets():
    """(name, addends in float64) of every tensor the exact-regime GPU cases sum."""
    for dtype in (F32, BF16):
        for (rows, D) in CS.COLREDUCE_SHAPES + CS.COLREDUCE_VEC_SHAPES + [(CS.MASKED["B"] * CS.MASKED["Tn"], 8), (CS.MASKED["B"] * CS.MASKED["Tn"], 72)]:
            for mode in CS.COLREDUCE_MODES:
                for i, t in enumerate(CS.colreduce_terms(mode, CS.colreduce_inputs(mode, rows, D, dtype, exact=True), F64)):
                    if t is not None:
                        yield f"colreduce {dtype} {rows}x{D} mode {mode} sum {i}", t
    for C in CS.BN_VEC_C:
        for rows in CS.BN_VEC_ROWS:
            x = CS.ints(rows, C, seed=rows + C, dtype=BF16).to(F64)
            yield f"bn_stats_vec {rows}x{C} x", x
            yield f"bn_stats_vec {rows}x{C} x^2", x * x
            dz, xx = CS.ints(rows, C, seed=rows + C + 3, dtype=BF16).to(F64), CS.ints(rows, C, seed=rows + C + 4, dtype=BF16).to(F64)
            yield f"bn_act_bwd_vec {rows}x{C} dz", dz
            yield f"bn_act_bwd_vec {rows}x{C} dz x", dz * xx
    for (rows, C) in CS.BN_SCALAR_SHAPES:
        x = CS.ints(rows, C, seed=rows + C).to(F64)
        yield f"bn_stats {rows}x{C} x", x
        yield f"bn_stats {rows}x{C} x^2", x * x
    for (B, T, C, ks, _) in CS.CONVMOD_SHAPES:
        a = CS.convmod_exact_inputs(B, T, C, ks, seed=B * T + C)[3].reshape(B * T, C).to(F64)
        yield f"convmod B{B} T{T} C{C} z", a
        yield f"convmod B{B} T{T} C{C} z^2", a * a


def test_exact_regime_premise_holds_on_every_case():
    """Non-zero integers whose every partial sum stays below 2^24: float32 equals float64 in any order of additions."""
    n = 0
    for name, t in _exact_term_sets():
        bound, same = CS.exact_premise(t)
        assert bound < 2 ** 24 and same, f"{name}: sum of |addends| {bound}, float32 sum == float64 sum: {same}"
        n += 1
    assert n > 300
    assert all(bool((CS.ints(64, 8, seed=s, dtype=BF16) != 0).all()) and bool((CS.ints(64, 8, seed=s).abs() <= 3).all()) for s in range(4))


# ---- five planted errors, each rejected by the regime that is there for it ---------------------------------------------------
def test_planted_dropped_last_chunk_fails_exact():
    rows, D = 4097, 64
    x = CS.ints(rows, D, seed=1).to(F64)
    chunks, rpc = CS.colreduce_chunks(rows)
    want = CS.colsum(x).to(F32)
    assert R.bits_equal(CS.chunked_colsum(x, chunks, rpc).to(F32), want)
    assert not R.bits_equal(CS.chunked_colsum(x, chunks, rpc, drop_last=True).to(F32), want)      # 2 rows of 4097 are missing
    ws = CS.ints(5, 72, seed=2)                                                                   # and in stage 2 alone (mode 7)
    assert R.bits_equal(CS.stage2_ordered(ws), ws.to(F64).sum(0).to(F32)) and not R.bits_equal(CS.stage2_ordered(ws, drop_last=True), ws.to(F64).sum(0).to(F32))


def test_planted_mask_ignoring_an_empty_utterance_fails_exact():
    m = CS.MASKED
    rows = m["B"] * m["Tn"]
    for mode in CS.MASKED_MODES:
        t0, _ = CS.colreduce_terms(mode, CS.colreduce_inputs(mode, rows, 8, F32, exact=True), F64)
        want = CS.finish(CS.colsum(t0, CS.present(rows, m["Tn"], m["vlens"])).to(F32), R.f32(1.0 / 28))
        got = CS.finish(CS.colsum(t0, CS.present_ignoring_empty(rows, m["Tn"], m["vlens"])).to(F32), R.f32(1.0 / 28))
        assert not R.bits_equal(got, want), f"mode {mode}"


def test_planted_accumulate_ignored_fails_exact():
    for mode in CS.COLREDUCE_MODES:
        t0, _ = CS.colreduce_terms(mode, CS.colreduce_inputs(mode, 63, 40, BF16, exact=True), F64)
        prev = CS.ints(40, seed=11 + mode)
        assert bool((prev != 0).all())
        assert not R.bits_equal(CS.finish(CS.colsum(t0).to(F32), 1.0), CS.finish(CS.colsum(t0).to(F32), 1.0, prev))


def test_planted_missing_unbiased_factor_fails_rule():
    rows, C = 65, 72
    x = R.randn(rows, C, seed=rows + C)
    rm0, rv0 = R.randn(C, seed=1), R.randn(C, seed=2).abs() + 0.5
    ref, yard = CS.bn_stats64(x, EPS, MOM, rm0, rv0), CS.bn_stats_yard(x, EPS, MOM, rm0, rv0)
    s, q = x.sum(0) / rows, (x * x).sum(0) / rows
    good = CS.bn_finalize(s, q, rows, EPS, MOM, rm0, rv0, F32, True)
    bad = CS.bn_finalize(s, q, rows, EPS, MOM, rm0, rv0, F32, True, unbiased=False)
    assert R.compare(good[2], ref[3], yard[3], F32)[0]
    assert not R.compare(bad[2], ref[3], yard[3], F32)[0]                 # off by momentum * var / (n - 1) ~ 1.5e-3
    assert R.compare(bad[0], ref[1], yard[1], F32)[0]                     # rstd does not see the factor: only the running variance does


def test_planted_group_order_fails_order_pin():
    rows, D = 4097, 64
    x = R.randn(rows, D, seed=5)
    chunks, rpc = CS.colreduce_chunks(rows)
    ws = CS.stage1_ordered(x, chunks, rpc)
    want = CS.stage2_ordered(ws)
    assert R.bits_equal(CS.ordered_colsum(x, chunks, rpc), want)
    assert not R.bits_equal(CS.stage2_ordered(ws, group_order=(3, 2, 1, 0)), want)
    assert R.compare(CS.stage2_ordered(ws, group_order=(3, 2, 1, 0)), x.to(F64).sum(0), x.sum(0), F32)[0]      # the rule cannot see it
