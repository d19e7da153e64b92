"""CPU side of the attention-with-projection checks: tests/attn_proj_ref.py is pinned to float64 autograd of F.linear around the attention
restatement of tests/attn_kernels_ref.py, and the comparison rule of tests/gpu_attn_proj_kernel_check.py is shown to have power on the GPU
cases' own inputs: each planted error of attn_proj_ref.PLANTS fails it there."""
import pytest
import torch
import torch.nn.functional as F

import attn_kernels_ref as A
import attn_proj_ref as P
import step_kernels_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


@pytest.mark.parametrize("case", [P.CASES[1], P.CASES[4], P.CASES[7]], ids=lambda c: f"D{c[0]}_{c[3]}_{c[4]}x{c[5]}")
@pytest.mark.parametrize("p", [0.0, P.P_DROP])
def test_restatement_vs_float64_autograd_of_linear_and_attention(case, p):
    """dq / dk / dv of attn_proj_ref.proj_bwd are the gradients autograd gives for  y = F.linear(attention(q, k, v), W_o, b_o)  with dY on y
    and dattn on the map, all in float64, when the restatement is handed the float64 map itself."""
    D, H, dk, kind, T1, T2, causal = case
    inp = P.inputs(case)
    keep = A.keep_of(A.host_keep(P.B_, H, T1, A.round8(T2), p, seed=9), T2).to(F64) if p else None
    q, k, v = (inp[n].to(F64).requires_grad_(True) for n in ("q", "k", "v"))
    w_o, b_o = inp["w_o"].to(F64), R.randn(D, seed=77).to(F64)
    pmap, _, ctx = A.attn_fwd(q, k, v, inp["klen"], causal, inp["scale"], H, F64, keep=keep)
    y = F.linear(ctx, w_o, b_o)
    ((y * inp["dy"].to(F64)).sum() + (pmap * inp["dattn"].to(F64)).sum()).backward()
    _, dq, dkk, dv = P.proj_bwd(pmap.detach(), inp["dy"], inp["w_o"], inp["v"], inp["k"], inp["q"], inp["scale"], H, F64, dattn=inp["dattn"],
                                keep=keep)
    for name, got, ref in (("dq", dq, q.grad), ("dk", dkk, k.grad), ("dv", dv, v.grad)):
        assert torch.allclose(got, ref, rtol=1e-11, atol=1e-12), f"{name}: max diff {float((got - ref).abs().max()):.3e}"


def test_yard_rounds_dctx_once_after_the_sum():
    inp = P.inputs(P.CASES[4])
    H = P.CASES[4][1]
    d32, d16 = P.dctx_of(inp["dy"], inp["w_o"], H, F32), P.dctx_of(inp["dy"], inp["w_o"], H, F32, bf16=True)
    assert torch.equal(d16, d32.to(BF16).to(F32)) and not torch.equal(d16, d32)


def _fails(got, ref, yard, H):
    """True if some (utterance, head) slice of `got` is outside 4 d + ulp of its own slice (the unplanted yard passes by construction)."""
    return any(not R.compare(g, r, y, BF16)[0] for (_, g), (_, r), (_, y) in zip(A.slices(got, H), A.slices(ref, H), A.slices(yard, H)))


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: f"D{c[0]}_dk{c[2]}_{c[3]}_{c[4]}x{c[5]}")
def test_power_each_planted_error_fails_the_rule_on_the_gpu_inputs(case):
    """Wrong head's weight rows, W_o untransposed, the K range short by one 32-step: each is outside the rule on every case's inputs, with
    and without dropout.  (The planted errors of a folded FORWARD projection -- bias dropped, bias added after the rounding, Q / K / V
    blocks swapped -- have no counterpart here: the backward fold reads no bias and one weight block.)"""
    D, H, dk, kind, T1, T2, causal = case
    inp = P.inputs(case)
    pm = A.stored_map(inp)
    for p in (0.0, P.P_DROP):
        keep = A.keep_of(A.host_keep(P.B_, H, T1, A.round8(T2), p, seed=11), T2) if p else None
        a = (pm, inp["dy"], inp["w_o"], inp["v"], inp["k"], inp["q"], inp["scale"], H)
        ref, yard = P.proj_bwd(*a, F64, dattn=inp["dattn"], keep=keep), P.proj_bwd(*a, F32, dattn=inp["dattn"], keep=keep, bf16=True)
        assert not any(_fails(y, r, y, H) for r, y in zip(ref[1:], yard[1:]))
        for plant in P.PLANTS:
            got = P.proj_bwd(*a, F32, dattn=inp["dattn"], keep=keep, bf16=True, plant=plant)
            assert any(_fails(g, r, y, H) for g, r, y in zip(got[1:], ref[1:], yard[1:])), f"{plant} (p {p}) passes the rule"
