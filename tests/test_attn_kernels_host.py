"""CPU tests behind tests/gpu_attn_kernel_check.py: the float64 restatements of tests/attn_kernels_ref.py are pinned to oracle/nets.py (mha,
rel_mha, rel_shift) and to torch autograd through the same formula, and the power check shows that the inputs of the GPU cases are chosen
well: on those very tensors each planted error fails the comparison rule, while on a flat softmax with a small map gradient the dropped
`dattn` term of the row sum would go unseen.  None of this touches the package's kernels."""
import math

import pytest
import torch

import attn_kernels_ref as A
import step_kernels_ref as R
from oracle import nets as ON

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def close64(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def _eye_params(D, H=None, u=None, v=None):
    sd = {f"a.linear_{n}.weight": torch.eye(D, dtype=F64) for n in ("q", "k", "v", "out", "pos")}
    if u is not None:
        sd["a.pos_bias_u"], sd["a.pos_bias_v"] = u.double().view(H, D // H), v.double().view(H, D // H)
    return ON.P(sd, "a.")


# ---------------------------------------------------------------------------------------------------------------------------
# pins
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T1,T2,causal", [(5, 9, False), (7, 7, True), (1, 4, False)])
def test_plain_attention_restatement_vs_oracle_and_autograd(T1, T2, causal):
    B, H, dk = 3, 2, 4
    inp = A.plain_inputs(T1, T2, dk, causal, seed=100 + T1, B=B, H=H)
    inp["klen"] = [T2, max(1, T2 - 2), 0]                                         # the last utterance has no admissible key at all
    q, k, v, dctx = (inp[n].double() for n in ("q", "k", "v", "dctx"))
    klen, scale = inp["klen"], 1.0 / math.sqrt(dk)
    m = A.key_mask(klen, T1, T2, causal)
    dattn = torch.where(m, R.randn(B, H, T1, T2, seed=7).double(), torch.zeros((), dtype=F64))
    pmap, pdrop, ctx = A.attn_fwd(q, k, v, klen, causal, scale, H, F64)
    rt = ON.Runtime()
    out = ON.mha(_eye_params(H * dk), q, k, v, m[:, 0], H, rt, name="x")
    close64(pmap, rt.attn["x"]), close64(ctx, out)
    assert bool((pmap[~m.expand_as(pmap)] == 0).all()) and bool((pmap[2] == 0).all()) and bool((ctx[2] == 0).all())
    # the backward, with dropout as data, against autograd through the same formula
    keep = A.keep_of(A.host_keep(B, H, T1, A.round8(T2), 0.3, seed=8), T2).double()
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    s = torch.matmul(A.heads(leaves[0], H, F64), A.heads(leaves[1], H, F64).transpose(-2, -1)) * scale
    p = A.masked_softmax(s, m)
    c = A.unheads(torch.matmul(p * keep, A.heads(leaves[2], H, F64)))
    close64(c.detach(), A.attn_fwd(q, k, v, klen, causal, scale, H, F64, keep=keep)[2])
    ((c * dctx).sum() + (p * dattn).sum()).backward()
    ds, dq, dk_, dv = A.attn_bwd(p.detach(), dctx, v, k, q, scale, H, F64, dattn=dattn, keep=keep)
    close64(dq, leaves[0].grad), close64(dk_, leaves[1].grad), close64(dv, leaves[2].grad)


def test_plain_attention_ds_is_the_gradient_of_the_unscaled_scores():
    B, H, dk, T = 2, 2, 4, 6
    inp = A.plain_inputs(T, T, dk, False, seed=31, B=B, H=H)
    q, k, v, dctx = (inp[n].double() for n in ("q", "k", "v", "dctx"))
    raw = torch.matmul(A.heads(q, H, F64), A.heads(k, H, F64).transpose(-2, -1)).requires_grad_(True)
    m = A.key_mask(inp["klen"], T, T, False)
    p = A.masked_softmax(raw * 0.5, m)
    (A.unheads(torch.matmul(p, A.heads(v, H, F64))) * dctx).sum().backward()
    close64(A.attn_bwd(p.detach(), dctx, v, k, q, 0.5, H, F64)[0], raw.grad)


@pytest.mark.parametrize("T", [1, 2, 7])
def test_rel_attention_restatement_vs_oracle_and_autograd(T):
    B, H, dk = 3, 2, 4
    inp = A.rel_inputs(T, dk, seed=200 + T, B=B, H=H)
    q, k, pos, u, v = (inp[n].double() for n in ("q", "k", "pos", "u", "v"))
    klen, scale = [T, max(1, T - 2), 1], 1.0 / math.sqrt(dk)
    pmap, _, qu, qv = A.rel_attn_fwd(q, k, pos, u, v, klen, scale, H, F64)
    rt = ON.Runtime()
    m = A.key_mask(klen, T, T, False)
    vals = R.randn(B, T, H * dk, seed=9).double()
    # rel_mha projects keys and values from ONE input: hand it k and read the map (the context then is map . k)
    out = ON.rel_mha(_eye_params(H * dk, H, u, v), q, k, pos[None], m[:, 0], H, rt, name="x")
    close64(pmap, rt.attn["x"])
    close64(out, A.unheads(torch.matmul(pmap, A.heads(k, H, F64))))
    close64(qu, q + u), close64(qv, q + v)
    # the shift alone, new and legacy, against the oracle's pad-and-view
    bd = R.randn(B, H, T, 2 * T - 1, seed=10).double()
    close64(A.rel_shift_new(bd), ON.rel_shift(bd, legacy=False))
    bl = R.randn(B, H, T, T, seed=11).double()
    close64(A.rel_shift_legacy(bl), ON.rel_shift(bl, legacy=True))
    # dbd: autograd through the oracle's shift
    for legacy, x in ((False, bd), (True, bl)):
        xx = x.clone().requires_grad_(True)
        sc = R.randn(B, H, T, T, seed=12).double().requires_grad_(True)
        p = A.masked_softmax((sc + ON.rel_shift(xx, legacy)) * scale, m)
        dp, dattn = R.randn(B, H, T, T, seed=13).double(), torch.where(m, R.randn(B, H, T, T, seed=14).double(), torch.zeros((), dtype=F64))
        close64(p.detach(), A.softmax_fwd(sc.detach(), scale, klen, False, F64, bd=x, rel_mode=2 if legacy else 1)[0])
        ((p * dp).sum() + (p * dattn).sum()).backward()
        ds, dbd = A.softmax_bwd(p.detach(), dp, scale, F64, dattn=dattn, rel_mode=2 if legacy else 1)
        close64(ds, sc.grad), close64(dbd, xx.grad)
        if not legacy:
            close64(A.attn_bwd(p.detach(), vals, vals, None, None, scale, H, F64, rel=True)[4],
                    A.unshift(A.attn_bwd(p.detach(), vals, vals, None, None, scale, H, F64)[0]))


@pytest.mark.parametrize("causal", [False, True])
def test_softmax_restatement_vs_autograd(causal):
    B, H, T1, T2 = 3, 2, 6, 6
    inp = A.softmax_inputs(T1, T2, causal, 0, seed=300, B=B, H=H)
    keep = A.keep_of(A.host_keep(B, H, T1, 8, 0.1, seed=1), T2).double()
    sc = inp["scores"].double().requires_grad_(True)
    m = A.key_mask(inp["klen"], T1, T2, causal)
    p = torch.softmax((sc * inp["scale"]).masked_fill(~m, torch.finfo(F64).min), -1).masked_fill(~m, 0.0)
    pm, pd = A.softmax_fwd(inp["scores"], inp["scale"], inp["klen"], causal, F64, keep=keep)
    close64(pm, p.detach()), close64(pd, p.detach() * keep)
    dp, dattn = inp["dp"].double(), inp["dattn"].double()
    ((p * keep * dp).sum() + (p * dattn).sum()).backward()
    close64(A.softmax_bwd(p.detach(), dp, inp["scale"], F64, dattn=dattn, keep=keep)[0], sc.grad)


def test_yard_rounds_only_where_the_kernels_document_it():
    inp = A.plain_inputs(9, 12, 32, False, seed=5)
    keep = A.keep_of(A.host_keep(A.B_, A.H_, 9, 16, 0.3, seed=2), 12)
    args = (inp["q"], inp["k"], inp["v"], inp["klen"], False, inp["scale"], inp["H"], F32)
    p32 = A.attn_fwd(*args)[0]
    ps, pd, ctx = A.attn_fwd(*args, keep=keep, bf16=True, drop_stored=True)
    assert torch.equal(ps, p32.to(BF16).float()) and torch.equal(pd, (ps * keep).to(BF16).float())
    assert torch.equal(ctx, A.unheads(torch.matmul(pd, A.heads(inp["v"], inp["H"], F32))).to(BF16).float())
    assert torch.equal(A.attn_fwd(*args, keep=keep, bf16=True, drop_stored=False)[1], (p32 * keep).to(BF16).float())
    assert A.klens(64) == [64, 59, 1] and A.klens(21) == [21, 15, 1] and A.klens(1) == [1, 1, 1] and all(c[1] % 16 for c in map(A.klens, range(2, 600)))


# ---------------------------------------------------------------------------------------------------------------------------
# power: each planted error fails the rule on the inputs of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------------
def _fails(got, ref, yard, H, out_dtype):
    """True if some (utterance, head) slice of `got` is outside 4 d + ulp of its own slice (the unplanted yard passes by construction)."""
    bad = False
    for (_, g), (_, r), (_, y) in zip(A.slices(got, H), A.slices(ref, H), A.slices(yard, H)):
        assert R.compare(y, r, y, out_dtype, R.MARGIN)[0]
        bad = bad or not R.compare(g, r, y, out_dtype, R.MARGIN)[0]
    return bad


def _plain_outputs(inp, dt, bf16, keepfull, drop_stored, plant):
    T2, H = inp["k"].shape[1], inp["H"]
    keep = None if keepfull is None else A.keep_of(keepfull, T2, plant)
    fwd = A.attn_fwd(inp["q"], inp["k"], inp["v"], inp["klen"], inp["causal"], inp["scale"], H, dt, keep=keep, bf16=bf16, drop_stored=drop_stored, plant=plant)
    bwd = A.attn_bwd(A.stored_map(inp), inp["dctx"], inp["v"], inp["k"], inp["q"], inp["scale"], H, dt, dattn=inp["dattn"], keep=keep, bf16=bf16, plant=plant)
    return list(fwd) + list(bwd)


def _plant_found(shapes, outputs, H, max_shapes=6):
    """plant -> True if it fails the rule on some output of one of the first shapes (outputs(shape, dt, bf16, plant) -> list of tensors)."""
    found = {}
    for shape in shapes[:max_shapes]:
        ref, yard = outputs(shape, F64, False, None), outputs(shape, F32, True, None)
        for plant in A.PLANTS:
            if found.get(plant):
                continue
            got = outputs(shape, F32, True, plant)
            found[plant] = any(_fails(g, r, y, H, BF16) for g, r, y in zip(got, ref, yard) if g is not None)
    return found


def test_power_fused_attention_inputs():
    def outputs(shape, dt, bf16, plant):
        T1, T2, dk, causal = shape
        inp = A.fused_inputs(shape)
        return _plain_outputs(inp, dt, bf16, A.host_keep(A.B_, A.H_, T1, A.round8(T2), 0.3, seed=3), True, plant)
    found = _plant_found([s for s in A.FUSED_SHAPES if s[0] > 16 and s[1] > 16], outputs, A.H_)
    for plant in ("klen+1", "causal<", "no_dattn", "ds*0.97", "dv_last_row", "drop_T2"):
        assert found[plant], plant


def test_power_attention_map_inputs():
    def outputs(shape, dt, bf16, plant):
        T1, T2, dk, causal = shape
        inp = A.map_inputs(shape)
        return _plain_outputs(inp, dt, bf16, A.host_keep(A.B_, A.H_, T1, A.round8(T2), 0.1, seed=4), False, plant)
    found = _plant_found([s for s in A.MAP_SHAPES if s[3] and s[0] > 16] + [s for s in A.MAP_SHAPES if 8 < s[1] < 200 and s[0] > 1], outputs, A.H_)
    for plant in ("klen+1", "causal<", "no_dattn", "ds*0.97", "drop_T2"):
        assert found[plant], plant


def test_power_rel_attention_inputs():
    def outputs(shape, dt, bf16, plant):
        T, dk = shape
        inp = A.rel_case_inputs(shape)
        keep = A.keep_of(A.host_keep(A.B_, A.H_, T, A.round8(T), 0.1, seed=5), T, plant)
        return list(A.rel_attn_fwd(inp["q"], inp["k"], inp["pos"], inp["u"], inp["v"], inp["klen"], inp["scale"], inp["H"], dt, keep=keep, bf16=bf16, plant=plant))
    found = _plant_found([s for s in A.REL_SHAPES if 60 < s[0] < 130], outputs, A.H_)
    for plant in ("klen+1", "drop_T2", "shift+1", "uv_swapped"):
        assert found[plant], plant


def test_power_softmax_inputs():
    def outputs(shape, dt, bf16, plant):
        T1, T2, ld, causal, rel_mode = shape
        inp = A.softmax_case_inputs(shape)
        keep = A.keep_of(A.host_keep(A.B_, A.H_, T1, ld, 0.3, seed=6), T2, plant)
        fwd = A.softmax_fwd(inp["scores"], inp["scale"], inp["klen"], causal, dt, bd=inp["bd"], rel_mode=rel_mode, keep=keep, out_bf16=bf16, plant=plant)
        pm = A.softmax_fwd(inp["scores"], inp["scale"], inp["klen"], causal, F64, bd=inp["bd"], rel_mode=rel_mode)[0].to(BF16)
        bwd = A.softmax_bwd(pm, inp["dp"], inp["scale"], dt, dattn=inp["dattn"], keep=keep, rel_mode=rel_mode, out_bf16=bf16, plant=plant)
        return list(fwd) + [bwd[0]]
    found = _plant_found([s for s in A.SOFTMAX_SHAPES if s[0] > 16], outputs, A.H_)
    for plant in ("klen+1", "causal<", "no_dattn", "ds*0.97", "drop_T2", "shift+1"):
        assert found[plant], plant


def test_edge_klen_inputs_no_key_gives_zero_and_a_length_beyond_the_keys_is_the_full_length():
    """The second run of A.EDGE_KLEN_SHAPES: klen = (0, T2 + 3, the cut).  On those very inputs the utterance without a key has every output
    0, klen = T2 + 3 is klen = T2, the yard passes the rule at margin 4 on every slice, and klen off by one is seen."""
    for family, table in (("fused", A.FUSED_SHAPES), ("map", A.MAP_SHAPES), ("rel", A.REL_SHAPES), ("softmax", A.SOFTMAX_SHAPES)):
        edges = [s for s, edge in A.with_edges(table, family) if edge]
        assert edges and edges == A.EDGE_KLEN_SHAPES[family], family               # every listed shape is one of its table
    assert A.edge_klens(63) == [0, 66, 58] and A.edge_klens(17) == [0, 20, 12]
    for shape in A.EDGE_KLEN_SHAPES["fused"] + A.EDGE_KLEN_SHAPES["map"]:
        T1, T2, dk, causal = shape
        inp = (A.fused_inputs if shape in A.FUSED_SHAPES else A.map_inputs)(shape, edge=True)
        assert inp["klen"] == A.edge_klens(T2)
        keepfull = A.host_keep(A.B_, A.H_, T1, A.round8(T2), 0.3, seed=3)
        ref, yard, off = (_plain_outputs(inp, dt, b, keepfull, True, plant) for dt, b, plant in ((F64, False, None), (F32, True, None), (F32, True, "klen+1")))
        assert all(bool((o[0] == 0).all()) for o in ref + yard)                     # utterance 0: map, dropped map, context, dS, dq, dk, dv
        full = dict(inp, klen=[0, T2, inp["klen"][2]])
        assert all(torch.equal(a, b) for a, b in zip(ref, _plain_outputs(full, F64, False, keepfull, True, None)))
        seen = [_fails(g, r, y, A.H_, BF16) for g, r, y in zip(off, ref, yard)]      # (_fails asserts that the yard itself passes)
        assert seen[0] and seen[2], shape                                            # klen 0 taken for 1: the map and the context
    for shape in A.EDGE_KLEN_SHAPES["rel"]:
        inp = A.rel_case_inputs(shape, edge=True)
        out = A.rel_attn_fwd(inp["q"], inp["k"], inp["pos"], inp["u"], inp["v"], inp["klen"], inp["scale"], inp["H"], F64)
        full = A.rel_attn_fwd(inp["q"], inp["k"], inp["pos"], inp["u"], inp["v"], [0, shape[0], inp["klen"][2]], inp["scale"], inp["H"], F64)
        assert bool((out[0][0] == 0).all()) and torch.equal(out[0], full[0])
    for shape in A.EDGE_KLEN_SHAPES["softmax"]:
        T1, T2, ld, causal, rel_mode = shape
        inp = A.softmax_case_inputs(shape, edge=True)
        pm = A.softmax_fwd(inp["scores"], inp["scale"], inp["klen"], causal, F64, bd=inp["bd"], rel_mode=rel_mode)[0]
        full = A.softmax_fwd(inp["scores"], inp["scale"], [0, T2, inp["klen"][2]], causal, F64, bd=inp["bd"], rel_mode=rel_mode)[0]
        ds, dbd = A.softmax_bwd(pm, inp["dp"], inp["scale"], F64, dattn=inp["dattn"], rel_mode=rel_mode)
        assert bool((pm[0] == 0).all()) and torch.equal(pm, full) and bool((ds[0] == 0).all()) and (dbd is None or bool((dbd[0] == 0).all()))


def test_flat_softmax_with_a_small_map_gradient_does_not_see_the_dattn_term():
    """Why the inputs are what they are: unit-scale q (a flat softmax over 31 - 63 keys) and a map gradient of 0.1 leave the dropped `dattn` term of
    the row sum inside 4 d + ulp at every element of dq, dk, dv -- and SCORE_STD = 3 with a unit map gradient does not."""
    T, dk = 63, 96
    for flat in (True, False):
        inp = A.plain_inputs(T, T, dk, False, seed=77)
        if flat:
            inp["q"] = (inp["q"].float() / A.SCORE_STD).to(BF16)
            inp["klen"] = [T, T - 7, T // 2]                                      # no utterance whose softmax is peaked by its length alone
            inp["dattn"] = R.randn(A.B_, A.H_, T, T, seed=78, scale=0.1, dtype=BF16)
        ref, yard, got = (_plain_outputs(inp, dt, b, None, True, plant)[4:] for dt, b, plant in ((F64, False, None), (F32, True, None), (F32, True, "no_dattn")))
        seen = any(_fails(g, r, y, A.H_, BF16) for g, r, y in zip(got, ref, yard))
        assert seen != flat, ("flat" if flat else "peaked", seen)
