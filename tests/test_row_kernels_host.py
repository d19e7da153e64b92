"""CPU tests behind tests/gpu_row_kernel_check.py: the float64 restatements of tests/row_kernels_ref.py are pinned to stock torch (with
autograd) and to oracle/nets.py, the exact premise is asserted on every exact case, the conditions the GPU cases rely on are asserted on
their own inputs, the restated dispatch is held to the source, and every planted error is rejected by the regime that exists for it."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import row_kernels_ref as RK
import step_kernels_ref as R
from oracle import nets as ON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TORCH_ACT = {None: lambda x: x, "relu": torch.relu, "tanh": torch.tanh, "swish": F.silu, "gelu": F.gelu, "sigmoid": torch.sigmoid}


def close64(a, b, tol=1e-12):
    a, b = a.detach().to(F64), b.detach().to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def leaf(t):
    return t.to(F64).clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements against stock torch and the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", RK.ACTS)
def test_activations_vs_torch_and_autograd(a):
    x = leaf(R.randn(300, seed=1, scale=3.0))
    y = TORCH_ACT[a](x)
    close64(RK.act(x.detach(), a), y)
    (g,) = torch.autograd.grad(y.sum(), x)
    close64(RK.act_deriv(x.detach(), a), g)
    assert RK.act(torch.tensor([1.0]), "swish").item() == ON.swish(torch.tensor([1.0])).item()
    # act + dropout forward and backward from what is saved
    keep = RK.host_keep((300,), 0.5, 2)
    dz = R.randn(300, seed=3).to(F64)
    z = TORCH_ACT[a](x) * keep.to(F64)
    close64(RK.act_dropout_fwd(x.detach(), a, keep, F64), z)
    (g,) = torch.autograd.grad((z * dz).sum(), x)
    saved = z.detach() if a in RK.SAVED_IS_OUTPUT else x.detach()
    close64(RK.act_dropout_bwd(dz, saved, a, keep, F64), g)


@pytest.mark.parametrize("with_res,p,hscale", [(False, 0.0, 1.0), (True, 0.0, 1.0), (True, 0.5, 0.5)])
def test_layernorm_vs_torch_autograd_and_oracle(with_res, p, hscale):
    rows, D = 7, 50
    inp = RK.ln_rule_inputs(rows, D, F32, with_res, seed=5)
    keep = RK.host_keep((rows, D), p, 6)
    x, gamma, beta = leaf(inp["x"]), leaf(inp["gamma"]), leaf(inp["beta"])
    s = x
    if with_res:
        s = inp["res"].to(F64) + hscale * (x if keep is None else x * keep.to(F64))
    s.retain_grad()
    y = F.layer_norm(s, (D,), gamma, beta, RK.LN_EPS)
    got = RK.ln_fwd(inp["x"], inp["res"], keep, hscale, inp["gamma"], inp["beta"], RK.LN_EPS, F64)
    close64(got[0], y)
    close64(got[0], ON.layer_norm({"weight": inp["gamma"].to(F64), "bias": inp["beta"].to(F64)}, s.detach()))
    if with_res:
        close64(got[1], s)
    close64(got[2], s.detach().mean(-1))
    close64(got[3], 1.0 / torch.sqrt(s.detach().var(-1, unbiased=False) + RK.LN_EPS), tol=1e-9)
    dy, extra = R.randn(rows, D, seed=7), R.randn(rows, D, seed=8)
    ((y * dy.to(F64)).sum() + (s * extra.to(F64)).sum()).backward()
    ds, dh, sdy, sdyx = RK.ln_bwd(dy, s.detach(), got[2], got[3], inp["gamma"], extra, keep, hscale, F64)
    # the last row is constant (rstd 1e6): its gradient is a difference of large numbers, held to 1e-6 of them
    close64(ds[:-1], s.grad[:-1], tol=1e-10)
    close64(ds[-1], s.grad[-1], tol=1e-3)
    if with_res:
        close64(dh[:-1], x.grad[:-1], tol=1e-10)
    close64(sdy, beta.grad)
    close64(sdyx, gamma.grad, tol=1e-6)


@pytest.mark.parametrize("a", RK.LN_ACT_ACTS)
def test_ln_act_vs_torch_autograd(a):
    m = RK.LN_ACT_LENS
    B, T, lens, D = m["B"], m["T"], m["lens"], 24
    x, res = leaf(R.randn(B * T, D, seed=11)), leaf(R.randn(B * T, D, seed=12))
    gamma, beta = 1.0 + R.randn(D, seed=13, scale=0.2), R.randn(D, seed=14, scale=0.2)
    keep = RK.host_keep((B * T, D), 0.5, 15)
    valid = ON.non_pad_mask(lens, T).reshape(B * T, 1).to(F64)
    assert valid.reshape(-1).bool().tolist() == RK.row_valid(B * T, T, lens).tolist()
    u = F.layer_norm(x, (D,), gamma.to(F64), beta.to(F64), 1e-5)
    y = valid * (res + keep.to(F64) * TORCH_ACT[a](u))
    gy, gm, gr = RK.ln_act_fwd(x.detach(), gamma, beta, 1e-5, a, res.detach(), lens, T, keep, F64)
    close64(gy, y)
    dy = R.randn(B * T, D, seed=16)
    (y * dy.to(F64)).sum().backward()
    du, dx, dres = RK.ln_act_bwd(dy, x.detach(), gm, gr, gamma, beta, a, lens, T, keep, F64)
    close64(dx, x.grad, tol=1e-10)
    close64(dres, res.grad)
    close64(du, valid * dy.to(F64) * keep.to(F64) * RK.act_deriv(u.detach(), a))
    assert R.bits_equal(gy[T + 1:].to(F32), torch.zeros(B * T - T - 1, D))        # the partial utterance's tail and the empty utterance: +0


@pytest.mark.parametrize("ks,dil", RK.DW_KS_DIL)
@pytest.mark.parametrize("T", RK.DW_T)
def test_dwconv_vs_conv1d(ks, dil, T):
    B, D = 2, 12
    x, w, b = R.randn(B, T, D, seed=21), R.randn(D, ks, seed=22), R.randn(D, seed=23)
    want = F.conv1d(x.to(F64).transpose(1, 2), w.to(F64)[:, None, :], b.to(F64), padding=(ks - 1) // 2 * dil, dilation=dil, groups=D).transpose(1, 2)
    close64(RK.dwconv(x, w, b, ks, dil, F64), want)
    gamma, beta = 1.0 + R.randn(D, seed=24, scale=0.2), R.randn(D, seed=25, scale=0.2)
    u, y, _, _ = RK.dw_ln_act_fwd(x, w, b, ks, dil, gamma, beta, 1e-5, "gelu", F64)
    close64(y, F.gelu(F.layer_norm(want, (D,), gamma.to(F64), beta.to(F64), 1e-5)))


def test_posenc_and_glu_vs_torch_and_oracle():
    B, T, D = 3, 17, 32
    x, pe = leaf(R.randn(B, T, D, seed=31)), ON.sin_table(T + 3, D)
    alpha = leaf(torch.tensor([0.7]))
    keep = RK.host_keep((B, T, D), 0.1, 32)
    y = (x * math.sqrt(D) + alpha * pe[:T].to(F64)) * keep.to(F64)
    close64(RK.posenc_fwd(x.detach(), math.sqrt(D), alpha.detach(), pe, keep, F64), y)
    close64(RK.posenc_fwd(x.detach(), math.sqrt(D), None, pe, None, F64), ON.abs_posenc(x.detach(), ON.Runtime(), 0.0))
    close64(RK.posenc_fwd(x.detach(), 1.0, alpha.detach(), pe, None, F64), ON.scaled_posenc({"alpha": alpha.detach()}, x.detach(), ON.Runtime(), 0.0))
    close64(RK.posenc_fwd(x.detach(), 2.0, None, None, None, F64), x.detach() * 2.0)
    dy = R.randn(B, T, D, seed=33)
    (y * dy.to(F64)).sum().backward()
    dx, dalpha = RK.posenc_bwd(dy, math.sqrt(D), pe, keep, F64)
    close64(dx, x.grad)
    close64(dalpha, alpha.grad)
    assert dalpha.shape == (1,) and RK.posenc_bwd(dy, 1.0, None, None, F64)[1] is None
    g = leaf(R.randn(9, 2 * 20, seed=34))
    yg = F.glu(g, -1)
    close64(RK.glu_fwd(g.detach(), F64), yg)
    dyg = R.randn(9, 20, seed=35)
    (yg * dyg.to(F64)).sum().backward()
    close64(RK.glu_bwd(g.detach(), dyg, F64), g.grad)


@pytest.mark.parametrize("a", (None, "tanh", "swish"))
def test_batchnorm_elementwise_vs_torch(a):
    m = RK.MASKED
    rows, C, eps = m["B"] * m["Tn"], 8, 1e-5
    x, gamma, beta = leaf(R.randn(rows, C, seed=41)), 1.0 + R.randn(C, seed=42, scale=0.2), R.randn(C, seed=43, scale=0.2)
    ok = RK.present(rows, m["Tn"], m["vlens"])
    assert int(ok.sum()) == 28
    # training mode over the present rows: stock batch_norm on the cropped batch
    xp = x[ok]
    mean, var = xp.detach().mean(0), xp.detach().var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = F.batch_norm(xp, None, None, gamma.to(F64), beta.to(F64), True, 0.1, eps)
    y, p_ = RK.bn_apply(x.detach(), mean, rstd, gamma, beta, a, None, m["vlens"], m["Tn"], F64)
    close64(y[ok], TORCH_ACT[a](pre))
    close64(p_[ok], pre)
    assert R.bits_equal(y[~ok].to(F32), torch.zeros(int((~ok).sum()), C))
    g = R.randn(rows, C, seed=44).to(F64)
    (pre * g[ok]).sum().backward()
    xh = (x.detach() - mean) * rstd
    sdy, sdyx = g[ok].sum(0), (g * xh)[ok].sum(0)
    dx = RK.bn_bwd(g, x.detach(), mean, rstd, gamma, sdy, sdyx, True, m["vlens"], m["Tn"], F64)
    close64(dx, x.grad, tol=1e-10)
    # eval mode: running statistics, no batch terms
    x2 = leaf(x.detach())
    pe_ = F.batch_norm(x2, mean.clone(), var.clone(), gamma.to(F64), beta.to(F64), False, 0.1, eps)
    (pe_ * g).sum().backward()
    close64(RK.bn_bwd(g, x.detach(), mean, rstd, gamma, sdy, sdyx, False, None, 0, F64), x2.grad, tol=1e-10)
    close64(RK.bn_apply(x.detach(), mean, rstd, gamma, beta, None, None, None, 0, F64)[0], pe_)


def test_small_launchers_restatements():
    xs = [R.randn(40, seed=50 + i, dtype=BF16) for i in range(4)]
    assert R.bits_equal(RK.add_n(xs[:2], BF16), (xs[0].float() + xs[1].float()).to(BF16))
    assert R.bits_equal(RK.add_n(xs, F32), ((xs[0].float() + xs[1].float()) + xs[2].float()) + xs[3].float())
    assert R.bits_equal(RK.axpby(0.5, xs[0], -2.0, xs[1], F32), 0.5 * xs[0].float() - 2.0 * xs[1].float())
    u, v = R.randn(8, seed=60), R.randn(8, seed=61)
    q = R.randn(5, 8, seed=62, dtype=BF16)
    assert R.bits_equal(RK.add_head_bias(q, u, v, BF16)[1], (q.float() + v).to(BF16))


# ---------------------------------------------------------------------------------------------------------------------------
# the exact premise and the conditions the GPU cases rely on
# ---------------------------------------------------------------------------------------------------------------------------
def ln_fwd_exact_fn(inp, keep, hscale, store, **plant):
    return lambda dt: RK.ln_fwd(inp["x"], inp["res"], keep, hscale, inp["gamma"], inp["beta"], RK.LN_EPS, dt, store=store, **plant)[:4]


@pytest.mark.parametrize("dtype,D,aligned", [c for c in RK.LN_CASES if c[1] % 2 == 0], ids=lambda v: str(v).replace("torch.", ""))
def test_layernorm_fwd_exact_premise(dtype, D, aligned):
    for rows in RK.ROWS:
        for with_res, p, hscale in ((False, 0.0, 1.0), (True, 0.0, 1.0), (True, 0.0, 0.5), (True, 0.5, 1.0), (True, 0.5, 0.5)):
            keep = RK.host_keep((rows, D), p, D + rows)
            inp = RK.ln_fwd_exact_inputs(rows, D, dtype, with_res, keep, hscale, seed=D + rows)
            for v in (inp["x"], inp["res"]):
                assert v is None or R.bits_equal(v.to(F32).to(dtype), v)
            y, s, mean, rstd = RK.exact_premise(ln_fwd_exact_fn(inp, keep, hscale, dtype))
            assert bool((mean == 0).all()) and bool((rstd.to(F32) == 1).all())
            assert R.bits_equal(y.to(F32), (inp["s"] * inp["gamma"] + inp["beta"]))
            assert bool((y.to(F32).to(BF16).to(F32) == y.to(F32)).all()) and bool((y != 0).all())
            if with_res:
                assert R.bits_equal(s.to(F32), inp["s"])


@pytest.mark.parametrize("dtype,D", [(dt, D) for dt, D, al in RK.LN_CASES if D & (D - 1) == 0 and al], ids=lambda v: str(v).replace("torch.", ""))
def test_layernorm_bwd_exact_premise(dtype, D):
    for rows in RK.ROWS:
        for p, hscale in ((0.0, 1.0), (0.5, 0.5)):
            inp = RK.ln_bwd_inputs(rows, D, dtype, seed=D + rows, exact=True)
            keep = RK.host_keep((rows, D), p, D + rows)
            a32 = RK.ln_bwd(inp["dy"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], inp["ds_extra"], keep, hscale, F32)
            a64 = RK.ln_bwd(inp["dy"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], inp["ds_extra"], keep, hscale, F64)
            for u, v in zip(a32[:2], a64[:2]):
                assert bool((u.to(F64) == v).all())


def test_batchnorm_bwd_exact_premise():
    for rows, C in ((1, 8), (64, 72), (256, 136)):
        for dtype in (F32, BF16):
            inp = RK.bn_bwd_exact_inputs(rows, C, dtype, seed=rows + C)
            a32, a64 = (RK.bn_bwd(inp["g"], inp["x"], inp["mean"], inp["rstd"], inp["gamma"], inp["sdy"], inp["sdyx"], True, None, 0, d) for d in (F32, F64))
            assert bool((a32.to(F64) == a64).all())


def test_offset_rows_and_constant_row_and_tails():
    for dtype in (F32, BF16):
        inp = RK.ln_rule_inputs(9, 512, dtype, True, seed=3, offset=True)
        x = inp["x"].to(F64)[:-1]
        ratio = x.mean(-1).abs() / x.std(-1)
        assert bool((ratio > 100).all()), ratio
        assert float(inp["x"].to(F64)[-1].var()) == 0.0
        y, s, mean, rstd = RK.ln_fwd(inp["x"], None, None, 1.0, inp["gamma"], inp["beta"], RK.LN_EPS, F64, store=dtype)
        assert abs(float(rstd[-1]) - 1e6) < 1.0 and R.bits_equal(y[-1], inp["beta"].to(F64))
        sb = RK.ln_bwd_inputs(9, 512, dtype, seed=3, exact=False, offset=True)["s"].to(F64)
        assert bool((sb.mean(-1).abs() / sb.std(-1) > 100).all())
        t = RK.tails(dtype).to(F64)
        for v in RK.TAILS:
            want = float(torch.tensor(v, dtype=F32).to(dtype))
            assert bool((t == want).any()) and bool((t == -want).any()), v
        assert bool((torch.signbit(t) & (t == 0)).any()) and bool((~torch.signbit(t) & (t == 0)).any())      # both zeros
        assert float(torch.tensor(1e-30).to(dtype)) != 0.0


def test_case_tables_are_what_the_issue_lists():
    assert RK.EW_BIG == 2048 * 256 + 11 and RK.EW_BIG > 524288
    B, T, D = RK.POSENC_SHAPES[1]
    assert B * T * D > 2048 * 256
    for rows, D in RK.LN_PG_SHAPES:
        assert RK.pg_eligible(BF16, rows, D) > 0
    for rows, D in RK.LN_PG_DECLINED:
        assert RK.pg_eligible(BF16, rows, D) == 0
    assert RK.pg_eligible(F32, 2931, 512) == 0
    assert RK.pg_eligible(BF16, 2931, 512) == (2931 + 15) // 16 and 2931 % 16 != 0      # 2 rows per wave, the last block partial
    assert RK.pg_eligible(BF16, 2049, 1032) == 129 and 2049 - 128 * 16 == 1              # the last block holds one row


# ---------------------------------------------------------------------------------------------------------------------------
# the restated dispatch against the source
# ---------------------------------------------------------------------------------------------------------------------------
def _body(src, fn):
    i = src.index('extern "C" int %s(' % fn)
    j = src.find('\nextern "C"', i + 10)
    return src[i:j if j > 0 else len(src)]


def _source_routes():
    norm = open(os.path.join(ROOT, "seq2seq_vc_amd", "csrc", "norm.hip")).read()
    sdp = open(os.path.join(ROOT, "seq2seq_vc_amd", "csrc", "sdp.hip")).read()
    out = {}
    b = _body(norm, "s2svc_layernorm_fwd")
    out["s2svc_layernorm_fwd"] = (set(re.findall(r"S2S_LN_FWD\(\(?([a-z_]+<[^>]*>)", b)), set(map(int, re.findall(r"D <= (\d+)", b))))
    b = _body(norm, "s2svc_layernorm_bwd")
    out["s2svc_layernorm_bwd"] = (set(re.findall(r"hipLaunchKernelGGL\(\(?([a-z_]+<[^>]*>)", b)), set(map(int, re.findall(r"D <= (\d+)", b))))
    b = _body(norm, "s2svc_layernorm_bwd_pg")
    out["s2svc_layernorm_bwd_pg"] = ({"ln_bwd_vec_pg_kernel<%s>" % n for n in re.findall(r"S2S_LN_PG\((\d)\);", b)}, set(map(int, re.findall(r"D <= (\d+)", b))))
    for fn, macro, kern in (("s2svc_ln_act_fwd", "S2S_LNACT", "ln_act_fwd_kernel"), ("s2svc_ln_act_bwd", "S2S_LNACTB", "ln_act_bwd_kernel")):
        b = _body(sdp, fn)
        out[fn] = ({"%s<%s>" % (kern, a) for a in re.findall(macro + r"\(([^)]*)\);", b)}, set(map(int, re.findall(r"D <= (\d+)", b))))
    b = _body(sdp, "s2svc_dw_ln_act_fwd")
    out["s2svc_dw_ln_act_fwd"] = ({"dw_ln_act_fwd_kernel<float, %s>" % a for a in re.findall(r"S2S_DWLN\(([^)]*)\);", b)}, set(map(int, re.findall(r"D <= (\d+)", b))))
    vec = norm[norm.index("static bool ln_vec_ok("):]
    out["ln_vec_ok"] = (set(), set(map(int, re.findall(r"D > (\d+)", vec[:vec.index("}\n\n")]))))
    return out


def test_dispatch_matches_source_and_every_instantiation_has_a_case():
    src = _source_routes()
    counts = {"s2svc_layernorm_fwd": 9, "s2svc_layernorm_bwd": 5, "s2svc_layernorm_bwd_pg": 3, "s2svc_ln_act_fwd": 8, "s2svc_ln_act_bwd": 8, "s2svc_dw_ln_act_fwd": 3}
    for fn, n in counts.items():
        assert len(src[fn][0]) == n, (fn, sorted(src[fn][0]))
    assert src["s2svc_layernorm_fwd"][1] == set(RK.LN_THRESH) and src["s2svc_layernorm_bwd"][1] == set(RK.LN_THRESH)
    assert src["s2svc_layernorm_bwd_pg"][1] == set(RK.LN_THRESH)
    assert src["ln_vec_ok"][1] == {RK.LN_VEC_MAX}
    assert src["s2svc_ln_act_fwd"][1] == set(RK.LN_ACT_THRESH) | {RK.LN_ACT_MAX} and src["s2svc_ln_act_bwd"][1] == src["s2svc_ln_act_fwd"][1]
    assert src["s2svc_dw_ln_act_fwd"][1] == set(RK.DW_LN_ACT_THRESH) | {RK.DW_LN_ACT_MAX}
    in_source = set().union(*(v[0] for v in src.values()))
    covered = RK.ln_routes_covered()
    assert in_source - set(covered) == set(), f"kernel instantiations without a case: {sorted(in_source - set(covered))}"
    assert set(covered) - in_source == set(), f"the restated dispatch names kernels the source does not launch: {sorted(set(covered) - in_source)}"
    # the tables sit on both sides of every threshold
    for dtype in (F32, BF16):
        ds = [D for dt, D, al in RK.LN_CASES if dt == dtype and al]
        for th in RK.LN_THRESH + ((RK.LN_VEC_MAX,) if dtype == BF16 else ()):        # (fp32 has one kernel above 1024)
            assert th in ds and th + 8 in ds, (dtype, th)
    for th in RK.LN_ACT_THRESH:
        assert th in RK.LN_ACT_D and th + 8 in RK.LN_ACT_D
    assert RK.LN_ACT_MAX in RK.LN_ACT_D and RK.DW_LN_ACT_MAX in RK.DW_D and 256 in RK.DW_D and 264 in RK.DW_D
    # misaligned pointers and D % 8 != 0 leave the 16-byte routes
    assert RK.ln_fwd_route(BF16, 384, True) == "ln_fwd_vec_kernel<1>" and RK.ln_fwd_route(BF16, 384, False) == "ln_fwd_reg_kernel<bf16_t, 8>"
    assert RK.ln_fwd_route(BF16, 1004, True) == "ln_fwd_reg_kernel<bf16_t, 16>" and RK.ln_fwd_route(BF16, 1030, True) == "ln_fwd_kernel<bf16_t>"
    assert RK.ln_fwd_route(BF16, 2056, True) == "ln_fwd_kernel<bf16_t>" and RK.ln_bwd_route(BF16, 2056, True) == "ln_bwd_kernel<bf16_t>"


# ---------------------------------------------------------------------------------------------------------------------------
# power: every planted error is rejected by the regime that exists for it (applied to the restatement, on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------
def rule_rejects(got, ref64, yard, out_dtype):
    ok, ratio, d, msg = R.compare(got, ref64, yard, out_dtype, R.MARGIN)
    return not ok


def rule_accepts_own_yard(ref64, yard, out_dtype):
    return R.compare(yard, ref64, yard, out_dtype, R.MARGIN)[0]


def test_planted_one_pass_variance_rule():
    for dtype in (F32, BF16):
        inp = RK.ln_rule_inputs(9, 512, dtype, False, seed=3, offset=True)
        a = (inp["x"], None, None, 1.0, inp["gamma"], inp["beta"], RK.LN_EPS)
        ref, yard, bad = RK.ln_fwd(*a, F64, store=dtype), RK.ln_fwd(*a, F32, store=dtype), RK.ln_fwd(*a, F32, store=dtype, one_pass=True)
        assert rule_accepts_own_yard(ref[3][:-1], yard[3][:-1], F32)
        assert rule_rejects(bad[3][:-1], ref[3][:-1], yard[3][:-1], F32)            # rstd
        if dtype == F32:                                                            # (a bf16 ulp of y hides a 0.5 % error of rstd)
            assert rule_rejects(bad[0], ref[0], yard[0], dtype)


def test_planted_statistics_before_rounding_rule():
    inp = RK.ln_rule_inputs(9, 512, BF16, True, seed=4)
    keep = RK.host_keep((9, 512), 0.5, 4)
    a = (inp["x"], inp["res"], keep, 0.5, inp["gamma"], inp["beta"], RK.LN_EPS)
    ref, yard = RK.ln_fwd(*a, F64, store=BF16), RK.ln_fwd(*a, F32, store=BF16)
    bad = RK.ln_fwd(*a, F32, store=BF16, stats_before_rounding=True)
    assert rule_accepts_own_yard(ref[2], yard[2], F32)
    assert rule_rejects(bad[2], ref[2], yard[2], F32)                               # mean
    assert rule_rejects(bad[3][:-1], ref[3][:-1], yard[3][:-1], F32)                # rstd


def exact_rejects(inp, keep, hscale, store, **plant):
    want = RK.exact_premise(ln_fwd_exact_fn(inp, keep, hscale, store))
    bad = ln_fwd_exact_fn(inp, keep, hscale, store, **plant)(F32)
    return not R.bits_equal(bad[0].to(store), want[0].to(F32).to(store))


def test_planted_gamma_shift_exact():
    for dtype, D in ((F32, 520), (BF16, 512), (BF16, 1032)):
        inp = RK.ln_fwd_exact_inputs(5, D, dtype, False, None, 1.0, seed=D)
        assert exact_rejects(inp, None, 1.0, dtype, gamma_shift=8)


def test_planted_tail_channels_left_out_exact():
    for dtype, D in ((F32, 50), (BF16, 504), (BF16, 1032)):
        assert D % 64
        inp = RK.ln_fwd_exact_inputs(5, D, dtype, False, None, 1.0, seed=D)
        assert exact_rejects(inp, None, 1.0, dtype, skip_tail=D % 64)


def test_planted_hscale_after_residual_exact():
    inp = RK.ln_fwd_exact_inputs(5, 64, BF16, True, None, 0.5, seed=1)
    assert exact_rejects(inp, None, 0.5, BF16, hscale_after=True)
    assert not exact_rejects(inp, None, 0.5, BF16)


def test_planted_missing_dropout_scale_in_dh_exact():
    inp = RK.ln_bwd_inputs(5, 64, BF16, seed=2, exact=True)
    keep = RK.host_keep((5, 64), 0.5, 2)
    a = (inp["dy"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], inp["ds_extra"], keep, 0.5)
    want, bad = RK.ln_bwd(*a, F64), RK.ln_bwd(*a, F32, no_keep_scale=True)
    assert R.bits_equal(bad[0].to(BF16), want[0].to(F32).to(BF16)) and not R.bits_equal(bad[1].to(BF16), want[1].to(F32).to(BF16))


def test_planted_mask_by_column_exact():
    rows, D = 5, 64
    keep = RK.host_keep((rows, D), 0.5, 9)
    inp = RK.ln_fwd_exact_inputs(rows, D, BF16, True, keep, 1.0, seed=9)
    want = RK.exact_premise(ln_fwd_exact_fn(inp, keep, 1.0, BF16))
    bad = ln_fwd_exact_fn(inp, keep[0:1].expand(rows, D), 1.0, BF16)(F32)          # every row under row 0's mask: the index is the column
    assert not R.bits_equal(bad[1].to(BF16), want[1].to(F32).to(BF16)) and not R.bits_equal(bad[0].to(BF16), want[0].to(F32).to(BF16))


def test_planted_empty_utterance_not_zeroed_bits():
    m = RK.LN_ACT_LENS
    rows, D = m["B"] * m["T"], 24
    x, res = R.randn(rows, D, seed=1), R.randn(rows, D, seed=2)
    gamma, beta = torch.ones(D), torch.zeros(D)
    bad = RK.ln_act_fwd(x, gamma, beta, 1e-5, "gelu", res, m["lens"], m["T"], None, F32, zero_empty=False)[0]
    good = RK.ln_act_fwd(x, gamma, beta, 1e-5, "gelu", res, m["lens"], m["T"], None, F32)[0]
    masked = ~RK.row_valid(rows, m["T"], m["lens"])
    assert int(masked.sum()) == 5
    assert R.bits_equal(good[masked], torch.zeros(5, D)) and not R.bits_equal(bad[masked], torch.zeros(5, D))


def test_planted_tanh_derivative_of_dropped_output_rule():
    for dtype in (F32, BF16):
        n = 4099
        x, dz = R.randn(n, seed=5, dtype=dtype), R.randn(n, seed=6, dtype=dtype)
        keep = RK.host_keep((n,), 0.5, 7)
        saved = RK.act_dropout_fwd(x, "tanh", keep, F32, store=dtype).to(dtype)
        ref, yard = (RK.act_dropout_bwd(dz, saved, "tanh", keep, d, store=dtype) for d in (F64, F32))
        bad = RK.act_dropout_bwd(dz, saved, "tanh", keep, F32, store=dtype, divide=False)
        assert rule_accepts_own_yard(ref, yard, dtype) and rule_rejects(bad, ref, yard, dtype)


def test_planted_add_n_pairwise_bit_pin():
    xs = [R.randn(4099, seed=70 + i) for i in range(4)]
    assert not R.bits_equal(RK.add_n(xs, F32, pairwise=True), RK.add_n(xs, F32))
    assert R.bits_equal(RK.add_n(xs[:3], F32, pairwise=True), RK.add_n(xs[:3], F32))          # (three inputs have one order)
