"""CPU tests behind tests/gpu_step_kernel_check.py: the float64 restatements of tests/step_kernels_ref.py are pinned to oracle/models.py and to
stock torch (so the GPU checks compare the kernels with something that is itself proven), the comparison rule is checked on known
values, the conditions the GPU cases rely on are asserted on the very inputs they use, and the coverage ledger requires a
kernel-level check for every launcher include/s2svc_hip.h declares.  None of this touches the package's kernels."""
import ast
import glob
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_kernels_ref as R
from oracle import models as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def close64(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------------------
def test_ulp_out_is_the_spacing_of_the_output_type():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, 3.0e-5, 1000.0, 3.0e38], dtype=F64)
    want32 = (torch.nextafter(x.float(), torch.tensor(float("inf"))).double() - x.float().double())
    assert torch.equal(R.ulp_out(x, F32), want32)
    assert torch.equal(R.ulp_out(-x, F32), want32)
    assert torch.equal(R.ulp_out(x, BF16), want32 * 2.0 ** 16)
    assert float(R.ulp_out(torch.tensor([0.0], dtype=F64), F32)) == 2.0 ** -149 and float(R.ulp_out(torch.tensor([1e-42], dtype=F64), BF16)) == 2.0 ** -133


def test_compare_rule():
    ref = torch.tensor([1.0, 2.0, 0.0], dtype=F64)
    yard = ref + torch.tensor([1e-6, 0.0, 0.0], dtype=F64)                    # d = 1e-6
    ok, ratio, d, _ = R.compare(ref + 3.9e-6, ref, yard, F32)
    assert ok and abs(d - 1e-6) < 1e-15 and abs(ratio - 3.9) < 1e-6
    assert not R.compare(ref + torch.tensor([0.0, 0.0, 4.2e-6], dtype=F64), ref, yard, F32)[0]     # every element is held to the bound
    assert not R.compare(torch.tensor([1.0, float("nan"), 0.0], dtype=F64), ref, yard, F32)[0]
    assert R.compare(ref + torch.tensor([0.0, 2.0 ** -22, 0.0], dtype=F64), ref, ref, F32)[0]      # d = 0: one ulp of the output is left
    assert not R.compare(ref + torch.tensor([0.0, 2.0 ** -21, 0.0], dtype=F64), ref, ref, F32)[0]
    assert R.bits_equal(torch.tensor([0.0]), torch.tensor([0.0])) and not R.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))


# ---------------------------------------------------------------------------------------------------------------------------
# decode step
# ---------------------------------------------------------------------------------------------------------------------------
def test_decode_attn_restatement_vs_explicit_softmax():
    B, H, dk, Tk = 3, 2, 5, 9
    q, k, v = R.randn(B, H, dk, seed=1).double(), R.randn(B, Tk, H, dk, seed=2).double(), R.randn(B, Tk, H, dk, seed=3).double()
    n = [9, 4, 0]
    ctx, att = R.decode_attn(q, k, v, n, 0.37, F64)
    for b in range(B):
        for h in range(H):
            s = np.array([0.37 * float((q[b, h] * k[b, j, h]).sum()) for j in range(n[b])])
            p = np.exp(s - s.max()) / np.exp(s - s.max()).sum() if n[b] else np.zeros(0)
            close64(att[b, h, :n[b]], p)
            assert bool((att[b, h, n[b]:] == 0).all())
            close64(ctx[b, h], sum((p[j] * v[b, j, h] for j in range(n[b])), torch.zeros(dk, dtype=F64)))
    # and against torch.softmax over the masked scores, as attention.py states it
    sc = torch.einsum("bthd,bhd->bht", k, q) * 0.37
    mask = torch.arange(Tk)[None, None, :] >= torch.tensor(n)[:, None, None]
    pr = torch.softmax(sc.masked_fill(mask, -float("inf")), -1).masked_fill(mask, 0.0).nan_to_num(0.0)
    close64(att, pr)
    close64(ctx, torch.einsum("bht,bthd->bhd", pr, v))


def test_ln_linear_restatement_vs_explicit_formula():
    M, Kd, N = 5, 12, 7
    x, w, b = R.randn(M, Kd, seed=4).double(), R.randn(N, Kd, seed=5).double(), R.randn(N, seed=6).double()
    g, be, r = R.randn(Kd, seed=7).double(), R.randn(Kd, seed=8).double(), R.randn(M, N, seed=9).double()
    out, y = R.ln_linear(x, w, b, (g, be, 1e-5), "relu", r, F64)
    mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    y_ = (x - mu) / torch.sqrt(var + 1e-5) * g + be
    close64(y, y_)
    close64(out, torch.clamp(y_ @ w.t() + b, min=0) + r)
    close64(R.ln_linear(x, w, b, None, None, None, F64)[0], F.linear(x, w, b))
    close64(R.ln_linear(x, w, b, (g, be, 1e-5), None, None, F64)[0], F.linear(F.layer_norm(x, (Kd,), g, be, 1e-5), w, b))
    # the float32 yardstick rounds LayerNorm's output and the result to bf16, nothing else
    xb, wb = x.to(BF16), w.to(BF16)
    o, yb = R.ln_linear(xb, wb, b.float(), (g.float(), be.float(), 1e-5), None, None, F32, bf16=True)
    y32 = F.layer_norm(xb.float(), (Kd,), g.float(), be.float(), 1e-5).to(BF16).float()
    assert torch.equal(yb, y32) and torch.equal(o, F.linear(y32, wb.float(), b.float()).to(BF16).float())


def test_stop_rule_rows():
    for r in (1, 4):
        lg, minlen, maxlen, stop0, want = R.emit_rows(r)
        assert want == [3, 5, 4, 2, 0]
        assert float(torch.sigmoid(lg[0, 2, r - 1])) == 0.5                       # the planted logit is exactly at the threshold
        p = torch.sigmoid(lg.double())
        assert float((p - 0.5).abs()[p != 0.5].min()) > 0.4                        # every other decision is far from it
    assert R.stop_rule([[0.1], [0.9]], 0.5, 0, 100) == 2 and R.stop_rule([[0.9], [0.1], [0.1]], 0.5, 3, 100) == 0
    assert R.stop_rule([[0.1]] * 5, 0.5, 0, 3) == 3 and R.stop_rule([[0.1]] * 5, 0.5, 5, 3) == 5


def test_decode_posenc_restatement():
    x, pe = R.randn(3, 8, seed=10).double(), R.randn(5, 8, seed=11).double()
    close64(R.decode_posenc(x, 2.5, torch.tensor([0.7], dtype=F64), pe, 4, F64), x * 2.5 + 0.7 * pe[4])
    close64(R.decode_posenc(x, 2.5, None, pe, 0, F64), x * 2.5 + pe[0])


# ---------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 80])
@pytest.mark.parametrize("pos_weight", [1.0, 10.0])
def test_seq_loss_restatement_vs_oracle_and_stock_torch(D, pos_weight):
    B, Tm, olens = 5, 37, [37, 1, 0, 20, 36]
    ys, after, before = (R.randn(B, Tm, D, seed=20 + i).double() for i in range(3))
    after[0, 3] = ys[0, 3]
    logits = 3 * R.randn(B, Tm, seed=24).double()
    logits[0, :4] = torch.tensor([30.0, -30.0, 90.0, -90.0], dtype=F64)
    labels = (torch.rand(B, Tm, generator=R.gen(25)) < 0.3).double()
    l1, bce, cnt, da, db, dl = R.seq_loss(after, before, logits, ys, labels, olens, pos_weight, F64, g_l1=0.7, g_bce=1.3, want_grads=True)
    o1, o2 = OM.seq2seq_loss(after, before, logits, ys, labels, torch.tensor(olens), bce_pos_weight=pos_weight)
    close64(l1, o1), close64(bce, o2.double())
    s = R.seq_loss_stock(after, before, logits, ys, labels, olens, pos_weight, F64, g_l1=0.7, g_bce=1.3, want_grads=True)
    close64(l1, s[0]), close64(bce, s[1])
    assert cnt == s[2] == sum(olens)
    close64(da, s[3]), close64(db, s[4]), close64(dl, s[5])
    m = R.frame_mask(olens, Tm)
    assert bool((da[~m] == 0).all() and (dl[~m] == 0).all() and (da[0, 3] == 0).all())
    # the variants without `after` / `logits`
    l1b, bceb, _, dab, dbb, dlb = R.seq_loss(None, before, None, ys, labels, olens, pos_weight, F64, want_grads=True)
    sb = R.seq_loss_stock(None, before, None, ys, labels, olens, pos_weight, F64, want_grads=True)
    close64(l1b, F.l1_loss(before.masked_select(m[:, :, None]), ys.masked_select(m[:, :, None])))
    assert float(bceb) == 0.0 and dab is None and dlb is None
    close64(dbb, sb[4])


@pytest.mark.parametrize("sigma", [0.4, 0.2])
def test_guided_attn_restatement_vs_oracle(sigma):
    B, H, To, Ti = 3, 2, 37, 29
    att = torch.rand(B, H, To, Ti, generator=R.gen(30)).double()
    for ilens, olens in (([29, 1, 0], [37, 1, 12]), ([29, 13, 29], [37, 20, 0])):
        loss, cnt, datt = R.guided_attn_loss(att, ilens, olens, sigma, 5.0, F64, gout=0.6)
        # the oracle builds its weights in float32 (as the reference does): agreement to float32 accuracy, not float64
        close64(loss, OM.guided_attention_loss(att, torch.tensor(ilens), torch.tensor(olens), sigma=sigma, alpha=5.0), tol=1e-6)
        a = att.clone().requires_grad_(True)
        w = R.guided_attn_weights(To, Ti, ilens, olens, sigma, F64)
        m = (R.frame_mask(olens, To)[:, :, None] & R.frame_mask(ilens, Ti)[:, None, :])[:, None]
        stock = 5.0 * torch.mean((w[:, None] * a).masked_select(m))
        close64(loss, stock.detach())
        (0.6 * stock).backward()
        close64(datt, a.grad)
        assert cnt == int(m.expand(B, H, To, Ti).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# length regulator, durations, bin loss
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tx", [1, 255, 257])
def test_length_regulator_restatement_vs_repeat_interleave_and_oracle(Tx):
    B, D = 3, 4
    ds = torch.randint(0, 5, (B, Tx), generator=R.gen(40 + Tx), dtype=torch.int64)
    ds[0, Tx // 2] = 40
    x = R.randn(B, Tx, D, seed=41).double()
    tot = int(ds.sum(1).max())
    start, idx, total = R.length_regulate_index(ds.numpy(), tot)
    assert np.array_equal(total, ds.sum(1).numpy()) and np.array_equal(start, (torch.cumsum(ds, 1) - ds).numpy())
    y = R.length_regulate_fwd(x, idx, -3.5)
    for b in range(B):
        rep = torch.repeat_interleave(x[b], ds[b], dim=0)
        assert torch.equal(y[b, :rep.shape[0]], rep) and bool((y[b, rep.shape[0]:] == -3.5).all())
    assert torch.equal(y, OM.length_regulator(x, ds, pad_value=-3.5))
    # a negative duration counts as 0; a Tout below the total cuts the run, above it leaves -1 / pad
    dn = ds.clone()
    dn[1, Tx - 1] = -3
    s2, i2, t2 = R.length_regulate_index(dn.numpy(), tot + 5)
    assert np.array_equal(t2, dn.clamp(min=0).sum(1).numpy()) and (i2[:, tot:] == -1).all()
    s3, i3, _ = R.length_regulate_index(dn.numpy(), max(tot - 17, 1))
    assert np.array_equal(i3, i2[:, :max(tot - 17, 1)])
    # the gradient: autograd through the gather, and the stock index_add_ form
    dy = R.randn(B, i3.shape[1], D, seed=42).double()
    xx = x.clone().requires_grad_(True)
    (R.length_regulate_fwd(xx, i3, 0.0) * dy).sum().backward()
    close64(R.length_regulate_bwd(dy, s3, dn.numpy(), Tx, F64), xx.grad)
    close64(R.length_regulate_bwd_stock(dy, i3, Tx, F64), xx.grad)


def test_attn_durations_restatement_vs_oracle_and_input_conditions():
    inputs = [(s, R.attn_durations_input(*s, seed=1700 + i)) for i, s in enumerate(R.ATTN_DUR_SHAPES)]
    for (NH, Tf, Tx), att in inputs:
        dur, scores, head = R.attn_durations(att, F64)
        d_o, f_o = OM.duration_calculator(att.double()[None])                    # (layers = 1, heads, Tf, Tx)
        assert torch.equal(dur, d_o) and float(f_o) == float(scores[head]) and int(dur.sum()) == Tf
        if NH > 1:                                                                 # the condition of the GPU case: the best two heads are apart
            top = torch.sort(scores, descending=True)[0]
            assert float(top[0] - top[1]) > 1e-3, (NH, Tf, Tx, float(top[0] - top[1]))
        if Tx > 1:                                                                 # duplicated row maxima are there, so the first arg-max decides
            row = att[head].double()
            assert int((row == row.max(-1, keepdim=True)[0]).sum(-1).max()) >= 2
    twin = R.attn_durations_input(4, 257, 7, seed=1790, twin_heads=True)
    _, scores, head = R.attn_durations(twin, F64)
    assert head == 0 and float(scores[0]) == float(scores[1]) == float(scores.max())


def test_mas_binloss_bwd_restatement_vs_autograd():
    B, Tf, Tx = 3, 20, 6
    flens = [20, 11, 29]
    path = torch.randint(0, Tx, (B, Tf), generator=R.gen(50), dtype=torch.int32)
    path[1, 11:] = -1
    lp = R.randn(B, Tf, Tx, seed=51).double().requires_grad_(True)
    loss = 0
    for b in range(B):                                                            # modules/alignments.py:299-309
        n = min(flens[b], Tf)
        loss = loss - lp[b, torch.arange(n), path[b, :n].long()].mean()
    (0.8 * loss / B).backward()
    base = R.randn(B, Tf, Tx, seed=52).double()
    close64(R.mas_binloss_bwd(path, flens, 0.8, base, F64), base + lp.grad)


# ---------------------------------------------------------------------------------------------------------------------------
# optimiser
# ---------------------------------------------------------------------------------------------------------------------------
def test_warmup_lr_restatement_vs_oracle():
    for w in (2, 4000):
        for step in (1, 2, 3, 4000, 5000):
            close64(R.warmup_lr(1e-3, step, w, F64), OM.warmup_lr(1e-3, step, w))
    assert float(R.warmup_lr(0.05, 7, 0, F64)) == 0.05


@pytest.mark.parametrize("n", [1, 5, 1021])
@pytest.mark.parametrize("max_norm", [0.0, 1e6, 0.5])
def test_adam_restatement_vs_oracle_and_torch_optim(n, max_norm):
    betas, eps, lr, warm = (R.f32(0.9), R.f32(0.999)), R.f32(1e-8), 0.05, 2
    p, m, v = R.randn(n, seed=60).double(), 0.1 * R.randn(n, seed=61).double(), 0.01 * torch.rand(n, generator=R.gen(62)).double() + 1e-4
    tp = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps)
    opt.state[tp] = {"step": torch.tensor(0.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    op, om, ov = p.clone(), m.clone(), v.clone()
    for step in (1, 2, 3):
        g = R.randn(n, seed=63 + step).double()
        p, m, v, state = R.adam_step(p, g, m, v, step, lr, betas, eps, max_norm, warm, F64)
        rate = OM.warmup_lr(lr, step, warm)
        close64(state[1], rate)
        # stock torch
        tp.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([tp], max_norm)
        for grp in opt.param_groups:
            grp["lr"] = rate
        opt.step()
        close64(p, tp.detach(), tol=1e-11), close64(m, opt.state[tp]["exp_avg"]), close64(v, opt.state[tp]["exp_avg_sq"])
        # the oracle's replay (its clip is always on: compare where this one clips too)
        if max_norm > 0:
            OM.adam_step([op], [g.clone()], [(om, ov)], rate, step, betas=betas, eps=eps, grad_clip=max_norm)
            close64(p, op, tol=1e-6), close64(m, om, tol=1e-6), close64(v, ov, tol=1e-6)     # the oracle rounds its norm to float32
        close64(state[2], torch.linalg.vector_norm(g))
        assert float(state[0]) == step and (max_norm != 1e6 or float(state[3]) == 1.0)


def test_shadow_probe_values_hold_the_cases_they_name():
    pv = R.shadow_probe_values()
    bits = pv.view(torch.int32) & 0xFFFF
    assert int((bits == 0x8000).sum()) >= 5                                       # exact ties
    b = pv.to(BF16).float()
    assert float(b[0]) == 1.0 and float(b[1]) == 1.015625 and float(b[4]) == 2.0  # to even: down, up, and up into the next exponent
    assert math.copysign(1.0, float(pv[7])) == -1.0 and float(pv[7]) == 0.0
    assert 0 < float(pv[9]) < 2.0 ** -126
    assert float(b[14]) == float(b[13]) == -float(b[15]) and torch.isfinite(b[14])         # 3.39e38 rounds to the largest bf16 ...
    assert torch.isinf(b[16]) and torch.isinf(b[17])                                        # ... 3.40e38 to infinity


# ---------------------------------------------------------------------------------------------------------------------------
# glue
# ---------------------------------------------------------------------------------------------------------------------------
def test_glue_restatements_on_small_examples():
    ys = torch.arange(2 * 7 * 1, dtype=F32).view(2, 7, 1) + 1
    assert R.decoder_input(ys, 3)[0, :, 0].tolist() == [0.0, 3.0] and R.decoder_input(ys, 1)[1, :, 0].tolist() == [0.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0]
    xs = torch.tensor([[5, 6, 7], [8, 9, 9]])
    assert R.append_eos(xs, [3, 1], 1, 0).tolist() == [[5, 6, 7, 1], [8, 1, 9, 0]]
    lab = torch.zeros(3, 5)
    lab[2, 1] = 1.0
    assert R.stop_labels(lab, [4, 1, 0], 4).tolist() == [[0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]]
    xs_ = [torch.tensor([1.0, 2.0]), torch.tensor([4.0])]
    assert float(R.weighted_sum(xs_, [2.0, -1.0], F64)) == 2.0
    nan = torch.full((2,), float("nan"))
    assert R.scalars_axpy(xs_, [2.0, -1.0], nan, 0.0, F64).tolist() == [6.0, -4.0]
    assert R.scalars_axpy(xs_, [2.0, -1.0], torch.tensor([1.0, 1.0]), 0.5, F64).tolist() == [6.5, -3.5]


# ---------------------------------------------------------------------------------------------------------------------------
# s2svc_decode_ln_linear_supported: a host function of the library, callable without a device
# ---------------------------------------------------------------------------------------------------------------------------
def test_ln_linear_supported_table():
    from seq2seq_vc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library(verbose=False)
    L = _lib.lib()
    for dtype, M, Kd, want in R.ln_linear_supported_table():
        assert L.s2svc_decode_ln_linear_supported(0 if dtype == F32 else 1, M, Kd) == want, (dtype, M, Kd)
    assert L.s2svc_decode_ln_linear_supported(7, 16, 80) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the coverage ledger
# ---------------------------------------------------------------------------------------------------------------------------
# Launchers that no tests/gpu_*check*.py module calls by name or through its Python wrapper.  ("case", module, case name): the case of that
# module that reaches the launcher through a functional layer; ("not a kernel", reason): an entry point that computes nothing on the GPU.
LEDGER = {
    "s2svc_abi_version": ("not a kernel", "returns a constant; test_host_logic checks it"),
    "s2svc_event_create": ("not a kernel", "hipEventCreate for the stage graphs: stream ordering, no arithmetic"),
    "s2svc_event_destroy": ("not a kernel", "hipEventDestroy"),
    "s2svc_event_record": ("not a kernel", "hipEventRecord"),
    "s2svc_stream_wait_event": ("not a kernel", "hipStreamWaitEvent"),
    "s2svc_gemm_last_route": ("not a kernel", "returns the name of the kernel the last s2svc_gemm call launched; gpu_gemm_kernel_check holds every case to it"),
    "s2svc_launch_floor": ("not a kernel", "launches a kernel that computes nothing: a timing probe of tools/ and bench.py"),
    "s2svc_gl_supported": ("not a kernel", "host-side size query; test_griffin_lim_host pins its table"),
    "s2svc_hifigan_cin_padded": ("not a kernel", "host-side padding query of the vocoder's weight layout"),
    "s2svc_stft_logmel_fft_supported": ("not a kernel", "host-side size query of the STFT front-end"),
    "s2svc_dwconv": ("case", "gpu_kernel_check_aas", "depthwise_conv"),                       # = s2svc_dwconv_add with add = NULL
    "s2svc_rstd_from_var": ("case", "gpu_kernel_check", "batchnorm_act_dropout_vectorised"),
    "s2svc_convmod_supported": ("case", "gpu_kernel_check_aas", "conformer_conv_module_fused"),
    "s2svc_convmod_wgrad_final": ("case", "gpu_kernel_check_aas", "conformer_conv_module_fused"),
    "s2svc_bn_swish_apply": ("case", "gpu_kernel_check_aas", "conformer_conv_module_fused"),
    "s2svc_embedding_fwd": ("case", "gpu_kernel_check_aas", "embedding_and_duration_loss"),
    "s2svc_embedding_bwd": ("case", "gpu_kernel_check_aas", "embedding_and_duration_loss"),
    "s2svc_duration_loss_fwd": ("case", "gpu_kernel_check_aas", "embedding_and_duration_loss"),
    "s2svc_duration_loss_bwd": ("case", "gpu_kernel_check_aas", "embedding_and_duration_loss"),
    "s2svc_expand_fwd": ("case", "gpu_kernel_check_aas", "sdp_ln_act_expand_mask"),
    "s2svc_expand_bwd": ("case", "gpu_kernel_check_aas", "sdp_ln_act_expand_mask"),
    "s2svc_forward_sum": ("case", "gpu_kernel_check_aas", "forward_sum_ctc"),
    "s2svc_forward_sum_ws_bytes": ("case", "gpu_kernel_check_aas", "forward_sum_ctc"),
    "s2svc_rowscale": ("case", "gpu_kernel_check_aas", "forward_sum_ctc"),
    "s2svc_sdp_head_fwd": ("case", "gpu_kernel_check_aas", "sdp_module_vs_oracle"),
    "s2svc_sdp_head_bwd": ("case", "gpu_kernel_check_aas", "sdp_module_vs_oracle"),
    "s2svc_sdp_mid_fwd": ("case", "gpu_kernel_check_aas", "sdp_module_vs_oracle"),
    "s2svc_sdp_mid_bwd": ("case", "gpu_kernel_check_aas", "sdp_module_vs_oracle"),
    "s2svc_sdp_tail_fwd": ("case", "gpu_kernel_check_aas", "sdp_module_vs_oracle"),
    "s2svc_sdp_tail_bwd": ("case", "gpu_kernel_check_aas", "sdp_module_vs_oracle"),
    "s2svc_sdp_inverse_out": ("case", "gpu_kernel_check_aas", "sdp_module_vs_oracle"),
    "s2svc_stft_logmel_fft": ("case", "gpu_kernel_check_aas", "stft_logmel_frontend"),
    "s2svc_stft_logmel_fft8": ("case", "gpu_kernel_check_aas", "stft_logmel_frontend"),
    "s2svc_ragged_to_padded": ("case", "gpu_kernel_check_aas", "stft_logmel_batched_and_device_collaters"),
    "s2svc_gl_prepare": ("case", "gpu_griffin_lim_check", "decode_normalised_logmel"),
    "s2svc_gl_ola": ("case", "gpu_griffin_lim_check", "istft_alone"),
    "s2svc_hifigan_input": ("case", "gpu_vocoder_check", "hifigan_tiny_vs_reference_fp32"),
    "s2svc_mask_rows": ("case", "gpu_kernel_check_aas", "sdp_ln_act_expand_mask"),
    "s2svc_useg_stretch": ("case", "gpu_urhythmic_check", "stretch_segments_vs_interpolate"),
}


def _declared_launchers():
    from seq2seq_vc_amd import _lib
    return _lib.exported_symbols()


def _wrappers(declared):
    """symbol -> {(module, function)}: the Python functions of ops/kernels*.py and frontend.py whose body names it."""
    files = sorted(glob.glob(os.path.join(ROOT, "seq2seq_vc_amd", "ops", "kernels*.py"))) + [os.path.join(ROOT, "seq2seq_vc_amd", "frontend.py")]
    out = {n: set() for n in declared}
    for f in files:
        src = open(f).read()
        for node in ast.walk(ast.parse(src)):
            if isinstance(node, ast.FunctionDef) and not (node.name.startswith("__") and node.name.endswith("__")):
                seg = ast.get_source_segment(src, node)
                for n in re.findall(r"\bs2svc_[a-z0-9_]+\b", seg):
                    if n in out:
                        out[n].add((os.path.basename(f)[:-3], node.name))
    return out


# tests/gpu_model_check.py is a MODEL-level module: a launcher it reaches is not thereby checked at kernel level
MODEL_LEVEL = {"gpu_model_check"}


def _check_modules():
    """kernel-level module name -> (source text, names of its cases: functions decorated with @case or listed in CASES = [...],
    aliases: the names under which it imports ops/kernels*.py and frontend.py, alias -> module)."""
    mods = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "gpu_*check*.py"))):
        name = os.path.basename(f)[:-3]
        if name in MODEL_LEVEL:
            continue
        src = open(f).read()
        tree, cases, aliases = ast.parse(src), set(), {}
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and any((isinstance(d, ast.Name) and d.id == "case") for d in node.decorator_list):
                cases.add(node.name)
            if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "CASES" for t in node.targets) and isinstance(node.value, ast.List):
                cases |= {e.id for e in node.value.elts if isinstance(e, ast.Name)}
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module in ("seq2seq_vc_amd.ops", "seq2seq_vc_amd"):
                for a in node.names:
                    if a.name.startswith("kernels") or a.name == "frontend":
                        aliases[a.asname or a.name] = a.name
            if isinstance(node, ast.ImportFrom) and node.module and re.fullmatch(r"seq2seq_vc_amd\.(ops\.kernels\w*|frontend)", node.module):
                for a in node.names:                     # from seq2seq_vc_amd.frontend import logmelfilterbank
                    aliases[":" + (a.asname or a.name)] = node.module.rsplit(".", 1)[1] + ":" + a.name
        mods[name] = (src, cases, aliases)
    return mods


def _called_in(mod, wrapper):
    """True if the kernel-level module calls `wrapper` = (module, function) under one of the names it imports that module by."""
    src, _, aliases = mod
    for al, m in aliases.items():
        if al.startswith(":"):                           # the function itself, imported by name
            if m == "%s:%s" % wrapper and re.search(r"(?<![A-Za-z0-9_.])%s\(" % re.escape(al[1:]), src):
                return True
        elif m == wrapper[0] and re.search(r"(?<![A-Za-z0-9_.])%s\.%s\(" % (re.escape(al), re.escape(wrapper[1])), src):
            return True
    return False


def test_every_launcher_has_a_kernel_level_check():
    declared = _declared_launchers()
    assert len(declared) > 100
    wrappers, mods = _wrappers(declared), _check_modules()
    texts = [m[0] for m in mods.values()]
    missing, stale = [], []
    for sym in declared:
        direct = any(re.search(r"\b%s\(" % sym, t) for t in texts) or any(_called_in(m, w) for w in wrappers[sym] for m in mods.values())
        if direct:
            if sym in LEDGER:
                stale.append(sym)
            continue
        entry = LEDGER.get(sym)
        if entry is None:
            missing.append(f"{sym} (wrappers: {sorted(wrappers[sym]) or 'none in ops/kernels*.py, frontend.py'})")
        elif entry[0] == "case":
            assert entry[1] in mods and entry[2] in mods[entry[1]][1], f"{sym}: tests/{entry[1]}.py has no case {entry[2]}"
        else:
            assert entry[0] == "not a kernel" and len(entry[1]) > 10, f"{sym}: a ledger entry names a case or says why the entry point is no kernel"
    assert not missing, "launchers without a kernel-level check (call the wrapper in a tests/gpu_*check*.py module, or add a LEDGER entry):\n  " + "\n  ".join(missing)
    assert not stale, f"LEDGER entries for launchers that a check module now calls itself: {stale}"
    assert not set(LEDGER) - set(declared), f"LEDGER entries for symbols the header no longer declares: {sorted(set(LEDGER) - set(declared))}"
    # the families this ledger was written for are called by name in tests/gpu_step_kernel_check.py itself
    step = mods["gpu_step_kernel_check"]
    for sym in ("s2svc_decode_attn", "s2svc_decode_ln_linear", "s2svc_decode_ln_linear_supported", "s2svc_decode_posenc", "s2svc_decode_emit", "s2svc_decode_advance",
                "s2svc_seq_loss_fwd", "s2svc_seq_loss_bwd", "s2svc_guided_attn_loss_fwd", "s2svc_guided_attn_loss_bwd", "s2svc_mas_binloss_bwd",
                "s2svc_length_regulate_index", "s2svc_length_regulate_fwd", "s2svc_length_regulate_bwd", "s2svc_attn_durations", "s2svc_adam_step",
                "s2svc_weighted_sum", "s2svc_weighted_sum_bwd", "s2svc_scalars_axpy", "s2svc_pad_cols", "s2svc_decoder_input", "s2svc_append_eos",
                "s2svc_copy_rows", "s2svc_stop_labels", "s2svc_add_n", "s2svc_fill_zero", "s2svc_seed_advance"):
        assert re.search(r"\b%s\(" % sym, step[0]) or any(_called_in(step, w) for w in wrappers[sym]), f"{sym} is no longer called by tests/gpu_step_kernel_check.py"
    # ... and the attention launchers in tests/gpu_attn_kernel_check.py
    attn = mods["gpu_attn_kernel_check"]
    for sym in ("s2svc_attn_fused_supported", "s2svc_attn_fused_fwd", "s2svc_attn_fused_bwd", "s2svc_attn_map_supported", "s2svc_attn_map_product_supported",
                "s2svc_attn_map_fwd", "s2svc_attn_map_bwd", "s2svc_relattn_supported", "s2svc_relattn_fwd", "s2svc_attn_softmax_fwd", "s2svc_attn_softmax_bwd"):
        assert re.search(r"\b%s\(" % sym, attn[0]) or any(_called_in(attn, w) for w in wrappers[sym]), f"{sym} is no longer called by tests/gpu_attn_kernel_check.py"
    # ... and the GEMM families in tests/gpu_gemm_kernel_check.py
    gemm = mods["gpu_gemm_kernel_check"]
    for sym in ("s2svc_gemm", "s2svc_gemm_grouped", "s2svc_gemm_grouped_ok", "s2svc_gemm_grouped_batched", "s2svc_gemm_wgrad_ok", "s2svc_gemm_wgrad_ws_floats",
                "s2svc_gemm_wgrad_grouped", "s2svc_gemm_wgrad_grouped_bg", "s2svc_gemm_set_w8", "s2svc_gemm_set_8ph", "s2svc_tconv2d_weights"):
        assert re.search(r"\b%s\(" % sym, gemm[0]), f"{sym} is no longer called by name in tests/gpu_gemm_kernel_check.py"
