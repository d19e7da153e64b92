"""HiFi-GAN generator backward on the MI355X (csrc/hifigan_bwd.hip, HifiganGenerator.trainable()): every backward kernel alone
against float64 torch autograd on the CPU, then the tiny generator's 234 parameter gradients, gradient accumulation, bit-equal
repeats and two SGD steps.  Each case returns [(ok, message)]; tests/test_gpu_vocoder_bwd.py turns them into pytest tests.

Yardsticks: float64 autograd of stock torch operators (kernel cases) and of tests/vocoder_ref.generator_forward (model cases;
tests/vocoder_bwd_ref.py, pinned to the reference's gradients on the CPU).  fp32: max abs error <= FP32_BAR relative to the
largest reference magnitude, per tensor.  bf16: relL2(HIP, f64) <= 1.5 relL2(torch CPU bf16 autocast autograd, f64) + 1e-3 per
tensor, the yardstick computed here on the same input.  Outputs are sentinel-filled before each launch; mask tensors of the kernel
cases keep |v| >= 0.05, the model-level input keeps a measured margin (vocoder_bwd_ref.margin), so no leaky-relu mask can flip (the training forward keeps fp32 activations in bf16 mode too: see model_gradients_bf16)."""
import contextlib

import torch
import torch.nn.functional as F

import vocoder_bwd_ref as VB
import vocoder_ref as VR
from seq2seq_vc_amd import _lib
from seq2seq_vc_amd.ops import functional as Fn
from seq2seq_vc_amd.ops import kernels_vocoder as KV
from seq2seq_vc_amd.vocoder import HifiganGenerator

DEV = "cuda:0"
FP32_BAR = 1e-4
BF16_VS_AUTOCAST = 1.5
SENTINEL = 7.0e4
TCONV_PAIRS = ((8, 4), (4, 2), (20, 10), (16, 8))
CONV_PAIRS = ((3, 1), (7, 3), (11, 5))


class _mode:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.prev = Fn.compute_dtype()
        Fn.set_compute_dtype(self.dtype)

    def __exit__(self, *a):
        Fn.set_compute_dtype(self.prev)


def _rel(a, b):
    return float((a.double() - b.double()).pow(2).sum().sqrt() / b.double().pow(2).sum().sqrt().clamp_min(1e-30))


def _relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _verdict(dtype, got, ref, amp):
    """(ok, text) of one tensor under the bar of its dtype"""
    got = got.detach().float().cpu()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return False, f"shape {tuple(got.shape)} vs {tuple(ref.shape)} or not finite"
    if dtype == torch.float32:
        e = _relmax(got, ref)
        return e <= FP32_BAR, f"fp32 rel-to-max {e:.2e}"
    h, a = _rel(got, ref), _rel(amp, ref)
    return h <= BF16_VS_AUTOCAST * a + 1e-3, f"bf16 relL2 {h:.2e} vs autocast {a:.2e}"


def _away_from_zero(shape, g):
    v = torch.randn(shape, generator=g)
    return torch.sign(v) * (0.05 + v.abs())


def _sentinel(shape, dtype):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def _cl(t):
    """channel-first CPU -> channel-last"""
    return t.transpose(1, 2).contiguous()


def _autograd(fn, tensors, dy, amp):
    """gradients of fn(*tensors) for the incoming dy, in float64 or (amp) under torch.autocast("cpu", bfloat16) over fp32 leaves"""
    cast = (lambda t: t.float()) if amp else (lambda t: t.double())
    leaves = [cast(t).clone().requires_grad_(True) for t in tensors]
    with (torch.autocast("cpu", dtype=torch.bfloat16) if amp else contextlib.nullcontext()):
        y = fn(*leaves)
    return [g.float() if amp else g for g in torch.autograd.grad(y, leaves, cast(dy).to(y.dtype))]


# ---- data gradients ---------------------------------------------------------------------------------------------------------
def _dgrad_conv1d_shape(res, g, cin, cout, pairs, combos):
    B, T = 2, 150                                            # two row tiles with a ragged edge; the halo lands on both utterance ends
    for k, dil in pairs:
        w = torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5 * 2
        for dtype in (torch.float32, torch.bfloat16):
            m = _away_from_zero((B, cin, T), g).to(dtype)
            dy = torch.randn(B, cout, T, generator=g).to(dtype)
            r = torch.randn(B, cin, T, generator=g).to(dtype)
            prev = torch.randn(B, cin, T, generator=g).to(dtype)
            w32, _ = KV.hifigan_fold(0, w.to(DEV), None, dtype)
            opT = KV.hifigan_fold_bwd(0, w32, dtype)
            for use_mask, use_res, scale, acc in combos:
                slope = 0.1 if use_mask else 0.0

                def truth(amp):
                    wv = w.to(dtype) if amp else w
                    (dx,) = _autograd(lambda a: F.conv1d(F.leaky_relu(a, slope) if slope else a, wv.to(a.dtype), None, dilation=dil,
                                                         padding=(k - 1) // 2 * dil), [m], dy, amp)
                    v = dx.to(dtype).double() if amp else dx
                    v = (v + r.double() if use_res else v) * scale
                    return v + prev.double() if acc else v

                out = _cl(prev).to(DEV) if acc else _sentinel((B, T, cin), dtype)
                got = KV.hifigan_conv1d_dgrad(_cl(dy).to(DEV), opT, k, dil, cin, mask_src=_cl(m).to(DEV) if use_mask else None, slope=slope,
                                              res=_cl(r).to(DEV) if use_res else None, accumulate=acc, scale=scale, out=out)
                amp = truth(True).to(dtype) if dtype == torch.bfloat16 else None
                ok, msg = _verdict(dtype, got.transpose(1, 2), truth(False), amp)
                res.append((ok, f"conv1d dgrad {cout} -> {cin} k {k} dil {dil} mask {use_mask} res {use_res} scale {scale:.3f} accumulate {acc}: {msg}"))


def dgrad_conv1d_kernel():
    """C_in = 40 is the 64-column tile with vector loads of dy in both dtypes.  C_in = 8 / 24 are the 16- and 32-column tiles (the
    tile body is one template over all three); C_out = 18 makes dy's loads element-wise in both dtypes, C_out = 20 in bf16 only."""
    res = []
    combos = [(False, False, 1.0, False), (True, False, 1.0, False), (True, True, 1.0, False), (True, True, 1.0 / 3, True),
              (False, True, 1.0 / 3, False), (False, False, 1.0, True)]
    g = torch.Generator().manual_seed(11)
    _dgrad_conv1d_shape(res, g, 40, 24, CONV_PAIRS, combos)
    for cin, cout in ((8, 18), (24, 20)):
        _dgrad_conv1d_shape(res, g, cin, cout, (CONV_PAIRS[0], CONV_PAIRS[-1]), (combos[3], combos[0]))
    return res


def _dgrad_tconv1d_shape(res, g, cin, cout, pairs):
    B, T = 2, 37
    for k, u in pairs:
        w = torch.randn(cin, cout, k, generator=g) / (cin * k / u) ** 0.5
        for dtype in (torch.float32, torch.bfloat16):
            for use_mask, scale in ((True, 1.0 / 3), (False, 1.0)):
                slope = 0.1 if use_mask else 0.0
                m = _away_from_zero((B, cin, T), g).to(dtype)
                dy = torch.randn(B, cout, u * T, generator=g).to(dtype)

                def truth(amp):
                    wv = w.to(dtype) if amp else w
                    (dx,) = _autograd(lambda a: F.conv_transpose1d(F.leaky_relu(a, slope) if slope else a, wv.to(a.dtype), None, stride=u,
                                                                   padding=(k - u) // 2), [m], dy, amp)
                    return dx * scale

                w32, _ = KV.hifigan_fold(1, w.to(DEV), None, dtype, u=u)
                opT = KV.hifigan_fold_bwd(1, w32, dtype, u=u)
                got = KV.hifigan_tconv1d_dgrad(_cl(dy).to(DEV), opT, k, u, cin, mask_src=_cl(m).to(DEV) if use_mask else None, slope=slope,
                                               scale=scale, out=_sentinel((B, T, cin), dtype))
                amp = truth(True).to(dtype) if dtype == torch.bfloat16 else None
                ok, msg = _verdict(dtype, got.transpose(1, 2), truth(False), amp)
                res.append((ok, f"tconv1d dgrad {cout} -> {cin} k {k} u {u} mask {use_mask} scale {scale:.3f}: {msg}"))


def dgrad_tconv1d_kernel():
    """The shapes of dgrad_conv1d_kernel for the transposed convolution: C_in = 48 (64 columns, vector loads), then 8 / 24 (16 / 32
    columns) with C_out = 18 / 20 at the smallest and the largest (k, u)."""
    res = []
    g = torch.Generator().manual_seed(12)
    _dgrad_tconv1d_shape(res, g, 48, 24, TCONV_PAIRS)
    small, large = min(TCONV_PAIRS), max(TCONV_PAIRS)
    for cin, cout in ((8, 18), (24, 20)):
        _dgrad_tconv1d_shape(res, g, cin, cout, (small, large))
    return res


# ---- weight and bias gradients ----------------------------------------------------------------------------------------------
def _wgrad_case(res, kind, k, step, B, T, cin, cout, g, chunk):
    u = step if kind == 1 else 1
    w = torch.randn((cout, cin, k) if kind == 0 else (cin, cout, k), generator=g)
    bias = torch.zeros(cout)
    for dtype in (torch.float32, torch.bfloat16):
        x = _away_from_zero((B, cin, T), g).to(dtype)
        dy = torch.randn(B, cout, u * T, generator=g).to(dtype)

        def fn(wv, bv):
            a = F.leaky_relu(x.to(wv.dtype), 0.1)
            if kind == 0:
                return F.conv1d(a, wv, bv, dilation=step, padding=(k - 1) // 2 * step)
            return F.conv_transpose1d(a, wv, bv, stride=u, padding=(k - u) // 2)

        ref = _autograd(fn, [w, bias], dy, False)
        amp = _autograd(fn, [w, bias], dy, True) if dtype == torch.bfloat16 else [None, None]
        rows = KV.wgrad_rows(kind, T, k, u)
        plan = KV.wgrad_plan(B, rows, chunk)
        inside = any(0 < r0 < rows for _, r0, _ in plan)
        na, ntaps = (cout, k) if kind == 0 else (u * cout, -(-k // u))
        runs = []
        for _ in range(2):
            wp, bp = KV.hifigan_wgrad(kind, _cl(dy).to(DEV), _cl(x).to(DEV), k, step, slope=0.1, plan=plan,
                                      wpart=_sentinel((len(plan), na, ntaps, cin), torch.float32), bpart=_sentinel((len(plan), na), torch.float32))
            gw, gg, gb = KV.hifigan_wgrad_finish(kind, wp, bp, w.to(DEV), None, u=u,
                                                 out=(_sentinel(tuple(w.shape), torch.float32), None, _sentinel((cout,), torch.float32)))
            runs.append((gw, gb, wp, bp))
        same = all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
        okw, mw = _verdict(dtype, runs[0][0], ref[0], amp[0])
        okb, mb = _verdict(dtype, runs[0][1], ref[1], amp[1])
        res.append((okw and okb and same and gg is None and inside,
                    f"{'conv1d' if kind == 0 else 'tconv1d'} wgrad k {k} {'dil' if kind == 0 else 'u'} {step}, {len(plan)} chunks (an edge inside an "
                    f"utterance: {inside}): weight {mw}; bias {mb}; two passes bit-equal: {same}"))


def wgrad_kernels():
    res = []
    g = torch.Generator().manual_seed(13)
    for k, dil in CONV_PAIRS:
        _wgrad_case(res, 0, k, dil, 3, 150, 40, 24, g, None)          # the default plan: 128 + 22 rows per utterance
    for k, u in TCONV_PAIRS:
        _wgrad_case(res, 1, k, u, 3, 37, 48, 24, g, 32)               # 37 (+ tail) rows: chunks of 32 put an edge inside
    return res


def conv_out_bwd_kernel():
    res = []
    B, T, k = 2, 300, 7
    g = torch.Generator().manual_seed(14)
    for C in (8, 32):
        w = torch.randn(1, C, k, generator=g) / (C * k) ** 0.5
        bias = torch.randn(1, generator=g) * 0.1
        for dtype in (torch.float32, torch.bfloat16):
            x = _away_from_zero((B, C, T), g).to(dtype)
            dy = torch.randn(B, 1, T, generator=g)
            scale = 1.0 / 3

            def fn(a, wv, bv):
                pre = F.conv1d(F.leaky_relu(a, 0.01), wv, bv, padding=3)
                return torch.tanh(pre if pre.dtype == torch.float64 else pre.float())       # the kernel applies tanh in fp32

            ref = _autograd(fn, [x, w, bias], dy, False)
            amp = _autograd(fn, [x, w, bias], dy, True) if dtype == torch.bfloat16 else [None] * 3
            _, op = KV.hifigan_fold(2, w.to(DEV), None, torch.float32)
            y, _ = KV.hifigan_conv_out(_cl(x).to(DEV), op, bias.to(DEV), k, slope=0.01, tanh=True)
            nch = B * -(-T // KV.OUT_BWD_CHUNK)
            dx, wp, bp = KV.hifigan_conv_out_bwd(_cl(x).to(DEV), op, y, dy.view(B, T).to(DEV), k, slope=0.01, scale=scale,
                                                 out=(_sentinel((B, T, C), dtype), _sentinel((nch, k, C), torch.float32), _sentinel((nch,), torch.float32)))
            gw, _, gb = KV.hifigan_wgrad_finish(2, wp, bp, w.to(DEV), None)
            oks, msgs = [], []
            for name, got, r, a in (("dx", dx.transpose(1, 2), ref[0] * scale, None if amp[0] is None else (amp[0] * scale).to(dtype)),
                                    ("weight", gw, ref[1], amp[1]), ("bias", gb, ref[2], amp[2])):
                ok, msg = _verdict(dtype, got, r, a)
                oks.append(ok)
                msgs.append(f"{name} {msg}")
            res.append((all(oks), f"conv_post backward C {C}, {nch} chunks: " + "; ".join(msgs)))
    return res


def finish_weight_norm_kernel():
    res = []
    g = torch.Generator().manual_seed(15)
    for shape, u in (((5, 7, 3), 1), ((64, 32, 8), 4)):
        D0, D1, k = shape
        v = torch.randn(shape, generator=g)
        gn = 0.5 + torch.rand(D0, 1, 1, generator=g)
        for mode in (0, 1):
            for nparts in (1, 3):
                for normed in (True, False):
                    uu = u if mode == 1 else 1
                    ntaps = -(-k // uu)
                    if mode == 0:
                        wp = torch.randn(nparts, D0, k, D1, generator=g)
                        bp = torch.randn(nparts, D0, generator=g)
                        dw = wp.double().sum(0).permute(0, 2, 1)
                        db = bp.double().sum(0)
                    else:
                        wp = torch.randn(nparts, uu * D1, ntaps, D0, generator=g)
                        bp = torch.randn(nparts, uu * D1, generator=g)
                        s = wp.double().sum(0).view(uu, D1, ntaps, D0)
                        dw = torch.zeros(D0, D1, k, dtype=torch.float64)
                        for p in range(uu):
                            for n in range(ntaps):
                                if p + uu * n < k:
                                    dw[:, :, p + uu * n] = s[p, :, n].t()
                        db = bp.double().sum(0).view(uu, D1).sum(0)
                    if normed:
                        dv, dg = _autograd(lambda a, b: torch._weight_norm(a, b, 0), [v, gn], dw, False)
                    else:
                        dv, dg = dw, None
                    nb = D0 if mode == 0 else D1
                    out = (_sentinel(shape, torch.float32), _sentinel((D0, 1, 1), torch.float32) if normed else None, _sentinel((nb,), torch.float32))
                    gw, gg, gb = KV.hifigan_wgrad_finish(mode, wp.to(DEV), bp.to(DEV), v.to(DEV), gn.to(DEV) if normed else None, u=uu, out=out)
                    errs = {"weight": _relmax(gw.cpu(), dv), "bias": _relmax(gb.cpu(), db)}
                    if normed:
                        errs["g"] = _relmax(gg.cpu(), dg)
                    res.append((all(e <= FP32_BAR for e in errs.values()) and (gg is None) == (not normed),
                                f"finish mode {mode} v {shape} u {uu} partials {nparts} weight norm {normed}: rel-to-max "
                                + ", ".join(f"{n} {e:.2e}" for n, e in errs.items())))
    return res


# ---- the model --------------------------------------------------------------------------------------------------------------
_REF = {}


def _model_reference(form):
    """float64 / fp32 / bf16-autocast gradients of the restatement for the committed input, computed once and shared"""
    if form not in _REF:
        cfg, sd, _, _, _ = VR.load_fixture()
        if form == "plain":
            sd = {(k[:-2] if k.endswith("weight_v") else k): (VR.weight(sd, k[:-9]) if k.endswith("weight_v") else v)
                  for k, v in sd.items() if not k.endswith("weight_g")}
        x = VB.grad_input()
        y64, loss64, g64 = VB.generator_grads(sd, cfg, x)
        _, _, g32 = VB.generator_grads(sd, cfg, x, dtype=torch.float32)
        _, _, gamp = VB.generator_grads(sd, cfg, x, dtype=torch.float32, autocast=True)
        _REF[form] = (cfg, sd, x, y64, loss64, g64, g32, gamp)
    return _REF[form]


def _hip_grads(gen, x, r, passes=1):
    gen.zero_grad(set_to_none=True)
    for _ in range(passes):
        y = gen(x)
        VB.loss_fn(y, r).backward()
    return y, {k: p.grad.detach().clone() for k, p in gen.named_parameters()}


def _model_case(res, form, dtype):
    cfg, sd, x, y64, loss64, g64, g32, gamp = _model_reference(form)
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(sd)
    gen.to(DEV).trainable()
    xd, r = x.to(DEV), VB.loss_weights(y64.shape).to(DEV)
    tag = f"tiny generator, {form}, {'fp32' if dtype == torch.float32 else 'bf16'}"
    with _mode(dtype):
        y, grads = _hip_grads(gen, xd, r)
        _, again = _hip_grads(gen, xd, r)
        _, twice = _hip_grads(gen, xd, r, passes=2)
        if dtype == torch.float32 and form == "weight-normed":         # the margin holds for the HIP forward's own error too
            taps = {}
            with torch.no_grad():
                gen(xd, taps=taps)
            t64 = {}
            VR.generator_forward({k: v.double() for k, v in sd.items()}, cfg, x.double(), taps=t64)
            m, e, _ = VB.margin(sd, cfg, x)
            worst = 0.0
            for name, v in taps.items():
                v = v.float().cpu()
                v = v.unsqueeze(1) if v.dim() == 2 else v.transpose(1, 2)
                if name != "conv_post":
                    worst = max(worst, float((v.double() - t64[name]).abs().max() / t64[name].pow(2).mean().sqrt()))
            # m >= 4 e itself is asserted on the host (tests/test_vocoder_bwd_host.py); e is stock torch's error and is only printed here
            res.append((worst < m / 2, f"{tag}: leaky-relu margin m {m:.2e} (torch fp32 error e {e:.2e}); HIP forward distance at the taps "
                        f"{worst:.2e} < m / 2"))
    res.append((y.requires_grad and y.grad_fn is not None and tuple(y.shape) == tuple(y64.shape) and y.dtype == torch.float32,
                f"{tag}: output {tuple(y.shape)} {y.dtype} with grad_fn"))
    if dtype != torch.float32:                                         # the training forward keeps fp32 activations in either mode
        with _mode(torch.float32):
            y32 = gen(xd)
        res.append((torch.equal(y.detach(), y32.detach()), f"{tag}: the training forward's output equals the fp32 mode's bit for bit"))
    res.append((sorted(grads) == sorted(g64) and len(grads) == (234 if form == "weight-normed" else 156)
                and all(grads[k].shape == g64[k].shape and grads[k].dtype == torch.float32 for k in g64), f"{tag}: {len(grads)} fp32 gradients in the parameters' shapes"))
    bad, worst, ratio = [], 0.0, 0.0
    for k in g64:
        got = grads[k].cpu()
        if dtype == torch.float32:
            e, t = _relmax(got, g64[k]), _relmax(g32[k], g64[k])
            ok = e <= FP32_BAR
        else:
            e, t = _rel(got, g64[k]), _rel(gamp[k], g64[k])
            ok = e <= BF16_VS_AUTOCAST * t + 1e-3
        worst, ratio = max(worst, e), max(ratio, e / max(t, 1e-12))
        if not ok or not bool(torch.isfinite(got).all()):
            bad.append(f"{k} {e:.2e} (torch {t:.2e})")
    what = "rel-to-max" if dtype == torch.float32 else "relL2"
    res.append((not bad, f"{tag}: worst {what} vs float64 {worst:.2e}; worst HIP / torch CPU {'fp32' if dtype == torch.float32 else 'bf16 autocast'} "
                f"distance ratio {ratio:.2f}" + (f"; over the bar: {bad[:8]}" if bad else "")))
    res.append((all(torch.equal(grads[k], again[k]) for k in grads), f"{tag}: two runs bit-equal"))
    acc = max(_relmax(twice[k], 2 * grads[k]) for k in grads)
    res.append((acc <= 1e-6, f"{tag}: two accumulated backward passes vs twice one pass, rel-to-max {acc:.2e}"))


def model_gradients_fp32():
    res = []
    _model_case(res, "weight-normed", torch.float32)
    _model_case(res, "plain", torch.float32)
    return res


def model_gradients_bf16():
    """bf16 mode of a trainable generator: the training forward keeps fp32 activations (its output equals the fp32 mode's bit for bit),
    the backward's GEMMs run in bf16 over bf16 copies of them.  With a bf16 FORWARD the per-tensor bar cannot be met by any backward:
    370 of the 170 880 leaky-relu masks flip under torch's CPU autocast on this input, and float64 arithmetic over autocast's own
    masks already sits a median relL2 of 9.3e-2 from float64 (autocast itself: 9.4e-2), at other places than a second bf16 forward's
    flips (measured: 5 of 234 tensors over the bar, ratio 0.20 .. 3.7 around a median of 0.85; profiles/AB_LOG.md)."""
    res = []
    _model_case(res, "weight-normed", torch.bfloat16)
    _model_case(res, "plain", torch.bfloat16)
    return res


def two_sgd_steps():
    res = []
    cfg, sd, x, y64, _, _, _, _ = _model_reference("weight-normed")
    lr = 1e-2
    r = VB.loss_weights(y64.shape)
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(sd)
    gen.to(DEV).trainable()
    opt = torch.optim.SGD(gen.parameters(), lr=lr)
    ref = {k: v.double().clone() for k, v in sd.items()}
    with _mode(torch.float32):
        with torch.no_grad():
            y_before = gen(x.to(DEV))                                # fills whatever the module caches before the weights move
        for _ in range(2):
            opt.zero_grad()
            VB.loss_fn(gen(x.to(DEV)), r.to(DEV)).backward()
            opt.step()
            _, _, g = VB.generator_grads(ref, cfg, x, r=r)
            ref = {k: v - lr * g[k] for k, v in ref.items()}
        with torch.no_grad():
            y_after = gen(x.to(DEV))
            loss = float(VB.loss_fn(y_after, r.to(DEV)))
    with torch.no_grad():
        y_ref = VR.generator_forward(ref, cfg, x.double())
        loss_ref = float(VB.loss_fn(y_ref, r))
    errs = {k: _relmax(p.detach().cpu(), ref[k]) for k, p in gen.named_parameters()}
    worst = max(errs, key=errs.get)
    res.append((errs[worst] <= FP32_BAR, f"two SGD steps (lr {lr}): parameters vs float64, worst rel-to-max {errs[worst]:.2e} ({worst})"))
    res.append((abs(loss - loss_ref) <= FP32_BAR * max(1.0, abs(loss_ref)), f"loss after the steps {loss:.6f} vs float64 {loss_ref:.6f}"))
    e = float((y_after.cpu() - y_ref).abs().max())
    moved = float((y_after - y_before).abs().max())
    res.append((e <= FP32_BAR and moved > 10 * FP32_BAR and not y_after.requires_grad,
                f"inference after the steps vs the restatement with the stepped weights: max abs {e:.2e} (the output moved by {moved:.2e})"))
    try:
        gen(x.to(DEV).requires_grad_(True))
        res.append((False, "a trainable generator accepted an input that requires grad"))
    except NotImplementedError as ex:
        res.append((True, f"grad input refused: {ex}"))
    return res


def _recorded(fn):
    """the names of the library calls fn() makes, in order"""
    real, names = _lib.check, []

    def counting(rc, what):
        names.append(what)
        return real(rc, what)
    _lib.check = counting
    try:
        fn()
    finally:
        _lib.check = real
    return names


def plans_are_the_recorded_calls():
    """The library calls of one trainable forward (tiny generator, B = 2, 8 frames) are calls(train_plan(dtype)) and those of its
    backward calls(backward_plan()), name for name and in order; bf16 mode adds the casts of the kept buffers to the forward."""
    res = []
    gen = HifiganGenerator(**VR.TINY_CFG).to(DEV).trainable()
    x = torch.randn(2, VR.TINY_CFG["in_channels"], 8, generator=torch.Generator().manual_seed(16)).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        tag = "fp32" if dtype == torch.float32 else "bf16"
        with _mode(dtype):
            y = []
            fwd = _recorded(lambda: y.append(gen(x)))
            bwd = _recorded(lambda: y[0].sum().backward())
        want_fwd = [e["call"] for e in gen.calls(gen.train_plan(dtype))]
        want_bwd = [e["call"] for e in gen.calls(gen.backward_plan())]
        casts = sum(1 for e in gen.train_plan(dtype) if e["kind"] == "cast")
        res.append((fwd == want_fwd and (casts > 0) == (dtype != torch.float32),
                    f"{tag}: {len(fwd)} recorded calls of the training forward, {len(want_fwd)} in calls(train_plan()) ({casts} casts), equal in order: {fwd == want_fwd}"))
        res.append((bwd == want_bwd, f"{tag}: {len(bwd)} recorded calls of the backward, {len(want_bwd)} in calls(backward_plan()), equal in order: {bwd == want_bwd}"))
    return res


CASES = [dgrad_conv1d_kernel, dgrad_tconv1d_kernel, wgrad_kernels, conv_out_bwd_kernel, finish_weight_norm_kernel, model_gradients_fp32,
         model_gradients_bf16, two_sgd_steps, plans_are_the_recorded_calls]
