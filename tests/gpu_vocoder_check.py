"""HiFi-GAN vocoder on the MI355X: the generator against the reference's fixture, the two convolution kernels alone against float64
torch on the CPU, the full-size generator in fp32 and bf16, batched rows against single calls, checkpoint forms and the decode
wrapper.  Each case returns [(ok, message)]; tests/test_gpu_vocoder.py turns them into pytest tests.

Yardsticks: tests/vocoder_ref.py (stock torch operators over the state_dict; pinned to the reference's fixture on the CPU) in
float64 is the truth.  fp32 mode: the project's parity bar, max abs <= 1e-4 (kernel cases: relative to max |ref|).  bf16 mode: the
project's rule for bf16 paths -- relL2(HIP bf16, f64) <= BF16_VS_AUTOCAST x relL2(the same computation under
torch.autocast("cpu", bfloat16), f64) + 1e-3, the yardstick computed here on the same input."""
import itertools

import torch
import torch.nn.functional as F

import vocoder_ref as VR
from seq2seq_vc_amd.ops import functional as Fn
from seq2seq_vc_amd.ops import kernels_vocoder as KV
from seq2seq_vc_amd.vocoder import HifiganGenerator, HifiganVocoder
from seq2seq_vc_amd.vocoder import hifigan as H

DEV = "cuda:0"
FP32_BAR = 1e-4
BF16_VS_AUTOCAST = 1.5
BATCH_BAR = 1e-6


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


def _hip_taps(taps):
    """channel-last device taps of the generator -> channel-first CPU fp32, as torch computes them"""
    out = {}
    for k, v in taps.items():
        v = v.float().cpu()
        out[k] = v.unsqueeze(1) if v.dim() == 2 else v.transpose(1, 2)
    return out


def _bf16_verdict(res, tag, hip, ref64, amp):
    """per tap: relL2(hip, f64) <= 1.5 relL2(autocast, f64) + 1e-3"""
    rows, bad = [], []
    for k in ref64:
        h, a = _rel(hip[k], ref64[k]), _rel(amp[k], ref64[k])
        rows.append(f"{k} {h:.2e}/{a:.2e}={h / max(a, 1e-12):.2f}")
        if not h <= BF16_VS_AUTOCAST * a + 1e-3:
            bad.append(k)
    res.append((not bad, f"{tag}: relL2 HIP bf16 / torch CPU bf16 autocast (both vs float64) per tap: " + ", ".join(rows)
                + (f"; over {BF16_VS_AUTOCAST} x + 1e-3: {bad}" if bad else "")))


def hifigan_tiny_vs_reference_fp32():
    cfg, sd, x, y, taps = VR.load_fixture()
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(sd)
    gen.to(DEV)
    res, got = [], {}
    with _mode(torch.float32), torch.no_grad():
        yh = gen(x.to(DEV), taps=got)
    got = _hip_taps(got)
    res.append((sorted(got) == sorted(taps), f"taps {sorted(got)}"))
    errs = {k: float((got[k] - taps[k]).abs().max()) for k in taps if k in got and got[k].shape == taps[k].shape}
    errs["waveform"] = float((yh.cpu() - y).abs().max()) if yh.shape == y.shape else float("inf")
    res.append((len(errs) == len(taps) + 1 and all(e <= FP32_BAR for e in errs.values()) and not yh.requires_grad,
                "tiny generator vs the reference's fixture, fp32, max abs per tap: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())))
    return res


# ---- the kernels alone --------------------------------------------------------------------------------------------------------
def _ragged_truth(fn, x64, lens, scale_t=1):
    """fn on every utterance ALONE (its own zero padding), stacked into a zero-padded batch: (B, C, T) float64"""
    outs = [fn(b, x64[b:b + 1, :, :n]) for b, n in enumerate(lens)]
    full = torch.zeros(len(lens), outs[0].shape[1], x64.shape[2] * scale_t, dtype=outs[0].dtype)
    for b, o in enumerate(outs):
        full[b, :, :o.shape[2]] = o[0]
    return full


def _conv_case(res, tag, cin, cout, k, dil, slope, use_res, accumulate, scale, tanh, seed):
    g = torch.Generator().manual_seed(seed)
    B, T, lens = 3, 333, [333, 200, 57]
    w = torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5 * 2
    bias = torch.randn(cout, generator=g)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(B, T, cin, generator=g).to(dtype)
        r = torch.randn(B, T, cout, generator=g).to(dtype)
        prev = torch.randn(B, T, cout, generator=g).to(dtype)
        xd, rd, pd = x.clone(), r.clone(), prev.clone()
        for b, n in enumerate(lens):                                     # NaN in every absent input / residual / accumulator row
            xd[b, n:], rd[b, n:], pd[b, n:] = float("nan"), float("nan"), float("nan")

        def fn(b, xb, cast=lambda t: t.double()):
            n = xb.shape[2]
            v = F.conv1d(F.leaky_relu(xb, slope) if slope else xb, cast(w), cast(bias), dilation=dil, padding=(k - 1) // 2 * dil)
            if use_res:
                v = v + cast(r[b:b + 1, :n].transpose(1, 2).float())
            v = v * scale
            if accumulate:
                v = v + cast(prev[b:b + 1, :n].transpose(1, 2).float())
            return torch.tanh(v) if tanh else v

        ref = _ragged_truth(fn, x.double().transpose(1, 2), lens)
        _, op = KV.hifigan_fold(0, w.to(DEV), None, dtype)
        out = pd.to(DEV) if accumulate else None
        vl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        got = KV.hifigan_conv1d(xd.to(DEV), op, bias.to(DEV), k, dil, cout, slope=slope, res=rd.to(DEV) if use_res else None,
                                accumulate=accumulate, scale=scale, tanh=tanh, out=out, vlens=vl)
        got = got.float().cpu().transpose(1, 2)
        absent_zero = all(bool((got[b, :, n:] == 0).all()) for b, n in enumerate(lens))
        if dtype == torch.float32:
            err = float((got - ref).abs().max() / ref.abs().max())
            ok = err <= FP32_BAR and absent_zero
            msg = f"fp32 rel-to-max {err:.2e}"
        else:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                amp = _ragged_truth(lambda b, xb: fn(b, xb, cast=lambda t: t.float()).float(), x.float().transpose(1, 2), lens)
            h, a = _rel(got, ref), _rel(amp.to(torch.bfloat16), ref)     # the HIP kernel STORES bf16; so does the yardstick here
            ok = h <= BF16_VS_AUTOCAST * a + 1e-3 and absent_zero and bool(torch.isfinite(got).all())
            msg = f"bf16 relL2 {h:.2e} vs autocast {a:.2e}"
        res.append((ok, f"{tag} [{msg}; absent rows zero: {absent_zero}]"))


def hifigan_conv1d_kernel():
    res = []
    # epilogue / prologue option sets, cycled over the shape grid so that each option is seen on and off at every channel count
    opts = [dict(slope=0.1, use_res=False, accumulate=False, scale=1.0, tanh=False),
            dict(slope=0.1, use_res=True, accumulate=False, scale=1.0, tanh=False),
            dict(slope=0.1, use_res=True, accumulate=True, scale=1.0 / 3, tanh=False),
            dict(slope=0.0, use_res=False, accumulate=False, scale=1.0, tanh=False),
            dict(slope=0.01, use_res=False, accumulate=False, scale=1.0, tanh=True),
            dict(slope=0.1, use_res=True, accumulate=False, scale=1.0 / 3, tanh=False),
            dict(slope=0.0, use_res=False, accumulate=True, scale=1.0, tanh=True)]
    for i, (c, k, dil) in enumerate(itertools.product((32, 64, 128, 256, 512), (3, 7, 11), (1, 3, 5))):
        o = opts[i % len(opts)]
        _conv_case(res, f"conv1d C={c} k={k} dil={dil} {o}", c, c, k, dil, seed=100 + i, **o)
    _conv_case(res, "conv1d 80 -> 512 k=5 (conv_pre)", 80, 512, 5, 1, 0.0, False, False, 1.0, False, seed=7)
    _conv_case(res, "conv1d 24 -> 40 k=3 dil=2 (channels not a multiple of the vector / tile)", 24, 40, 3, 2, 0.1, True, False, 1.0, False, seed=8)
    _conv_case(res, "conv1d 4 -> 4 k=11 dil=5 (the tiny fixture's last stage)", 4, 4, 11, 5, 0.1, True, True, 0.5, False, seed=9)
    # the output convolution 32 -> 1, k = 7: its own kernel
    g = torch.Generator().manual_seed(11)
    B, T, C, lens = 3, 333, 32, [333, 200, 57]
    w, bias = torch.randn(1, C, 7, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(B, T, C, generator=g).to(dtype)
        xd = x.clone()
        for b, n in enumerate(lens):
            xd[b, n:] = float("nan")
        ref = _ragged_truth(lambda b, xb: F.conv1d(F.leaky_relu(xb, 0.01), w.double(), bias.double(), padding=3), x.double().transpose(1, 2), lens)
        _, op = KV.hifigan_fold(2, w.to(DEV), None, torch.float32)
        y, pre = KV.hifigan_conv_out(xd.to(DEV), op, bias.to(DEV), 7, slope=0.01, tanh=True, want_pre=True,
                                     vlens=torch.tensor(lens, dtype=torch.int32, device=DEV))
        y, pre = y.cpu().unsqueeze(1), pre.cpu().unsqueeze(1)
        zero = all(bool((y[b, :, n:] == 0).all() and (pre[b, :, n:] == 0).all()) for b, n in enumerate(lens))
        if dtype == torch.float32:
            e1, e2 = float((pre - ref).abs().max() / ref.abs().max()), float((y - torch.tanh(ref)).abs().max())
            res.append((e1 <= FP32_BAR and e2 <= FP32_BAR and zero, f"conv_out 32 -> 1 k=7 fp32: pre-tanh rel-to-max {e1:.2e}, tanh max abs {e2:.2e}, absent zero {zero}"))
        else:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                amp = _ragged_truth(lambda b, xb: F.conv1d(F.leaky_relu(xb, 0.01), w, bias, padding=3).float(), x.float().transpose(1, 2), lens)
            h, a = _rel(pre, ref), _rel(amp, ref)
            ht, at = _rel(y, torch.tanh(ref)), _rel(torch.tanh(amp), torch.tanh(ref))
            res.append((h <= BF16_VS_AUTOCAST * a + 1e-3 and ht <= BF16_VS_AUTOCAST * at + 1e-3 and zero,
                        f"conv_out 32 -> 1 k=7 bf16: relL2 pre-tanh {h:.2e} vs autocast {a:.2e}, tanh {ht:.2e} vs {at:.2e}, absent zero {zero}"))
    return res


def hifigan_tconv1d_kernel():
    res = []
    B, T, lens = 3, 77, [77, 40, 9]
    for i, (k, u, cin) in enumerate([(20, 10, 512), (16, 8, 256), (4, 2, 128), (4, 2, 64), (8, 4, 64), (12, 4, 32), (8, 4, 8)]):
        cout = cin // 2
        g = torch.Generator().manual_seed(300 + i)
        w = torch.randn(cin, cout, k, generator=g) / (cin * k / u) ** 0.5 * 2
        bias = torch.randn(cout, generator=g)
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn(B, T, cin, generator=g).to(dtype)
            xd = x.clone()
            for b, n in enumerate(lens):
                xd[b, n:] = float("nan")

            def fn(b, xb, cast=lambda t: t.double()):
                return F.conv_transpose1d(F.leaky_relu(xb, 0.1), cast(w), cast(bias), stride=u, padding=(k - u) // 2)

            ref = _ragged_truth(fn, x.double().transpose(1, 2), lens, scale_t=u)
            w32, op = KV.hifigan_fold(1, w.to(DEV), None, dtype, u=u)
            host_op = H.tconv1d_operand(w, u, cin_padded=KV.cin_padded(cin)).to(dtype)
            same_op = torch.equal(op.cpu(), host_op) and torch.equal(w32.cpu(), w)
            got = KV.hifigan_tconv1d(xd.to(DEV), op, bias.to(DEV), k, u, cout, slope=0.1,
                                     vlens=torch.tensor(lens, dtype=torch.int32, device=DEV)).float().cpu().transpose(1, 2)
            zero = all(bool((got[b, :, u * n:] == 0).all()) for b, n in enumerate(lens))
            if dtype == torch.float32:
                err = float((got - ref).abs().max() / ref.abs().max())
                ok, msg = err <= FP32_BAR, f"fp32 rel-to-max {err:.2e}"
            else:
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    amp = _ragged_truth(lambda b, xb: fn(b, xb, cast=lambda t: t.float()).float(), x.float().transpose(1, 2), lens, scale_t=u)
                h, a = _rel(got, ref), _rel(amp.to(torch.bfloat16), ref)
                ok, msg = h <= BF16_VS_AUTOCAST * a + 1e-3 and bool(torch.isfinite(got).all()), f"bf16 relL2 {h:.2e} vs autocast {a:.2e}"
            res.append((ok and zero and same_op and got.shape[2] == u * T,
                        f"tconv1d k={k} u={u} {cin} -> {cout} [{msg}; absent rows zero: {zero}; fold operand == host layout: {same_op}]"))
    return res


# ---- the generator at full size ----------------------------------------------------------------------------------------------
FULL_CFG = dict(in_channels=80)
FULL_SEED = 20240807


def _full_generator():
    gen = HifiganGenerator(**FULL_CFG)
    sd = VR.seed_state_dict(gen.state_dict(), FULL_SEED)
    gen.load_state_dict(sd)
    return gen.to(DEV), sd


def hifigan_full_size_fp32_and_bf16():
    res = []
    gen, sd = _full_generator()
    x = torch.randn(2, 80, 60, generator=torch.Generator().manual_seed(1))
    ref = {}
    with torch.no_grad():
        y64 = VR.generator_forward({k: v.double() for k, v in sd.items()}, FULL_CFG, x.double(), ref)
    ref["waveform"] = y64
    ok, msg = VR.alive(y64, ref, FULL_CFG)
    res.append((ok, "seeded full-size generator is alive and unsaturated: " + msg))
    got = {}
    with _mode(torch.float32), torch.no_grad():
        y = gen(x.to(DEV), taps=got)
    got = _hip_taps(got)
    got["waveform"] = y.cpu()
    errs = {k: float((got[k] - ref[k]).abs().max()) for k in ref}
    res.append((all(e <= FP32_BAR for e in errs.values()), "full size fp32 vs float64 restatement, max abs per tap: "
                + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())))
    amp = {}
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        amp["waveform"] = VR.generator_forward(sd, FULL_CFG, x, amp).float()
    amp = {k: v.float() for k, v in amp.items()}
    got16 = {}
    with _mode(torch.bfloat16), torch.no_grad():
        y16 = gen(x.to(DEV), taps=got16)
    got16 = _hip_taps(got16)
    got16["waveform"] = y16.cpu()
    _bf16_verdict(res, "full size bf16", got16, ref, amp)
    d = (got16["waveform"] - ref["waveform"]).abs()
    da = (amp["waveform"] - ref["waveform"]).abs()
    res.append((bool(torch.isfinite(y16).all()), f"full size bf16 waveform error max {float(d.max()):.2e} mean {float(d.mean()):.2e} "
                f"(the autocast yardstick's own: max {float(da.max()):.2e} mean {float(da.mean()):.2e})"))
    return res


def hifigan_batch_rows_equal_single_calls():
    res = []
    lens = [60, 41, 17, 1]
    for tag, make in (("default-80", lambda: _full_generator()[0]), ("tiny", None)):
        if make is None:
            cfg, sd, _, _, _ = VR.load_fixture()
            gen = HifiganGenerator(**cfg)
            gen.load_state_dict(sd)
            gen.to(DEV)
        else:
            gen = make()
        total = 1
        for f in gen.upsample_factors:
            total *= f
        g = torch.Generator().manual_seed(5)
        xs = torch.randn(4, 60, 80, generator=g)
        dirty = xs.clone()
        for b, n in enumerate(lens):                      # garbage in the padded frames: 1e4 and NaN, alternating
            dirty[b, n:] = 1e4
            dirty[b, n + 1::2] = float("nan")
        for dtype in (torch.float32, torch.bfloat16):
            with _mode(dtype), torch.no_grad():
                ys = gen.forward_batch(dirty.to(DEV), torch.tensor(lens))
                singles = [gen(xs[b:b + 1, :n].transpose(1, 2).contiguous().to(DEV)).view(-1) for b, n in enumerate(lens)]
            shapes = [tuple(y.shape) for y in ys] == [(n * total,) for n in lens] == [tuple(s.shape) for s in singles]
            err = max(float((a - b).abs().max()) for a, b in zip(ys, singles)) if shapes else float("inf")
            exact = shapes and all(torch.equal(a, b) for a, b in zip(ys, singles))
            finite = all(bool(torch.isfinite(y).all()) for y in ys)
            # bf16: the same fixed reduction order, so a row of a batch must get the very bits it gets alone
            ok = shapes and finite and (err <= BATCH_BAR if dtype == torch.float32 else exact)
            res.append((ok, f"{tag} {str(dtype)[6:]}: forward_batch rows vs single calls max abs {err:.2e} (bit-exact: {exact}); lengths exact: "
                            f"{shapes}; the reduction order of an output element does not depend on the number of rows (no split-K)"))
    return res


def hifigan_checkpoint_forms_and_wrapper():
    res = []
    cfg, sd, x, y, _ = VR.load_fixture()
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(sd)
    gen.to(DEV)
    total = 64
    with _mode(torch.float32), torch.no_grad():
        y1 = gen(x.to(DEV))
        gen.remove_weight_norm()
        y2 = gen(x.to(DEV))
        plain = {k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
        other = HifiganGenerator(**cfg)
        other.load_state_dict(plain)
        other.to(DEV)
        y3 = other(x.to(DEV))
        # torch's own fold of the same checkpoint, loaded in the remove_weight_norm form
        tplain = {(k[:-2] if k.endswith("weight_v") else k): (VR.weight(sd, k[:-9]) if k.endswith("weight_v") else v)
                  for k, v in sd.items() if not k.endswith("weight_g")}
        other.load_state_dict(tplain)
        y4 = other(x.to(DEV))
    res.append((all(k.endswith((".weight", ".bias")) for k in plain) and len(plain) == 156, f"remove_weight_norm form has {len(plain)} keys"))
    res.append((torch.equal(y1, y2) and torch.equal(y1, y3), f"weight-normed / remove_weight_norm() / reloaded plain checkpoint: bit-identical "
                f"{torch.equal(y1, y2)} / {torch.equal(y1, y3)}"))
    e4 = float((y4 - y1).abs().max())
    res.append((e4 <= FP32_BAR, f"torch-folded plain checkpoint vs weight-normed: max abs {e4:.2e}"))
    # the decode wrapper
    g = torch.Generator().manual_seed(9)
    T = 29
    c = torch.randn(T, 80, generator=g)
    stats = dict(mean=torch.randn(80, generator=g).numpy(), scale=(0.5 + torch.rand(80, generator=g)).numpy())
    trg = dict(mean=torch.randn(80, generator=g).numpy(), scale=(0.5 + torch.rand(80, generator=g)).numpy())
    gen.load_state_dict(sd)
    voc = HifiganVocoder(gen, stats, trg_stats=trg)
    with _mode(torch.float32), torch.no_grad():
        yw, sr = voc.decode(c.to(DEV))
        cn = (c.double() * torch.from_numpy(trg["scale"]).double() + torch.from_numpy(trg["mean"]).double()
              - torch.from_numpy(stats["mean"]).double()) / torch.from_numpy(stats["scale"]).double()
        ref = VR.generator_forward({k: v.double() for k, v in sd.items()}, cfg, cn.t().unsqueeze(0)).view(-1)
        ys, sr2 = voc.decode_batch(torch.stack([c, c.flip(0)]).to(DEV), [T, 11])
    ew = float((yw.cpu() - ref).abs().max())
    res.append((tuple(yw.shape) == (T * total,) and sr == 16000 and ew <= FP32_BAR, f"HifiganVocoder.decode vs restatement on the normalised mel: "
                f"shape {tuple(yw.shape)}, rate {sr}, max abs {ew:.2e}"))
    res.append((torch.equal(ys[0], yw) and tuple(ys[1].shape) == (11 * total,) and sr2 == 16000, "decode_batch row 0 equals decode; row 1 has 11 frames' samples"))
    # a second load_state_dict drops the cached operands
    sd2 = VR.seed_state_dict(sd, 77)
    gen.load_state_dict(sd2)
    with _mode(torch.float32), torch.no_grad():
        y5 = gen(x.to(DEV))
        r5 = VR.generator_forward({k: v.double() for k, v in sd2.items()}, cfg, x.double())
    e5 = float((y5.cpu() - r5).abs().max())
    res.append((not torch.equal(y5, y1) and e5 <= FP32_BAR, f"second load_state_dict: output changed, and matches the new weights (max abs {e5:.2e})"))
    # refusals
    try:
        gen(x.to(DEV).requires_grad_(True))
        res.append((False, "forward on an input that requires grad did not raise"))
    except NotImplementedError as e:
        res.append((True, f"grad input refused: {e}"))
    return res


CASES = [hifigan_tiny_vs_reference_fp32, hifigan_conv1d_kernel, hifigan_tconv1d_kernel, hifigan_full_size_fp32_and_bf16,
         hifigan_batch_rows_equal_single_calls, hifigan_checkpoint_forms_and_wrapper]
