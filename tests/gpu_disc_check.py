"""HiFi-GAN multi-period discriminator on the MI355X (csrc/hifigan_disc.hip, seq2seq_vc_amd/urhythmic/vocoder.py): every launcher
alone in an exact regime, and the whole discriminator, forward and backward, against the plain-torch restatement tests/disc_ref.py.
Each case returns [(ok, message)]; tests/test_gpu_disc.py turns them into pytest tests.

Kernel level (zero tolerance): inputs are small integers, the slope is 0.5, so every sum is exact in fp32 whatever its order and the
float64 result of stock torch (conv2d and its autograd) must be met bit for bit.  Inputs live inside NaN-filled allocations (a read
before the first or past the last row poisons the result), outputs inside sentinel-filled ones (a write outside shows).

Model level: step_kernels_ref.compare, unchanged -- per tensor |got - ref64| <= 4 d + ulp, d = max |restatement in float32 - restatement
in float64| on the same inputs.  Nothing here is fitted to what the kernels return."""
import torch
import torch.nn.functional as F

import disc_ref as DR
import step_kernels_ref as R
import vocoder_ref as VR
from seq2seq_vc_amd.ops import kernels_disc as KD
from seq2seq_vc_amd.ops import kernels_vocoder as KV
from seq2seq_vc_amd.urhythmic.vocoder import MultiPeriodDiscriminator, PeriodDiscriminator
from seq2seq_vc_amd.vocoder import HifiganGenerator

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SLACK = 64                   # floats of NaN in front of and behind every input (a multiple of 4: the views stay 16-byte aligned)
SENTINEL = 7.0e4
SLOPE = 0.5                  # exact in fp32


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _in_nan(t):
    """t (CPU float64, integers) as fp32 on the device inside a NaN-filled allocation"""
    big = torch.full((t.numel() + 2 * SLACK,), float("nan"), dtype=F32, device=DEV)
    view = big[SLACK:SLACK + t.numel()].view(t.shape)
    view.copy_(t.to(F32))
    return view


class _Guarded:
    """An output buffer inside a sentinel-filled allocation"""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.big = torch.full((n + 2 * SLACK,), SENTINEL, dtype=F32, device=DEV)
        self.view = self.big[SLACK:SLACK + n].view(shape)
        self.n = n

    def intact(self):
        return bool((self.big[:SLACK] == SENTINEL).all()) and bool((self.big[SLACK + self.n:] == SENTINEL).all())


def _exact(res, tag, got, want, guards=()):
    got, want = got.detach().cpu().to(F64), want.detach().to(F64)
    same = got.shape == want.shape and bool(torch.equal(got, want))
    worst = float((got - want).abs().max()) if got.shape == want.shape and got.numel() else float("nan")
    res.append((same and all(g.intact() for g in guards), f"{tag}: exact (max |diff| {worst:g}), nothing written outside the output"))


def _lrelu(v, slope=SLOPE):
    return torch.where(v > 0, v, v * slope)


def _cf(t):
    """channel-last (B, L, p, C) -> channel-first (B, C, L, p)"""
    return t.permute(0, 3, 1, 2)


def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _held(res, tag, got, ref64, ref32, ratios=None):
    ok, ratio, d, msg = R.compare(got.detach().cpu(), ref64, ref32, F32)
    if ratios is not None:
        ratios.append(ratio)
    res.append((ok, f"{tag}: {msg}"))


# ---------------------------------------------------------------------------------------------------------------------------
# case 4: the launchers alone, exact regime
# ---------------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = (
    # (B, L, p, C_in, C_out, stride): partial column tiles (48, 16 of 64), one K step (C_in 16), rows that cross a 128-row tile inside an
    # utterance (L * p > 128) and between the two, every (L - 1) % 3, L = 1 and 2 (every tap but the centre is padding)
    (2, 40, 5, 32, 48, 3), (2, 41, 5, 32, 48, 1), (2, 27, 11, 32, 48, 3), (2, 9, 2, 1024, 16, 3), (2, 70, 2, 1024, 16, 1),
    (2, 42, 7, 16, 48, 3), (3, 1, 11, 32, 48, 3), (2, 2, 3, 32, 48, 1), (1, 130, 1, 32, 80, 3),
)


def conv_kernels_exact():
    """disc_conv, disc_dgrad, disc_wgrad (+ the finish launch) against stock torch conv2d and its autograd"""
    res = []
    for n, (B, L, p, cin, cout, s) in enumerate(CONV_SHAPES):
        g = torch.Generator().manual_seed(100 + n)
        tag = f"B {B} L {L} p {p} {cin} -> {cout} stride {s}"
        Lo = KD.out_len(L, s)
        x, w, bias = _ints((B, L, p, cin), g), _ints((cout, cin, 5), g, -1, 1), _ints((cout,), g)
        xc = _cf(x).clone().requires_grad_(True)
        wc = w.unsqueeze(-1).clone().requires_grad_(True)
        pre = F.conv2d(xc, wc, bias, stride=(s, 1), padding=(2, 0))
        ok_shape = tuple(pre.shape) == (B, cout, Lo, p)
        _, op = KV.hifigan_fold(0, w.to(F32).to(DEV), None, F32, want_w32=False)
        out = _Guarded((B, Lo, p, cout))
        KD.disc_conv(_in_nan(x), op, bias.to(F32).to(DEV), cout, s, slope=SLOPE, out=out.view)
        res.append((ok_shape, f"{tag}: output rows {Lo}"))
        _exact(res, f"{tag}: forward", out.view, _cl(_lrelu(pre.detach())), (out,))
        # backward: dy, the stored output of the layer below (zeros included: leaky_relu'(0) = slope) and that feature's own gradient
        dy, mask, add = _ints((B, Lo, p, cout), g), _ints((B, L, p, cin), g, -1, 1), _ints((B, L, p, cin), g)
        dxr, dwr = torch.autograd.grad(pre, [xc, wc], _cf(dy))
        want = torch.where(mask > 0, torch.ones_like(mask), torch.full_like(mask, SLOPE)) * (add + _cl(dxr))
        if cout % 16 == 0:
            opT = KV.hifigan_fold_bwd(0, w.to(F32).to(DEV), F32)
            dx = _Guarded((B, L, p, cin))
            KD.disc_dgrad(_in_nan(dy), opT, L, cin, s, mask_src=_in_nan(mask), add=_in_nan(add), slope=SLOPE, out=dx.view)
            _exact(res, f"{tag}: data gradient with mask and feature gradient", dx.view, want, (dx,))
            dx2 = _Guarded((B, L, p, cin))
            KD.disc_dgrad(_in_nan(dy), opT, L, cin, s, out=dx2.view)
            _exact(res, f"{tag}: data gradient alone", dx2.view, _cl(dxr), (dx2,))
        nch = KD.chunks(B * Lo * p)
        wp, bp = _Guarded((nch, cout, 5, cin)), _Guarded((nch, cout))
        KD.disc_wgrad(_in_nan(dy), _in_nan(x), s, out=(wp.view, bp.view))
        _exact(res, f"{tag}: weight partials, summed over {nch} chunks", wp.view.sum(0).permute(0, 2, 1), dwr[..., 0], (wp,))
        _exact(res, f"{tag}: bias partials", bp.view.sum(0), dy.sum((0, 1, 2)), (bp,))
        gw, _, gb = KV.hifigan_wgrad_finish(0, wp.view.contiguous(), bp.view.contiguous(), w.to(F32).to(DEV))
        _exact(res, f"{tag}: finish launch over the partials", gw, dwr[..., 0])
        _exact(res, f"{tag}: finish launch, bias", gb, dy.sum((0, 1, 2)))
    return res


INPUT_SHAPES = ((2, 700, 11), (2, 331, 7), (2, 331, 3), (3, 23, 11), (2, 64, 2), (1, 1000, 5), (2, 12, 11))


def input_kernels_exact():
    """disc_input, disc_input_wgrad, disc_input_dgrad against F.pad(reflect) + view + conv2d and their autograd"""
    res = []
    for n, (B, T, p) in enumerate(INPUT_SHAPES):
        g = torch.Generator().manual_seed(200 + n)
        tag = f"B {B} T {T} p {p}"
        L0, pad = KD.folded_len(T, p)
        L1 = KD.out_len(L0, 3)
        x, w, bias = _ints((B, 1, T), g), _ints((32, 1, 5), g, -1, 1), _ints((32,), g)
        xc, wc = x.clone().requires_grad_(True), w.unsqueeze(-1).clone().requires_grad_(True)
        xp = F.pad(xc, (0, pad), "reflect") if pad else xc
        pre = F.conv2d(xp.view(B, 1, L0, p), wc, bias, stride=(3, 1), padding=(2, 0))
        out = _Guarded((B, L1, p, 32))
        KD.disc_input(_in_nan(x.view(B, T)), w.to(F32).to(DEV), bias.to(F32).to(DEV), p, slope=SLOPE, out=out.view)
        _exact(res, f"{tag} (pad {pad}): forward", out.view, _cl(_lrelu(pre.detach())), (out,))
        dy = _ints((B, L1, p, 32), g)
        dxr, dwr = torch.autograd.grad(pre, [xc, wc], _cf(dy))
        nch = KD.chunks(B * L1 * p)
        wp, bp = _Guarded((nch, 32, 5, 1)), _Guarded((nch, 32))
        KD.disc_input_wgrad(_in_nan(dy), _in_nan(x.view(B, T)), p, out=(wp.view, bp.view))
        _exact(res, f"{tag}: weight partials, summed over {nch} chunks", wp.view.sum(0).permute(0, 2, 1), dwr[..., 0], (wp,))
        _exact(res, f"{tag}: bias partials", bp.view.sum(0), dy.sum((0, 1, 2)), (bp,))
        dx = _Guarded((B, T))
        KD.disc_input_dgrad(_in_nan(dy), w.to(F32).to(DEV), T, p, out=dx.view)
        _exact(res, f"{tag}: dx with the mirror terms", dx.view, dxr.view(B, T), (dx,))
    return res


POST_SHAPES = ((2, 40, 5, 1024), (2, 1, 11, 1024), (2, 2, 3, 1024), (3, 100, 2, 64), (1, 30, 11, 1024))


def post_kernels_exact():
    """disc_post, disc_post_bwd (+ the finish launch, mode 2) against conv2d (k 3, padding 1) and its autograd"""
    res = []
    for n, (B, L, p, C) in enumerate(POST_SHAPES):
        g = torch.Generator().manual_seed(300 + n)
        tag = f"B {B} L {L} p {p} C {C}"
        x, w, bias = _ints((B, L, p, C), g, -1, 1), _ints((1, C, 3), g, -1, 1), _ints((1,), g)
        xc, wc = _cf(x).clone().requires_grad_(True), w.unsqueeze(-1).clone().requires_grad_(True)
        y = F.conv2d(xc, wc, bias, padding=(1, 0))
        _, op = KV.hifigan_fold(2, w.to(F32).to(DEV), None, F32, want_w32=False)
        out = _Guarded((B, L * p))
        KD.disc_post(_in_nan(x), op, bias.to(F32).to(DEV), out=out.view)
        _exact(res, f"{tag}: forward", out.view, y.detach().flatten(1), (out,))
        dy1, dy2, add = _ints((B, L * p), g), _ints((B, L * p), g), _ints((B, L, p, C), g)
        dxr, dwr = torch.autograd.grad(y, [xc, wc], (dy1 + dy2).view(B, 1, L, p))
        want = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, SLOPE)) * (add + _cl(dxr))
        nch = KD.chunks(B * L * p)
        dx, wp, bp = _Guarded((B, L, p, C)), _Guarded((nch, 3, C)), _Guarded((nch,))
        KD.disc_post_bwd(_in_nan(x), op, dy1=_in_nan(dy1), dy2=_in_nan(dy2), add=_in_nan(add), slope=SLOPE, out=(dx.view, wp.view, bp.view))
        _exact(res, f"{tag}: data gradient, both score gradients, feature gradient, mask", dx.view, want, (dx,))
        _exact(res, f"{tag}: weight partials, summed over {nch} chunks", wp.view.sum(0).t(), dwr[0, :, :, 0], (wp,))
        _exact(res, f"{tag}: bias partials", bp.view.sum(0, keepdim=True), (dy1 + dy2).sum().view(1), (bp,))
        gw, _, gb = KV.hifigan_wgrad_finish(2, wp.view.contiguous(), bp.view.contiguous(), w.to(F32).to(DEV))
        _exact(res, f"{tag}: finish launch over the partials", gw, dwr[..., 0])
        dx1 = KD.disc_post_bwd(_in_nan(x), op, dy2=_in_nan(dy2), slope=SLOPE)[0]
        (dxr1,) = torch.autograd.grad(F.conv2d(xc, wc, bias, padding=(1, 0)), [xc], dy2.view(B, 1, L, p))
        _exact(res, f"{tag}: data gradient from the feature's gradient alone", dx1,
               torch.where(x > 0, torch.ones_like(x), torch.full_like(x, SLOPE)) * _cl(dxr1))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# cases 1 - 3: the whole discriminator
# ---------------------------------------------------------------------------------------------------------------------------
_SHARED = {}


def _seeded():
    if "sd" not in _SHARED:
        _SHARED["sd"] = DR.seeded_state_dict(DR.SEED)
        mpd = MultiPeriodDiscriminator()
        mpd.load_state_dict(_SHARED["sd"])
        _SHARED["mpd"] = mpd.to(DEV)
    return _SHARED["sd"], _SHARED["mpd"]


def _pass(mpd, xr, xg):
    """one forward + backward of the fixed loss -> (scores, feats, dx or None, {name: grad})"""
    mpd.zero_grad(set_to_none=True)
    xg.grad = None
    sr, fr = mpd(xr)
    sg, fg = mpd(xg)
    DR.total_loss(sr, fr, sg, fg).backward()
    return sg, fg, xg.grad, {k: p.grad.clone() for k, p in mpd.named_parameters()}


def _model_case(name, xr, xg):
    res, ratios = [], []
    sd, mpd = _seeded()
    ref64, ref32 = DR.run(sd, xr, xg, F64), DR.run(sd, xr, xg, F32)
    B, _, T = xg.shape
    xr_d, xg_d = xr.to(DEV), xg.to(DEV).requires_grad_(True)
    sg, fg, dx, grads = _pass(mpd, xr_d, xg_d)
    dx = dx.clone()
    node = type(sg[0].grad_fn).__name__
    one_node = all(f.grad_fn is sg[i].grad_fn for i, fl in enumerate(fg) for f in fl) and node.startswith("_PeriodFunction")
    res.append((one_node, f"{name}: every discriminator call is one autograd node ({node}) with the score and six features as outputs"))
    for i in range(5):
        _held(res, f"{name}: score {i}", sg[i], ref64["scores"][i], ref32["scores"][i], ratios)
        for j in range(6):
            shape_ok = tuple(fg[i][j].shape) == tuple(ref64["feats"][i][j].shape)
            _held(res, f"{name}: feature {i}.{j} {tuple(fg[i][j].shape) if shape_ok else 'WRONG SHAPE'}", fg[i][j], ref64["feats"][i][j], ref32["feats"][i][j], ratios)
        res.append((R.bits_equal(sg[i], fg[i][5].flatten(1)), f"{name}: score {i} is the flattening of the last feature"))
    _held(res, f"{name}: dx", dx, ref64["dxg"], ref32["dxg"], ratios)
    res.append((len(grads) == 90, f"{name}: 90 parameter gradients"))
    for k, gv in grads.items():
        _held(res, f"{name}: grad {k}", gv, ref64["grads"][k], ref32["grads"][k], ratios)
    fin = [r for r in ratios if r != float("inf")]
    res.append((True, f"{name}: ratios max|got - ref64| / d over {len(ratios)} tensors: largest {max(fin):.3f}, median {sorted(fin)[len(fin) // 2]:.3f}"))
    # a second call gives the same bits
    sg2, fg2, dx2, grads2 = _pass(mpd, xr_d, xg_d)
    same = (all(R.bits_equal(a, b) for a, b in zip(sg, sg2)) and all(R.bits_equal(a, b) for fa, fb in zip(fg, fg2) for a, b in zip(fa, fb))
            and R.bits_equal(dx, dx2) and all(R.bits_equal(grads[k], grads2[k]) for k in grads))
    res.append((same, f"{name}: a second forward + backward gives the same bits (scores, features, dx, 90 gradients)"))
    # D(x.detach()): the same parameter gradients, no dx
    xdet = xg_d.detach()
    xg_d.grad = None
    _, _, dx3, grads3 = _pass(mpd, xr_d, xdet)
    res.append((dx3 is None and xg_d.grad is None and all(R.bits_equal(grads[k], grads3[k]) for k in grads),
                f"{name}: D(x.detach()) gives the same parameter gradients bit for bit and no dx"))
    # every row equals its own B = 1 call
    with torch.no_grad():
        rows_ok = True
        for b in range(B):
            s1, f1 = mpd(xdet[b:b + 1])
            rows_ok = rows_ok and all(R.bits_equal(s1[i], sg[i][b:b + 1]) for i in range(5))
            rows_ok = rows_ok and all(R.bits_equal(f1[i][j], fg[i][j][b:b + 1]) for i in range(5) for j in range(6))
        res.append((rows_ok, f"{name}: every row of the batched forward has the bits of its own B = 1 call"))
    mpd.zero_grad(set_to_none=True)
    return res, (sg, fg)


def case_t700():
    """T % p = 0, 1, 0, 0, 7: pads of 0, 2, 0, 0, 4 samples; the lengths per layer cover (L - 1) % 3 = 0, 1, 2"""
    xr, xg = DR.inputs(700)
    chains = [DR.length_chain(700, p) for p in DR.PERIODS]
    covered = {(L - 1) % 3 for c in chains for L in c[:4]}
    res, _ = _model_case("T 700", xr, xg)
    return [(covered == {0, 1, 2}, f"T 700: lengths {chains} cover every (L - 1) % 3")] + res


def case_t331():
    """the last stride-3 layers run at L = 1 for p = 5, 7, 11; T % 3 = 1 gives the largest pad, p - 1"""
    xr, xg = DR.inputs(331)
    chains = {p: DR.length_chain(331, p) for p in DR.PERIODS}
    ok = all(chains[p][4] == 1 for p in (5, 7, 11)) and 331 % 3 == 1
    res, _ = _model_case("T 331", xr, xg)
    return [(ok, f"T 331: lengths {chains}")] + res


def case_zero_utterance():
    """utterance 0 all zeros, utterance 1 large, rows that cross a 128-row tile inside an utterance and between the two: a value of
    utterance 1 that leaked into utterance 0 shows as a non-bias value there (and breaks the equality with the B = 1 call)"""
    T = 450
    xr, xg = DR.inputs(T)
    xg = xg.clone()
    xg[0] = 0
    xg[1] *= 300.0
    rows = [DR.length_chain(T, p)[1] * p for p in DR.PERIODS]
    res, (sg, fg) = _model_case("zero utterance", xr, xg)
    res.insert(0, (all(r > 128 and r % 128 for r in rows), f"zero utterance: rows per utterance after the input layer {rows}: tiles cross inside and between"))
    _, mpd = _seeded()
    for i, d in enumerate(mpd.discriminators):
        want = F.leaky_relu(d.convs[0].bias.detach(), 0.1).view(1, -1, 1, 1).expand_as(fg[i][0][0:1])
        res.append((R.bits_equal(fg[i][0][0:1], want), f"zero utterance: feature {i}.0 of utterance 0 is leaky_relu(bias) at every position"))
        with torch.no_grad():
            s0, _ = d(torch.zeros(1, 1, T, device=DEV))
        res.append((R.bits_equal(s0, sg[i][0:1]), f"zero utterance: score {i} of utterance 0 has the bits of a call on zeros alone"))
    return res


def chain_generator():
    """generator (tiny, trainable) -> discriminator -> loss -> backward: dx flows into HifiganGenerator.trainable() unchanged"""
    res = []
    cfg, gsd, _, _, _ = VR.load_fixture()
    sd, mpd = _seeded()
    g = torch.Generator().manual_seed(7)
    mel = torch.randn(2, cfg["in_channels"], 8, generator=g)
    T = 8 * 64
    xr = 0.3 * torch.randn(2, 1, T, generator=g)
    refs = []
    for dt in (F64, F32):
        prm = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in gsd.items()}
        dsd = {k: v.to(dt) for k, v in sd.items()}
        y = VR.generator_forward(prm, cfg, mel.to(dt))
        sr, fr = DR.mpd_forward(dsd, xr.to(dt))
        sg, fg = DR.mpd_forward(dsd, y)
        grads = torch.autograd.grad(DR.total_loss(sr, fr, sg, fg), list(prm.values()))
        refs.append((y.detach(), dict(zip(prm.keys(), grads))))
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(gsd)
    gen.to(DEV).trainable()
    mpd.zero_grad(set_to_none=True)
    y = gen(mel.to(DEV))
    res.append((tuple(y.shape) == (2, 1, T) and y.grad_fn is not None, f"chain: generator output {tuple(y.shape)} with a grad_fn"))
    sr, fr = mpd(xr.to(DEV))
    sg, fg = mpd(y)
    DR.total_loss(sr, fr, sg, fg).backward()
    _held(res, "chain: generator output", y, refs[0][0], refs[1][0])
    for k, p in gen.named_parameters():
        _held(res, f"chain: generator grad {k}", p.grad, refs[0][1][k], refs[1][1][k])
    mpd.zero_grad(set_to_none=True)
    return res


def module_refusals():
    """what the module refuses on the device: bf16, a period longer than the input; and a single PeriodDiscriminator under no_grad"""
    res = []
    d = PeriodDiscriminator(3).to(DEV)
    x = torch.randn(2, 1, 100, device=DEV)
    for what, fn, exc in (("bf16 input", lambda: d(x.bfloat16()), NotImplementedError), ("T < period", lambda: PeriodDiscriminator(11).to(DEV)(x[:, :, :10]), ValueError),
                          ("CPU input", lambda: d(x.cpu()), RuntimeError)):
        try:
            fn()
            res.append((False, f"{what}: not refused"))
        except exc as e:
            res.append((True, f"{what}: {type(e).__name__}: {str(e)[:60]}"))
    with torch.no_grad():
        s, f = d(x)
    res.append((s.grad_fn is None and tuple(s.shape) == (2, DR.length_chain(100, 3)[5] * 3) and len(f) == 6, "no_grad call: plain tensors, the reference's shapes"))
    for prm in d.parameters():
        prm.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    s, f = d(xg)
    (s.sum() + f[2].abs().sum()).backward()
    res.append((xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and all(prm.grad is None for prm in d.parameters()),
                "frozen parameters: dx alone (the weight-gradient launches are skipped)"))
    return res


CASES = [conv_kernels_exact, input_kernels_exact, post_kernels_exact, case_t700, case_t331, case_zero_utterance, chain_generator, module_refusals]


if __name__ == "__main__":
    import sys
    bad = 0
    for c in CASES:
        if len(sys.argv) > 1 and c.__name__ not in sys.argv[1:]:
            continue
        for ok, msg in c():
            print(("ok   " if ok else "FAIL ") + msg, flush=True)
            bad += not ok
    sys.exit(1 if bad else 0)
