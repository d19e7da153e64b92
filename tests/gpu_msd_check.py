"""HiFi-GAN multi-scale discriminator on the MI355X (csrc/hifigan_msd.hip, seq2seq_vc_amd/urhythmic/vocoder.py): every launcher
alone, and the whole discriminator, forward and backward, against the plain-torch restatement tests/msd_ref.py.
Each case returns [(ok, message)]; tests/test_gpu_msd.py turns them into pytest tests.

Kernel level (zero tolerance): inputs are small integers (|x| <= 2, |w| <= 1), the slope is 0.5, so every sum stays below 2^24 and is
exact in fp32 whatever its order, and the float64 result of stock torch (conv1d, avg_pool1d and their autograd) must be met bit for
bit.  Inputs live inside NaN-filled allocations (a read before the first or past the last row poisons the result), outputs inside
sentinel-filled ones (a write outside shows).  The spectral-norm launches are not exact: they are held to the real-number rule below.

Model level: step_kernels_ref.compare, unchanged -- per tensor |got - ref64| <= 4 d + ulp, d = max |restatement in float32 - restatement
in float64| on the same inputs.  Nothing here is fitted to what the kernels return."""
import torch
import torch.nn.functional as F

import disc_ref as DR
import msd_ref as MR
import step_kernels_ref as R
import vocoder_ref as VR
from gpu_disc_check import DEV, F32, F64, SLOPE, _exact, _Guarded, _held, _in_nan, _ints, _lrelu
from seq2seq_vc_amd.ops import kernels_msd as KM
from seq2seq_vc_amd.ops import kernels_vocoder as KV
from seq2seq_vc_amd.urhythmic.vocoder import HifiganDiscriminator, MultiScaleDiscriminator, ScaleDiscriminator
from seq2seq_vc_amd.vocoder import HifiganGenerator


def _cl(t):
    """channel-first (B, C, L) -> contiguous channel-last (B, L, C)"""
    return t.permute(0, 2, 1).contiguous()


def _cf(t):
    return t.permute(0, 2, 1)


def _dmask(m):
    return torch.where(m > 0, torch.ones_like(m), torch.full_like(m, SLOPE))


# ---------------------------------------------------------------------------------------------------------------------------
# the launchers alone, exact regime
# ---------------------------------------------------------------------------------------------------------------------------
GCONV_SHAPES = (
    # (B, L, C_in, C_out, groups, stride): the five real layer widths at short lengths
    (2, 45, 128, 128, 4, 2), (2, 46, 128, 256, 16, 2), (2, 150, 256, 512, 16, 4), (2, 48, 256, 512, 16, 4), (2, 131, 512, 1024, 16, 4),
    (3, 1, 512, 1024, 16, 4), (2, 2, 1024, 1024, 16, 1),
    (2, 133, 1024, 1024, 16, 1),          # rows cross a 128-row tile inside an utterance and between two
    (1, 260, 128, 128, 4, 2),
)


def gconv_kernels_exact():
    """msd_gconv, msd_fold_bwd + msd_gconv_dgrad, msd_gconv_wgrad (+ the finish launch) against stock torch conv1d and its autograd"""
    res = []
    shapes = GCONV_SHAPES
    covered = {(s, (L - 1) % s) for _, L, _, _, _, s in shapes}
    want_cov = {(s, r) for s in (1, 2, 4) for r in range(s)}
    res.append((covered == want_cov and any(L == 1 for _, L, *_ in shapes) and any(1 < L < 41 for _, L, *_ in shapes)
                and {g for *_, g, _ in shapes} == {4, 16},
                f"shapes cover every (L - 1) % s {sorted(covered)}, L = 1, 1 < L < 41 and both group counts"))
    for n, (B, L, cin, cout, groups, s) in enumerate(shapes):
        g = torch.Generator().manual_seed(400 + n)
        tag = f"B {B} L {L} {cin} -> {cout} groups {groups} stride {s}"
        Lo, cg = KM.out_len(L, s), cin // groups
        x, w, bias = _ints((B, L, cin), g), _ints((cout, cg, 41), g, -1, 1), _ints((cout,), g)
        xc, wc = _cf(x).clone().requires_grad_(True), w.clone().requires_grad_(True)
        pre = F.conv1d(xc, wc, bias, stride=s, padding=20, groups=groups)
        w_d = w.to(F32).to(DEV)
        _, op = KV.hifigan_fold(0, w_d, None, F32, want_w32=False)
        out = _Guarded((B, Lo, cout))
        KM.msd_gconv(_in_nan(x), op, bias.to(F32).to(DEV), cout, groups, s, slope=SLOPE, out=out.view)
        res.append((tuple(pre.shape) == (B, cout, Lo), f"{tag}: output rows {Lo}"))
        _exact(res, f"{tag}: forward", out.view, _cl(_lrelu(pre.detach())), (out,))
        # backward: dy, the stored output of the layer below (zeros included: leaky_relu'(0) = slope) and that feature's own gradient
        dy, mask, add = _ints((B, Lo, cout), g), _ints((B, L, cin), g, -1, 1), _ints((B, L, cin), g)
        dxr, dwr = torch.autograd.grad(pre, [xc, wc], _cf(dy))
        opT = _Guarded((cin, 41 * KV.cin_padded(cout // groups)))
        KM.msd_fold_bwd(w_d, groups, out=opT.view)
        res.append((opT.intact(), f"{tag}: transposed operand, nothing written outside"))
        dx = _Guarded((B, L, cin))
        KM.msd_gconv_dgrad(_in_nan(dy), opT.view, L, cin, groups, s, mask_src=_in_nan(mask), add=_in_nan(add), slope=SLOPE, out=dx.view)
        _exact(res, f"{tag}: data gradient with mask and feature gradient", dx.view, _dmask(mask) * (add + _cl(dxr)), (dx,))
        dx2 = _Guarded((B, L, cin))
        KM.msd_gconv_dgrad(_in_nan(dy), opT.view, L, cin, groups, s, out=dx2.view)
        _exact(res, f"{tag}: data gradient alone", dx2.view, _cl(dxr), (dx2,))
        nch = KM.gconv_chunks(B, Lo)
        res.append((nch == B * -(-Lo // KM.gconv_chunk(Lo)) and KM.gconv_chunk(Lo) == max(256, 32 * -(-Lo // 256)), f"{tag}: {nch} chunks of {KM.gconv_chunk(Lo)} rows"))
        wp, bp = _Guarded((nch, cout, 41, cg)), _Guarded((nch, cout))
        KM.msd_gconv_wgrad(_in_nan(dy), _in_nan(x), groups, s, out=(wp.view, bp.view))
        _exact(res, f"{tag}: weight partials, summed over {nch} chunks", wp.view.sum(0).permute(0, 2, 1), dwr, (wp,))
        _exact(res, f"{tag}: bias partials", bp.view.sum(0), dy.sum((0, 1)), (bp,))
        gw, _, gb = KV.hifigan_wgrad_finish(0, wp.view.contiguous(), bp.view.contiguous(), w_d)
        _exact(res, f"{tag}: finish launch over the partials", gw, dwr)
        _exact(res, f"{tag}: finish launch, bias", gb, dy.sum((0, 1)))
    return res


def wgrad_chunks_exact():
    """more than one chunk per utterance: 300 output rows at stride 1 cut at 256, the halo crossing the cut"""
    res = []
    B, L, cin, cout, groups, s = 2, 300, 32, 32, 4, 1
    g = torch.Generator().manual_seed(450)
    x, w, dy = _ints((B, L, cin), g), _ints((cout, cin // groups, 41), g, -1, 1), _ints((B, L, cout), g)
    xc, wc = _cf(x).clone().requires_grad_(True), w.clone().requires_grad_(True)
    (dwr,) = torch.autograd.grad(F.conv1d(xc, wc, None, stride=s, padding=20, groups=groups), [wc], _cf(dy))
    nch = KM.gconv_chunks(B, L)
    wp, bp = _Guarded((nch, cout, 41, cin // groups)), _Guarded((nch, cout))
    KM.msd_gconv_wgrad(_in_nan(dy), _in_nan(x), groups, s, out=(wp.view, bp.view))
    res.append((nch == 4, f"{nch} chunks for 2 x 300 rows"))
    _exact(res, "weight partials over two chunks per utterance", wp.view.sum(0).permute(0, 2, 1), dwr, (wp,))
    _exact(res, "bias partials of chunk 1 of utterance 0", bp.view[1], dy[0, 256:].sum(0), (bp,))
    return res


def input_kernels_exact():
    """msd_input, msd_input_wgrad, msd_input_dgrad against conv1d (15 taps, padding 7) and its autograd"""
    res = []
    for n, (B, T) in enumerate((b, t) for t in (1, 7, 14, 331, 700) for b in (2, 3)):
        g = torch.Generator().manual_seed(500 + n)
        tag = f"B {B} T {T}"
        x, w, bias = _ints((B, 1, T), g), _ints((128, 1, 15), g, -1, 1), _ints((128,), g)
        xc, wc = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        pre = F.conv1d(xc, wc, bias, padding=7)
        w_d = w.to(F32).to(DEV)
        out = _Guarded((B, T, 128))
        KM.msd_input(_in_nan(x.view(B, T)), w_d, bias.to(F32).to(DEV), slope=SLOPE, out=out.view)
        _exact(res, f"{tag}: forward", out.view, _cl(_lrelu(pre.detach())), (out,))
        dy = _ints((B, T, 128), g)
        dxr, dwr = torch.autograd.grad(pre, [xc, wc], _cf(dy))
        nch = -(-B * T // KM.IN_CHUNK)
        wp, bp = _Guarded((nch, 128, 15, 1)), _Guarded((nch, 128))
        KM.msd_input_wgrad(_in_nan(dy), _in_nan(x.view(B, T)), out=(wp.view, bp.view))
        _exact(res, f"{tag}: weight partials, summed over {nch} chunks", wp.view.sum(0).permute(0, 2, 1), dwr, (wp,))
        _exact(res, f"{tag}: bias partials", bp.view.sum(0), dy.sum((0, 1)), (bp,))
        gw, _, gb = KV.hifigan_wgrad_finish(0, wp.view.contiguous(), bp.view.contiguous(), w_d)
        _exact(res, f"{tag}: finish launch over the partials", gw, dwr)
        dx = _Guarded((B, T))
        KM.msd_input_dgrad(_in_nan(dy), w_d, out=dx.view)
        _exact(res, f"{tag}: dx", dx.view, dxr.view(B, T), (dx,))
    return res


def pool_kernels_exact():
    """msd_pool, msd_pool_bwd against avg_pool1d(4, 2, padding 2) and its autograd"""
    res = []
    for n, T in enumerate((1, 2, 3, 7, 331, 332)):
        g = torch.Generator().manual_seed(600 + n)
        B = 2 + n % 2
        x = _ints((B, 1, T), g)
        xc = x.clone().requires_grad_(True)
        y = F.avg_pool1d(xc, 4, 2, padding=2)
        To = KM.pool_len(T)
        out = _Guarded((B, To))
        KM.msd_pool(_in_nan(x.view(B, T)), out=out.view)
        res.append((y.shape[-1] == To, f"T {T}: {To} samples after the pool"))
        _exact(res, f"B {B} T {T}: pool", out.view, y.detach().view(B, To), (out,))
        dy = _ints((B, To), g)
        (dxr,) = torch.autograd.grad(y, [xc], dy.view(B, 1, To))
        dx = _Guarded((B, T))
        KM.msd_pool_bwd(_in_nan(dy), T, out=dx.view)
        _exact(res, f"B {B} T {T}: adjoint", dx.view, dxr.view(B, T), (dx,))
    return res


def spectral_kernels():
    """msd_sn_power (iterate on and off), msd_sn_scale, msd_sn_finish under the real-number rule: |got - ref64| <= 4 d + ulp with
    d = |the same formulas in float32 - in float64|"""
    res = []
    for n, (O, K) in enumerate(((128, 15), (128, 1312), (1024, 2624))):
        g = torch.Generator().manual_seed(700 + n)
        W = 0.05 * torch.randn(O, K // 41 if K % 41 == 0 else 1, 41 if K % 41 == 0 else K, generator=g)
        u0, v0 = F.normalize(torch.randn(O, generator=g), dim=0), F.normalize(torch.randn(K, generator=g), dim=0)
        dW = torch.randn(W.shape, generator=g)
        W_d, dW_d = W.to(DEV), dW.to(DEV)
        for iterate in (True, False):
            tag = f"({O}, {K}) iterate {iterate}"
            refs = []
            for dt in (F64, F32):
                u, v = MR.power_iteration(W.to(dt), u0.to(dt), v0.to(dt), iterate)
                refs.append((u, v, torch.dot(u, W.to(dt).flatten(1) @ v).view(1)))
            u_d, v_d = u0.to(DEV), v0.to(DEV)
            sigma = KM.msd_sn_power(W_d, u_d, v_d, iterate)
            if iterate:
                _held(res, f"{tag}: u", u_d, refs[0][0], refs[1][0])
                _held(res, f"{tag}: v", v_d, refs[0][1], refs[1][1])
            else:
                res.append((R.bits_equal(u_d, u0) and R.bits_equal(v_d, v0), f"{tag}: the buffers are untouched"))
            _held(res, f"{tag}: sigma", sigma, refs[0][2], refs[1][2])
            # the division and its backward from the float32 u, v, sigma the launch left (the inputs of both references)
            u_c, v_c, s_c = u_d.cpu(), v_d.cpu(), sigma.cpu()
            _held(res, f"{tag}: W / sigma", KM.msd_sn_scale(W_d, sigma), W.to(F64) / s_c.to(F64), W / s_c)
            r64 = MR.spectral_grad(dW.to(F64), W.to(F64), u_c.to(F64), v_c.to(F64), s_c.to(F64)[0])
            r32 = MR.spectral_grad(dW, W, u_c, v_c, s_c[0])
            _held(res, f"{tag}: gradient of weight_orig", KM.msd_sn_finish(dW_d, W_d, u_d, v_d, sigma), r64, r32)
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the whole discriminator
# ---------------------------------------------------------------------------------------------------------------------------
_SHARED = {}


def _seeded():
    if "sd" not in _SHARED:
        _SHARED["sd"] = MR.seeded_state_dict(MR.SEED)
        _SHARED["msd"] = MultiScaleDiscriminator().to(DEV)
    _SHARED["msd"].load_state_dict(_SHARED["sd"])            # the seeded buffers again: a training call moves u, v
    _SHARED["msd"].train()
    return _SHARED["sd"], _SHARED["msd"]


def _pass(msd, xr, xg):
    """one forward + backward of the fixed loss -> (scores, feats, dx or None, {name: grad})"""
    msd.zero_grad(set_to_none=True)
    xg.grad = None
    sr, fr = msd(xr)
    sg, fg = msd(xg)
    MR.total_loss(sr, fr, sg, fg).backward()
    return sg, fg, xg.grad, {k: p.grad.clone() for k, p in msd.named_parameters()}


def _model_case(name, xr, xg):
    res, ratios = [], []
    sd, msd = _seeded()
    ref64, ref32 = MR.run(sd, xr, xg, F64), MR.run(sd, xr, xg, F32)
    B, _, T = xg.shape
    xr_d, xg_d = xr.to(DEV), xg.to(DEV).requires_grad_(True)
    sg, fg, dx, grads = _pass(msd, xr_d, xg_d)
    dx = dx.clone()
    buffers = {k: v.clone() for k, v in msd.named_buffers()}
    node = type(sg[0].grad_fn).__name__
    one_node = all(f.grad_fn is sg[i].grad_fn for i, fl in enumerate(fg) for f in fl) and node.startswith("_ScaleFunction")
    res.append((one_node, f"{name}: every discriminator call is one autograd node ({node}) with the score and eight features as outputs"))
    for i in range(3):
        _held(res, f"{name}: score {i}", sg[i], ref64["scores"][i], ref32["scores"][i], ratios)
        for j in range(8):
            shape_ok = tuple(fg[i][j].shape) == tuple(ref64["feats"][i][j].shape)
            _held(res, f"{name}: feature {i}.{j} {tuple(fg[i][j].shape) if shape_ok else 'WRONG SHAPE'}", fg[i][j], ref64["feats"][i][j], ref32["feats"][i][j], ratios)
        res.append((R.bits_equal(sg[i], fg[i][7].flatten(1)), f"{name}: score {i} is the flattening of the last feature"))
    _held(res, f"{name}: dx", dx, ref64["dxg"], ref32["dxg"], ratios)
    res.append((len(grads) == 64, f"{name}: 64 parameter gradients"))
    for k, gv in grads.items():
        _held(res, f"{name}: grad {k}", gv, ref64["grads"][k], ref32["grads"][k], ratios)
    res.append((len(buffers) == 16, f"{name}: 16 buffers"))
    for k, bv in buffers.items():
        _held(res, f"{name}: buffer {k} after two calls", bv, ref64["buffers"][k], ref32["buffers"][k], ratios)
    fin = [r for r in ratios if r != float("inf")]
    res.append((True, f"{name}: ratios max|got - ref64| / d over {len(ratios)} tensors: largest {max(fin):.3f}, median {sorted(fin)[len(fin) // 2]:.3f}"))
    # from the seeded buffers again, a second call gives the same bits
    _seeded()
    sg2, fg2, dx2, grads2 = _pass(msd, xr_d, xg_d)
    same = (all(R.bits_equal(a, b) for a, b in zip(sg, sg2)) and all(R.bits_equal(a, b) for fa, fb in zip(fg, fg2) for a, b in zip(fa, fb))
            and R.bits_equal(dx, dx2) and all(R.bits_equal(grads[k], grads2[k]) for k in grads)
            and all(R.bits_equal(buffers[k], v) for k, v in msd.named_buffers()))
    res.append((same, f"{name}: a second forward + backward from the same buffers gives the same bits (scores, features, dx, 64 gradients, u, v)"))
    # D(x.detach()): the same parameter gradients, no dx
    _seeded()
    xdet = xg_d.detach()
    xg_d.grad = None
    _, _, dx3, grads3 = _pass(msd, xr_d, xdet)
    res.append((dx3 is None and xg_d.grad is None and all(R.bits_equal(grads[k], grads3[k]) for k in grads),
                f"{name}: D(x.detach()) gives the same parameter gradients bit for bit and no dx"))
    # every row equals its own B = 1 call (eval(): the buffers stay)
    msd.eval()
    with torch.no_grad():
        sb, fb = msd(xdet)
        rows_ok = True
        for b in range(B):
            s1, f1 = msd(xdet[b:b + 1])
            rows_ok = rows_ok and all(R.bits_equal(s1[i], sb[i][b:b + 1]) for i in range(3))
            rows_ok = rows_ok and all(R.bits_equal(f1[i][j], fb[i][j][b:b + 1]) for i in range(3) for j in range(8))
        res.append((rows_ok, f"{name}: every row of the batched forward has the bits of its own B = 1 call"))
    msd.train()
    msd.zero_grad(set_to_none=True)
    return res, (sg, fg, buffers)


def _chain_cover(Ts):
    return {(L - 1) % 4 for T in Ts for row in MR.length_chain(T) for L in row[2:4]}


def case_t331():
    """the chains end at L = 6 / 3 / 2"""
    xr, xg = MR.inputs(331)
    chains = MR.length_chain(331)
    res, _ = _model_case("T 331", xr, xg)
    ok = [c[-1] for c in chains] == [6, 3, 2] and _chain_cover((331, 97)) == {0, 1, 2, 3}
    return [(ok, f"T 331: lengths {chains}; with T 97 the inputs of the stride-4 layers cover every (L - 1) % 4")] + res


def case_t97():
    """the chains end at L = 2 / 1 / 1"""
    xr, xg = MR.inputs(97)
    chains = MR.length_chain(97)
    res, _ = _model_case("T 97", xr, xg)
    return [([c[-1] for c in chains] == [2, 1, 1], f"T 97: lengths {chains}")] + res


def case_zero_utterance():
    """utterance 0 all zeros, utterance 1 large: a value of utterance 1 that leaked into utterance 0 shows as a non-bias value there"""
    T = 450
    xr, xg = MR.inputs(T)
    xg = xg.clone()
    xg[0] = 0
    xg[1] *= 300.0
    res, (sg, fg, after_two) = _model_case("zero utterance", xr, xg)
    sd, msd = _seeded()
    # _model_case ran D(xr), D(xg) from the seeded buffers: repeat the first call so that the buffers are those D(xg) started from
    with torch.no_grad():
        msd(xr.to(DEV))
        x = torch.zeros(1, 1, T, device=DEV)
        for i, d in enumerate(msd.discriminators):
            if i:
                x = msd.meanpools[i - 1](x)
            want = F.leaky_relu(d.convs[0].bias.detach(), 0.1).view(1, -1, 1).expand_as(fg[i][0][0:1])
            res.append((R.bits_equal(fg[i][0][0:1], want), f"zero utterance: feature {i}.0 of utterance 0 is leaky_relu(bias) at every position"))
            s0, _ = d(x)
            res.append((R.bits_equal(s0, sg[i][0:1]), f"zero utterance: score {i} of utterance 0 has the bits of a call on zeros alone"))
    # the iteration does not depend on x: D(xr) and the calls on zeros leave the u, v that D(xr), D(xg) left, so the weights were the same
    res.append((len(after_two) == 16 and all(R.bits_equal(after_two[k], v) for k, v in msd.named_buffers()),
                "zero utterance: the calls on zeros ran from the buffers D(xg) ran from (the 16 buffers end with the same bits)"))
    return res


def buffer_semantics():
    """train(): every call moves u, v, under no_grad too; eval(): the buffers stay and the stored u, v give sigma"""
    res = []
    sd, msd = _seeded()
    x = MR.inputs(97)[1].to(DEV)
    start = {k: v.clone() for k, v in msd.named_buffers()}
    with torch.no_grad():
        s1, _ = msd(x)
    moved = {k: v.clone() for k, v in msd.named_buffers()}
    # conv_post's u has one element: a unit vector of length 1 is +-1 and stays where it is
    res.append((all(R.bits_equal(start[k], moved[k]) == (start[k].numel() == 1) for k in start) and sum(v.numel() == 1 for v in start.values()) == 1,
                "train(), no_grad: one call moves the 15 buffers with more than one element"))
    after = {}
    ref, _ = MR.msd_forward({k: v.double() for k, v in sd.items()}, x.cpu().double(), True, after)
    ref32, _ = MR.msd_forward(sd, x.cpu(), True)
    _held(res, "train(), no_grad: scores of scale 0 use the iterated u, v", s1[0], ref[0], ref32[0])
    msd.eval()
    with torch.no_grad():
        s2, _ = msd(x)
        s3, _ = msd(x)
    res.append((all(R.bits_equal(moved[k], v) for k, v in msd.named_buffers()), "eval(): two calls leave the buffers as they were"))
    res.append((R.bits_equal(s2[0], s3[0]), "eval(): two calls give the same bits"))
    ref_e, _ = MR.msd_forward({**{k: v.double() for k, v in sd.items()}, **{k: v.cpu().double() for k, v in moved.items()}}, x.cpu().double(), False)
    ref_e32, _ = MR.msd_forward({**sd, **{k: v.cpu() for k, v in moved.items()}}, x.cpu(), False)
    _held(res, "eval(): scores of scale 0 from the stored u, v", s2[0], ref_e[0], ref_e32[0])
    msd.train()
    xg = x.clone().requires_grad_(True)
    s4, _ = msd(xg)
    # conv_post has one output channel: u = +-1 and v = +-W / |W| from the first iteration on, a fixed point
    res.append((all(R.bits_equal(moved[k], v) == ("conv_post" in k) for k, v in msd.named_buffers()) and s4[0].grad_fn is not None,
                "train(), grad mode: the buffers of the seven wide layers move again, conv_post's stay at their fixed point"))
    return res


def chain_generator():
    """generator (tiny, trainable) -> HifiganDiscriminator -> loss -> backward: dx of both halves flows into HifiganGenerator.trainable()"""
    res = []
    cfg, gsd, _, _, _ = VR.load_fixture()
    msd_sd, dsd = MR.seeded_state_dict(MR.SEED), DR.seeded_state_dict(DR.SEED)
    g = torch.Generator().manual_seed(7)
    mel = torch.randn(2, cfg["in_channels"], 8, generator=g)
    T = 8 * 64
    xr = 0.3 * torch.randn(2, 1, T, generator=g)
    refs = []
    for dt in (F64, F32):
        prm = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in gsd.items()}
        d1, d2 = {k: v.to(dt) for k, v in dsd.items()}, {k: v.to(dt) for k, v in msd_sd.items()}
        y = VR.generator_forward(prm, cfg, mel.to(dt))
        after = {}
        sr, fr = DR.mpd_forward(d1, xr.to(dt))
        sr2, fr2 = MR.msd_forward(d2, xr.to(dt), True, after)
        sg, fg = DR.mpd_forward(d1, y)
        sg2, fg2 = MR.msd_forward({**d2, **after}, y, True)
        grads = torch.autograd.grad(MR.total_loss(sr + sr2, fr + fr2, sg + sg2, fg + fg2), list(prm.values()))
        refs.append((y.detach(), dict(zip(prm.keys(), grads))))
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(gsd)
    gen.to(DEV).trainable()
    disc = HifiganDiscriminator()
    disc.load_state_dict({**{"mpd." + k: v for k, v in dsd.items()}, **{"msd." + k: v for k, v in msd_sd.items()}})
    disc.to(DEV).train()
    y = gen(mel.to(DEV))
    res.append((tuple(y.shape) == (2, 1, T) and y.grad_fn is not None, f"chain: generator output {tuple(y.shape)} with a grad_fn"))
    sr, fr = disc(xr.to(DEV))
    sg, fg = disc(y)
    res.append((len(sg) == 8 and [len(f) for f in fg] == [6] * 5 + [8] * 3, "chain: eight scores, 5 x 6 + 3 x 8 features"))
    MR.total_loss(sr, fr, sg, fg).backward()
    _held(res, "chain: generator output", y, refs[0][0], refs[1][0])
    n = 0
    for k, p in gen.named_parameters():
        _held(res, f"chain: generator grad {k}", p.grad, refs[0][1][k], refs[1][1][k])
        n += 1
    res.append((n == 234, f"chain: {n} generator gradients"))
    return res


def module_refusals():
    """what the module refuses on the device, a single ScaleDiscriminator under no_grad, and frozen parameters"""
    res = []
    for spectral in (False, True):
        d = ScaleDiscriminator(use_spectral_norm=spectral).to(DEV)
        x = torch.randn(2, 1, 100, device=DEV)
        for what, fn, exc in (("bf16 input", lambda: d(x.bfloat16()), NotImplementedError), ("(B, T) input", lambda: d(x[:, 0]), ValueError),
                              ("float64 input", lambda: d(x.double()), TypeError), ("CPU input", lambda: d(x.cpu()), RuntimeError)):
            try:
                fn()
                res.append((False, f"spectral {spectral}, {what}: not refused"))
            except exc as e:
                res.append((True, f"spectral {spectral}, {what}: {type(e).__name__}: {str(e)[:60]}"))
        with torch.no_grad():
            s, f = d(x)
        res.append((s.grad_fn is None and tuple(s.shape) == (2, MR.length_chain(100)[0][-1]) and len(f) == 8, f"spectral {spectral}, no_grad call: plain tensors, the reference's shapes"))
        for prm in d.parameters():
            prm.requires_grad_(False)
        xg = x.clone().requires_grad_(True)
        s, f = d(xg)
        (s.sum() + f[2].abs().sum()).backward()
        res.append((xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and all(prm.grad is None for prm in d.parameters()),
                    f"spectral {spectral}, frozen parameters: dx alone (the weight-gradient launches are skipped)"))
    return res


CASES = [gconv_kernels_exact, wgrad_chunks_exact, input_kernels_exact, pool_kernels_exact, spectral_kernels, case_t331, case_t97, case_zero_utterance,
         buffer_semantics, chain_generator, module_refusals]


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
