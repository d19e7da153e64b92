"""The vocoder fine-tuning step on the MI355X: the GAN-loss kernels (csrc/gan_loss.hip) and MultiAdamW (csrc/adamw_multi.hip) alone, then
VocoderFineTuner.step (seq2seq_vc_amd/urhythmic/fine_tune.py) on the tiny generator of tests/vocoder_ref.py feeding the full
discriminator.  Each case returns [(ok, message)]; tests/test_gpu_finetune.py turns them into pytest tests.

Bounds.  Loss values: 1 fp32 ulp from the float64 restatement (tests/ganloss_ref.py) on the same fp32 inputs -- double sums and one
final rounding give that by construction.  Feature-loss gradients: the bits of stock torch's fp32 autograd on the card, signed zeros
included (where r == g torch's chain gives +0 for `real` and its negation, -0, for `generated`).  Score-loss gradients: 2 fp32 ulp from
the float64 gradient (two roundings allowed: a division and a product).  MultiAdamW: per tensor |got - ref64| <= 4 d + ulp with d the
distance of stock torch.optim.AdamW (fp32, on the card, same inputs) from the float64 restatement.  The step: bit for bit between the
modes and against the loop written out from the public pieces.  Nothing here is fitted to what the kernels return."""
import collections
import copy

import torch

import disc_ref as DR
import ganloss_ref as GR
import msd_ref as MR
import step_kernels_ref as R
import vocoder_ref as VR
from gpu_disc_check import DEV, F32, F64, SENTINEL, SLACK, _Guarded
from seq2seq_vc_amd import _lib
from seq2seq_vc_amd.ops import kernels as K
from seq2seq_vc_amd.ops import kernels_ganloss as KG
from seq2seq_vc_amd.optim import ADAMW_CHUNK, ADAMW_GROUP, MultiAdamW, plan_moments
from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram
from seq2seq_vc_amd.urhythmic.fine_tune import VocoderFineTuner
from seq2seq_vc_amd.urhythmic.vocoder import HifiganDiscriminator, discriminator_loss, feature_loss, generator_loss
from seq2seq_vc_amd.vocoder import HifiganGenerator


def _nan_wrapped(t, shift=0):
    """t (CPU fp32) on the device inside a NaN-filled allocation, in t's own strides; shift: extra floats in front (1: not 16-byte aligned)"""
    big = torch.full((t.numel() + 2 * SLACK + shift,), float("nan"), dtype=F32, device=DEV)
    view = torch.as_strided(big, t.shape, t.stride(), SLACK + shift)
    view.copy_(t)
    return view


def _guard_like(t):
    """a sentinel-surrounded gradient buffer in t's physical layout"""
    g = _Guarded((t.numel(),))
    off = g.view.storage_offset()
    return g, torch.as_strided(g.big, t.shape, t.stride(), off)


def _channel_last(shape, gen):
    """a (B, C, L[, p]) view of dense channel-last storage, as the discriminators return their features"""
    if len(shape) == 4:
        B, C, L, p = shape
        return torch.randn(B, L, p, C, generator=gen).permute(0, 3, 1, 2)
    B, C, L = shape
    return torch.randn(B, L, C, generator=gen).permute(0, 2, 1)


def _feature_pairs():
    """-> [(name, r, g, planted index or None)] CPU fp32: the hand-built pairs"""
    pairs = []
    for n, numel in enumerate(GR.FEATURE_NUMELS):
        r, g, idx = GR.seeded_pair(numel, 900 + n)
        pairs.append((f"numel {numel}", r, g, idx))
    gen = torch.Generator().manual_seed(950)
    for shape in GR.CHANNEL_LAST_SHAPES:
        r, g = _channel_last(shape, gen), _channel_last(shape, gen)
        g[0, 1] = r[0, 1]                                  # a planted run of equal elements
        pairs.append((f"channel-last view {shape}", r, g, None))
    return pairs


def feature_loss_kernels():
    """feature_loss on hand-built pairs: values, gradients for upstream 1 and 2, layouts, NaN around the inputs, sentinels around the gradients"""
    res = []
    cases = _feature_pairs()
    dev = [(_nan_wrapped(r, shift=(1 if i == 2 else 0)), _nan_wrapped(g, shift=(1 if i == 2 else 0))) for i, (_, r, g, _) in enumerate(cases)]
    res.append((all(not a.is_contiguous() and KG.dense_like(a) for a, _ in dev[len(GR.FEATURE_NUMELS):]) and dev[2][0].data_ptr() % 16 != 0,
                "the channel-last pairs are dense, not contiguous; one pair is not 16-byte aligned (the element-wise path)"))
    out = KG.feature_loss_fwd(dev)
    out2 = KG.feature_loss_fwd(dev)
    res.append((R.bits_equal(out, out2), "two calls give the same bits"))
    means64, total64 = GR.feature_loss([(r, g) for _, r, g, _ in cases])
    for i, (name, _, _, _) in enumerate(cases):
        ok, worst = GR.within_ulps(out[i], means64[i], 1)
        res.append((ok, f"{name}: mean within 1 ulp of float64 ({worst:.3f} ulp)"))
    ok, worst = GR.within_ulps(out[len(cases)], total64, 1)
    res.append((ok, f"total of {len(cases)} pairs within 1 ulp of float64 ({worst:.3f} ulp)"))
    # the launcher alone into guarded buffers: nothing outside is written, only the requested side is produced
    up = torch.tensor([2.0], device=DEV)
    guards_a, guards_b = zip(*[_guard_like(a) for a, _ in dev]), zip(*[_guard_like(b) for _, b in dev])
    (ga_guard, ga_buf), (gb_guard, gb_buf) = guards_a, guards_b
    KG.feature_loss_bwd(dev, up, [True] * len(dev), [True] * len(dev), out_a=list(ga_buf), out_b=list(gb_buf))
    res.append((all(g.intact() for g in ga_guard + gb_guard), "backward launch: the sentinels around all gradient buffers are intact"))
    ga, gb = KG.feature_loss_bwd(dev[4:5], up, [False], [True])
    res.append((ga == [None] and gb[0] is not None and R.bits_equal(gb[0], gb_buf[4]), "only the side that needs a gradient is produced, with the same bits"))
    # against stock torch's fp32 autograd on the card, through the public function
    for upstream in (1.0, 2.0):
        ours_r = [a.detach().requires_grad_(True) for a, _ in dev]
        ours_g = [b.detach().requires_grad_(True) for _, b in dev]
        (upstream * feature_loss([ours_r], [ours_g])).backward()
        t_r = [a.detach().clone().requires_grad_(True) for a, _ in dev]
        t_g = [b.detach().clone().requires_grad_(True) for _, b in dev]
        loss = 0
        for rl, gl in zip(t_r, t_g):
            loss = loss + torch.mean(torch.abs(rl - gl))
        (upstream * loss).backward()
        for i, (name, r, g, idx) in enumerate(cases):
            same = R.bits_equal(ours_g[i].grad, t_g[i].grad) and R.bits_equal(ours_r[i].grad, t_r[i].grad)
            res.append((same, f"{name}, upstream {upstream:g}: both gradients have the bits of stock torch's fp32 autograd on the card"))
            if upstream == 2.0:
                res.append((R.bits_equal(ours_g[i].grad, gb_buf[i]) and R.bits_equal(ours_r[i].grad, ga_buf[i]), f"{name}: the autograd node returns what the launch wrote"))
            eq = (r == g)
            gg, gr = ours_g[i].grad.cpu(), ours_r[i].grad.cpu()
            zero_ok = bool((gg[eq] == 0).all()) and bool((gr[eq] == 0).all()) and bool((gg[~eq] != 0).all())
            # torch's chain: sgn(0) * c = +0 for `real`, its negation -0 for `generated`
            signs_ok = bool((~torch.signbit(gr[eq])).all()) and bool(torch.signbit(gg[eq]).all())
            res.append((zero_ok and signs_ok and int(eq.sum()) >= 1, f"{name}, upstream {upstream:g}: {int(eq.sum())} planted equal elements get a zero "
                        "(+0 for real, -0 for generated, as torch's chain), every other element a non-zero"))
        for i in range(len(GR.FEATURE_NUMELS), len(cases)):
            g_ = ours_g[i].grad
            perm = (0, 2, 3, 1) if g_.dim() == 4 else (0, 2, 1)
            res.append((g_.permute(*perm).is_contiguous() and ours_r[i].grad.permute(*perm).is_contiguous(),
                        f"{cases[i][0]}: the gradients are channel-last-strided (the discriminator's backward reads them without a copy)"))
    # a pair that is not dense: one contiguous copy, the same values
    gen = torch.Generator().manual_seed(960)
    big_r, big_g = torch.randn(3, 10, 7, generator=gen), torch.randn(3, 10, 7, generator=gen)
    r_nd, g_nd = big_r.to(DEV)[:, ::2], big_g.to(DEV)[:, ::2]
    res.append((not KG.dense_like(r_nd), "a strided slice is not dense"))
    a = r_nd.detach().requires_grad_(True)
    b = g_nd.detach().requires_grad_(True)
    val = feature_loss([[a]], [[b]])
    val.backward()
    ok, worst = GR.within_ulps(val, GR.feature_loss([(big_r[:, ::2], big_g[:, ::2])])[1], 1)
    a2, b2 = r_nd.detach().clone().requires_grad_(True), g_nd.detach().clone().requires_grad_(True)
    torch.mean(torch.abs(a2 - b2)).backward()
    res.append((ok and R.bits_equal(b.grad, b2.grad) and R.bits_equal(a.grad, a2.grad), f"non-dense pair (the copy path): value within 1 ulp ({worst:.3f}), torch's gradient bits"))
    # mismatched strides inside a pair (one channel-last, one contiguous): the copy path again
    r_cl = _channel_last((2, 8, 5, 3), gen).to(DEV)
    g_cf = torch.randn(2, 8, 5, 3, generator=gen).to(DEV)
    val = feature_loss([[r_cl]], [[g_cf]])
    ok, worst = GR.within_ulps(val, GR.feature_loss([(r_cl.cpu(), g_cf.cpu())])[1], 1)
    res.append((ok, f"a pair of different strides goes through the copy: value within 1 ulp ({worst:.3f})"))
    return res


def _score_tensors():
    gen = torch.Generator().manual_seed(970)
    sizes = ((2, 1), (2, 63), (2, 32), (1, 65), (2, 4095), (2, 4096), (1, GR.CHUNK + 1), (2, 330))
    real = [1.0 + 0.7 * torch.randn(s, generator=gen) for s in sizes]
    fake = [0.7 * torch.randn(s, generator=gen) for s in sizes]
    real[2][0, 3] = 1.0                                    # residual exactly zero
    fake[2][0, 3] = 0.0
    return real, fake


def score_loss_kernels():
    """discriminator_loss and generator_loss: values within 1 ulp, gradients within 2 ulp of float64, the host read of `detail`"""
    res = []
    real, fake = _score_tensors()
    n = len(real)
    real_d = [_nan_wrapped(t, shift=(1 if i == 1 else 0)) for i, t in enumerate(real)]
    fake_d = [_nan_wrapped(t) for t in fake]
    entries64 = [(t, GR.KIND_ONE_MINUS_SQ) for t in real] + [(t, GR.KIND_SQ) for t in fake]
    means64, total64 = GR.score_losses(entries64)
    for upstream in (1.0, 2.0):
        rs = [t.detach().requires_grad_(True) for t in real_d]
        fs = [t.detach().requires_grad_(True) for t in fake_d]
        loss, rl, fl = discriminator_loss(rs, fs)
        ok, worst = GR.within_ulps(loss, total64, 1)
        res.append((ok and loss.is_cuda and loss.dim() == 0, f"discriminator_loss: total within 1 ulp of float64 ({worst:.3f} ulp)"))
        worst = max(GR.within_ulps(torch.tensor(v, dtype=F32), m, 1)[1] for v, m in zip(rl + fl, means64))
        res.append((len(rl) == len(fl) == n and all(isinstance(v, float) for v in rl + fl) and worst <= 1, f"the 2 x {n} per-tensor losses are Python floats within 1 ulp ({worst:.3f})"))
        (upstream * loss).backward()
        grads64 = GR.score_grads(entries64, upstream)
        worst = 0.0
        for t, g64 in zip(rs + fs, grads64):
            ok, w = GR.within_ulps(t.grad, g64, 2)
            worst = max(worst, w)
            res.append((ok, f"discriminator_loss, upstream {upstream:g}: gradient of a {tuple(t.shape)} tensor within 2 ulp of float64 ({w:.3f})"))
    res.append((float(rs[2].grad[0, 3]) == 0.0 and float(fs[2].grad[0, 3]) == 0.0, "a zero residual gets a zero gradient"))
    # into guarded buffers
    up = torch.tensor([1.0], device=DEV)
    ents = [(t, 0) for t in real_d] + [(t, 1) for t in fake_d]
    guards, bufs = zip(*[_guard_like(t) for t, _ in ents])
    KG.score_loss_bwd(ents, up, [True] * len(ents), out=list(bufs))
    res.append((all(g.intact() for g in guards), "backward launch: the sentinels around all gradient buffers are intact"))
    # the forward launcher alone: the bits the public function returns; the library's chunk and table size are the host model's
    raw = KG.score_loss_fwd(ents)
    res.append((R.bits_equal(raw[len(ents)], loss) and R.bits_equal(raw[:len(ents)].cpu(), torch.tensor(rl + fl, dtype=F32)), "score_loss_fwd alone returns the same 16 means and total"))
    res.append((_lib.lib().s2svc_gan_loss_chunk() == GR.CHUNK == KG.CHUNK and _lib.lib().s2svc_gan_loss_max() == KG.MAX_ENTRIES,
                f"the library cuts chunks of {GR.CHUNK} elements and takes {KG.MAX_ENTRIES} entries per call, as the host tables assume"))
    # detail=False: empty lists, a device tensor, no host read
    loss2, a, b = discriminator_loss(real_d, fake_d, detail=False)
    res.append((a == [] and b == [] and loss2.is_cuda and R.bits_equal(loss2, loss), "detail=False: empty lists and the same loss on the device"))
    # generator_loss
    xs = [t.detach().requires_grad_(True) for t in fake_d]
    gl, parts = generator_loss(xs)
    m64, t64 = GR.score_losses([(t, GR.KIND_ONE_MINUS_SQ) for t in fake])
    ok, worst = GR.within_ulps(gl, t64, 1)
    parts_ok = len(parts) == n and all(p.dim() == 0 and p.is_cuda for p in parts) and len({p.untyped_storage().data_ptr() for p in parts}) == 1
    worst_p = max(GR.within_ulps(p, m, 1)[1] for p, m in zip(parts, m64))
    res.append((ok and parts_ok and worst_p <= 1, f"generator_loss: total within 1 ulp ({worst:.3f}), eight 0-dim views of one device vector within 1 ulp ({worst_p:.3f})"))
    (2.0 * gl).backward()
    for t, g64 in zip(xs, GR.score_grads([(q, 0) for q in fake], 2.0)):
        ok, w = GR.within_ulps(t.grad, g64, 2)
        res.append((ok, f"generator_loss, upstream 2: gradient of a {tuple(t.shape)} tensor within 2 ulp of float64 ({w:.3f})"))
    res.append((type(gl.grad_fn).__name__.startswith("_ScoreLossFunction"), "one autograd node"))
    return res


def multi_adamw_steps():
    """3 steps over tensors of 1, 3, 4, 5, 1023 and 70 001 elements: 4 d + ulp against float64 with stock torch's fp32 AdamW as the yardstick"""
    res, ratios = [], []
    params, grads = GR.adamw_case()
    kw = dict(lr=GR.ADAMW_LRS[0], **GR.ADAMW_HYPER)
    ref_p, ref_m, ref_v, ref_steps = GR.adamw(params, grads, GR.ADAMW_LRS, **GR.ADAMW_HYPER)
    topt, tps = GR.run_optimizer(lambda q: torch.optim.AdamW(q, **kw), params, grads, GR.ADAMW_LRS, device=DEV)
    made = {}

    def make(ps):
        opt = MultiAdamW(ps, **kw)
        gap = torch.ones(opt.numel, dtype=torch.bool)
        for o, p in zip(opt.offsets, ps):
            gap[o:o + p.numel()] = False
        made["gap"] = gap.to(DEV)
        opt.exp_avg[made["gap"]] = SENTINEL
        opt.exp_avg_sq[made["gap"]] = SENTINEL
        return opt
    opt, ps = GR.run_optimizer(make, params, grads, GR.ADAMW_LRS, device=DEV)
    res.append((int(made["gap"].sum()) == opt.numel - sum(GR.ADAMW_SIZES) > 0 and bool((opt.exp_avg[made["gap"]] == SENTINEL).all())
                and bool((opt.exp_avg_sq[made["gap"]] == SENTINEL).all()), f"the {int(made['gap'].sum())} sentinels between the chunks of the flat moment buffers are untouched"))
    for i, n in enumerate(GR.ADAMW_SIZES):
        st, tst = opt.state[ps[i]], topt.state[tps[i]]
        res.append((int(st["step"]) == ref_steps[i] == int(tst["step"]), f"tensor of {n}: step count {int(st['step'])} (a None gradient does not advance it)"))
        for what, got, ref, yard in (("parameter", ps[i], ref_p[i], tps[i]), ("exp_avg", st["exp_avg"], ref_m[i], tst["exp_avg"]),
                                     ("exp_avg_sq", st["exp_avg_sq"], ref_v[i], tst["exp_avg_sq"])):
            ok, ratio, d, msg = R.compare(got.detach().cpu(), ref, yard.detach().cpu(), F32)
            ratios.append(ratio)
            res.append((ok, f"tensor of {n}, {what}: {msg}"))
    fin = [r for r in ratios if r != float("inf")]
    res.append((True, f"ratios max|got - ref64| / d over {len(ratios)} tensors: largest {max(fin):.3f}, median {sorted(fin)[len(fin) // 2]:.3f}"))
    # load_state_dict(torch's) + one step == continuing
    extra = [0.1 * torch.randn(n, generator=torch.Generator().manual_seed(77 + n)) for n in GR.ADAMW_SIZES]
    fresh_ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    fresh = MultiAdamW(fresh_ps, **kw)
    fresh.load_state_dict(copy.deepcopy(topt.state_dict()))
    ours_sd = copy.deepcopy(opt.state_dict())
    cont_ps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    cont = MultiAdamW(cont_ps, **kw)
    cont.load_state_dict(ours_sd)
    for group in (opt, cont, fresh):
        group.param_groups[0]["lr"] = GR.ADAMW_LRS[-1]
    for plist, o in ((ps, opt), (cont_ps, cont), (fresh_ps, fresh)):
        for p, g in zip(plist, extra):
            p.grad = g.to(DEV)
        o.step()
    same = all(R.bits_equal(a, b) for a, b in zip(ps, cont_ps)) and R.bits_equal(opt.exp_avg[~made["gap"]], cont.exp_avg[~made["gap"]]) \
        and R.bits_equal(opt.exp_avg_sq[~made["gap"]], cont.exp_avg_sq[~made["gap"]])
    res.append((same, "state_dict() -> a fresh MultiAdamW -> one step has the bits of continuing"))
    # from torch's state: the moments differ in the last bits from ours, so the fourth step is compared under the same rule
    g4 = [row for row in grads] + [extra]
    lrs4 = GR.ADAMW_LRS + (GR.ADAMW_LRS[-1],)
    ref4 = GR.adamw(params, g4, lrs4, **GR.ADAMW_HYPER)
    for p, g in zip(tps, extra):
        p.grad = g.to(DEV)
    topt.param_groups[0]["lr"] = GR.ADAMW_LRS[-1]
    topt.step()
    ok_all = True
    for i, n in enumerate(GR.ADAMW_SIZES):
        ok, ratio, d, msg = R.compare(fresh_ps[i].detach().cpu(), ref4[0][i], tps[i].detach().cpu(), F32)
        ok_all = ok_all and ok and int(fresh.state[fresh_ps[i]]["step"]) == ref4[3][i]
    res.append((ok_all, "load_state_dict(torch.optim.AdamW's state) followed by one step: parameters within 4 d + ulp of four float64 steps, step counts continued"))
    res.append((opt.launches_per_step() == 1, "six tensors: one launch per step"))
    # the launcher alone, step 1 of the case: the bits MultiAdamW's own first step leaves
    first, fps = GR.run_optimizer(lambda q: MultiAdamW(q, **kw), params, grads[:1], GR.ADAMW_LRS[:1], device=DEV)
    offsets, total = plan_moments(GR.ADAMW_SIZES)
    m, v = torch.zeros(total, device=DEV), torch.zeros(total, device=DEV)
    lone = [t.to(DEV).clone() for t in params]
    b1, b2 = GR.ADAMW_HYPER["betas"]
    lr = GR.ADAMW_LRS[0]
    K.adamw_multi([(p, g.to(DEV), o, lr / (1.0 - b1), (1.0 - b2) ** 0.5) for p, g, o in zip(lone, grads[0], offsets)], m, v,
                  1.0 - lr * GR.ADAMW_HYPER["weight_decay"], b1, b2, GR.ADAMW_HYPER["eps"])
    res.append((all(R.bits_equal(a, b) for a, b in zip(lone, fps)) and R.bits_equal(m, first.exp_avg) and R.bits_equal(v, first.exp_avg_sq),
                "adamw_multi alone (step 1): the parameters and both flat moment buffers have the bits of MultiAdamW's first step"))
    res.append((_lib.lib().s2svc_adamw_multi_group() == ADAMW_GROUP and _lib.lib().s2svc_adamw_multi_chunk() == ADAMW_CHUNK,
                f"the library takes {ADAMW_GROUP} tensors per launch in chunks of {ADAMW_CHUNK} elements, as the host tables assume"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------------
_SHARED = {}
FRAMES, B = 15, 2


def _nets():
    """fresh copies of the seeded tiny generator and the seeded full discriminator on the device"""
    if "gen" not in _SHARED:
        cfg, gsd, _, _, _ = VR.load_fixture()
        gen = HifiganGenerator(**cfg)
        gen.load_state_dict(gsd)
        disc = HifiganDiscriminator()
        disc.load_state_dict({**{"mpd." + k: v for k, v in DR.seeded_state_dict(DR.SEED).items()},
                              **{"msd." + k: v for k, v in MR.seeded_state_dict(MR.SEED).items()}})
        _SHARED["cfg"], _SHARED["gen"], _SHARED["disc"] = cfg, gen.to(DEV), disc.to(DEV)
        _SHARED["mel"] = LogMelSpectrogram().to(DEV)
        g = torch.Generator().manual_seed(21)
        T = FRAMES * 64
        batches = []
        for _ in range(3):
            wavs = 0.3 * torch.randn(B, 1, T, generator=g)
            units = torch.randn(B, cfg["in_channels"], FRAMES, generator=g)
            tgts = torch.randn(_SHARED["mel"].output_shape((B, 1, T)), generator=g)
            batches.append((wavs.to(DEV), units.to(DEV), tgts.to(DEV)))
        _SHARED["batches"] = batches
    return copy.deepcopy(_SHARED["gen"]), copy.deepcopy(_SHARED["disc"])


def _tuner(mode):
    gen, disc = _nets()
    return VocoderFineTuner(gen, disc, _SHARED["mel"], mode=mode)


def _snapshot(tuner):
    """everything the two modes must agree on, as {name: tensor}"""
    snap = {}
    for tag, model, opt in (("G", tuner.generator, tuner.optimizer_generator), ("D", tuner.discriminator, tuner.optimizer_discriminator)):
        for k, v in model.state_dict().items():           # parameters and the weight_u / weight_v buffers
            snap[f"{tag}.{k}"] = v.detach().clone()
        for (k, p) in model.named_parameters():
            st = opt.state[p]
            snap[f"{tag}.opt.{k}.exp_avg"], snap[f"{tag}.opt.{k}.exp_avg_sq"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
            snap[f"{tag}.opt.{k}.step"] = st["step"].clone()
    return snap


def _same(a, b):
    bad = [k for k in a if k not in b or not R.bits_equal(a[k], b[k])]
    return (not bad and a.keys() == b.keys()), bad


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


def _two_steps(mode):
    if ("run", mode) not in _SHARED:
        tuner = _tuner(mode)
        losses = [tuner.step(*_SHARED["batches"][0])]
        names = _recorded(lambda: losses.append(tuner.step(*_SHARED["batches"][1])))
        dgrad = {k: (None if p.grad is None else p.grad.clone()) for k, p in tuner.discriminator.named_parameters()}
        _SHARED["run", mode] = (tuner, losses, names, _snapshot(tuner), dgrad)
    return _SHARED["run", mode]


def lean_equals_reference():
    """two steps in each mode from the same seeded state: the same bits everywhere but in the discriminator's .grad; the launch plans"""
    res = []
    lean, l_loss, l_names, l_snap, l_grad = _two_steps("lean")
    ref, r_loss, r_names, r_snap, r_grad = _two_steps("reference")
    ok, bad = _same(l_snap, r_snap)
    n_buf = sum(1 for k in l_snap if k.endswith(("weight_u", "weight_v")) and ".opt." not in k and "msd.discriminators.0" in k)
    res.append((ok and n_buf == 16, f"{len(l_snap)} tensors (parameters, {n_buf} weight_u / weight_v buffers, exp_avg, exp_avg_sq, step of both optimisers) are "
                f"bit-equal after two steps{'' if ok else ': differ ' + ', '.join(bad[:4])}"))
    same_losses = all(R.bits_equal(a[k], b[k]) for a, b in zip(l_loss, r_loss) for k in ("loss_mel", "loss_discriminator", "loss_generator"))
    shapes = all(v.dim() == 0 and v.is_cuda and not v.requires_grad for d in l_loss for v in d.values()) and set(l_loss[0]) == {"loss_mel", "loss_discriminator", "loss_generator"}
    res.append((same_losses and shapes, "the six losses are bit-equal 0-dim device tensors: " + ", ".join(f"{k} {float(v):.6f}" for k, v in l_loss[1].items())))
    finite = all(bool(torch.isfinite(v).all()) for v in l_snap.values())
    moved = not R.bits_equal(l_snap["G.conv_pre.weight_v"], _SHARED["gen"].state_dict()["conv_pre.weight_v"]) and \
        not R.bits_equal(l_snap["D.mpd.discriminators.0.convs.1.weight_v"], _SHARED["disc"].state_dict()["mpd.discriminators.0.convs.1.weight_v"])
    res.append((finite and moved, "everything is finite and both nets moved"))
    differ = sum(1 for k in l_grad if not R.bits_equal(l_grad[k], r_grad[k]))
    res.append((differ > 0 and all(v is not None for v in l_grad.values()), f"the one observable difference: {differ} of {len(l_grad)} discriminator .grad tensors (reference mode "
                "leaves the sums its next zero_grad() discards)"))
    # plans
    lp, rp = lean.launch_plan(), ref.launch_plan()
    D = lean.discriminator
    saved = [e for e in rp if e["stage"] == "generator half: backward of D(wavs)"]
    gen_ref = [e for e in rp if e["stage"] == "generator half: backward of D(wavs_)"]
    gen_lean = [e for e in lp if e["stage"] == "generator half: backward of D(wavs_)"]
    res.append((len(lp) < len(rp) and len(rp) - len(lp) == len(saved) + len(gen_ref) - len(gen_lean) and len(saved) > 0,
                f"launch_plan(): {len(lp)} launches lean, {len(rp)} reference: {len(rp) - len(lp)} fewer, the parameter-gradient work of the generator half's two "
                f"discriminator backward passes ({len(gen_ref)} -> {len(gen_lean)} for D(wavs_), {len(saved)} -> 0 for D(wavs))"))
    res.append((len(D.backward_plan(True, False)) < len(D.backward_plan(True, True)), f"backward_plan entries: {len(D.backward_plan(True, False))} with need_params=False, "
                f"{len(D.backward_plan(True, True))} with"))
    for mode, plan, names in (("lean", lp, l_names), ("reference", rp, r_names)):
        want, got = collections.Counter(e["call"] for e in plan), collections.Counter(names)
        diff = {k: (want.get(k, 0), got.get(k, 0)) for k in set(want) | set(got) if want.get(k, 0) != got.get(k, 0)}
        res.append((len(names) == len(plan) and not diff, f"{mode}: {len(names)} counted library launches in a step, {len(plan)} in the plan{'' if not diff else ' -- (plan, counted) ' + str(diff)}"))
        res.append(([e["call"] for e in plan] == names, f"{mode}: the counted calls come in the plan's order"))
    return res


def _written_out_step(G, D, mel, opt_g, opt_d, wavs, units, tgts, record=None):
    """the reference's loop body from the public pieces"""
    opt_d.zero_grad()
    wavs_ = G(units)
    scores, _ = D(wavs)
    scores_, _ = D(wavs_.detach())
    loss_discriminator, _, _ = discriminator_loss(scores, scores_, detail=False)
    if record is not None:
        record["scores"] = ([s.detach().clone() for s in scores], [s.detach().clone() for s in scores_])
    loss_discriminator.backward()
    opt_d.step()
    opt_g.zero_grad()
    scores, features = D(wavs)
    scores_, features_ = D(wavs_)
    loss_mel, _ = mel.l1_loss(wavs_, tgts)
    loss_features = feature_loss(features, features_)
    loss_adv, _ = generator_loss(scores_)
    if record is not None:
        record["gen"] = ([s.detach().clone() for s in scores_], [[f.detach().clone() for f in fl] for fl in features], [[f.detach().clone() for f in fl] for fl in features_])
        record["ours"] = (loss_discriminator.detach(), loss_adv.detach(), loss_features.detach())
    loss_generator = 45 * loss_mel + 2 * loss_features + loss_adv
    loss_generator.backward()
    opt_g.step()
    return {"loss_mel": loss_mel.detach(), "loss_discriminator": loss_discriminator.detach(), "loss_generator": loss_generator.detach()}


def step_adds_nothing():
    """reference mode equals the loop written out from the public pieces, bit for bit after two steps; step 1's losses against stock torch"""
    res = []
    ref, r_loss, _, r_snap, r_grad = _two_steps("reference")
    gen, disc = _nets()
    gen.trainable().train()
    disc.train()
    kw = dict(lr=5e-5, betas=(0.8, 0.99), weight_decay=1e-2)
    opt_g, opt_d = MultiAdamW(gen.parameters(), **kw), MultiAdamW(disc.parameters(), **kw)
    rec = {}
    losses = [_written_out_step(gen, disc, _SHARED["mel"], opt_g, opt_d, *_SHARED["batches"][0], record=rec),
              _written_out_step(gen, disc, _SHARED["mel"], opt_g, opt_d, *_SHARED["batches"][1])]

    class _Loop:
        generator, discriminator, optimizer_generator, optimizer_discriminator = gen, disc, opt_g, opt_d
    ok, bad = _same(_snapshot(_Loop), r_snap)
    res.append((ok, f"{len(r_snap)} tensors bit-equal to the written-out loop after two steps{'' if ok else ': differ ' + ', '.join(bad[:4])}"))
    res.append((all(R.bits_equal(a[k], b[k]) for a, b in zip(losses, r_loss) for k in a), "the six losses are bit-equal"))
    res.append((all(R.bits_equal(p.grad, r_grad[k]) for k, p in disc.named_parameters()), "and so is what reference mode leaves in the discriminator's .grad"))
    # step 1's loss terms against stock torch on the same scores and features: 4 d + ulp, d = stock torch fp32 - float64
    (scores, scores_), (gscores, feats, feats_), (ours_d, ours_adv, ours_f) = rec["scores"], rec["gen"], rec["ours"]
    t_d = sum(torch.mean((1 - r) ** 2) + torch.mean(g ** 2) for r, g in zip(scores, scores_))
    t_adv = sum(torch.mean((1 - x) ** 2) for x in gscores)
    t_f = 0
    pairs = [(a, b) for fa, fb in zip(feats, feats_) for a, b in zip(fa, fb)]
    for a, b in pairs:
        t_f = t_f + torch.mean(torch.abs(a - b))
    ref_d = GR.score_losses([(s.cpu(), 0) for s in scores] + [(s.cpu(), 1) for s in scores_])[1]
    ref_adv = GR.score_losses([(s.cpu(), 0) for s in gscores])[1]
    ref_f = GR.feature_loss([(a.cpu(), b.cpu()) for a, b in pairs])[1]
    res.append((len(pairs) == 54 and len(scores) == 8, "8 scores, 54 feature pairs"))
    for name, got, ref64, yard in (("loss_discriminator", ours_d, ref_d, t_d), ("adversarial term", ours_adv, ref_adv, t_adv), ("feature term", ours_f, ref_f, t_f)):
        ok, ratio, d, msg = R.compare(got.cpu().reshape(1), ref64.reshape(1), yard.detach().cpu().reshape(1), F32)
        res.append((ok, f"step 1 {name} {float(got):.6f} (stock torch {float(yard):.6f}): {msg}"))
    return res


def checkpoint_roundtrip():
    """checkpoint() -> a fresh tuner's load_checkpoint -> one more step equals continuing; finetune=True loads the models alone"""
    res = []
    a = _tuner("lean")
    a.step(*_SHARED["batches"][0])
    a.end_epoch()
    state = a.checkpoint(1, 0.5)
    b = _tuner("lean")
    got = b.load_checkpoint(state, finetune=False)
    res.append((got == (1, 0.5) and b.optimizer_generator.param_groups[0]["lr"] == a.optimizer_generator.param_groups[0]["lr"] != 5e-5, f"load_checkpoint -> {got}, the decayed rate restored"))
    la, lb = a.step(*_SHARED["batches"][1]), b.step(*_SHARED["batches"][1])
    ok, bad = _same(_snapshot(a), _snapshot(b))
    res.append((ok and all(R.bits_equal(la[k], lb[k]) for k in la), f"one more step after the round trip has the bits of continuing{'' if ok else ': differ ' + ', '.join(bad[:4])}"))
    c = _tuner("lean")
    got = c.load_checkpoint(state, finetune=True)
    models = all(R.bits_equal(v, state["generator"]["model"][k]) for k, v in c.generator.state_dict().items()) and \
        all(R.bits_equal(v, state["discriminator"]["model"][k]) for k, v in c.discriminator.state_dict().items())
    fresh = not c.optimizer_generator.state and not c.optimizer_discriminator.state and float(c.optimizer_generator.exp_avg.abs().max()) == 0.0 \
        and float(c.optimizer_discriminator.exp_avg_sq.abs().max()) == 0.0 and c.optimizer_generator.param_groups[0]["lr"] == 5e-5
    res.append((got == (0, float("inf")) and models and fresh, f"finetune=True -> {got}: the two models loaded, optimiser states at zero, the rate at its start"))
    v = c.validate(*_SHARED["batches"][2])
    wavs, units, tgts = _SHARED["batches"][2]
    with torch.no_grad():
        mels_ = _SHARED["mel"](c.generator(units))
        want = torch.nn.functional.l1_loss(mels_.cpu().double(), tgts.cpu().double())
    ok, worst = GR.within_ulps(v, want, 1)
    res.append((ok and v.dim() == 0 and v.is_cuda and not v.requires_grad, f"validate(): the no_grad mel loss {float(v):.6f} within 1 ulp of float64 ({worst:.3f})"))
    return res


def refusals():
    """what the tuner and the loss functions refuse on the device"""
    res = []
    gen, disc = _nets()
    wavs, units, tgts = _SHARED["batches"][0]

    def refused(what, fn, exc):
        try:
            fn()
            res.append((False, f"{what}: not refused"))
        except exc as e:
            res.append((True, f"{what}: {type(e).__name__}: {str(e)[:70]}"))
    refused("a stock torch.nn.Module as generator", lambda: VocoderFineTuner(torch.nn.Conv1d(80, 1, 3).to(DEV), disc), TypeError)
    refused("a stock torch.nn.Module as discriminator", lambda: VocoderFineTuner(gen, torch.nn.Conv1d(1, 1, 3).to(DEV)), TypeError)
    tuner = VocoderFineTuner(gen, disc, _SHARED["mel"])
    before = _snapshot_models(tuner)
    refused("CPU wavs", lambda: tuner.step(wavs.cpu(), units, tgts), RuntimeError)
    refused("CPU units", lambda: tuner.step(wavs, units.cpu(), tgts), RuntimeError)
    refused("bf16 wavs", lambda: tuner.step(wavs.bfloat16(), units, tgts), NotImplementedError)
    refused("bf16 units", lambda: tuner.step(wavs, units.bfloat16(), tgts), NotImplementedError)
    refused("bf16 tgts", lambda: tuner.step(wavs, units, tgts.bfloat16()), NotImplementedError)
    s = [torch.randn(2, 5, device=DEV)]
    refused("bf16 scores", lambda: generator_loss([s[0].bfloat16()]), NotImplementedError)
    refused("CPU features", lambda: feature_loss([[s[0].cpu()]], [[s[0].cpu()]]), RuntimeError)
    refused("float64 scores", lambda: discriminator_loss([s[0].double()], [s[0].double()]), TypeError)
    refused("a pair of different shapes", lambda: feature_loss([[s[0]]], [[s[0][:, :3]]]), ValueError)
    ok, bad = _same(before, _snapshot_models(tuner))
    res.append((ok and all(p.requires_grad for p in disc.parameters()), "a refused step leaves both nets as they were, the discriminator's parameters requiring grad"))
    # an exception inside the frozen region restores requires_grad
    try:
        with tuner._frozen_discriminator():
            frozen = not any(p.requires_grad for p in disc.parameters())
            raise KeyError("inside")
    except KeyError:
        pass
    res.append((frozen and all(p.requires_grad for p in disc.parameters()), "the discriminator's parameters require grad again after an exception in the frozen call"))
    return res


def _snapshot_models(tuner):
    return {**{"G." + k: v.detach().clone() for k, v in tuner.generator.state_dict().items()},
            **{"D." + k: v.detach().clone() for k, v in tuner.discriminator.state_dict().items()}}


CASES = [feature_loss_kernels, score_loss_kernels, multi_adamw_steps, lean_equals_reference, step_adds_nothing, checkpoint_roundtrip, refusals]


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
