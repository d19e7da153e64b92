"""Host tests of the vocoder fine-tuning pieces: the float64 restatements of tests/ganloss_ref.py pinned to stock torch, the two host
index models (each with one planted error that its checker must catch), the state-dict layout of MultiAdamW, the checkpoint layout of
VocoderFineTuner and the new entry points in the built library.  No GPU."""
import copy

import pytest
import torch

import abi_header
import ganloss_ref as GR
import vocoder_ref as VR
from seq2seq_vc_amd import _lib
from seq2seq_vc_amd.ops import kernels_ganloss as KG
from seq2seq_vc_amd.optim import ADAMW_CHUNK, ADAMW_GROUP, MultiAdamW, adamw_table, plan_moments
from seq2seq_vc_amd.urhythmic.fine_tune import VocoderFineTuner
from seq2seq_vc_amd.urhythmic.vocoder import HifiganDiscriminator, discriminator_loss, feature_loss, generator_loss
from seq2seq_vc_amd.vocoder import HifiganGenerator

F64 = torch.float64


def test_loss_restatements_are_stock_torch():
    g = torch.Generator().manual_seed(0)
    feats_r = [[torch.randn(2, 4, 9, generator=g, dtype=F64) for _ in range(3)] for _ in range(2)]
    feats_g = [[torch.randn(2, 4, 9, generator=g, dtype=F64) for _ in range(3)] for _ in range(2)]
    loss = 0
    for r, q in zip(feats_r, feats_g):                    # the reference's loops
        for rl, gl in zip(r, q):
            loss += torch.mean(torch.abs(rl - gl))
    means, total = GR.feature_loss([(a, b) for fa, fb in zip(feats_r, feats_g) for a, b in zip(fa, fb)])
    assert len(means) == 6 and torch.equal(total, loss)
    real, gen = [torch.randn(2, 7, generator=g, dtype=F64) for _ in range(8)], [torch.randn(2, 7, generator=g, dtype=F64) for _ in range(8)]
    d = sum(torch.mean((1 - r) ** 2) + torch.mean(q ** 2) for r, q in zip(real, gen))
    means, total = GR.score_losses([(r, 0) for r in real] + [(q, 1) for q in gen])
    assert torch.allclose(total, d, rtol=1e-14, atol=0) and torch.equal(means[8], torch.mean(gen[0] ** 2))
    adv = sum(torch.mean((1 - q) ** 2) for q in gen)
    assert torch.equal(GR.score_losses([(q, 0) for q in gen])[1], adv)
    # the gradients against autograd
    xs = [q.clone().requires_grad_(True) for q in gen]
    (3.0 * GR.score_losses([(x, i % 2) for i, x in enumerate(xs)])[1]).backward()
    for x, want in zip(xs, GR.score_grads([(q, i % 2) for i, q in enumerate(gen)], 3.0)):
        assert torch.allclose(x.grad, want, rtol=1e-14, atol=0)


def test_adamw_restatement_is_torch_adamw_in_float64():
    params, grads = GR.adamw_case()
    assert any(g is None for row in grads for g in row) and len(set(GR.ADAMW_LRS)) > 1
    assert all(bool((g == 0).any()) for g in grads[0] if g.numel() >= 4)
    opt, ps = GR.run_optimizer(lambda q: torch.optim.AdamW(q, lr=GR.ADAMW_LRS[0], **GR.ADAMW_HYPER), params, grads, GR.ADAMW_LRS, dtype=F64)
    p, m, v, steps = GR.adamw(params, grads, GR.ADAMW_LRS, **GR.ADAMW_HYPER)
    for i, q in enumerate(ps):
        st = opt.state[q]
        assert int(st["step"]) == steps[i] == (2 if i == GR.ADAMW_NONE[1] else 3)
        assert torch.allclose(q.detach(), p[i], rtol=1e-12, atol=1e-16)
        assert torch.allclose(st["exp_avg"], m[i], rtol=1e-12, atol=1e-16) and torch.allclose(st["exp_avg_sq"], v[i], rtol=1e-12, atol=1e-16)


NUMELS = (1, 63, 64, 65, 17, 33, 16, 15, 100)


def test_prefix_table_and_one_planted_error():
    chunk = 16
    prefix = KG.chunk_prefix(NUMELS, chunk)
    assert prefix[-1] == sum(-(-n // chunk) for n in NUMELS)
    assert GR.check_prefix_table(NUMELS, prefix, chunk, KG.locate, KG.chunk_range) == []
    assert KG.locate(prefix, 0) == (0, 0) and KG.locate(prefix, prefix[-1] - 1) == (len(NUMELS) - 1, -(-NUMELS[-1] // chunk) - 1)
    # the real chunk, one chunk +- 1
    real = (GR.CHUNK - 1, GR.CHUNK, GR.CHUNK + 1)
    assert KG.CHUNK == GR.CHUNK == _lib.lib().s2svc_gan_loss_chunk() and KG.chunk_prefix(real) == [0, 1, 2, 4]
    # planted: an off-by-one chunk boundary (the chunk ends one element early)
    off_by_one = lambda numel, c, ch: (c * ch, min(numel, (c + 1) * ch - 1))           # noqa: E731
    bad = GR.check_prefix_table(NUMELS, prefix, chunk, KG.locate, off_by_one)
    assert bad and "not walked exactly once" in bad[0]
    # and a prefix table that gives an entry one workgroup too few
    short = list(prefix)
    for i in range(3, len(short)):
        short[i] -= 1
    assert GR.check_prefix_table(NUMELS, short, chunk, KG.locate, KG.chunk_range)
    with pytest.raises(ValueError):
        KG.locate(prefix, prefix[-1])
    with pytest.raises(ValueError):
        KG.chunk_prefix([4, 0])


def test_adamw_table_and_one_planted_error():
    numels = GR.ADAMW_SIZES
    offsets, total = plan_moments(numels)
    assert offsets == [0, 4, 8, 12, 20, 1044] and total == 71048
    assert ADAMW_CHUNK == _lib.lib().s2svc_adamw_multi_chunk() and ADAMW_GROUP == _lib.lib().s2svc_adamw_multi_group()
    prefix, work = adamw_table(numels, offsets)
    assert prefix == [0, 1, 2, 3, 4, 5, 5 + -(-70001 // ADAMW_CHUNK)]
    assert GR.check_adamw_table(numels, offsets, total, prefix, work) == []
    assert [w[3:] for w in work[:5]] == [(0, 1), (0, 3), (4, 0), (4, 1), (1020, 3)] and work[-1][3:] == (70001 % ADAMW_CHUNK // 4 * 4, 1)
    # planted: the tail of a tensor is rounded up to a whole vector, which reaches into the gap / the neighbour tensor
    padded = [(i, lo, hi, nvec + (4 if ntail else 0), 0) for i, lo, hi, nvec, ntail in work]
    bad = GR.check_adamw_table(numels, offsets, total, prefix, padded)
    assert bad and ("belongs to" in " ".join(bad) or "elements for" in " ".join(bad))
    # planted: chunks packed without the alignment gap, the tail assigned to the neighbour's first vector
    packed = [sum(numels[:i]) for i in range(len(numels))]
    assert any("not 16-byte aligned" in b for b in GR.check_adamw_table(numels, packed, sum(numels), *adamw_table(numels, packed)))


def test_multiadamw_state_dict_layout_is_torch_adamws():
    shapes = [(3, 2, 5), (7,), (1, 1, 1), (4, 4)]
    ps = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    kw = dict(lr=5e-5, betas=(0.8, 0.99), eps=1e-8, weight_decay=1e-2)
    ours, theirs = MultiAdamW(ps, **kw), torch.optim.AdamW(ps, **kw)
    a, b = ours.state_dict(), theirs.state_dict()
    assert a.keys() == b.keys() and a["state"] == b["state"] == {}
    assert len(a["param_groups"]) == 1 and a["param_groups"][0].keys() == b["param_groups"][0].keys() and a["param_groups"] == b["param_groups"]
    assert isinstance(ours, torch.optim.Optimizer)
    sched = torch.optim.lr_scheduler.ExponentialLR(ours, gamma=0.5)
    sched.step()
    assert ours.param_groups[0]["lr"] == pytest.approx(2.5e-5)
    # a stepped torch AdamW loads: keys, shapes, and the flat buffers are written, not rebound
    for p in ps[:3]:
        p.grad = torch.randn_like(p)
    theirs.step()
    flat_m, flat_v = ours.exp_avg, ours.exp_avg_sq
    ours.load_state_dict(theirs.state_dict())
    assert ours.exp_avg is flat_m and ours.exp_avg_sq is flat_v
    a, b = ours.state_dict(), theirs.state_dict()
    assert sorted(a["state"]) == sorted(b["state"]) == [0, 1, 2]
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for k in ("exp_avg", "exp_avg_sq"):
            assert a["state"][i][k].shape == b["state"][i][k].shape == ps[i].shape and torch.equal(a["state"][i][k], b["state"][i][k])
        assert float(a["state"][i]["step"]) == float(b["state"][i]["step"]) == 1.0
    o = ours.offsets[1]
    assert ours.state[ps[1]]["exp_avg"].data_ptr() == flat_m[o:].data_ptr() and torch.equal(flat_m[o:o + 7], theirs.state[ps[1]]["exp_avg"])
    # and ours loads into torch.optim.AdamW
    again = torch.optim.AdamW(ps, **kw)
    again.load_state_dict(copy.deepcopy(ours.state_dict()))
    assert torch.equal(again.state[ps[0]]["exp_avg_sq"], theirs.state[ps[0]]["exp_avg_sq"])
    with pytest.raises(RuntimeError):
        ours.step()                                       # no CPU path
    with pytest.raises(TypeError):
        MultiAdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))])


def test_launches_per_step_of_the_two_nets():
    gen, disc = HifiganGenerator(), HifiganDiscriminator()
    assert len(list(gen.parameters())) == 234 and len(list(disc.parameters())) == 154
    assert MultiAdamW(gen.parameters()).launches_per_step() == 3 and MultiAdamW(disc.parameters()).launches_per_step() == 2


def _tuner(mode="lean"):
    return VocoderFineTuner(HifiganGenerator(**VR.TINY_CFG), HifiganDiscriminator(), mode=mode)


def test_fine_tuner_checkpoint_layout_and_plan():
    tuner = _tuner()
    state = tuner.checkpoint(7, 0.25)
    assert set(state) == {"generator", "discriminator", "step", "loss"} and state["step"] == 7 and state["loss"] == 0.25
    for name, model in (("generator", tuner.generator), ("discriminator", tuner.discriminator)):
        assert set(state[name]) == {"model", "optimizer", "scheduler"}
        assert state[name]["model"].keys() == model.state_dict().keys()
        assert set(state[name]["optimizer"]) == {"state", "param_groups"}
        assert state[name]["scheduler"]["gamma"] == 0.999 and state[name]["scheduler"]["last_epoch"] == 0
    g = state["generator"]["optimizer"]["param_groups"][0]
    assert g["lr"] == 5e-5 and tuple(g["betas"]) == (0.8, 0.99) and g["weight_decay"] == 1e-2
    k = next(iter(state["generator"]["model"]))
    assert state["generator"]["model"][k].data_ptr() != tuner.generator.state_dict()[k].data_ptr()      # copies
    fresh = _tuner()
    assert fresh.load_checkpoint(state) == (7, 0.25)
    assert fresh.load_checkpoint(state, finetune=True) == (0, float("inf"))
    assert all(torch.equal(a, b) for a, b in zip(fresh.generator.state_dict().values(), tuner.generator.state_dict().values()))
    tuner.end_epoch()
    assert tuner.optimizer_generator.param_groups[0]["lr"] == pytest.approx(5e-5 * 0.999)
    assert tuner.optimizer_discriminator.param_groups[0]["lr"] == pytest.approx(5e-5 * 0.999)
    # the plans: lean is reference minus the parameter-gradient work of the generator half's two discriminator backward passes
    D = tuner.discriminator
    lean, ref = tuner.launch_plan(), _tuner("reference").launch_plan()
    assert all({"stage", "call"} <= set(e) for e in lean)

    def stage(plan, name):
        return [e for e in plan if e["stage"].startswith(name)]
    assert stage(ref, "generator half: backward of D(wavs)") and not stage(lean, "generator half: backward of D(wavs)")
    assert len(ref) - len(lean) == (len(stage(ref, "generator half: backward of D(wavs_)")) - len(stage(lean, "generator half: backward of D(wavs_)"))
                                    + len(stage(ref, "generator half: backward of D(wavs)")))
    assert len(lean) < len(ref)
    calls = lambda plan: [e["call"] for e in plan]                                       # noqa: E731
    assert calls(lean).count("adamw_multi") == 3 + 2 and calls(lean).count("gan_feature_loss") == 1 and calls(lean).count("gan_score_loss") == 2
    assert not any(c in ("hifigan_wgrad_finish", "hifigan_disc_wgrad") for c in calls(stage(lean, "generator half: backward of D(wavs_)")))
    assert len(D.backward_plan(True, False)) < len(D.backward_plan(True, True))


def test_every_plan_kind_has_a_handler_that_names_known_library_calls():
    import itertools
    import os
    import re

    from seq2seq_vc_amd.urhythmic import vocoder as V
    gen = HifiganGenerator(**VR.TINY_CFG)
    cases = [(gen, gen.launch_plan() + gen.train_plan(torch.float32) + gen.train_plan(torch.bfloat16) + gen.backward_plan())]
    for net in (V.PeriodDiscriminator(3), V.ScaleDiscriminator(), V.ScaleDiscriminator(use_spectral_norm=True)):
        for training in (True, False):
            net.train(training)
            cases.append((net, net.launch_plan() + [e for flags in itertools.product((False, True), repeat=2) for e in net.backward_plan(*flags)]))
    for net, plan in cases:
        expanded = []
        for e in plan:
            handler = net._HANDLERS[e["kind"]]
            names = handler.calls(e) if callable(handler.calls) else handler.calls
            assert names and all("s2svc_" + n in _lib._FUNCTIONS for n in names), (type(net).__name__, e["kind"], names)
            expanded += [dict(e, stage="s", call=n) for n in names]
        assert net.calls(plan, "s") == expanded
    assert all("s2svc_" + n in _lib._FUNCTIONS for n in V._PoolFunction.CALLS)
    assert all("s2svc_" + e["call"] in _lib._FUNCTIONS for e in _tuner("reference").launch_plan())
    # the handler registrations are the only place that maps a kind to library calls
    pkg = os.path.dirname(_lib.__file__)
    for path in ("urhythmic/fine_tune.py", "urhythmic/vocoder.py", "vocoder/hifigan.py", "vocoder/plan.py"):
        src = open(os.path.join(pkg, path)).read()
        assert "_CALLS" not in src and not re.search(r'"\w+":\s*\(?\s*"(hifigan_|fill_zero)', src), path


def test_refusals_on_the_host():
    with pytest.raises(TypeError):
        VocoderFineTuner(torch.nn.Linear(2, 2), HifiganDiscriminator())
    with pytest.raises(TypeError):
        VocoderFineTuner(HifiganGenerator(**VR.TINY_CFG), torch.nn.Linear(2, 2))
    with pytest.raises(TypeError):
        VocoderFineTuner(HifiganGenerator(**VR.TINY_CFG), HifiganDiscriminator(), melspectrogram=torch.nn.Identity())
    with pytest.raises(ValueError):
        _tuner("fast")
    tuner = _tuner()
    x = torch.zeros(2, 1, 960)
    with pytest.raises(RuntimeError):                     # CPU tensors
        tuner.step(x, torch.zeros(2, 80, 15), torch.zeros(2, 1, 80, 3))
    with pytest.raises(NotImplementedError):
        tuner.step(x.bfloat16(), torch.zeros(2, 80, 15), torch.zeros(2, 1, 80, 3))
    a = [torch.zeros(2, 3)]
    for fn in (lambda t: feature_loss([t], [t]), lambda t: discriminator_loss(t, t), generator_loss):
        with pytest.raises(RuntimeError):
            fn(a)
        with pytest.raises(NotImplementedError):
            fn([a[0].bfloat16()])
        with pytest.raises(TypeError):
            fn([a[0].double()])


def test_dense_layout_predicates():
    buf = torch.zeros(2, 5, 3, 8)
    view = buf.permute(0, 3, 1, 2)                        # what the discriminators hand out
    assert KG.dense_like(view) and KG.same_layout(view, torch.zeros(2, 5, 3, 8).permute(0, 3, 1, 2)) and not view.is_contiguous()
    assert not KG.dense_like(buf[:, :, :, ::2]) and not KG.dense_like(buf[:, 1:]) and KG.dense_like(buf[1:])
    assert not KG.same_layout(view, torch.zeros(2, 8, 5, 3)) and KG.dense_like(torch.zeros(2, 1, 7).permute(0, 2, 1))


def test_new_abi_symbols_are_in_the_built_library():
    names = ["s2svc_gan_loss_chunk", "s2svc_gan_loss_max", "s2svc_gan_feature_loss", "s2svc_gan_feature_loss_bwd", "s2svc_gan_score_loss",
             "s2svc_gan_score_loss_bwd", "s2svc_adamw_multi_group", "s2svc_adamw_multi_chunk", "s2svc_adamw_multi"]
    L = abi_header.library()
    for n in names:
        assert n in _lib._FUNCTIONS and n in _lib.exported_symbols() and n in abi_header.declared(), f"{n} missing from the ctypes binding"
        assert getattr(L, n) is not None
    assert sorted(n for n in _lib.exported_symbols() if n.startswith(("s2svc_gan_", "s2svc_adamw_"))) == sorted(names)
    header = abi_header.text()
    assert "replaces: urhythmic/vocoder.py:428-465" in header and "replaces: torch.optim.AdamW.step()" in header
    assert L.s2svc_gan_loss_max() == KG.MAX_ENTRIES == 64
    # a refused call launches nothing and says why (host arguments only: no device is touched)
    assert L.s2svc_gan_feature_loss(0, None, None, None, None, None) == -1
    assert L.s2svc_adamw_multi(81, None, None, None, None, 0, None, None, 1.0, 0.2, 0.99, 0.01, 1e-8, None) == -1
    assert b"adamw_multi" in L.s2svc_last_error()
