"""HiFi-GAN generator backward, host side (no GPU): the yardstick of the GPU cases (tests/vocoder_bwd_ref.py) against the reference's
gradients and against torch autograd, the chunk plan of the weight-gradient kernel, the backward launch list, and a table of
planted errors that the fp32 bar of the GPU cases must be able to see."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocoder_bwd_ref as VB
import vocoder_ref as VR

FP32_BAR = 1e-4          # the bar of tests/gpu_vocoder_bwd_check.py
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hifigan_tiny_grads.npz")


def _relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def truth():
    cfg, sd, _, _, _ = VR.load_fixture()
    x = VB.grad_input()
    y, loss, grads = VB.generator_grads(sd, cfg, x)
    return cfg, sd, x, y, loss, grads


def test_fixture_equals_the_restatements_autograd(truth):
    cfg, sd, x, y, loss, grads = truth
    z = np.load(GOLD)
    assert sorted(k[5:] for k in z.files if k.startswith("grad/")) == sorted(sd) and len(grads) == 234
    assert abs(float(z["loss"]) - float(loss)) < 1e-12
    for k, g in grads.items():
        ref = torch.from_numpy(z["grad/" + k])
        assert ref.shape == g.shape
        assert _relmax(g, ref) < 2e-7, k                   # the fixture stores the reference's float64 gradients rounded to fp32


def test_explicit_restatement_equals_the_generator_and_its_autograd(truth):
    cfg, sd, x, y, loss, grads = truth
    y2, loss2, grads2 = VB.generator_grads(sd, cfg, x, forward=VB.generator_forward_explicit)
    assert float((y2 - y).abs().max()) < 1e-12
    assert max(_relmax(grads2[k], grads[k]) for k in grads) < 1e-10


def test_committed_input_keeps_its_leaky_relu_margin(truth):
    cfg, sd, x, *_ = truth
    assert x.dtype == torch.float32 and tuple(x.shape) == (2, 80, 5)
    m, e, count = VB.margin(sd, cfg, x)
    assert count == 170880
    assert m >= 4 * e, f"smallest leaky-relu input / rms {m:.2e} against torch's fp32 error {e:.2e}"


@pytest.mark.parametrize("k,dil", [(3, 1), (7, 3), (11, 5)])
def test_conv1d_restatement_equals_autograd(k, dil):
    g = torch.Generator().manual_seed(k)
    x = torch.randn(2, 6, 40, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(5, 6, k, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(5, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(2, 5, 40, generator=g, dtype=torch.float64)
    y = F.conv1d(F.leaky_relu(x, 0.1), w, b, dilation=dil, padding=(k - 1) // 2 * dil)
    ref = torch.autograd.grad(y, (x, w, b), dy)
    got = VB.conv1d_backward(x.detach(), w.detach(), dy, dil, 0.1)
    for a, r in zip(got, ref):
        assert _relmax(a, r) < 1e-12


@pytest.mark.parametrize("k,u", [(8, 4), (4, 2), (20, 10), (16, 8)])
def test_transposed_convolution_view_and_operand_equal_autograd(k, u):
    from seq2seq_vc_amd.vocoder import hifigan as H
    g = torch.Generator().manual_seed(k)
    B, T, cin, cout = 2, 9, 6, 5
    x = torch.randn(B, cin, T, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(cin, cout, k, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(B, cout, u * T, generator=g, dtype=torch.float64)
    y = F.conv_transpose1d(F.leaky_relu(x, 0.1), w, b, stride=u, padding=(k - u) // 2)
    ref = torch.autograd.grad(y, (x, w, b), dy)
    dx, dw, db = VB.tconv_backward(x.detach().transpose(1, 2), w.detach(), dy.transpose(1, 2).contiguous(), u, 0.1)
    assert _relmax(dx.transpose(1, 2), ref[0]) < 1e-12 and _relmax(dw, ref[1]) < 1e-12 and _relmax(db, ref[2]) < 1e-12
    # the operand is the forward's, and the view rows are the forward's GEMM rows
    assert torch.equal(VB.tconv_operand(w.detach(), u).reshape(u * cout, -1), H.tconv1d_operand(w.detach(), u))
    rows = H.tconv1d_rows(T, k, u)
    view = VB.tconv_dy_view(dy.transpose(1, 2).contiguous(), k, u, rows)
    for i in (0, rows - 1):
        for p in (0, u - 1):
            t = H.tconv1d_out_frame(i, p, k, u)
            want = dy[:, :, t] if 0 <= t < u * T else torch.zeros(B, cout, dtype=torch.float64)
            assert torch.equal(view[:, i, p * cout:(p + 1) * cout], want)


@pytest.mark.parametrize("shape", [(5, 7, 3), (64, 32, 8)])
def test_weight_norm_restatement_equals_autograd(shape):
    g = torch.Generator().manual_seed(3)
    v = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_(True)
    gn = (0.5 + torch.rand(shape[0], 1, 1, generator=g, dtype=torch.float64)).requires_grad_(True)
    dw = torch.randn(shape, generator=g, dtype=torch.float64)
    ref = torch.autograd.grad(torch._weight_norm(v, gn, 0), (v, gn), dw)
    dg, dv = VB.weight_norm_backward(v.detach(), gn.detach(), dw)
    assert _relmax(dv, ref[0]) < 1e-12 and _relmax(dg, ref[1]) < 1e-12


def test_wgrad_plan_covers_every_frame_exactly_once():
    from seq2seq_vc_amd.ops import kernels_vocoder as KV
    for B, rows in [(1, 1), (1, 31), (2, 32), (3, 127), (3, 128), (3, 129), (3, 150), (2, 1024), (2, 1025), (8, 8320), (1, 1537)]:
        for chunk in (None, 32, 96):
            plan = KV.wgrad_plan(B, rows, chunk)
            seen = np.zeros((B, rows), dtype=np.int64)
            for b, r0, r1 in plan:
                assert 0 <= r0 < r1 <= rows and r0 % KV.WGRAD_STEP == 0
                seen[b, r0:r1] += 1
            assert (seen == 1).all()
            assert plan == sorted(plan)                                  # ascending: the order the finish launch sums in
            size = chunk or (128 if rows <= 1024 else 512)
            assert len(plan) == B * -(-rows // size)
            assert plan == KV.wgrad_plan(B, rows, chunk)                 # shapes only
    assert KV.wgrad_rows(0, 150, 7) == 150 and KV.wgrad_rows(1, 37, 20, 10) == 38 and KV.wgrad_rows(1, 37, 4, 2) == 38
    with pytest.raises(ValueError):
        KV.wgrad_plan(2, 100, 48)


def test_backward_plan_of_the_default_configuration():
    """conv_post: backward + finish = 2.  Every other convolution: partials + finish + data gradient = 3, except conv_pre, whose input
    is data: 2.  4 ups + 72 ResBlock convolutions = 76 -> 2 + 3 * 76 + 2 = 232 launches, no element-wise one among them."""
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    from seq2seq_vc_amd.vocoder import hifigan as H
    gen = HifiganGenerator()
    plan = gen.backward_plan()
    kinds = [e["kind"] for e in plan]
    assert len(plan) == 232 and set(kinds) == set(H.BWD_KINDS)
    assert kinds.count("conv_out_bwd") == 1 and kinds.count("wgrad") == 77 and kinds.count("finish") == 78
    assert kinds.count("conv1d_dgrad") == 72 and kinds.count("tconv1d_dgrad") == 4
    assert kinds[0] == "conv_out_bwd" and plan[-1]["layer"] == "conv_pre" and kinds[-2:] == ["wgrad", "finish"]
    # every finish follows its own layer's partials
    for a, b in zip(plan, plan[1:]):
        if b["kind"] == "finish":
            assert a["kind"] in ("wgrad", "conv_out_bwd") and a["layer"] == b["layer"]
    # every gradient buffer is written by one launch, except d:up{i}: the three blocks of a stage accumulate into it
    writers = {}
    for e in plan:
        if "dst" in e:
            writers.setdefault(e["dst"], []).append(e)
    for dst, es in writers.items():
        if dst.startswith("d:up"):
            assert [e["accumulate"] for e in es] == [False, True, True]
        else:
            assert len(es) == 1 and not es[0].get("accumulate", False)
    # a gradient is read only after it was written; the 1 / 3 of the MRF average rides on the launch that writes d:s{i}
    done = set()
    for e in plan:
        for key in ("dy", "res"):
            assert e.get(key) is None or e[key] in done
        if "dst" in e:
            done.add(e["dst"])
            if e["dst"].startswith("d:s"):
                assert abs(e["scale"] - 1 / 3) < 1e-12
            else:
                assert e["scale"] == 1.0
    # convs1's data gradient carries the residual of its unit, masks are the forward's raw layer inputs
    c1 = [e for e in plan if e["kind"] == "conv1d_dgrad" and ".convs1." in e["layer"]]
    assert len(c1) == 36 and all(e["res"] is not None and e["mask"] == e["dst"][2:] for e in c1)
    # the training forward keeps every convolution's input: no buffer is written twice except the stage sums
    train = gen.train_plan(torch.float32)
    fwd = [e for e in train if e["kind"] in H.KINDS]
    dsts = [e["dst"] for e in fwd if "dst" in e and not e.get("accumulate")]
    assert len(dsts) == len(set(dsts)) and [e["kind"] for e in fwd] == [e["kind"] for e in gen.launch_plan()]
    # in front of the convolutions: one fold per leaf, and the data gradient's operand for every leaf but conv_pre and conv_post
    leaves = [name for name, _ in gen._leaves()]
    folds = train[:-len(fwd)]
    assert train[len(folds):] == fwd and {e["kind"] for e in folds} == {"fold", "fold_bwd"} and set(H.TRAIN_KINDS) >= {e["kind"] for e in train}
    assert [e["layer"] for e in folds if e["kind"] == "fold"] == leaves and all(e["op"] for e in folds if e["kind"] == "fold")
    assert [e["layer"] for e in folds if e["kind"] == "fold_bwd"] == [name for name in leaves if name not in ("conv_pre", "conv_post")]
    # bf16 mode: the same list, then one cast per kept buffer
    bf16 = gen.train_plan(torch.bfloat16)
    assert bf16[:len(train)] == train and [e["kind"] for e in bf16[len(train):]] == ["cast"] * len(set(dsts))
    assert sorted(e["src"] for e in bf16[len(train):]) == sorted(set(dsts))


def test_trainable_off_changes_nothing_on_the_host():
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    gen = HifiganGenerator(**VR.TINY_CFG)
    before = gen.launch_plan()
    assert gen._trainable is False
    assert gen.trainable() is gen and gen._trainable is True
    assert gen.launch_plan() == before
    assert gen.trainable(False) is gen and gen._trainable is False and gen.launch_plan() == before
    x = torch.zeros(1, 80, 4)
    for mode in (False, True):                   # no CPU path in either mode
        gen.trainable(mode)
        with pytest.raises(RuntimeError):
            gen(x)
    with pytest.raises(NotImplementedError):     # the input never gets a gradient
        gen.trainable(True)(x.requires_grad_(True))
    assert "nference only" in HifiganGenerator.forward_batch.__doc__


def test_every_plant_moves_a_gradient_by_ten_bars(truth):
    """The GPU cases compare every gradient with float64 at FP32_BAR relative to its largest magnitude.  Each planted error must move
    some parameter's gradient by at least 10 bars on the committed input, or that comparison could not see it."""
    cfg, sd, x, y, loss, grads = truth
    moved = {}
    for plant in VB.PLANTS:
        y2, _, g2 = VB.generator_grads(sd, cfg, x, forward=VB.generator_forward_explicit, plant=plant)
        assert float((y2 - y).abs().max()) < 1e-12                    # a plant changes the backward only
        moved[plant] = max(_relmax(g2[k], grads[k]) for k in grads)
    assert sorted(moved) == sorted(VB.PLANTS) and len(moved) == 8
    weak = {p: v for p, v in moved.items() if v < 10 * FP32_BAR}
    assert not weak, f"plants below 10 x FP32_BAR: {weak}"
