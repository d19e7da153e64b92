"""Host-side checks of the HiFi-GAN vocoder (no GPU): the test-side restatement against the reference's fixture, the drop-in
state_dict surface, the transposed convolution's GEMM addressing, the launch plan, and the no-fallback rule."""
import math

import pytest
import torch
import torch.nn.functional as F

import vocoder_ref as VR


def test_restatement_reproduces_the_reference_fixture():
    """Same torch operators as the reference, fp32: every tap and the waveform within 1e-5 (the reference's own fp32-vs-float64
    distance on this fixture is ~1e-6)."""
    cfg, sd, x, y, taps = VR.load_fixture()
    got = {}
    with torch.no_grad():
        yr = VR.generator_forward(sd, cfg, x, got)
    assert sorted(got) == sorted(taps) == sorted(VR.tap_names(cfg))
    for k in taps:
        assert got[k].shape == taps[k].shape, k
        err = float((got[k] - taps[k]).abs().max())
        print(f"{k}: max abs {err:.2e}")
        assert err <= 1e-5, f"{k}: {err}"
    err = float((yr - y).abs().max())
    print(f"waveform: max abs {err:.2e}")
    assert yr.shape == y.shape == (2, 1, 37 * 64) and err <= 1e-5
    ok, msg = VR.alive(y, taps, cfg)
    assert ok, msg


def _expected_keys(cfg):
    """The reference's key list and shapes in the weight-normed form, from its constructor (urhythmic/vocoder.py:56-85, 125-193)."""
    c = VR.full_cfg(cfg)
    uc, out = c["upsample_channels"], []

    def conv(name, shape, nb):
        out.extend([(name + ".bias", (nb,)), (name + ".weight_g", (shape[0], 1, 1)), (name + ".weight_v", tuple(shape))])

    conv("conv_pre", (uc, c["in_channels"], 5), uc)
    for i, k in enumerate(c["upsample_kernel_sizes"]):
        conv(f"ups.{i}", (uc // 2 ** i, uc // 2 ** (i + 1), k), uc // 2 ** (i + 1))
    nk = len(c["resblock_kernel_sizes"])
    for i in range(len(c["upsample_factors"])):
        ch = uc // 2 ** (i + 1)
        for j, (k, ds) in enumerate(zip(c["resblock_kernel_sizes"], c["resblock_dilation_sizes"])):
            for grp in ("convs1", "convs2"):
                for q in range(len(ds)):
                    conv(f"resblocks.{i * nk + j}.{grp}.{q}", (ch, ch, k), ch)
    conv("conv_post", (1, ch, 7), 1)
    return out


def test_generator_has_the_reference_state_dict_in_both_forms():
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    cfg, sd, _, _, _ = VR.load_fixture()
    tiny = HifiganGenerator(**cfg)
    assert list(tiny.state_dict().keys()) == list(sd.keys())
    assert all(tiny.state_dict()[k].shape == sd[k].shape for k in sd)
    tiny.load_state_dict(sd)                                            # strict
    default = HifiganGenerator()
    exp = _expected_keys({})
    assert len(exp) == 234
    assert [(k, tuple(v.shape)) for k, v in default.state_dict().items()] == exp
    assert default.sample_rate == 16000 and default.in_channels == 256
    # the remove_weight_norm form: *.weight / *.bias
    plain = {}
    for k, v in sd.items():
        if k.endswith("weight_v"):
            plain[k[:-2]] = VR.weight(sd, k[:-9])
        elif k.endswith("bias"):
            plain[k] = v
    other = HifiganGenerator(**cfg)
    other.load_state_dict(plain)
    assert sorted(other.state_dict().keys()) == sorted(plain.keys()) and len(plain) == 2 * 234 // 3
    assert all(torch.equal(other.state_dict()[k], plain[k]) for k in plain)
    other.load_state_dict(sd)                                           # and back
    assert list(other.state_dict().keys()) == list(sd.keys())
    tiny.remove_weight_norm()
    assert sorted(tiny.state_dict().keys()) == sorted(plain.keys())
    assert all(float((tiny.state_dict()[k] - plain[k]).abs().max()) <= 1e-6 for k in plain)


@pytest.mark.parametrize("k,u", [(20, 10), (16, 8), (4, 2), (8, 4), (12, 4)])
def test_transposed_convolution_as_one_gemm(k, u):
    """The (p, o) x (tap, c) operand and the row map of the package, evaluated with plain torch in float64, equal
    F.conv_transpose1d: four default layers, (8, 4) and the 3-tap case (12, 4); output length exactly u * T_in."""
    from seq2seq_vc_amd.vocoder import hifigan as H
    g = torch.Generator().manual_seed(k * 100 + u)
    cin, cout, B, T = 6, 5, 2, 23
    x = torch.randn(B, cin, T, generator=g, dtype=torch.float64)
    w = torch.randn(cin, cout, k, generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    ref = F.conv_transpose1d(x, w, bias, stride=u, padding=(k - u) // 2)
    pad, ntaps = H.tconv1d_geometry(k, u)
    assert (pad, ntaps) == ((k - u) // 2, math.ceil(k / u)) and ref.shape[-1] == u * T
    op = H.tconv1d_operand(w, u)                                         # [u * cout, ntaps * cin]
    rows = H.tconv1d_rows(T, k, u)
    xcl = x.transpose(1, 2)                                              # channel-last (B, T, cin)
    A = torch.zeros(B, rows, ntaps, cin, dtype=torch.float64)            # row i, tap n reads frame i - n (zero outside)
    for i in range(rows):
        for n in range(ntaps):
            if 0 <= i - n < T:
                A[:, i, n] = xcl[:, i - n]
    G = A.reshape(B, rows, ntaps * cin) @ op.t() + bias.repeat(u)        # columns (p, o)
    out = torch.full((B, u * T, cout), float("nan"), dtype=torch.float64)
    written = torch.zeros(u * T, dtype=torch.int64)
    for i in range(rows):
        for p in range(u):
            t = H.tconv1d_out_frame(i, p, k, u)
            if 0 <= t < u * T:
                out[:, t] = G[:, i, p * cout:(p + 1) * cout]
                written[t] += 1
    assert torch.equal(written, torch.ones_like(written)), "every output frame is stored exactly once"
    err = float((out.transpose(1, 2) - ref).abs().max())
    assert err <= 1e-12, err
    # the zero-padded operand the kernel reads (input channels padded to the reduction step)
    opp = H.tconv1d_operand(w, u, cin_padded=32).reshape(u * cout, ntaps, 32)
    assert torch.equal(opp[:, :, :cin].reshape(u * cout, -1), op) and float(opp[:, :, cin:].abs().max()) == 0.0


def test_transposed_convolution_geometry_rejects_what_the_kernel_does_not_take():
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    from seq2seq_vc_amd.vocoder import hifigan as H
    with pytest.raises(ValueError):
        H.tconv1d_geometry(7, 4)                                         # (k - u) odd
    with pytest.raises(ValueError):
        H.tconv1d_geometry(2, 4)                                         # k < u
    with pytest.raises(ValueError):
        HifiganGenerator(upsample_kernel_sizes=(20, 15, 4, 4))
    # per-stage length bookkeeping of a ragged batch
    assert H.stage_lengths([60, 41, 1], (10, 8, 2, 2)) == [[60, 41, 1], [600, 410, 10], [4800, 3280, 80], [9600, 6560, 160],
                                                          [19200, 13120, 320]]


def test_launch_plan_of_the_default_configuration():
    """No element-wise launch anywhere in a call: 1 input + conv_pre + 4 ups + 72 ResBlock convolutions + conv_post = 79."""
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    from seq2seq_vc_amd.vocoder import hifigan as H
    plan = HifiganGenerator().launch_plan()
    assert len(plan) <= 79
    kinds = [e["kind"] for e in plan]
    assert set(kinds) <= set(H.KINDS)
    assert kinds.count("input") == 1 and kinds.count("tconv1d") == 4 and kinds.count("conv_out") == 1 and kinds.count("conv1d") == 73
    # the fused options: every ResBlock convolution has the leaky_relu prologue, every convs2 the residual, the last one of
    # each block feeds the stage average (first block writes, the others accumulate), and conv_post uses torch's default slope
    rb = [e for e in plan if e["kind"] == "conv1d" and e["layer"].startswith("resblocks.")]
    assert all(e["slope"] == 0.1 for e in rb) and all(("res" in e) == (".convs2." in e["layer"]) for e in rb)
    avg = [e for e in rb if "scale" in e]
    assert len(avg) == 12 and all(abs(e["scale"] - 1 / 3) < 1e-12 for e in avg)
    assert [e["accumulate"] for e in avg] == [False, True, True] * 4
    assert plan[-1]["slope"] == 0.01 and plan[1]["slope"] == 0.0
    # no convolution writes the buffer it reads with a halo
    assert all(e.get("dst") != e.get("src") for e in plan)


def test_forward_on_cpu_tensors_raises():
    from seq2seq_vc_amd.vocoder import HifiganGenerator, HifiganVocoder
    cfg = dict(VR.TINY_CFG)
    gen = HifiganGenerator(**cfg)
    with pytest.raises(RuntimeError):
        gen(torch.zeros(1, 80, 8))
    with pytest.raises(RuntimeError):
        gen.forward_batch(torch.zeros(2, 8, 80), [8, 3])
    with pytest.raises(ValueError):
        HifiganGenerator(upsample_kernel_sizes=(9, 8, 4, 4), upsample_factors=(4, 4, 2, 2))
    with pytest.raises(ValueError):
        HifiganVocoder(gen, dict(mean=[0.0] * 80, scale=[1.0] * 80))     # take_norm_feat needs trg_stats

