"""Host tests of the HiFi-GAN multi-scale discriminator (seq2seq_vc_amd/urhythmic/vocoder.py, csrc/hifigan_msd.hip): the plain-torch
restatement tests/msd_ref.py against the fixture recorded from the reference, the new classes' state_dict against the recorded key
list, the length rules and index models against stock torch, the spectral-norm gradient formula against autograd, the launch plans,
the ABI, and the planted errors the restatement must catch.  No GPU.

Bound of the fixture comparison: the fixture holds the reference's float32 results, the restatement runs in float64, so they differ by
the reference's own rounding: 2^-24 per operation over reductions of up to 5 * 1024 terms, eight layers, forward and backward --
about 6e-8 * sqrt(5120) * 16 = 7e-5 of a tensor's largest magnitude at the very worst.  REL = 1e-4; a dropped tap is 1e-1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msd_ref as MR

REL = 1e-4


@pytest.fixture(scope="module")
def golden():
    return MR.load_golden()


@pytest.fixture(scope="module")
def seeded(golden):
    return MR.seeded_state_dict(int(golden["seed"]))


@pytest.fixture(scope="module")
def restated(golden, seeded):
    return MR.run(seeded, torch.from_numpy(golden["xr"]), torch.from_numpy(golden["xg"]), torch.float64)


def _close(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if scale is None else scale
    return float(np.abs(got - want).max()) <= REL * scale


def _sample(t):
    flat = t.detach().reshape(-1).numpy()
    return flat[MR.sample_positions(flat.size)]


def test_restatement_equals_the_reference_fixture(golden, restated):
    r = restated
    assert _close(r["loss"], golden["loss"])
    assert _close(r["dxg"], golden["dxg"]) and _close(r["dxr"], golden["dxr"])
    for i in range(3):
        assert _close(r["scores"][i], golden[f"score/{i}"]), i
        for j in range(8):
            f = r["feats"][i][j]
            assert tuple(f.shape) == tuple(golden[f"feat_shape/{i}.{j}"]), (i, j)
            assert _close(f.abs().mean(), golden[f"feat_mean/{i}.{j}"]), (i, j)
            assert _close(_sample(f), golden[f"feat_sample/{i}.{j}"], scale=float(f.abs().max())), (i, j)
    assert len(r["grads"]) == 64
    for k, g in r["grads"].items():
        assert _close(_sample(g), golden["grad_sample/" + k], scale=float(golden["grad_absmax/" + k])), k
    assert len(r["buffers"]) == 16
    for k, b in r["buffers"].items():
        assert _close(_sample(b), golden["buffer_sample/" + k], scale=float(b.abs().max())), k


def test_eval_mode_uses_the_stored_buffers(golden, seeded):
    sd = {k: v.double() for k, v in seeded.items()}
    after = {}
    scores, _ = MR.msd_forward(sd, torch.from_numpy(golden["xg"]).double(), train=False, buffers=after)
    for i in range(3):
        assert _close(scores[i], golden[f"eval_score/{i}"]), i
    assert all(torch.equal(after[k], sd[k]) for k in after) and len(after) == 16
    assert not _close(scores[0], golden["score/0"])          # two power iterations later the first scale's scores differ


def test_fixture_network_is_alive(golden, restated):
    ok, msg = MR.alive(torch.from_numpy(golden["xg"]), restated["feats"])
    assert ok, msg


def test_planted_dropped_tap_is_caught(golden, seeded):
    sd = {k: v.double() for k, v in seeded.items()}
    xg = MR.pool(torch.from_numpy(golden["xg"]).double())
    for layer, tap in ((0, 14), (1, 0), (5, 20)):         # at T = 331 layer 5 of scale 1 has 3 rows: taps 18 .. 22 read data
        s, _ = MR.scale_forward(sd, 1, xg, drop_tap=(layer, tap))
        assert not _close(s, golden["score/1"]), (layer, tap)
    s, _ = MR.scale_forward(sd, 1, xg)
    assert _close(s, golden["score/1"])


def test_state_dict_keys_shapes_and_buffers_are_the_references(golden, seeded):
    from seq2seq_vc_amd.urhythmic.vocoder import HifiganDiscriminator, MultiScaleDiscriminator, ScaleDiscriminator
    msd = MultiScaleDiscriminator()
    sd = msd.state_dict()
    want = [(str(k), tuple(int(v) for v in s.split(","))) for k, s in zip(golden["keys"], golden["shapes"])]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want == MR.state_dict_shapes()
    assert len(want) == 80 and sum(int(np.prod(s)) for _, s in want) == 29637357
    params = [k for k, _ in msd.named_parameters()]
    buffers = [k for k, _ in msd.named_buffers()]
    assert len(params) == 64 and sorted(buffers) == sorted(str(k) for k, b in zip(golden["keys"], golden["buffer"]) if b)
    assert all(MR.is_buffer(k) for k in buffers) and not any(MR.is_buffer(k) for k in params)
    res = msd.load_state_dict(seeded)
    assert not res.missing_keys and not res.unexpected_keys
    back = msd.state_dict()
    assert all(torch.equal(back[k], seeded[k]) for k in seeded)
    spectral, normed = ScaleDiscriminator(use_spectral_norm=True), ScaleDiscriminator()
    assert [n for n, _ in spectral.named_parameters()] == [f"{MR.layer_name(j)}.{leaf}" for j in range(8) for leaf in ("bias", "weight_orig")]
    assert [n for n, _ in normed.named_parameters()] == [f"{MR.layer_name(j)}.{leaf}" for j in range(8) for leaf in ("bias", "weight_g", "weight_v")]
    for m in spectral.modules():                          # fresh buffers: unit vectors
        if hasattr(m, "weight_u"):
            assert abs(float(m.weight_u.norm()) - 1) < 1e-5 and abs(float(m.weight_v.norm()) - 1) < 1e-5
    whole = HifiganDiscriminator()
    keys = list(whole.state_dict())
    assert [k for k in keys if k.startswith("msd.")] == ["msd." + k for k, _ in want] and len(keys) == 90 + 80
    assert keys[0].startswith("mpd.") and keys[-1].startswith("msd.")
    res = whole.load_state_dict({**{"msd." + k: v for k, v in seeded.items()}, **{k: v for k, v in whole.state_dict().items() if k.startswith("mpd.")}})
    assert not res.missing_keys and not res.unexpected_keys


def test_refusals():
    from seq2seq_vc_amd.urhythmic.vocoder import HifiganDiscriminator, MultiScaleDiscriminator, ScaleDiscriminator
    d = ScaleDiscriminator()
    with pytest.raises(RuntimeError, match="no CPU path"):
        d(torch.zeros(1, 1, 64))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        d(torch.zeros(1, 1, 64, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        d(torch.zeros(1, 1, 64, dtype=torch.float16))
    with pytest.raises(TypeError):
        d(torch.zeros(1, 1, 64, dtype=torch.float64))
    with pytest.raises(ValueError):
        d(torch.zeros(1, 64))
    with pytest.raises(ValueError):
        d(torch.zeros(1, 2, 64))
    for whole in (MultiScaleDiscriminator(), HifiganDiscriminator()):
        with pytest.raises(RuntimeError, match="no CPU path"):
            whole(torch.zeros(1, 1, 64))


def test_launch_plans_state_the_counts():
    from seq2seq_vc_amd.urhythmic import vocoder as V
    wn, sn = V.ScaleDiscriminator(), V.ScaleDiscriminator(use_spectral_norm=True)
    compute = ["input"] + ["gconv"] * 5 + ["conv", "post"]
    fwd = wn.launch_plan()
    assert [e["kind"] for e in fwd] == ["fold"] * 8 + compute and all(e["kind"] in V.MSD_KINDS for e in fwd)
    sfwd = sn.launch_plan()
    assert [e["kind"] for e in sfwd] == ["sn_power", "sn_scale"] + ["sn_power", "sn_scale", "fold"] * 7 + compute
    assert all(e["iterate"] for e in sfwd if e["kind"] == "sn_power")
    sn.eval()
    assert not any(e["iterate"] for e in sn.launch_plan() if e["kind"] == "sn_power")
    assert [(e["cin"], e["cout"], e["stride"], e["groups"]) for e in fwd if e["kind"] == "gconv"] == [(c, o, s, g) for c, o, k, s, g in MR.LAYERS[1:6]]
    full, disc_step, no_params = wn.backward_plan(need_dx=True), wn.backward_plan(need_dx=False), wn.backward_plan(need_dx=True, need_params=False)
    assert all(e["kind"] in V.MSD_BWD_KINDS for e in full)
    assert len(full) == len(disc_step) + 1 and full[-1]["kind"] == "input_dgrad"          # x.detach(): the first layer's data gradient is skipped
    assert [e["kind"] for e in no_params] == ["post_bwd", "fold_bwd", "dgrad"] + ["gfold_bwd", "gconv_dgrad"] * 5 + ["input_dgrad"]
    kinds = [e["kind"] for e in disc_step]
    assert kinds.count("finish") == 8 and kinds.count("gconv_wgrad") == 5 and kinds.count("wgrad") == 1 and kinds.count("sn_finish") == 0
    assert [e["kind"] for e in sn.backward_plan()].count("sn_finish") == 8
    assert [e["kind"] for e in sn.backward_plan(need_params=False)] == [e["kind"] for e in wn.backward_plan(need_params=False)]
    msd = V.MultiScaleDiscriminator()
    mf = msd.launch_plan()
    assert len(mf) == len(sn.launch_plan()) + 2 * len(fwd) + 2 and [e["kind"] for e in mf].count("pool") == 2
    assert sorted({e["scale"] for e in mf}) == [0, 1, 2]
    assert [e["kind"] for e in msd.backward_plan(need_dx=True)].count("pool_bwd") == 2
    assert [e["kind"] for e in msd.backward_plan(need_dx=False)].count("pool_bwd") == 0
    whole = V.HifiganDiscriminator()
    assert len(whole.launch_plan()) == 60 + len(mf)


@pytest.mark.parametrize("T", range(1, 201))
def test_length_rules_against_stock_torch(T):
    from seq2seq_vc_amd.ops import kernels_msd as KM
    from seq2seq_vc_amd.urhythmic.vocoder import scale_lengths
    x = torch.zeros(1, 1, T)
    chain = []
    for i in range(3):
        if i:
            x = F.avg_pool1d(x, 4, 2, padding=2)
            assert x.shape[-1] == MR.pool_len(x_prev) == KM.pool_len(x_prev)
        x_prev = x.shape[-1]
        h, row = x, []
        for cin, cout, k, s, g in MR.LAYERS:
            h = F.conv1d(h[:, :1].expand(1, g, -1), torch.zeros(g, 1, k), stride=s, padding=(k - 1) // 2, groups=g)
            row.append(h.shape[-1])
        assert row == scale_lengths(x_prev)
        assert all(KM.out_len(a, l[3]) == b for a, b, l in zip([x_prev] + row, row, MR.LAYERS))
        chain.append(row)
    assert chain == MR.length_chain(T)


def test_pool_restatement_equals_avg_pool1d():
    for T in (1, 2, 3, 7, 331, 332):
        x = torch.randn(2, 1, T, dtype=torch.float64, generator=torch.Generator().manual_seed(T))
        assert torch.allclose(MR.pool(x), F.avg_pool1d(x, 4, 2, padding=2), atol=1e-15), T


@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8, 43, 46])
def test_phase_decomposed_data_gradient_and_its_plant(L, stride):
    g = torch.Generator().manual_seed(10 * L + stride)
    cin, cout = 3, 2
    x = torch.randn(1, cin, L, dtype=torch.float64, generator=g).requires_grad_(True)
    w = torch.randn(cout, cin, 41, dtype=torch.float64, generator=g)
    y = F.conv1d(x, w, stride=stride, padding=20)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert torch.allclose(MR.dgrad_phase_model(dy[0].t(), w, L, stride), dx[0].t(), atol=1e-12)
    if stride > 1 and L > 1:
        assert not torch.allclose(MR.dgrad_phase_model(dy[0].t(), w, L, stride, plant=True), dx[0].t(), atol=1e-6)


def test_phase_tables_state_the_tap_counts():
    assert [len(MR.dgrad_phase_table(2, ph)) for ph in range(2)] == [21, 20]
    assert [len(MR.dgrad_phase_table(4, ph)) for ph in range(4)] == [11, 10, 10, 10]
    assert len(MR.dgrad_phase_table(1, 0)) == 41
    for s in (1, 2, 4):
        taps = sorted(j for ph in range(s) for _, j in MR.dgrad_phase_table(s, ph))
        assert taps == list(range(41))
        assert all((ph + 20 - j) % s == 0 and s * off + j - 20 == ph for ph in range(s) for off, j in MR.dgrad_phase_table(s, ph))


@pytest.mark.parametrize("stride", [1, 2, 4])
def test_grouped_rows_stay_in_their_group_and_utterance_and_the_plants(stride):
    g = torch.Generator().manual_seed(stride)
    B, L, groups, cg, og = 2, 9, 4, 2, 3
    x = torch.randn(B, L, groups * cg, dtype=torch.float64, generator=g)
    w = torch.randn(groups * og, cg, 41, dtype=torch.float64, generator=g)
    want = F.conv1d(x.permute(0, 2, 1), w, stride=stride, padding=20, groups=groups).permute(0, 2, 1)
    assert torch.allclose(MR.grouped_conv_model(x, w, groups, stride), want, atol=1e-12)
    assert not torch.allclose(MR.grouped_conv_model(x, w, groups, stride, neighbour=True), want, atol=1e-6)
    assert not torch.allclose(MR.grouped_conv_model(x, w, groups, stride, leak=True), want, atol=1e-6)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 8, 331, 332])
def test_pool_adjoint_at_both_edges_and_its_plant(T):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(1, 1, T, dtype=torch.float64, generator=g).requires_grad_(True)
    y = F.avg_pool1d(x, 4, 2, padding=2)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert torch.allclose(MR.pool_adjoint_model(dy[0, 0], T), dx[0, 0], atol=1e-14)
    for edge in ("left", "right"):
        assert not torch.allclose(MR.pool_adjoint_model(dy[0, 0], T, plant=edge), dx[0, 0], atol=1e-6), edge


@pytest.mark.parametrize("train", [True, False])
def test_spectral_gradient_formula_against_stock_spectral_norm(train):
    torch.manual_seed(3)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(256, 512, 41, 4, groups=16, padding=20)).double()
    conv.train(train)
    W = conv.weight_orig.detach().clone()
    u0, v0 = conv.weight_u.clone(), conv.weight_v.clone()
    x = torch.randn(2, 256, 50, dtype=torch.float64)
    y = conv(x)
    dy = torch.randn_like(y)
    (want,) = torch.autograd.grad(y, conv.weight_orig, dy)
    u, v = MR.power_iteration(W, u0, v0, train)
    assert torch.allclose(u, conv.weight_u, atol=1e-14) and torch.allclose(v, conv.weight_v, atol=1e-14)
    assert train != torch.equal(u, u0)
    sigma = torch.dot(u, W.flatten(1) @ v)
    w = (W / sigma).requires_grad_(True)
    (dW,) = torch.autograd.grad(F.conv1d(x, w, conv.bias, stride=4, padding=20, groups=16), w, dy)
    got = MR.spectral_grad(dW, W, u, v, sigma)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((dW / sigma - want).abs().max()) > 1e-3 * float(want.abs().max())          # the second term is no rounding matter


def test_header_sigs_exports_and_sources():
    import ctypes
    import os

    from seq2seq_vc_amd import _lib
    from seq2seq_vc_amd.ops import kernels_msd as KM
    names = ["s2svc_hifigan_msd_pool", "s2svc_hifigan_msd_pool_bwd", "s2svc_hifigan_msd_input", "s2svc_hifigan_msd_input_wgrad",
             "s2svc_hifigan_msd_input_dgrad", "s2svc_hifigan_msd_gconv", "s2svc_hifigan_msd_fold_bwd", "s2svc_hifigan_msd_gconv_dgrad",
             "s2svc_hifigan_msd_gconv_chunk", "s2svc_hifigan_msd_gconv_wgrad", "s2svc_hifigan_msd_sn_power", "s2svc_hifigan_msd_sn_scale",
             "s2svc_hifigan_msd_sn_finish"]
    assert "hifigan_msd.hip" in _lib.sources()
    assert sorted(n for n in _lib.exported_symbols() if n.startswith("s2svc_hifigan_msd")) == sorted(names)
    i, f, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    assert _lib._FUNCTIONS["s2svc_hifigan_msd_gconv"] == (i, [i] * 6 + [vp] * 3 + [f, vp, vp])
    assert _lib._FUNCTIONS["s2svc_hifigan_msd_pool_bwd"] == (i, [i] * 2 + [vp] * 3)
    header = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "s2svc_hip.h")).read()
    assert "replaces: urhythmic/vocoder.py:330-402" in header
    for n in names:                                      # every entry point carries its own `replaces:` comment
        decl = header.index("int " + n + "(")
        assert "replaces:" in header[header.rindex("/*", 0, decl):decl], n
    src = open(os.path.join(_lib.CSRC, "hifigan_msd.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and all(('extern "C" int ' + n + "(") in src for n in names)
    for n in names:                                      # one wrapper per entry point
        assert hasattr(KM, n[len("s2svc_hifigan_"):]) or hasattr(KM, n[len("s2svc_hifigan_msd_"):]), n
    # the chunk rule of the weight partials, as the header states it: at most eight partials per utterance, 256 rows at the least
    assert all(-(-Lo // max(256, 32 * -(-Lo // 256))) <= 8 for Lo in (1, 130, 520, 2080, 4160, 100000))
