"""Host tests of the HiFi-GAN multi-period discriminator (seq2seq_vc_amd/urhythmic/vocoder.py, csrc/hifigan_disc.hip): the plain-torch
restatement tests/disc_ref.py against the fixture recorded from the reference, the new classes' state_dict against the recorded key
list, the shape rules and index maps against stock torch, the ABI, and the planted errors the restatement must catch.  No GPU.

Bound of the fixture comparison: the fixture holds the reference's float32 results, the restatement runs in float64, so they differ by
the reference's own rounding: 2^-24 per operation over reductions of up to 5 * 1024 terms, six layers, forward and backward --
about 6e-8 * sqrt(5120) * 12 = 5e-5 of a tensor's largest magnitude at the very worst.  REL = 1e-4; a dropped tap is 1e-1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_ref as DR

REL = 1e-4


@pytest.fixture(scope="module")
def golden():
    return DR.load_golden()


@pytest.fixture(scope="module")
def restated(golden):
    sd = DR.seeded_state_dict(int(golden["seed"]))
    return DR.run(sd, torch.from_numpy(golden["xr"]), torch.from_numpy(golden["xg"]), torch.float64)


def _close(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if scale is None else scale
    return float(np.abs(got - want).max()) <= REL * scale


def _sample(t):
    flat = t.detach().reshape(-1).numpy()
    return flat[DR.sample_positions(flat.size)]


def test_restatement_equals_the_reference_fixture(golden, restated):
    r = restated
    assert _close(r["loss"], golden["loss"])
    assert _close(r["dxg"], golden["dxg"]) and _close(r["dxr"], golden["dxr"])
    for i in range(5):
        assert _close(r["scores"][i], golden[f"score/{i}"]), i
        for j in range(6):
            f = r["feats"][i][j]
            assert tuple(f.shape) == tuple(golden[f"feat_shape/{i}.{j}"]), (i, j)
            assert _close(f.abs().mean(), golden[f"feat_mean/{i}.{j}"]), (i, j)
            assert _close(_sample(f), golden[f"feat_sample/{i}.{j}"], scale=float(f.abs().max())), (i, j)
    assert len(r["grads"]) == 90
    for k, g in r["grads"].items():
        assert _close(_sample(g), golden["grad_sample/" + k], scale=float(golden["grad_absmax/" + k])), k


def test_fixture_network_is_alive(golden, restated):
    ok, msg = DR.alive(torch.from_numpy(golden["xg"]), restated["feats"])
    assert ok, msg


def test_planted_dropped_tap_is_caught(golden):
    sd = {k: v.double() for k, v in DR.seeded_state_dict(int(golden["seed"])).items()}
    xg = torch.from_numpy(golden["xg"]).double()
    for layer, tap in ((0, 4), (3, 2)):           # at T = 331 layer 3 of period 5 has one output row: only taps 2, 3, 4 read data
        s, _ = DR.period_forward(sd, 2, xg, drop_tap=(layer, tap))
        assert not _close(s, golden["score/2"]), (layer, tap)
    s, _ = DR.period_forward(sd, 2, xg)
    assert _close(s, golden["score/2"])


def test_state_dict_keys_and_shapes_are_the_references(golden):
    from seq2seq_vc_amd.urhythmic.vocoder import MultiPeriodDiscriminator, PeriodDiscriminator
    mpd = MultiPeriodDiscriminator()
    sd = mpd.state_dict()
    want = [(str(k), tuple(int(v) for v in s.split(","))) for k, s in zip(golden["keys"], golden["shapes"])]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want == DR.state_dict_shapes()
    assert sum(int(np.prod(s)) for _, s in want) == sum(p.numel() for p in mpd.parameters())
    seeded = DR.seeded_state_dict(int(golden["seed"]))
    res = mpd.load_state_dict(seeded)
    assert not res.missing_keys and not res.unexpected_keys
    back = mpd.state_dict()
    assert all(torch.equal(back[k], seeded[k]) for k in seeded)
    assert [d.period for d in mpd.discriminators] == list(DR.PERIODS)
    one = PeriodDiscriminator(7)
    assert [n for n, _ in one.named_parameters()] == [k[len("discriminators.0."):] for k, _ in want[:18]]


def test_constructor_and_input_refusals():
    from seq2seq_vc_amd.urhythmic.vocoder import MultiPeriodDiscriminator, PeriodDiscriminator
    with pytest.raises(NotImplementedError):
        PeriodDiscriminator(2, use_spectral_norm=True)
    with pytest.raises(ValueError):
        PeriodDiscriminator(2, kernel_size=3)
    with pytest.raises(ValueError):
        PeriodDiscriminator(2, stride=2)
    d = PeriodDiscriminator(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d(torch.zeros(1, 1, 64))
    with pytest.raises(NotImplementedError, match="fp32 only"):
        d(torch.zeros(1, 1, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        d(torch.zeros(1, 64))
    mpd = MultiPeriodDiscriminator()
    with pytest.raises(RuntimeError, match="no CPU path"):
        mpd(torch.zeros(1, 1, 64))


def test_launch_plans_state_the_counts():
    from seq2seq_vc_amd.urhythmic import vocoder as V
    d = V.PeriodDiscriminator(5)
    fwd = d.launch_plan()
    assert [e["kind"] for e in fwd] == ["fold"] * 6 + ["input"] + ["conv"] * 4 + ["post"] and all(e["kind"] in V.KINDS for e in fwd)
    full, disc_step, no_params = d.backward_plan(need_dx=True), d.backward_plan(need_dx=False), d.backward_plan(need_dx=True, need_params=False)
    assert all(e["kind"] in V.BWD_KINDS for e in full)
    assert len(full) == len(disc_step) + 1 == 21 and full[-1]["kind"] == "input_dgrad"          # x.detach(): the first layer's data gradient is skipped
    assert [e["kind"] for e in no_params] == ["post_bwd"] + ["fold_bwd", "dgrad"] * 4 + ["input_dgrad"]
    assert [e["kind"] for e in disc_step].count("finish") == 6 and [e["kind"] for e in disc_step].count("dgrad") == 4
    mpd = V.MultiPeriodDiscriminator()
    assert len(mpd.launch_plan()) == 5 * len(fwd) == 60 and len(mpd.backward_plan(need_dx=True)) == 105
    assert sorted({e["period"] for e in mpd.launch_plan()}) == list(DR.PERIODS)


@pytest.mark.parametrize("T", [700, 331, 64, 23, 11])
@pytest.mark.parametrize("p", DR.PERIODS)
def test_length_chain_and_reflect_map_against_stock_torch(T, p):
    from seq2seq_vc_amd.ops import kernels_disc as KD
    from seq2seq_vc_amd.urhythmic.vocoder import layer_lengths
    x = torch.arange(T, dtype=torch.float32).view(1, 1, T)
    n_pad = (p - T % p) % p
    padded = F.pad(x, (0, n_pad), "reflect") if n_pad else x
    assert padded.reshape(-1).long().tolist() == DR.reflect_map(T, p) == [KD.reflect_index(t, T) for t in range(T + n_pad)]
    assert KD.folded_len(T, p) == (padded.shape[-1] // p, n_pad)
    h = padded.view(1, 1, -1, p)
    assert torch.equal(h, DR.folded(x, p))
    chain = [h.shape[2]]
    for s in DR.STRIDES:
        h = F.conv2d(h, torch.zeros(1, 1, 5, 1), stride=(s, 1), padding=(2, 0))
        chain.append(h.shape[2])
        assert h.shape[3] == p
    assert chain == DR.length_chain(T, p) == layer_lengths(T, p)
    assert all(KD.out_len(a, s) == b for a, b, s in zip(chain, chain[1:], DR.STRIDES))


def test_period_larger_than_the_input_is_refused():
    from seq2seq_vc_amd.ops import kernels_disc as KD
    with pytest.raises(ValueError):
        KD.folded_len(10, 11)


@pytest.mark.parametrize("L", [1, 2, 3, 7, 8, 9])
def test_phase_decomposed_data_gradient_and_its_plant(L):
    g = torch.Generator().manual_seed(L)
    cin, cout = 3, 4
    x = torch.randn(1, cin, L, dtype=torch.float64, generator=g).requires_grad_(True)
    w = torch.randn(cout, cin, 5, dtype=torch.float64, generator=g)
    y = F.conv1d(x, w, stride=3, padding=2)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    (dx,) = torch.autograd.grad(y, x, dy)
    got = DR.dgrad_phase_model(dy[0].t(), w, L)
    assert torch.allclose(got, dx[0].t(), atol=1e-12)
    if L > 1:
        assert not torch.allclose(DR.dgrad_phase_model(dy[0].t(), w, L, plant=True), dx[0].t(), atol=1e-6)


@pytest.mark.parametrize("T,p", [(23, 11), (34, 11), (10, 3), (12, 5), (700, 11), (331, 7), (64, 2)])
def test_dx_gather_mirror_term_and_its_plant(T, p):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, dtype=torch.float64, generator=g).requires_grad_(True)
    idx = torch.tensor(DR.reflect_map(T, p))
    gpad = torch.randn(len(idx), dtype=torch.float64, generator=g)
    (dx,) = torch.autograd.grad(x[idx], x, gpad)
    assert torch.allclose(DR.dx_gather_model(gpad, T), dx, atol=1e-12)
    if len(idx) > T:
        assert not torch.allclose(DR.dx_gather_model(gpad, T, mirror=False), dx, atol=1e-6)


@pytest.mark.parametrize("stride", [1, 3])
def test_flat_row_convolution_never_leaves_its_sequence_and_its_plant(stride):
    g = torch.Generator().manual_seed(stride)
    B, L, p, cin, cout = 2, 5, 3, 2, 3
    x = torch.randn(B, L, p, cin, dtype=torch.float64, generator=g)
    w = torch.randn(cout, cin, 5, dtype=torch.float64, generator=g)
    want = F.conv2d(x.permute(0, 3, 1, 2), w.unsqueeze(-1), stride=(stride, 1), padding=(2, 0)).permute(0, 2, 3, 1)
    assert torch.allclose(DR.flat_row_conv_model(x, w, stride), want, atol=1e-12)
    assert not torch.allclose(DR.flat_row_conv_model(x, w, stride, leak=True), want, atol=1e-6)


def test_header_sigs_exports_and_sources():
    import ctypes
    import os

    from seq2seq_vc_amd import _lib
    names = ["s2svc_hifigan_disc_input", "s2svc_hifigan_disc_conv", "s2svc_hifigan_disc_post", "s2svc_hifigan_disc_post_bwd",
             "s2svc_hifigan_disc_wgrad", "s2svc_hifigan_disc_dgrad", "s2svc_hifigan_disc_input_wgrad", "s2svc_hifigan_disc_input_dgrad"]
    assert "hifigan_disc.hip" in _lib.sources()
    assert set(names) <= set(_lib.exported_symbols())
    assert sorted(n for n in _lib.exported_symbols() if n.startswith("s2svc_hifigan_disc")) == sorted(names)
    i, f, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    assert _lib._FUNCTIONS["s2svc_hifigan_disc_conv"] == (i, [i] * 6 + [vp] * 3 + [f, vp, vp])
    assert _lib._FUNCTIONS["s2svc_hifigan_disc_input_dgrad"] == (i, [i] * 3 + [vp] * 4)
    header = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "s2svc_hip.h")).read()
    assert "replaces: urhythmic/vocoder.py:211-327" in header
    for n in names:                                      # every entry point carries its own `replaces:` comment
        decl = header.index("int " + n + "(")
        assert "replaces:" in header[header.rindex("/*", 0, decl):decl], n
    src = open(os.path.join(_lib.CSRC, "hifigan_disc.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and all(('extern "C" int ' + n + "(") in src for n in names)


def test_both_halves_share_one_node_body_and_one_handler_table():
    from seq2seq_vc_amd.urhythmic import vocoder as V
    assert V._PeriodFunction.__mro__[1] is V._ScaleFunction.__mro__[1] is V._DiscFunction
    assert "forward" not in vars(V._PeriodFunction) and "backward" not in vars(V._ScaleFunction)
    assert issubclass(V.PeriodDiscriminator, V._Discriminator) and issubclass(V.ScaleDiscriminator, V._Discriminator)
    assert set(V.PeriodDiscriminator._HANDLERS) == set(V.KINDS) | set(V.BWD_KINDS)
    assert set(V.ScaleDiscriminator._HANDLERS) == set(V.MSD_KINDS) | set(V.MSD_BWD_KINDS)
    shared = ("fold", "conv", "post", "post_bwd", "wgrad", "finish", "fold_bwd", "dgrad")
    assert set(V._Discriminator._HANDLERS) == set(shared)
    for kind in shared[1:]:                       # the scale half folds a spectrally normed weight itself
        assert V.PeriodDiscriminator._HANDLERS[kind] is V.ScaleDiscriminator._HANDLERS[kind] is V._Discriminator._HANDLERS[kind], kind
