"""CPU tests behind tests/gpu_hubert_check.py: the package's HubertSoft mirrors the yardstick's (= upstream's) state_dict, and the
identities the HIP path leans on -- the frame-count recursion, feature convolutions as strided-row GEMMs, the positional convolution as
16 conv-mode GEMMs, the dim = 2 weight-norm fold, online softmax, row-by-row batches -- hold against stock torch."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hubert_ref as HR  # noqa: E402
from seq2seq_vc_amd.urhythmic import hubert as PH  # noqa: E402

F64 = torch.float64


def test_state_dict_keys_and_shapes_equal_the_yardsticks_both_ways():
    yard, mine = HR.HubertSoft(), PH.HubertSoft()
    ky = {k: tuple(v.shape) for k, v in yard.state_dict().items()}
    km = {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    assert km == ky and len(ky) == 166
    mine.load_state_dict(yard.state_dict())
    yard.load_state_dict(mine.state_dict())
    assert all(torch.equal(v, mine.state_dict()[k]) for k, v in yard.state_dict().items())
    tiny_y, tiny_m = HR.HubertSoft(**HR.TINY), PH.HubertSoft(_width=128, _heads=2, _ffn=256, _layers=2)
    tiny_m.load_state_dict(tiny_y.state_dict())
    tiny_y.load_state_dict(tiny_m.state_dict())
    base_y, base_m = HR.Hubert(num_label_embeddings=7, mask=False), PH.Hubert(num_label_embeddings=7, mask=False)
    base_m.load_state_dict(base_y.state_dict())


def test_frame_count_equals_the_yardsticks_output_length():
    yard = HR.HubertSoft(conv_dim=2, width=64, heads=1, ffn=8, layers=1).eval()      # the lengths do not depend on the widths
    with torch.no_grad():
        for n in range(320, 2001):
            got = yard.feature_extractor(torch.zeros(1, 1, n + 2 * HR.PAD)).shape[2]
            assert PH.frame_count(n + 2 * HR.PAD) == got == HR.out_frames(yard, n + 2 * HR.PAD), n
    assert PH.frame_count(320 + 80) == 1 and PH.frame_count(319 + 80) == 0 and PH.frame_count(640 + 80) == 2


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
@pytest.mark.parametrize("L", [10, 11, 3, 4])
def test_strided_row_gemm_is_the_feature_convolution(k, s, L):
    """Channel-last rows with ld = s C against the tap-major weight (O, tap C + c): exact in a small-integer regime."""
    g = torch.Generator().manual_seed(k * 100 + L)
    C, O, B = 6, 5, 2
    x = torch.randint(-4, 5, (B, L, C), generator=g).to(F64)                        # channel-last
    w = torch.randint(-3, 4, (O, C, k), generator=g).to(F64)
    ref = F.conv1d(x.transpose(1, 2), w, stride=s).transpose(1, 2)                  # (B, Lo, O)
    Lo = (L - k) // s + 1
    assert ref.shape[1] == Lo
    wt = w.permute(0, 2, 1).reshape(O, k * C)
    rows = torch.as_strided(x, (B, Lo, k * C), (L * C, s * C, 1))
    assert torch.equal(rows @ wt.t(), ref)


@pytest.mark.parametrize("L", [1, 63, 64, 65, 200])
def test_positional_convolution_is_16_conv_mode_gemms(L):
    """Row t of group g reads taps j at frame t + j - 64 (zero outside 0 .. L - 1): F.conv1d(padding=64, groups=16) without its last frame."""
    g = torch.Generator().manual_seed(L)
    W, G, Kt, B = 32, 16, 128, 2
    Cg = W // G
    x = torch.randint(-3, 4, (B, L, W), generator=g).to(F64)
    w = torch.randint(-2, 3, (W, Cg, Kt), generator=g).to(F64)
    ref = F.conv1d(x.transpose(1, 2), w, padding=64, groups=G)[..., :-1].transpose(1, 2)
    wt = w.permute(0, 2, 1).reshape(W, Kt * Cg)                                     # (O, tap Cg + c)
    out = torch.empty(B, L, W, dtype=F64)
    xp = F.pad(x, (0, 0, 64, 63))                                                   # frames -64 .. L + 62
    for gi in range(G):
        a = xp[:, :, gi * Cg:(gi + 1) * Cg].unfold(1, Kt, 1).permute(0, 1, 3, 2).reshape(B, L, Kt * Cg)   # (b, t, tap Cg + c)
        out[:, :, gi * Cg:(gi + 1) * Cg] = a @ wt[gi * Cg:(gi + 1) * Cg].t()
    assert torch.equal(out, ref)


def test_weight_norm_fold_equals_torchs():
    yard = HR.seeded(3, **HR.TINY)
    mine = PH.HubertSoft(_width=128, _heads=2, _ffn=256, _layers=2)
    mine.load_state_dict(yard.state_dict())
    conv = yard.positional_embedding.conv
    with torch.no_grad():
        conv(torch.zeros(1, 128, 4))                                                # the hook recomputes conv.weight
        want = torch._weight_norm(conv.weight_v, conv.weight_g, 2)
        got = mine.fold_positional_weight()
    assert got.shape == want.shape == (128, 8, 128)
    assert torch.allclose(got, want, rtol=1e-6, atol=0) and torch.allclose(got, conv.weight, rtol=1e-6, atol=0)
    with torch.no_grad():
        g64 = mine.double().fold_positional_weight()
        assert torch.allclose(g64, torch._weight_norm(conv.weight_v.double(), conv.weight_g.double(), 2), rtol=1e-14, atol=0)


@pytest.mark.parametrize("T,tile", [(1, 64), (63, 64), (64, 64), (65, 64), (129, 64), (200, 16)])
def test_online_softmax_equals_plain_attention(T, tile):
    H, dk, B = 2, 8, 3
    q = torch.randn(B, T, H * dk, dtype=F64, generator=torch.Generator().manual_seed(T)) * 3
    k = torch.randn(B, T, H * dk, dtype=F64, generator=torch.Generator().manual_seed(T + 1))
    v = torch.randn(B, T, H * dk, dtype=F64, generator=torch.Generator().manual_seed(T + 2))
    k[0, T - 1] = q[0, 0] * 4                                                       # a dominant key in the last tile: the rescale fires
    for klen in (None, [T, max(1, T - 5), 1], [0, T + 3, max(1, T // 2)]):
        a = HR.attention_plain(q, k, v, klen, 1 / math.sqrt(dk), H, F64)
        b = HR.attention_online(q, k, v, klen, 1 / math.sqrt(dk), H, F64, tile=tile)
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-13)
        if klen is not None:
            for i, n in enumerate(klen):
                assert not a[i, n:].any() and not b[i, n:].any()


def test_ragged_restatement_equals_single_calls():
    yard = HR.seeded(5, dtype=F64, **HR.TINY)
    g = torch.Generator().manual_seed(9)
    lens = [1700, 320, 999]
    wavs = torch.randn(3, 1, max(lens), generator=g, dtype=F64)
    units, log_probs, frame_lens = HR.ragged(yard, wavs, lens)
    assert frame_lens == [PH.frame_count(n + 80) for n in lens] == [5, 1, 3]
    for b, n in enumerate(lens):
        u1, lp1 = HR.encode(yard, wavs[b:b + 1, :, :n])
        assert torch.equal(units[b:b + 1, :, :frame_lens[b]], u1) and torch.equal(log_probs[b:b + 1, :frame_lens[b]], lp1)
        assert not units[b, :, frame_lens[b]:].any() and not log_probs[b, frame_lens[b]:].any()
    wavs2 = wavs.clone()
    wavs2[1, :, 320:] = float("nan")
    u2, lp2, _ = HR.ragged(yard, wavs2, lens)
    assert torch.equal(u2, units) and torch.equal(lp2, log_probs)


def test_layer0_and_log_prob_restatements_match_the_modules():
    yard = HR.seeded(7, dtype=F64, **HR.TINY)
    fe = yard.feature_extractor
    g = torch.Generator().manual_seed(1)
    wav = torch.randn(2, 900, generator=g, dtype=F64)
    with torch.no_grad():
        got = HR.layer0(wav, [900, 500], fe.conv0.weight, fe.norm0.weight, fe.norm0.bias, F64)
        want = F.gelu(fe.norm0(fe.conv0(F.pad(wav[1:2, None, :500], (HR.PAD, HR.PAD)))))[0].t()
        assert torch.equal(got[1, :want.shape[0]], want) and not got[1, want.shape[0]:].any()
        u = torch.randn(2, 5, 256, generator=g, dtype=F64)
        u[0, 2] = 0
        lp = HR.log_probs(u, yard.label_embedding.weight, F64, lens=[5, 3])
        assert torch.equal(lp[0], F.log_softmax(yard.logits(u[0:1]), dim=-1)[0]) and not lp[1, 3:].any()
        assert torch.allclose(lp[0, 2].exp(), torch.full((100,), 0.01, dtype=F64))   # an all-zero unit row: cosine 0 for every unit


def test_inference_only_and_argument_checks():
    m = PH.HubertSoft(_width=128, _heads=2, _ffn=256, _layers=2)
    with pytest.raises(NotImplementedError):
        m.units(torch.zeros(1, 1, 400))                                            # train() mode
    m.eval()
    with pytest.raises(NotImplementedError):
        m.units(torch.zeros(1, 1, 400))                                            # a CPU tensor
    with pytest.raises(NotImplementedError):
        m.encode(torch.zeros(1, 1, 400))                                           # grad enabled
    with pytest.raises(ValueError):
        PH.Hubert(_width=96, _heads=2)
    plan = PH.HubertSoft().launch_plan("model.encode", batched=True, dtype=torch.bfloat16)
    assert len(plan) == 2 + 6 + 2 + 1 + 16 + 1 + 12 * 7 + 1 + 1 + 1 + 1 and plan.count("attn_flash_fwd") == 12
    assert len(PH.HubertSoft().launch_plan("units", dtype=torch.float32)) == 2 + 6 + 2 + 16 + 1 + 12 * 7 + 1
