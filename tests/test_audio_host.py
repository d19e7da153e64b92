"""CPU tests behind tests/gpu_audio_check.py: the float64 restatements of tests/audio_ref.py are checked against each other (the banded
form the kernel implements against the dense form torchaudio states), against closed forms (the length formula, a tone, hand-built
trims) and the conditions the GPU cases rely on are asserted on the very arrays they use.  The package's host code (the tap table, the
length formula, the argument checks) is held to the restatements.  No kernel runs here."""
import math

import numpy as np
import pytest
import torch

import audio_ref as AR
from seq2seq_vc_amd import audio
from seq2seq_vc_amd.ops import kernels_audio as KA

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def tables():
    return {(o, n): AR.band_of(o, n) for o, n in AR.RATIOS}


def test_banded_equals_dense_on_every_gpu_input(tables):
    """The two forms differ by the dropped taps alone: (1) every kept tap is the dense tap, bit for bit; (2) what the dropped taps
    contribute -- the dense convolution with the kept taps zeroed -- is at most 1e-30 max|x| on every resample input of the GPU cases.
    The two float64 sums themselves add different numbers of terms, so they also differ by float64 rounding (~1e-16 |x|), far above
    1e-30: (3) bounds that by 1e-13 max|x|, and is what makes the banded form a float64 reference for the kernel."""
    worst = 0.0
    for orig, new, rows, kind in AR.resample_inputs():
        band, first, width, inside = tables[(orig, new)]
        _, taps, _ = AR.dense_kernel(orig, new)
        for p in range(new):
            n = int(inside[p].sum())
            assert torch.equal(band[:n, p], taps[p, first[p]:first[p] + n]) and not band[n:, p].any()
            assert bool(inside[p, first[p]:first[p] + n].all()) and int(inside[p].sum()) == n            # the band is one run
        dropped = torch.where(inside, torch.zeros_like(taps), taps)
        for x in rows:
            if x.numel() == 0:
                continue
            mx = float(x.abs().max())
            rest = AR.dense_resample(x, orig, new, dropped, width)
            assert float(rest.abs().max()) <= 1e-30 * mx, (orig, new, x.numel(), float(rest.abs().max()))
            worst = max(worst, float(rest.abs().max()) / mx if mx else 0.0)
            d = AR.dense_resample(x, orig, new, taps, width) - AR.banded_resample(x, orig, new, band, first, width)
            assert d.numel() == AR.out_length(x.numel(), orig, new) and float(d.abs().max()) <= 1e-13 * mx
    print(f"dropped taps contribute at most {worst:.3e} max|x|")


def test_issue_table_of_band_widths(tables):
    got = {(o, n): (tables[(o, n)][2], 2 * tables[(o, n)][2] + o, tables[(o, n)][0].shape[0]) for o, n in AR.RATIOS}
    assert got[(3, 1)] == (19, 41, 37) and got[(3, 2)] == (10, 23, 19) and got[(441, 320)] == (9, 459, 17)
    assert got[(441, 160)] == (17, 475, 34) and got[(2, 3)] == (7, 16, 13) and got[(1, 2)] == (7, 15, 13)


def test_length_formula():
    for orig, new in AR.RATIOS:
        for L in (0, 1, 2, orig - 1, orig, orig + 1, 1000, 19999, 2**31 - 1):
            if L < 0:
                continue
            want = (new * L + orig - 1) // orig
            assert KA.out_length(L, orig, new) == want
            if L < 10**6:
                assert AR.out_length(L, orig, new) == want and AR.dense_resample(torch.zeros(L), orig, new).numel() == want
    assert KA.out_length(1000, 441, 320) == 726 and (320 * 1000) // 441 == 725                        # ceil != floor
    assert KA.reduced(22050, 16000) == (441, 320) and KA.reduced(48000, 16000) == (3, 1)
    for orig, new in AR.RATIOS:                                                                       # the exact regime holds such a row
        if orig > 1:
            assert any((new * L) % orig for L in AR.exact_lengths(orig, new, AR.band_of(orig, new)[2]))


def test_same_rate_is_the_identity():
    x = torch.randn(100, generator=AR.gen(1))
    assert torch.equal(AR.dense_resample(x, 16000, 16000), x.double())
    assert audio.launch_plan("resample", orig_freq=16000, new_freq=16000) == []
    assert audio.launch_plan("resample", orig_freq=48000, new_freq=16000) == ["s2svc_resample_poly"]


def test_dc_gain_per_phase(tables):
    """Every phase's taps add up to the DC gain of the dense form: the two forms against each other, not against a constant."""
    for (orig, new), (band, first, width, inside) in tables.items():
        _, taps, _ = AR.dense_kernel(orig, new)
        for p in range(new):
            assert abs(float(band[:, p].sum()) - float(taps[p].sum())) <= 1e-12
            assert abs(float(taps[p][~inside[p]].sum())) <= 1e-30


def test_package_table_is_the_restatement(tables):
    """ops.kernels_audio.banded_taps (numpy) against band_of (torch, phase by phase): the same first taps and band length, taps equal
    to one fp32 ulp (two float64 libms may round a sine differently; one float64 ulp moves a fp32 rounding by at most one fp32 ulp)."""
    for (orig, new), (band, first, width, _) in tables.items():
        taps, f, o, n, w = KA.banded_taps(orig * 50, new * 50)
        assert (o, n, w) == (orig, new, width) and f.tolist() == first and taps.shape == tuple(band.shape) and taps.dtype == np.float32
        got, want = torch.from_numpy(taps), band.to(F32)
        ulp = torch.nextafter(want.abs(), torch.tensor(float("inf"))) - want.abs()
        assert bool(((got - want).abs() <= ulp).all()) and bool(((got == 0) == (want == 0)).all())


def test_tone_48k_to_16k_lands_on_the_analytic_tone(tables):
    """A 1 kHz tone: the resampled tone against sin(2 pi 1000 m / 16000), away from the edges (width / orig outputs on either side).
    The dense float64 restatement's own distance from the tone (the filter's pass-band error) is the yardstick, doubled."""
    n = torch.arange(12000, dtype=F64)
    x = torch.sin(2 * math.pi * 1000.0 * n / 48000.0).to(F32)
    m = torch.arange(4000, dtype=F64)
    want = torch.sin(2 * math.pi * 1000.0 * m / 16000.0)
    e_dense = float((AR.dense_resample(x, 48000, 16000) - want)[50:-50].abs().max())
    taps, first, orig, new, width = KA.banded_taps(48000, 16000)
    got = AR.banded_resample(x, orig, new, torch.from_numpy(taps).double(), first.tolist(), width)
    e_band = float((got - want)[50:-50].abs().max())
    print(f"1 kHz, 48 -> 16 kHz: dense float64 restatement {e_dense:.3e} from the analytic tone, banded (package table) {e_band:.3e}")
    assert 0 < e_dense < 1e-2 and e_band <= 2 * e_dense


def test_exact_regime_inputs_are_exact_in_fp32():
    """Integer taps in [-4, 4] and samples in [-8, 8]: a sum of Kb <= 37 products stays below 2^24, so fp32 makes no rounding."""
    for i, (orig, new) in enumerate(AR.RATIOS):
        band, first, width, rows = AR.exact_case(orig, new, 7100 + i)
        assert band.shape[0] * 32 < 2**24 and bool((band == band.round()).all())
        lens = [r.numel() for r in rows]
        assert {1, width - 1, width, width + 1, orig, orig + 1} <= set(lens) and max(lens) <= 20000
        outs = [AR.out_length(L, orig, new) for L in lens]
        assert any(o <= AR.TILE for o in outs) and any(o > AR.TILE for o in outs)
        for r in rows[:3]:
            assert torch.equal(AR.banded_resample(r, orig, new, band, first, width, F32).double(), AR.banded_resample(r, orig, new, band, first, width, F64))


# ---------------------------------------------------------------------------------------------------------------------------
# trim
# ---------------------------------------------------------------------------------------------------------------------------
def test_trim_on_hand_built_inputs():
    fl, hop = 2048, 512
    y = np.zeros(8192, np.float32)
    y[2048:5120] = 0.5
    # frame i covers [512 i - 1024, 512 i + 1024): it touches the burst for 3 <= i <= 11 (i = 2 ends at 2048, i = 12 starts at 5120)
    for mode in AR.PAD_MODES:
        assert AR.trim(y, 60, fl, hop, mode) == (3 * hop, 12 * hop)
    y[2047] = 0.5                                                   # one sample earlier: frame 2 hears it
    assert AR.trim(y, 60, fl, hop) == (2 * hop, 12 * hop)
    y[5120] = 0.5                                                   # one sample later: frame 12 does
    assert AR.trim(y, 60, fl, hop) == (2 * hop, 13 * hop)
    assert AR.trim(np.zeros(5000, np.float32), 60, fl, hop) == (0, 5000)           # every frame ties at the floor: nothing is silent
    assert AR.trim(np.full(4000, 0.5, np.float32), 60, fl, hop) == (0, 4000)
    assert AR.trim(y, 0, fl, hop) == (0, 0)                                        # nothing is louder than the loudest frame
    assert AR.trim(np.zeros(0, np.float32), 60, fl, hop) == (0, 5000 * 0)
    z = np.zeros(300, np.float32)
    z[100:200] = 0.5
    assert AR.trim(z, 60, fl, hop) == (0, 300)                                     # L < hop: one frame
    # reflect: a burst at the very start is heard again in the padding; the frame count is the same
    assert len(AR.frame_powers(y, fl, hop, "reflect")) == len(AR.frame_powers(y, fl, hop, "constant")) == 17
    e = np.zeros(4096, np.float32)
    e[1:65] = 0.5
    pc, pr = AR.frame_powers(e, fl, hop, "constant"), AR.frame_powers(e, fl, hop, "reflect")
    assert pr[0] == 2 * pc[0] and pr[3] == pc[3]


def test_trim_margin_on_every_gpu_input():
    """No frame of any trim input of the GPU cases lies within 1e-3 dB of the threshold, so the interval has one right answer whatever
    the order of the power sums.  top_db = 0 is the exception by construction: the loudest frame sits ON the threshold, and `>` is
    false for it and for every other frame in either form (x > x, and p_i <= p_max), so the answer is (0, 0) without a margin."""
    smallest = float("inf")
    for name, c in AR.trim_cases().items():
        for mode in AR.PAD_MODES:
            for y in c["rows"]:
                assert y.dtype == np.float32 and len(y) <= 20000
                db = AR.frame_db(y, c["frame_length"], c["hop_length"], mode)
                assert len(db) == 1 + len(y) // c["hop_length"] and db.max() == 0.0
                if c["top_db"] == 0:
                    assert AR.trim(y, 0, c["frame_length"], c["hop_length"], mode) == (0, 0)
                    continue
                margin = float(np.abs(db + c["top_db"]).min())
                smallest = min(smallest, margin)
                assert margin > 1e-3, (name, mode, margin)
    print(f"smallest distance of a frame from the threshold: {smallest:.4f} dB")
    c = AR.trim_cases()
    loud, quiet = c["zeros_constant_loud_quiet"]["rows"][2:]
    assert AR.trim(loud, 60, 2048, 512) != AR.trim(quiet, 60, 2048, 512) and AR.trim(np.concatenate([loud, quiet]), 60, 2048, 512)[1] < len(loud) + 1
    assert any(len(y) % c["short_rows"]["hop_length"] for y in c["short_rows"]["rows"])
    edges = [AR.trim(y, 60, 2048, 512) for y in c["burst_edges"]["rows"]]
    assert edges[0] == (3 * 512, 12 * 512) and len(set(edges)) >= 3


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks of the package, all before any device work
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    for bad in ((0, 16000), (16000, -1), (44100.5, 16000)):
        with pytest.raises(ValueError):
            KA.reduced(*bad)
    with pytest.raises(ValueError, match="cap"):                                   # one workgroup would stage 1024 x 48 samples
        KA.poly_table(48000, 1000, "cpu")
    with pytest.raises(ValueError, match="cap"):                                   # a table of more than 2^20 taps
        KA.make_table(np.zeros((1025, 1024), np.float32), np.zeros(1024, np.int32), 1, 1024, 7, "cpu")
    with pytest.raises(ValueError):                                                # first tap outside the dense kernel
        KA.make_table(np.zeros((3, 2), np.float32), np.array([0, 40], np.int32), 3, 2, 10, "cpu")
    table = KA.PolyTable(None, None, 3, 1, 19, 37, 0, 2)
    with pytest.raises(ValueError, match="2\\^31"):
        KA.resample_poly(torch.empty(1, 2**31, device="meta"), [5], table)
    with pytest.raises(ValueError, match="2\\^31"):                                # 2^31 - 1 samples at 1 -> 2 make 2^32 - 2 outputs
        KA.resample_poly(torch.empty(1, 2**31 - 1, device="meta"), [2**31 - 1], KA.PolyTable(None, None, 1, 2, 7, 13, 0, 1))
    with pytest.raises(ValueError):
        KA.resample_poly(torch.zeros(2, 10), [10, 11], table)                      # a length beyond the row
    with pytest.raises(ValueError):
        KA.resample_poly(torch.zeros(2, 10, dtype=torch.float64), [10, 10], table)
    for bad in (dict(top_db=-1), dict(frame_length=0), dict(hop_length=0), dict(hop_length=1.5), dict(pad_mode="edge")):
        kw = dict(dict(top_db=60, frame_length=2048, hop_length=512, pad_mode="constant"), **bad)
        with pytest.raises(ValueError):
            KA.check_trim_args(**kw)
    with pytest.raises(ValueError):
        audio.resample_batch(torch.zeros(2, 10), [10, 10], 48000, 16000)            # (B, 1, N) expected
    with pytest.raises(ValueError):
        audio.trim_batch(torch.zeros(2, 1, 10, dtype=torch.float64), [10, 10])
    with pytest.raises(RuntimeError):
        audio.resample_batch(torch.zeros(2, 1, 10), [10, 10], 48000, 16000)         # there is no CPU path
    with pytest.raises(ValueError):
        audio._trim_keys(dict(top_db=60))
    cfg = dict(sampling_rate=16000, trim_silence=True, trim_threshold_in_db=60, trim_frame_size=2048, trim_hop_size=512, global_gain_scale=0.5)
    assert audio.launch_plan("condition", fs=48000, config=cfg) == ["s2svc_resample_poly", "s2svc_trim_frames", "s2svc_trim_intervals", "s2svc_wav_gather_rows"]
    assert audio.launch_plan("condition", fs=16000, config=dict(cfg, trim_silence=False)) == ["s2svc_wav_gather_rows"]
    assert audio.launch_plan("condition", fs=16000, config=dict(sampling_rate=16000, trim_silence=False)) == []
    assert audio.launch_plan("trim") == ["s2svc_trim_frames", "s2svc_trim_intervals", "s2svc_wav_gather_rows"]
    assert KA.TILE == AR.TILE
