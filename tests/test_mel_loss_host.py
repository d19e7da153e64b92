"""CPU tests behind tests/gpu_mel_loss_check.py: the public interface of LogMelSpectrogram and its refusals, the filterbank and its
segment tables, the conditions the GPU cases rely on asserted on the very inputs they use, the power of the comparison rule against
planted errors, and the ABI ledger.  None of this launches a kernel."""
import inspect

import numpy as np
import pytest
import torch

import mel_loss_ref as MR
import step_kernels_ref as R
from oracle import logmel as OL

F32, F64 = torch.float32, torch.float64


# ---- 1. interface -------------------------------------------------------------------------------------------------------------
def test_import_path_and_constructor():
    from seq2seq_vc_amd.urhythmic import LogMelSpectrogram as A
    from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram as B
    assert A is B and issubclass(B, torch.nn.Module)
    sig = inspect.signature(B.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("sample_rate", 16000), ("n_fft", 1024), ("win_length", 1024), ("hop_length", 320), ("n_mels", 80)]
    m = B()
    assert m.pad == 352 and callable(m.l1_loss)
    assert B(22050, 1024, 1024, 256, 40).pad == 384


def test_refusals():
    from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram
    for kw in (dict(n_fft=512, win_length=512), dict(n_fft=2048, win_length=2048), dict(win_length=800), dict(n_mels=129)):
        with pytest.raises(NotImplementedError):
            LogMelSpectrogram(**kw)
    m = LogMelSpectrogram()
    with pytest.raises(ValueError):
        m(torch.zeros(2, 1, 352))                      # N <= pad: torch's reflect pad refuses that too
    with pytest.raises(ValueError):
        m(torch.zeros(2, 352))
    with pytest.raises(ValueError):
        LogMelSpectrogram(hop_length=1000)(torch.zeros(1, 900))      # pad 12: 924 padded samples do not fill a frame, T < 1
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 1, 8320))                     # CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        m.l1_loss(torch.zeros(2, 1, 8320), torch.zeros(2, 1, 80, 26))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 1, 8320, dtype=torch.float64))
    with pytest.raises(ValueError):
        m.l1_loss(torch.zeros(2, 1, 8320), torch.zeros(2, 1, 80, 25))


def test_a_filterbank_without_the_two_neighbour_property_is_refused(monkeypatch):
    from seq2seq_vc_amd.ops import kernels_melspec as KM
    from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram
    real = KM.mel_filterbank

    def three_per_bin(*a, **kw):
        fb = real(*a, **kw)
        fb[100, 5] = 0.25                              # a third filter at a bin that filters ~20 cover
        return fb
    assert np.count_nonzero(real(16000, 1024, 80)[100]) == 2
    monkeypatch.setattr(KM, "mel_filterbank", three_per_bin)
    with pytest.raises(NotImplementedError):
        LogMelSpectrogram()


def test_output_shapes():
    from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram
    for name, (B, N, cfg, T, _, _) in MR.CASES.items():
        m = LogMelSpectrogram(**cfg)
        assert m.output_shape((B, 1, N)) == (B, 1, cfg["n_mels"], T), name
        assert m.output_shape((B, N)) == (B, cfg["n_mels"], T), name
        assert tuple(MR.inputs(name)["tgt"].shape) == (B, cfg["n_mels"], T)
    assert LogMelSpectrogram().output_shape((1, 64000)) == (1, 80, 200)
    with pytest.raises(ValueError):
        LogMelSpectrogram().output_shape((2, 2, 8320))


# ---- 2. the filterbank --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [MR.DEFAULT, MR.OTHER], ids=["default", "other"])
def test_filterbank_and_segment_tables(cfg):
    from seq2seq_vc_amd.ops import kernels_melspec as KM
    sr, n_fft, n_mels = cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"]
    fb = KM.mel_filterbank(sr, n_fft, n_mels)
    assert fb.dtype == np.float64 and fb.shape == (n_fft // 2 + 1, n_mels)
    assert np.array_equal(fb, OL.mel_filterbank64(sr, n_fft, n_mels, 0, sr / 2).T)             # exactly, in float64
    for k in range(fb.shape[0]):
        nz = np.nonzero(fb[k])[0]
        assert len(nz) <= 2 and (len(nz) < 2 or nz[1] == nz[0] + 1), (k, nz)
    for basis in (fb, fb.astype(np.float32)):
        seg_lo, seg_len, wud, bin_seg = KM.segment_tables(basis)
        assert wud.dtype == basis.dtype and int((seg_lo + seg_len).max()) <= n_fft // 2 + 1 and int(seg_len.sum()) <= n_fft // 2 + 1
        assert int(bin_seg.min()) >= 0 and int(bin_seg.max()) <= n_mels
        assert np.array_equal(KM.dense_from_segments(seg_lo, seg_len, wud, n_mels), basis)
        # the product by segments, in the kernel's order (each side of a filter summed over ascending bins, then the two sides added),
        # against the dense basis summed in that same order: bit for bit in float64
        mag = np.abs(np.random.default_rng(0).standard_normal((2, n_fft // 2 + 1)))
        w64, b64 = wud.astype(np.float64), basis.astype(np.float64)
        for r in range(2):
            up, dn = np.zeros(n_mels + 1), np.zeros(n_mels + 1)
            for s_ in range(n_mels + 1):
                for k in range(seg_lo[s_], seg_lo[s_] + seg_len[s_]):
                    up[s_] += w64[k, 0] * mag[r, k]
                    dn[s_] += w64[k, 1] * mag[r, k]
            dense = np.zeros(n_mels)
            for m in range(n_mels):
                rise, fall = 0.0, 0.0
                for k in range(seg_lo[m], seg_lo[m] + seg_len[m]):
                    rise += b64[k, m] * mag[r, k]
                for k in range(seg_lo[m + 1], seg_lo[m + 1] + seg_len[m + 1]):
                    fall += b64[k, m] * mag[r, k]
                dense[m] = rise + fall
                covered = set(range(seg_lo[m], seg_lo[m] + seg_len[m])) | set(range(seg_lo[m + 1], seg_lo[m + 1] + seg_len[m + 1]))
                assert set(np.nonzero(b64[:, m])[0]) <= covered                   # no weight of the filter lies outside its two segments
            assert np.array_equal(up[:n_mels] + dn[1:], dense)
        # every bin's segment is the one that holds it
        for k in range(basis.shape[0]):
            if wud[k].any():
                assert seg_lo[bin_seg[k]] <= k < seg_lo[bin_seg[k]] + seg_len[bin_seg[k]]
    # a basis with three filters at one bin has no segment form
    bad = fb.copy()
    bad[100, 5] = 0.25
    assert KM.segment_tables(bad) is None


# ---- 3. the inputs of the GPU cases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MR.CASES))
def test_input_conditions(name):
    B, N, cfg, T, tails, clamped = MR.CASES[name]
    inp, ref = MR.inputs(name), MR.reference(name)
    ml = ref["mel64"]
    assert tuple(ml.shape) == (B, cfg["n_mels"], T)
    assert float(((ml - MR.EPS).abs() / MR.EPS).min()) >= 0.01                   # no mel within 1 % of the clamp value
    assert int((ml < MR.EPS).sum()) == clamped
    lm64, lm32 = ref["logmel"]
    assert float((lm64 - inp["tgt"].double()).abs().min()) >= 0.04               # no element near a sign flip of logmel - tgt
    for key in ("logmel", "dwav", "dwav_l1"):
        r64, yard = ref[key]
        assert yard.dtype == F32 and r64.dtype == F64 and float((yard.double() - r64).abs().max()) > 0, key
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(yard).all()), key
    for row, (start, factor) in tails.items():
        assert bool((inp["wav"][row, :start] != 0).any())
        if factor == 0:                                                          # wholly silent frames: 80 clamped mels each, |X| = 0
            assert bool((inp["wav"][row, start:] == 0).all()) and int((ml == 0).all(dim=1).sum()) * cfg["n_mels"] == clamped
        else:                                                                    # clamped, but with a spectrum: 0 < mel < 1e-7
            assert int(((ml > 0) & (ml < 1e-7)).all(dim=1).sum()) * cfg["n_mels"] == clamped and not bool((ml == 0).any())
    assert MR.loss_bound(name) > 0


def test_explicit_backward_equals_autograd_in_float64():
    """The hand-written chain (the semantics the kernels implement) against torch autograd on the restatement."""
    for name in MR.CASES:
        inp, ref = MR.inputs(name), MR.reference(name)
        lm, _, dw = MR.explicit(inp["wav"], F64, g_logmel=inp["g_logmel"], **inp["cfg"])
        assert float((lm - ref["logmel"][0]).abs().max()) <= 1e-12
        assert float((dw - ref["dwav"][0]).abs().max()) <= 1e-12 * max(1.0, float(ref["dwav"][0].abs().max()))
        _, loss, dwl = MR.explicit(inp["wav"], F64, tgt=inp["tgt"], **inp["cfg"])
        assert abs(float(loss) - float(ref["loss"][0])) <= 1e-12
        assert float((dwl - ref["dwav_l1"][0]).abs().max()) <= 1e-14
        ok = R.compare(dw, ref["dwav"][0], ref["dwav"][1], F32)[0] and R.compare(dwl, ref["dwav_l1"][0], ref["dwav_l1"][1], F32)[0]
        assert ok, name                                                          # and the rule accepts the unplanted chain


# ---- 4. power of the rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", MR.PLANTS)
def test_planted_errors_are_rejected(plant):
    rejected = []
    for name in MR.CASES:
        inp, ref = MR.inputs(name), MR.reference(name)
        if plant == "hop256" and inp["cfg"]["hop_length"] == 256:
            continue
        lm, _, dw = MR.explicit(inp["wav"], F64, g_logmel=inp["g_logmel"], plant=plant, **inp["cfg"])
        _, loss, dwl = MR.explicit(inp["wav"], F64, tgt=inp["tgt"], plant=plant, **inp["cfg"])
        verdicts = [R.compare(lm, *ref["logmel"], F32)[0], R.compare(dw, *ref["dwav"], F32)[0], R.compare(dwl, *ref["dwav_l1"], F32)[0],
                    abs(float(loss) - float(ref["loss"][0])) <= MR.loss_bound(name)]
        if not all(verdicts):
            rejected.append(name)
    assert rejected, f"the planted error {plant} passes the rule on every case"
    if plant == "nan_phase":
        assert "silence" in rejected and "finetune" in rejected
    if plant == "no_clamp_mask":
        assert rejected == ["quiet_frame"]             # |X| = 0 hides it in the silent frames


# ---- 5. the ledger ------------------------------------------------------------------------------------------------------------
def test_header_sigs_exports_and_sources():
    import abi_header
    from seq2seq_vc_amd import _lib
    new = ["s2svc_melspec_supported", "s2svc_melspec_fwd", "s2svc_melspec_loss_finish", "s2svc_melspec_bwd_frames", "s2svc_melspec_bwd_ola"]
    header, L = abi_header.text(), abi_header.library()
    assert "melspec.hip" in _lib.sources()
    for sym in new:
        assert (sym + "(") in header and sym in _lib._FUNCTIONS and hasattr(L, sym), sym
    assert "urhythmic/dataset.py:23-50" in header
    assert L.s2svc_melspec_supported(1024, 1024, 80) == 1 and L.s2svc_melspec_supported(1024, 1024, 128) == 1
    assert L.s2svc_melspec_supported(512, 512, 80) == 0 and L.s2svc_melspec_supported(1024, 800, 80) == 0
    assert L.s2svc_melspec_supported(1024, 1024, 129) == 0 and L.s2svc_melspec_supported(1024, 1024, 0) == 0
