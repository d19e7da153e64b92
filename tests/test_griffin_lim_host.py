"""Host-side checks of the Griffin-Lim vocoder (no GPU): the test-side restatement against torch.stft / torch.istft, the surface of
Spectrogram2Waveform against literal expectations from the reference file, the cached pseudo-inverse, the refusals and the C ABI."""
import importlib
import inspect

import numpy as np
import pytest
import torch

import griffin_lim_ref as GR

GEOMETRIES = [(512, 128, None), (1024, 256, None), (2048, 300, 1200), (2048, 512, None)]


def _torch_window(wl):
    return torch.hann_window(wl, periodic=True, dtype=torch.float64)


@pytest.mark.parametrize("n_fft,hop,wl", GEOMETRIES)
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_restated_stft_is_torch_stft(n_fft, hop, wl, pad_mode):
    y = GR.make_signal(0.5, 16000, seed=1)
    got = GR.stft(y, n_fft, hop, wl, pad_mode)
    w = n_fft if wl is None else wl
    want = torch.stft(torch.from_numpy(y), n_fft, hop, w, _torch_window(w), center=True, pad_mode=pad_mode, return_complex=True).numpy().T
    assert got.shape == want.shape == (1 + len(y) // hop, n_fft // 2 + 1)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"stft {n_fft}/{hop}/{wl} {pad_mode}: relative to max {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("n_fft,hop,wl", GEOMETRIES)
def test_restated_istft_is_torch_istft(n_fft, hop, wl):
    rng = np.random.default_rng(2)
    T = 19
    X = rng.standard_normal((T, n_fft // 2 + 1)) + 1j * rng.standard_normal((T, n_fft // 2 + 1))
    X[:, 0], X[:, -1] = X[:, 0].real, X[:, -1].real          # torch.istft checks nothing here; numpy's irfft ignores these parts
    got = GR.istft(X, n_fft, hop, wl)
    w = n_fft if wl is None else wl
    want = torch.istft(torch.from_numpy(X.T.copy()), n_fft, hop, w, _torch_window(w), center=True, length=hop * (T - 1)).numpy()
    assert got.shape == want.shape == (hop * (T - 1),)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"istft {n_fft}/{hop}/{wl}: relative to max {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("n_fft,hop,wl", GEOMETRIES)
def test_istft_inverts_stft_on_the_interior(n_fft, hop, wl):
    y = GR.make_signal(0.5, 16000, seed=3)
    back = GR.istft(GR.stft(y, n_fft, hop, wl, "constant"), n_fft, hop, wl)
    n = len(back)
    assert n == hop * (len(y) // hop)
    lo, hi = n_fft, n - n_fft                                 # away from the zero padding's edge effect
    assert np.abs(back[lo:hi] - y[lo:hi]).max() < 1e-12


def test_float32_leg_of_the_restatement_is_a_float32_computation():
    y = GR.make_signal(0.3, 16000, seed=4)
    X32 = GR.stft(y, 1024, 256, None, "constant", np.float32)
    assert X32.dtype == np.complex64 and GR.istft(X32, 1024, 256, None, np.float32).dtype == np.float32
    d = np.abs(X32 - GR.stft(y, 1024, 256)).max()
    assert 0 < d < 1e-3


def test_spectrogram2waveform_surface_matches_the_reference():
    from seq2seq_vc_amd.vocoder import Spectrogram2Waveform, griffin_lim, logmel2linear
    sig = inspect.signature(Spectrogram2Waveform.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [
        ("n_fft", inspect.Parameter.empty), ("n_shift", inspect.Parameter.empty), ("stats", None), ("fs", None), ("n_mels", None),
        ("win_length", None), ("window", "hann"), ("fmin", None), ("fmax", None), ("griffin_lim_iters", 8), ("take_norm_feat", True)]
    sig = inspect.signature(griffin_lim)
    assert [(k, p.default) for k, p in sig.parameters.items() if p.kind != p.KEYWORD_ONLY] == [
        ("spc", inspect.Parameter.empty), ("n_fft", inspect.Parameter.empty), ("n_shift", inspect.Parameter.empty), ("win_length", None),
        ("window", "hann"), ("n_iter", 32)]
    assert {k: p.default for k, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY} == dict(init_phase=None, seed=None, momentum=0.99,
                                                                                              pad_mode="constant")
    sig = inspect.signature(logmel2linear)
    assert [(k, p.default) for k, p in sig.parameters.items()] == [
        ("lmspc", inspect.Parameter.empty), ("fs", inspect.Parameter.empty), ("n_fft", inspect.Parameter.empty),
        ("n_mels", inspect.Parameter.empty), ("fmin", None), ("fmax", None)]
    stats = dict(mean=np.zeros(80), scale=np.ones(80))
    v = Spectrogram2Waveform(n_fft=1024, n_shift=256, stats=stats, fs=16000, n_mels=80, fmin=80, fmax=7600, griffin_lim_iters=64)
    assert v.params == dict(n_fft=1024, n_shift=256, win_length=None, window="hann", n_iter=64, fs=16000, n_mels=80, fmin=80, fmax=7600)
    assert list(v.params) == ["n_fft", "n_shift", "win_length", "window", "n_iter", "fs", "n_mels", "fmin", "fmax"]
    assert repr(v) == ("Spectrogram2Waveform(n_fft=1024, n_shift=256, win_length=None, window=hann, n_iter=64, fs=16000, n_mels=80, "
                       "fmin=80, fmax=7600, )")
    assert v.fs == 16000 and v.take_norm_feat is True and v.stats is stats and v.logmel2linear is not None
    lin = Spectrogram2Waveform(2048, 300, win_length=1200, take_norm_feat=False)
    assert lin.params == dict(n_fft=2048, n_shift=300, win_length=1200, window="hann", n_iter=8)
    assert repr(lin) == "Spectrogram2Waveform(n_fft=2048, n_shift=300, win_length=1200, window=hann, n_iter=8, )"
    assert lin.logmel2linear is None and lin.fs is None
    with pytest.raises(AssertionError, match="must specify stats if take_norm_feat=True."):
        Spectrogram2Waveform(1024, 256)


def test_cached_pinv_is_numpy_pinv_of_the_float32_basis():
    from seq2seq_vc_amd import frontend
    G = importlib.import_module("seq2seq_vc_amd.vocoder.griffin_lim")     # (the package exports the function of the same name)
    basis = frontend.mel_basis(16000, 1024, 80, 80, 7600)
    assert basis.dtype == np.float32
    want = np.linalg.pinv(basis.astype(np.float64))
    assert np.array_equal(G.inv_mel_basis(16000, 1024, 80, 80, 7600), want)
    table = G.pinv_table("cpu", 16000, 1024, 80, 80, 7600)              # the same builder the device path uses, kept on the host here
    assert table.dtype == torch.float32 and tuple(table.shape) == (80, 513) and table.is_contiguous()
    assert np.array_equal(table.numpy(), want.T.astype(np.float32))
    assert G.pinv_table("cpu", 16000, 1024, 80, 80, 7600) is table      # once per key
    # numpy's own float32 pinv of the same basis (what the reference calls) is the same matrix up to float32 SVD rounding
    ref32 = np.linalg.pinv(basis)
    assert np.abs(ref32 - want).max() <= 1e-3 * np.abs(want).max()
    # fmin / fmax defaults of the reference: 0 and fs / 2
    assert np.array_equal(G.inv_mel_basis(16000, 1024, 80), np.linalg.pinv(frontend.mel_basis(16000, 1024, 80, 0, 8000).astype(np.float64)))


def test_refusals_are_raised_before_any_device_work():
    from seq2seq_vc_amd.vocoder import Spectrogram2Waveform, griffin_lim, istft
    spc = np.ones((5, 513), np.float32)
    with pytest.raises(NotImplementedError):
        griffin_lim(spc, 1024, 256, window="hamming")
    with pytest.raises(NotImplementedError):
        istft(np.ones((5, 513), np.complex64), 1024, 256, window="blackman")
    with pytest.raises(ValueError, match="two frames"):
        griffin_lim(spc[:1], 1024, 256)
    with pytest.raises(ValueError, match="two frames"):
        Spectrogram2Waveform(1024, 256, take_norm_feat=False).decode(torch.ones(1, 513))
    with pytest.raises(ValueError, match="n_fft"):
        griffin_lim(np.ones((5, 401), np.float32), 800, 200)
    with pytest.raises(ValueError, match="n_fft"):
        istft(np.ones((5, 2049), np.complex64), 4096, 1024)
    with pytest.raises(ValueError, match="n_fft"):
        Spectrogram2Waveform(800, 200, take_norm_feat=False).decode(torch.ones(4, 401))
    with pytest.raises(ValueError):
        griffin_lim(np.ones((5, 400), np.float32), 1024, 256)           # wrong number of bins
    with pytest.raises(ValueError, match="pad_mode"):
        from seq2seq_vc_amd.vocoder.griffin_lim import griffin_lim_batch
        griffin_lim_batch(torch.ones(1, 5, 513), None, 1024, 256, pad_mode="edge")


def test_tables_are_float64_built_and_window_is_centred():
    from seq2seq_vc_amd.ops import kernels_griffin_lim as KG
    for n_fft, _, wl in GEOMETRIES:
        t = KG.tables("cpu", n_fft, wl).numpy()
        h = n_fft // 2
        assert t.dtype == np.float32 and len(t) % 4 == 0 and len(t) >= 3 * n_fft + 2
        w_half = t[:n_fft].reshape(h, 2)
        w_full = t[n_fft:2 * n_fft + 2].reshape(h + 1, 2)
        assert np.array_equal(w_half[:, 0] + 1j * w_half[:, 1], np.exp(-2j * np.pi * np.arange(h) / h).astype(np.complex64))
        assert np.abs(w_full[:, 0] + 1j * w_full[:, 1] - np.exp(-2j * np.pi * np.arange(h + 1) / n_fft)).max() < 1e-7
        assert np.array_equal(t[2 * n_fft + 2:3 * n_fft + 2], GR.hann(n_fft, wl, np.float32))
    with pytest.raises(ValueError):
        KG.tables("cpu", 800)


def test_new_entry_points_are_declared_bound_and_exported():
    import abi_header
    from seq2seq_vc_amd import _lib
    names = ["s2svc_gl_supported", "s2svc_gl_prepare", "s2svc_gl_synth", "s2svc_gl_analyse", "s2svc_gl_ola"]
    declared, L = abi_header.declared(), abi_header.library()
    for n in names:
        assert n in declared, f"{n} missing from the header"
        assert n in _lib._FUNCTIONS and n in _lib.exported_symbols(), f"{n} missing from the ctypes binding"
        assert hasattr(L, n), f"{n} not exported by the library"
    assert [L.s2svc_gl_supported(n) for n in (256, 512, 1024, 2048, 4096, 800)] == [0, 1, 1, 1, 0, 0]
    assert "griffin_lim.hip" in _lib.sources()
    # bad arguments are refused by the entry point itself, before any launch
    assert L.s2svc_gl_synth(1, 4, 800, None, None, None, None, None) == -1
    assert b"n_fft" in L.s2svc_last_error()
