"""CPU tests of the host tables of the one-wavefront FFT kernels (seq2seq_vc_amd/ops/fft_tables.py): the three kernel families read ONE
packed twiddle / window table and ONE segment form of a triangular mel basis.  None of this launches a kernel."""
import numpy as np
import pytest

from seq2seq_vc_amd import frontend as F
from seq2seq_vc_amd.ops import fft_tables as FT
from seq2seq_vc_amd.ops import kernels_griffin_lim as KG
from seq2seq_vc_amd.ops import kernels_melspec as KM

# (sample rate, n_mels, fmin, fmax) of the n_fft = 1024 front-end layouts
MEL_LAYOUTS = [(16000, 80, 80, 7600), (24000, 80, 80, 7600), (22050, 100, 0, None), (16000, 128, 50, 8000)]


@pytest.mark.parametrize("n_fft,win_length", [(512, None), (1024, None), (1024, 800), (2048, 1200), (2048, None)])
def test_frontend_table_starts_with_the_griffin_lim_table(n_fft, win_length):
    n = 3 * n_fft + 2                                      # w_half (n_fft floats) | w_full (n_fft + 2) | win (n_fft)
    gl = KG.tables("cpu", n_fft, win_length).numpy()
    fe = F._fft_tables("cpu", 16000, n_fft, win_length, 80, 80, 7600)[0].numpy()
    assert gl.dtype == fe.dtype == np.float32 and len(gl) % 4 == 0 and len(fe) % 4 == 0
    assert gl[:n].tobytes() == fe[:n].tobytes() == FT.packed_table(n_fft, win_length).tobytes()
    assert not gl[n:].any()
    h = n_fft // 2                                         # w_half[0] = w_full[0] = 1, w_full[H] = -1, the window behind them
    assert tuple(gl[:2]) == tuple(gl[2 * h:2 * h + 2]) == (1.0, 0.0)
    assert gl[4 * h] == -1.0 and gl[4 * h + 1] == pytest.approx(0.0, abs=1e-7)
    assert np.array_equal(gl[2 * h + 2 * (h + 1):n], FT.hann_padded(n_fft, win_length).astype(np.float32))


@pytest.mark.parametrize("sr,n_mels,fmin,fmax", MEL_LAYOUTS)
def test_fft8_tables_are_the_segment_tables_of_the_mel_basis(sr, n_mels, fmin, fmax):
    fmax = sr / 2 if fmax is None else fmax               # as logmelfilterbank resolves it before it asks for tables
    basis = F.mel_basis(sr, 1024, n_mels, fmin, fmax)
    got = F._fft8_tables("cpu", sr, 1024, n_mels, fmin, fmax)
    want = FT.segment_tables(basis.T)
    assert got is not None and want is not None and len(got) == 3
    for g, w in zip(got, want[:3]):
        assert g.numpy().dtype == w.dtype and g.numpy().shape == w.shape and g.numpy().tobytes() == np.ascontiguousarray(w).tobytes()
    seg_lo, seg_len, wud = (g.numpy() for g in got)
    rec = FT.dense_from_segments(seg_lo, seg_len, wud, n_mels)
    # bit for bit, up to the sign of a zero weight: with fmin = 0 the ramp of filter 0 gives -0.0 at bin 0, and a segment table
    # holds no weight where the basis is zero (adding +0.0 turns -0.0 into +0.0 and changes no other bit)
    assert rec.dtype == basis.dtype and rec.T.shape == basis.shape
    assert np.ascontiguousarray(rec.T).tobytes() == (basis + np.float32(0.0)).tobytes()


@pytest.mark.parametrize("n_fft", [512, 2048])
def test_fft8_tables_only_for_n_fft_1024(n_fft):
    assert F._fft8_tables("cpu", 16000, n_fft, 80, 80, 7600) is None


@pytest.mark.parametrize("n_fft,win_length", [(512, None), (1024, 800), (2048, 1200)])
def test_hann_padded_is_the_window_of_dft_basis(n_fft, win_length):
    win = FT.hann_padded(n_fft, win_length)
    assert win.dtype == np.float64 and win.shape == (n_fft,)
    # row 0 of the basis is w * cos(0) = w; the basis is float32
    assert np.array_equal(F.dft_basis(n_fft, win_length)[0], win.astype(np.float32))
    # dft_basis takes its window from hann_padded, so the window itself is held to the formula: periodic Hann, centred, zero-padded
    wl = n_fft if win_length is None else win_length
    lp = (n_fft - wl) // 2
    want = np.zeros(n_fft)
    want[lp:lp + wl] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wl) / wl)
    assert np.array_equal(win, want)
    assert not win[:lp].any() and not win[lp + wl:].any() and win[lp] == 0.0 and win[lp + wl // 2] == pytest.approx(1.0)


def test_names_the_launcher_modules_keep():
    assert KM.segment_tables is FT.segment_tables and KM.dense_from_segments is FT.dense_from_segments
    assert KG.hann_padded is FT.hann_padded
