"""Host tables of the one-wavefront FFT kernels (csrc/fft_wave.h: the log-mel front-end, Griffin-Lim, the mel L1 loss), numpy only:
the window, the packed twiddle / window table and the segment form of a triangular mel basis.  Everything is built in float64 and
rounded once."""
import numpy as np


def hann_padded(n_fft, win_length=None):
    """Periodic Hann window of win_length points, centred and zero-padded to n_fft -> float64 (librosa's get_window + pad_center)."""
    wl = n_fft if win_length is None else int(win_length)
    if not 0 < wl <= n_fft:
        raise ValueError(f"win_length must be in 1 .. n_fft, got {wl}")
    win = np.zeros(n_fft)
    lp = (n_fft - wl) // 2
    win[lp:lp + wl] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wl) / wl)
    return win


def pad_vec4(packed):
    """Zero-filled to whole 16-byte vectors."""
    return np.concatenate([packed, np.zeros((-len(packed)) % 4, np.float32)])


def packed_table(n_fft, win_length=None):
    """The table fft_wave.h views, float32, 3 n_fft + 2 values (H = n_fft / 2):
    w_half [H] complex exp(-2 pi i m / H) | w_full [H + 1] complex exp(-2 pi i k / n_fft) | win [n_fft]."""
    h = n_fft // 2
    a = -2 * np.pi * np.arange(h) / h
    w_half = np.stack([np.cos(a), np.sin(a)], 1)
    a = -2 * np.pi * np.arange(h + 1) / n_fft
    w_full = np.stack([np.cos(a), np.sin(a)], 1)
    return np.concatenate([w_half.reshape(-1), w_full.reshape(-1), hann_padded(n_fft, win_length)]).astype(np.float32)


def segment_tables(fb):
    """Segment form of a (bins, n_mels) mel basis, or None if it does not have the structure the kernels need: every bin has at most
    two non-zero weights, in neighbouring filters.  Segment s (0 .. n_mels) = the bins between the peaks of filters s - 1 and s: rising
    side of filter s (weight wud[k][0]), falling side of filter s - 1 (wud[k][1]), so that
        mel[m] = sum over segment m of wud[:, 0] |X| + sum over segment m + 1 of wud[:, 1] |X|.
    -> (seg_lo, seg_len (n_mels + 1) int32, wud (bins, 2) in fb's dtype, bin_seg (bins) int32: the segment of every bin, 0 with zero
    weights where no filter reaches)."""
    fb = np.asarray(fb)
    nb, n_mels = fb.shape
    peak = fb.argmax(axis=0)
    seg = np.full(nb, -1, np.int64)
    wud = np.zeros((nb, 2), fb.dtype)
    for k in range(nb):
        nz = np.nonzero(fb[k])[0]
        if len(nz) == 0:
            continue
        if len(nz) > 2 or (len(nz) == 2 and nz[1] != nz[0] + 1):
            return None
        if len(nz) == 2:
            seg[k], wud[k, 0], wud[k, 1] = nz[1], fb[k, nz[1]], fb[k, nz[0]]
        elif k <= peak[nz[0]]:                         # one filter only, on its rising side (or at its peak)
            seg[k], wud[k, 0] = nz[0], fb[k, nz[0]]
        else:                                          # ... on its falling side: the segment above
            seg[k], wud[k, 1] = nz[0] + 1, fb[k, nz[0]]
    seg_lo, seg_len = np.zeros(n_mels + 1, np.int32), np.zeros(n_mels + 1, np.int32)
    for m in range(n_mels + 1):
        ks = np.nonzero(seg == m)[0]
        if len(ks) == 0:
            continue
        if ks[-1] - ks[0] + 1 != len(ks):
            return None
        seg_lo[m], seg_len[m] = ks[0], len(ks)
    if not np.array_equal(dense_from_segments(seg_lo, seg_len, wud, n_mels), fb):      # the identity the kernels rely on
        return None
    return seg_lo, seg_len, wud, np.maximum(seg, 0).astype(np.int32)


def dense_from_segments(seg_lo, seg_len, wud, n_mels):
    """The (bins, n_mels) basis the segment tables stand for."""
    rec = np.zeros((wud.shape[0], n_mels), wud.dtype)
    for m in range(n_mels):
        sl = slice(seg_lo[m], seg_lo[m] + seg_len[m])
        rec[sl, m] += wud[sl, 0]
        sl = slice(seg_lo[m + 1], seg_lo[m + 1] + seg_len[m + 1])
        rec[sl, m] += wud[sl, 1]
    return rec
