"""Test-side restatement of the Griffin-Lim vocoder (reference seq2seq_vc/vocoder/griffin_lim.py over librosa.griffinlim) in numpy,
independent of the product code: np.fft, explicit overlap-add, a `dtype` switch (float64 = the truth, float32 = the yardstick's other
leg).  librosa is not installed here: this restates its documented algorithm (stft / istft with center=True, periodic Hann centred
and zero-padded to n_fft, window-sum-square normalisation where the sum exceeds tiny; griffinlim with init="random" and momentum),
and tests/test_griffin_lim_host.py pins stft / istft to torch.stft / torch.istft.  Also the stock-torch loop of the timing tool."""
import numpy as np

EPS = 1e-10


def _cdtype(dtype):
    return np.complex128 if np.dtype(dtype) == np.float64 else np.complex64


def hann(n_fft, win_length=None, dtype=np.float64):
    wl = n_fft if win_length is None else win_length
    w = np.zeros(n_fft)
    lp = (n_fft - wl) // 2
    w[lp:lp + wl] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wl) / wl)
    return w.astype(dtype)


def stft(y, n_fft, n_shift, win_length=None, pad_mode="constant", dtype=np.float64):
    """y (L,) -> (1 + L // n_shift, n_fft // 2 + 1) complex: centred frames of the padded signal, windowed, rfft."""
    y = np.asarray(y, dtype=dtype)
    yp = np.pad(y, n_fft // 2, mode=pad_mode)
    win = hann(n_fft, win_length, dtype)
    T = 1 + len(y) // n_shift
    out = np.empty((T, n_fft // 2 + 1), dtype=_cdtype(dtype))
    for t in range(T):
        out[t] = np.fft.rfft(yp[t * n_shift:t * n_shift + n_fft] * win)
    return out


def istft(X, n_fft, n_shift, win_length=None, dtype=np.float64):
    """X (T, n_fft // 2 + 1) complex -> n_shift * (T - 1) samples: irfft, window, overlap-add in frame order, division by the summed
    squared window where it exceeds tiny, trim of n_fft // 2 at both ends."""
    X = np.asarray(X, dtype=_cdtype(dtype))
    T = X.shape[0]
    win = hann(n_fft, win_length, dtype)
    y = np.zeros(n_fft + n_shift * (T - 1), dtype=dtype)
    env = np.zeros_like(y)
    wsq = win * win
    for t in range(T):
        y[t * n_shift:t * n_shift + n_fft] += win * np.fft.irfft(X[t], n=n_fft).astype(dtype)
        env[t * n_shift:t * n_shift + n_fft] += wsq
    nz = env > np.finfo(dtype).tiny
    y[nz] /= env[nz]
    return y[n_fft // 2:n_fft // 2 + n_shift * (T - 1)]


def gl_iteration(X, R_prev, S, n_fft, n_shift, win_length=None, momentum=0.99, pad_mode="constant", dtype=np.float64):
    """One iteration: (X, R_prev or None) -> (X_new, R)."""
    cd = _cdtype(dtype)
    S = np.asarray(S, dtype=dtype)
    R = stft(istft(X, n_fft, n_shift, win_length, dtype), n_fft, n_shift, win_length, pad_mode, dtype)
    A = R.copy()
    if R_prev is not None:
        A = (R - dtype(momentum / (1 + momentum)) * np.asarray(R_prev, dtype=cd)).astype(cd)
    Xn = (S * (A / (np.abs(A) + np.finfo(dtype).tiny))).astype(cd)
    return Xn, R


def initial(S, u, dtype=np.float64):
    S, u = np.asarray(S, dtype=dtype), np.asarray(u, dtype=dtype)
    return (S * np.exp(2j * np.pi * u)).astype(_cdtype(dtype))


def griffin_lim(S, u, n_fft, n_shift, win_length=None, n_iter=32, momentum=0.99, pad_mode="constant", dtype=np.float64):
    """S (T, bins) magnitudes, u (T, bins) uniform [0, 1) initial phases in turns -> waveform."""
    S = np.abs(np.asarray(S, dtype=dtype))
    X, R_prev = initial(S, u, dtype), None
    for _ in range(n_iter):
        X, R_prev = gl_iteration(X, R_prev, S, n_fft, n_shift, win_length, momentum, pad_mode, dtype)
    return istft(X, n_fft, n_shift, win_length, dtype)


def logmel2linear(lmspc, mel_basis, dtype=np.float64):
    """max(1e-10, pinv(mel_basis) . 10 ** lmspc); mel_basis (n_mels, bins) float32 as librosa returns it, its pseudo-inverse taken in
    float64 and then used in `dtype`."""
    inv = np.linalg.pinv(np.asarray(mel_basis, dtype=np.float64)).astype(dtype)
    mspc = np.power(dtype(10.0), np.asarray(lmspc, dtype=dtype))
    return np.maximum(dtype(EPS), (inv @ mspc.T).T).astype(dtype)


def decode(spc, mel_basis, stats, u, n_fft, n_shift, win_length=None, n_iter=8, pad_mode="constant", dtype=np.float64):
    """Spectrogram2Waveform.decode restated: de-normalise, logmel2linear (mel_basis given) and the loop."""
    spc = np.asarray(spc, dtype=dtype)
    if stats is not None:
        spc = spc * np.asarray(stats["scale"], dtype=dtype) + np.asarray(stats["mean"], dtype=dtype)
    if mel_basis is not None:
        spc = logmel2linear(spc, mel_basis, dtype)
    return griffin_lim(spc, u, n_fft, n_shift, win_length, n_iter, 0.99, pad_mode, dtype)


def spectral_convergence(y, S, n_fft, n_shift, win_length=None, pad_mode="constant"):
    """|| |STFT(y)| - S || / || S || in float64"""
    S = np.asarray(S, dtype=np.float64)
    M = np.abs(stft(np.asarray(y, dtype=np.float64), n_fft, n_shift, win_length, pad_mode, np.float64))
    return float(np.linalg.norm(M - S) / np.linalg.norm(S))


def make_signal(seconds=2.0, fs=16000, seed=0):
    """A seeded voiced-like signal: a few gliding harmonics under a slow envelope plus a little noise, peak about 0.7."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * fs)) / fs
    f0 = 120 + 40 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / fs
    y = sum(a * np.sin(k * ph + p) for k, (a, p) in enumerate(zip([0.5, 0.3, 0.2, 0.1, 0.05], rng.uniform(0, 6.28, 5)), start=1))
    y = y * (0.55 + 0.45 * np.sin(2 * np.pi * 1.3 * t)) + 0.01 * rng.standard_normal(len(t))
    return 0.7 * y / np.abs(y).max()


# ---- the stock-torch loop of tools/bench_griffin_lim.py: the same algorithm with torch.stft / torch.istft on a batch ----
def torch_griffin_lim(S, u, n_fft, n_shift, win_length=None, n_iter=32, momentum=0.99, pad_mode="constant"):
    """S, u (B, T, bins) real tensors on one device -> (B, n_shift * (T - 1)); every row has T frames."""
    import math

    import torch
    wl = n_fft if win_length is None else win_length
    win = torch.hann_window(wl, periodic=True, dtype=S.dtype, device=S.device)
    St = S.transpose(1, 2)
    X = St * torch.exp(2j * math.pi * u.transpose(1, 2))
    length = n_shift * (S.shape[1] - 1)
    tiny = torch.finfo(S.dtype).tiny
    coef = momentum / (1 + momentum)
    prev = None
    for _ in range(n_iter):
        y = torch.istft(X, n_fft, n_shift, wl, win, center=True, length=length)
        R = torch.stft(y, n_fft, n_shift, wl, win, center=True, pad_mode=pad_mode, return_complex=True)
        A = R if prev is None else R - coef * prev
        X = St * (A / (A.abs() + tiny))
        prev = R
    return torch.istft(X, n_fft, n_shift, wl, win, center=True, length=length)
