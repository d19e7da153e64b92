"""Launchers of the Griffin-Lim kernels (csrc/griffin_lim.hip; C ABI in include/s2svc_hip.h).  Non-differentiable, GPU tensors only,
fp32; every argument after the host-side table build is device-resident, so a sequence of these launches is capturable."""
import torch

from .. import _lib
from .fft_tables import hann_padded, pad_vec4, packed_table  # noqa: F401  (hann_padded: imported from here by tests and tools)
from .kernels import _f32c, _need_cuda, ptr, stream

N_FFT = (512, 1024, 2048)
_TABLES = {}
LAUNCHES = 0                 # launches queued by this module since import (tests and the bench read the difference around a call)


def tables(device, n_fft, win_length=None):
    """Twiddles of the n_fft/2-point FFT, of the real-FFT (un)pack step and the window: float64 on the host, rounded once."""
    if n_fft not in N_FFT:
        raise ValueError(f"n_fft must be one of {N_FFT}, got {n_fft}")
    key = (str(device), n_fft, win_length)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(pad_vec4(packed_table(n_fft, win_length))).to(device)
    return _TABLES[key]


def _lens(lens, B):
    if lens is not None and (lens.dtype != torch.int32 or not lens.is_contiguous() or lens.numel() != B):
        raise ValueError("lens: a contiguous int32 device tensor with one value per row")


def _count():
    global LAUNCHES
    LAUNCHES += 1


def gl_prepare(x, n_fft, n_shift, lens=None, pinv_t=None, scale=None, mean=None, eps=1e-10, u=None, seed=0, want_x=True, want_nsamp=False):
    """x (B, Tmax, D) fp32 -> (S (B, Tmax, bins), X (B, Tmax, bins, 2) or None, Rprev like X or None, nsamp (B) int32 or None)."""
    _need_cuda(x, lens, pinv_t, scale, mean, u)
    B, Tmax, D = x.shape
    nb = n_fft // 2 + 1
    _f32c(x, (B, Tmax, D), "gl_prepare x")
    _lens(lens, B)
    nmel = 0
    if pinv_t is not None:
        nmel = pinv_t.shape[0]
        _f32c(pinv_t, (nmel, nb), "gl_prepare pinv_t")
        if D != nmel:
            raise ValueError(f"gl_prepare: x has {D} bins, the mel basis {nmel}")
    elif D != nb:
        raise ValueError(f"gl_prepare: a linear spectrogram has n_fft // 2 + 1 = {nb} bins, got {D}")
    if (scale is None) != (mean is None):
        raise ValueError("gl_prepare: scale and mean come together")
    if scale is not None:
        _f32c(scale, (D,), "gl_prepare scale")
        _f32c(mean, (D,), "gl_prepare mean")
    if u is not None:
        _f32c(u, (B, Tmax, nb), "gl_prepare u")
    S = torch.empty(B, Tmax, nb, dtype=torch.float32, device=x.device)
    X = torch.empty(B, Tmax, nb, 2, dtype=torch.float32, device=x.device) if want_x else None
    P = torch.empty_like(X) if want_x else None
    ns = torch.empty(B, dtype=torch.int32, device=x.device) if want_nsamp else None
    _lib.check(_lib.lib().s2svc_gl_prepare(B, Tmax, nb, D, nmel, n_shift, ptr(x), ptr(scale), ptr(mean), ptr(pinv_t), float(eps), ptr(u),
                                           int(seed) & (2 ** 64 - 1), ptr(lens), ptr(S), ptr(X), ptr(P), ptr(ns), stream()), "gl_prepare")
    _count()
    return S, X, P, ns


def gl_synth(X, n_fft, tab, lens=None, frames=None):
    """X (B, Tmax, bins, 2) -> frames (B, Tmax, n_fft) = window * irfft(X); absent frames are left untouched (nothing reads them)."""
    _need_cuda(X, tab, lens, frames)
    B, Tmax = X.shape[:2]
    _f32c(X, (B, Tmax, n_fft // 2 + 1, 2), "gl_synth X")
    _lens(lens, B)
    if frames is None:
        frames = torch.empty(B, Tmax, n_fft, dtype=torch.float32, device=X.device)
    _f32c(frames, (B, Tmax, n_fft), "gl_synth frames")
    _lib.check(_lib.lib().s2svc_gl_synth(B, Tmax, n_fft, ptr(X), ptr(lens), ptr(tab), ptr(frames), stream()), "gl_synth")
    _count()
    return frames


def gl_analyse(frames, S, X, Rprev, n_fft, n_shift, tab, coef, have_prev, reflect=False, lens=None):
    """X, Rprev updated in place from the frame buffer: R = stft(istft), A = R - coef Rprev (have_prev), X = S A / (|A| + tiny), Rprev = R."""
    _need_cuda(frames, S, X, Rprev, tab, lens)
    B, Tmax = X.shape[:2]
    nb = n_fft // 2 + 1
    _f32c(frames, (B, Tmax, n_fft), "gl_analyse frames")
    _f32c(S, (B, Tmax, nb), "gl_analyse S")
    _f32c(X, (B, Tmax, nb, 2), "gl_analyse X")
    _f32c(Rprev, (B, Tmax, nb, 2), "gl_analyse Rprev")
    _lens(lens, B)
    _lib.check(_lib.lib().s2svc_gl_analyse(B, Tmax, n_fft, n_shift, int(bool(reflect)), ptr(frames), ptr(S), ptr(lens), ptr(tab), float(coef),
                                           int(bool(have_prev)), ptr(X), ptr(Rprev), stream()), "gl_analyse")
    _count()


def gl_ola(frames, n_fft, n_shift, tab, lens=None):
    """frames (B, Tmax, n_fft) -> y (B, n_shift * (Tmax - 1)), zero past each row's own samples."""
    _need_cuda(frames, tab, lens)
    B, Tmax = frames.shape[:2]
    _f32c(frames, (B, Tmax, n_fft), "gl_ola frames")
    _lens(lens, B)
    y = torch.empty(B, n_shift * (Tmax - 1), dtype=torch.float32, device=frames.device)
    _lib.check(_lib.lib().s2svc_gl_ola(B, Tmax, n_fft, n_shift, ptr(frames), ptr(lens), ptr(tab), ptr(y), stream()), "gl_ola")
    _count()
    return y
