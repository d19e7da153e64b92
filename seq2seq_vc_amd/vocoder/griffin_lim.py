"""Griffin-Lim vocoder on the HIP path: the surface of the reference's seq2seq_vc/vocoder/griffin_lim.py (logmel2linear,
griffin_lim, Spectrogram2Waveform) plus the inverse STFT on its own and a batched decode.

The algorithm is librosa.griffinlim with init="random", as the reference calls it, restated from its documentation (librosa is not
installed here, so this path is "parity unpinned", like the log-mel front-end: the yardstick is the numpy restatement in
tests/griffin_lim_ref.py, not librosa's own output):

    X <- S exp(2 pi i u);  n_iter times:  y <- istft(X);  R <- stft(y, center=True, pad_mode);
    A <- R - momentum / (1 + momentum) R_prev (no subtraction in the first iteration);  X <- S A / (|A| + tiny);  R_prev <- R;
    return istft(X)

in fp32 (the reference runs it in float64 on one CPU thread), in 2 n_iter + 3 launches whatever the batch (csrc/griffin_lim.hip).

Deviations from the reference, all deliberate:
  * the random initial phases come from a counter-based generator on the device: a run with a given `seed` is reproducible here, but
    it does NOT reproduce numpy's random stream (pass `init_phase` to fix the phases from outside);
  * only window="hann" (periodic, centred and zero-padded to n_fft when win_length < n_fft), n_fft in {512, 1024, 2048};
  * a spectrogram of ONE frame raises ValueError (the reference switches to center=False there; no recipe reaches that case).
"""
from functools import partial

import numpy as np
import torch

from .. import frontend
from ..ops import kernels_griffin_lim as KG

EPS = 1e-10
_PINV = {}


def _check_geometry(n_fft, n_shift, win_length, window):
    if window != "hann":
        raise NotImplementedError("only the hann window of the recipes is supported")
    if n_fft not in KG.N_FFT:
        raise ValueError(f"n_fft must be one of {KG.N_FFT}, got {n_fft}")
    if int(n_shift) < 1:
        raise ValueError("n_shift must be positive")
    if win_length is not None and not 0 < win_length <= n_fft:
        raise ValueError("win_length must be in 1 .. n_fft")


def _shape(x):
    return tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)


_ONE_FRAME = "Griffin-Lim needs at least two frames (the reference's center=False case for one frame is not supported)"


def inv_mel_basis(fs, n_fft, n_mels, fmin=None, fmax=None):
    """pinv of the float32 Slaney mel basis (frontend.mel_basis), computed with numpy in float64 -> (n_fft // 2 + 1, n_mels) float64."""
    fmin = 0 if fmin is None else fmin
    fmax = fs / 2 if fmax is None else fmax
    return np.linalg.pinv(frontend.mel_basis(fs, n_fft, n_mels, fmin, fmax).astype(np.float64))


def pinv_table(device, fs, n_fft, n_mels, fmin=None, fmax=None):
    """The device copy the prepare launch reads: pinv transposed, (n_mels, n_fft // 2 + 1) fp32; built once per key."""
    key = (str(device), fs, n_fft, n_mels, fmin, fmax)
    if key not in _PINV:
        _PINV[key] = torch.from_numpy(np.ascontiguousarray(inv_mel_basis(fs, n_fft, n_mels, fmin, fmax).T.astype(np.float32))).to(device)
    return _PINV[key]


def _device_f32(x, device=None):
    """-> (contiguous fp32 CUDA tensor, the device and dtype to hand the result back in)"""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    back = (x.device, x.dtype if x.dtype.is_floating_point else torch.float32)
    if not x.is_cuda:
        x = x.to(device or "cuda")
    return x.to(torch.float32).contiguous(), back


def _lens_arg(lens, B, Tmax, device):
    """lens: None, a list / CPU tensor, or an int32 device tensor (what the kernels read) -> int32 device tensor or None."""
    if lens is None:
        return None
    if isinstance(lens, torch.Tensor) and lens.is_cuda:
        if lens.dtype != torch.int32 or not lens.is_contiguous() or lens.numel() != B:
            raise ValueError("device lengths are a contiguous int32 tensor with one value per row")
        return lens
    host = [int(n) for n in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    if len(host) != B or any(n < 0 or n > Tmax for n in host):
        raise ValueError("one length per row, 0 <= lens[b] <= Tmax")
    return torch.tensor(host, dtype=torch.int32).to(device)


def _draw_seed(seed):
    if seed is not None:
        return int(seed)
    return int(torch.empty((), dtype=torch.int64).random_().item())       # torch's CPU generator: torch.manual_seed governs it


def griffin_lim_batch(x, lens, n_fft, n_shift, win_length=None, window="hann", n_iter=32, *, init_phase=None, seed=None, momentum=0.99,
                      pad_mode="constant", pinv_t=None, scale=None, mean=None, want_nsamp=False):
    """The whole loop on a zero-padded batch: x (B, Tmax, D) fp32 on the device -- linear magnitudes (D = n_fft // 2 + 1), or log-mel
    with `pinv_t` (and optionally the de-normalisation scale / mean), lens as _lens_arg takes them.
    -> (y (B, n_shift * (Tmax - 1)) fp32, n_samples (B) int32 on the device or None)."""
    _check_geometry(n_fft, n_shift, win_length, window)
    if pad_mode not in ("constant", "reflect"):
        raise ValueError("pad_mode must be 'constant' or 'reflect'")
    if not 0 <= momentum < 1 or n_iter < 0:
        raise ValueError("momentum in [0, 1) and n_iter >= 0 expected")
    B, Tmax, _ = x.shape
    if Tmax < 2:
        raise ValueError(_ONE_FRAME)
    dev = x.device
    lens_d = _lens_arg(lens, B, Tmax, dev)
    u = None
    if init_phase is not None:
        u, _ = _device_f32(init_phase, dev)
        u = u.reshape(B, Tmax, n_fft // 2 + 1)
    tab = KG.tables(dev, n_fft, win_length)
    S, X, P, ns = KG.gl_prepare(x, n_fft, n_shift, lens=lens_d, pinv_t=pinv_t, scale=scale, mean=mean, eps=EPS, u=u,
                                seed=0 if u is not None else _draw_seed(seed), want_nsamp=want_nsamp)
    coef = momentum / (1.0 + momentum)
    frames = None
    for i in range(n_iter):
        frames = KG.gl_synth(X, n_fft, tab, lens=lens_d, frames=frames)
        KG.gl_analyse(frames, S, X, P, n_fft, n_shift, tab, coef, have_prev=i > 0, reflect=pad_mode == "reflect", lens=lens_d)
    frames = KG.gl_synth(X, n_fft, tab, lens=lens_d, frames=frames)
    return KG.gl_ola(frames, n_fft, n_shift, tab, lens=lens_d), ns


def logmel2linear(lmspc, fs, n_fft, n_mels, fmin=None, fmax=None):
    """Log-mel filterbank (T, n_mels) -> linear spectrogram (T, n_fft // 2 + 1) fp32 on the device:
    max(1e-10, pinv(mel_basis) . 10 ** lmspc) (reference vocoder/griffin_lim.py:20-50), one launch."""
    x, _ = _device_f32(lmspc)
    if x.dim() != 2 or x.shape[1] != n_mels:
        raise ValueError(f"lmspc (T, {n_mels}) expected, got {tuple(x.shape)}")
    if n_fft % 2:
        raise ValueError("n_fft must be even")
    S, _, _, _ = KG.gl_prepare(x.unsqueeze(0), n_fft, 1, pinv_t=pinv_table(x.device, fs, n_fft, n_mels, fmin, fmax), eps=EPS, want_x=False)
    return S[0]


def griffin_lim(spc, n_fft, n_shift, win_length=None, window="hann", n_iter=32, *, init_phase=None, seed=None, momentum=0.99,
                pad_mode="constant"):
    """Linear spectrogram (T, n_fft // 2 + 1) -> waveform of n_shift * (T - 1) samples, fp32 on the device
    (reference vocoder/griffin_lim.py:53-106: librosa.griffinlim(S=|spc|.T, n_iter, hop_length, win_length, window, center=True)).

    init_phase: uniform [0, 1) values in the shape of spc, the initial phases in turns; otherwise they are drawn on the device from a
    generator seeded with `seed` (None: a seed from torch's CPU generator).  A seeded run is reproducible here; it does not reproduce
    numpy's random stream.  pad_mode: the padding of the forward STFT inside the loop, "constant" (librosa >= 0.10) or "reflect"."""
    _check_geometry(n_fft, n_shift, win_length, window)
    shape = _shape(spc)
    if len(shape) != 2 or shape[1] != n_fft // 2 + 1:
        raise ValueError(f"spc (T, {n_fft // 2 + 1}) expected, got {shape}")
    if shape[0] < 2:
        raise ValueError(_ONE_FRAME)
    x, _ = _device_f32(spc)
    y, _ = griffin_lim_batch(x.unsqueeze(0), None, n_fft, n_shift, win_length, window, n_iter, init_phase=init_phase, seed=seed,
                             momentum=momentum, pad_mode=pad_mode)
    return y[0]


def istft(spec, n_fft, n_shift, win_length=None, window="hann"):
    """Inverse STFT of a complex (T, n_fft // 2 + 1) tensor (or real (T, n_fft // 2 + 1, 2)): inverse real FFT per frame, window,
    overlap-add, division by the summed squared window where that sum exceeds the smallest normal fp32, center=True trim
    -> n_shift * (T - 1) samples, fp32 on the device (librosa.istft / torch.istft(center=True) semantics)."""
    _check_geometry(n_fft, n_shift, win_length, window)
    if not isinstance(spec, torch.Tensor):
        spec = torch.as_tensor(np.asarray(spec))
    if spec.dim() < 2 or spec.shape[0] < 2:
        raise ValueError("istft needs at least two frames")
    if spec.is_complex():
        spec = torch.view_as_real(spec.to(torch.complex64) if spec.is_cuda else spec.to(torch.complex64).cuda())
    X, _ = _device_f32(spec)
    if X.dim() != 3 or tuple(X.shape[1:]) != (n_fft // 2 + 1, 2):
        raise ValueError(f"spec: complex (T, {n_fft // 2 + 1}) or real (T, {n_fft // 2 + 1}, 2) expected, got {tuple(X.shape)}")
    if X.shape[0] < 2:
        raise ValueError("istft needs at least two frames")
    tab = KG.tables(X.device, n_fft, win_length)
    frames = KG.gl_synth(X.unsqueeze(0), n_fft, tab)
    return KG.gl_ola(frames, n_fft, n_shift, tab)[0]


class Spectrogram2Waveform(object):
    """Spectrogram to waveform conversion module: the reference's class (vocoder/griffin_lim.py:110-203) over the HIP kernels.
    stats: a dict of arrays `mean` and `scale` (reading the HDF5 stays the caller's business)."""

    def __init__(self, n_fft, n_shift, stats=None, fs=None, n_mels=None, win_length=None, window="hann", fmin=None, fmax=None,
                 griffin_lim_iters=8, take_norm_feat=True):
        self.take_norm_feat = take_norm_feat
        self.stats = stats
        if self.take_norm_feat:
            assert self.stats is not None, "must specify stats if take_norm_feat=True."
        self.fs = fs
        self.logmel2linear = (partial(logmel2linear, fs=fs, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax)
                              if n_mels is not None else None)
        self.griffin_lim = partial(griffin_lim, n_fft=n_fft, n_shift=n_shift, win_length=win_length, window=window,
                                   n_iter=griffin_lim_iters)
        self.params = dict(n_fft=n_fft, n_shift=n_shift, win_length=win_length, window=window, n_iter=griffin_lim_iters)
        if n_mels is not None:
            self.params.update(fs=fs, n_mels=n_mels, fmin=fmin, fmax=fmax)
        self._affine = None

    def __repr__(self):
        retval = f"{self.__class__.__name__}("
        for k, v in self.params.items():
            retval += f"{k}={v}, "
        retval += ")"
        return retval

    def _stats_on(self, device, D):
        if not self.take_norm_feat:
            return None, None
        if self._affine is None or self._affine[0].device != device:
            scale = torch.from_numpy(np.asarray(self.stats["scale"], np.float32).reshape(-1)).to(device)
            mean = torch.from_numpy(np.asarray(self.stats["mean"], np.float32).reshape(-1)).to(device)
            self._affine = (scale, mean)
        if self._affine[0].numel() != D:
            raise ValueError("statistics must have one value per bin of the spectrogram")
        return self._affine

    def decode_batch(self, spcs, lens, init_phase=None, seed=None, pad_mode="constant"):
        """spcs (B, Tmax, D) zero-padded (what the padding holds is never read), lens (B) frames: a list / CPU tensor or an int32
        device tensor -> (ys (B, n_shift * (Tmax - 1)) in spcs's dtype on its device, n_samples (B) int32 on the device, fs).
        Row b is what decode gives the utterance alone (with the matching init_phase rows: bit for bit); samples past
        n_shift * (lens[b] - 1) are zero."""
        p = self.params
        _check_geometry(p["n_fft"], p["n_shift"], p["win_length"], p["window"])
        shape = _shape(spcs)
        D = p["n_mels"] if "n_mels" in p else p["n_fft"] // 2 + 1
        if len(shape) != 3 or shape[2] != D:
            raise ValueError(f"spcs (B, Tmax, {D}) expected, got {shape}")
        if shape[1] < 2:
            raise ValueError(_ONE_FRAME)
        x, (dev0, dt0) = _device_f32(spcs)
        scale, mean = self._stats_on(x.device, D)
        pinv_t = pinv_table(x.device, p["fs"], p["n_fft"], p["n_mels"], p["fmin"], p["fmax"]) if "n_mels" in p else None
        y, ns = griffin_lim_batch(x, lens, p["n_fft"], p["n_shift"], p["win_length"], p["window"], p["n_iter"], init_phase=init_phase,
                                  seed=seed, pad_mode=pad_mode, pinv_t=pinv_t, scale=scale, mean=mean, want_nsamp=True)
        return y.to(device=dev0, dtype=dt0), ns, self.fs

    def decode(self, spc, init_phase=None, seed=None, pad_mode="constant"):
        """Log-mel filterbank (T_feats, n_mels) or, when n_mels is None, linear spectrogram (T_feats, n_fft // 2 + 1)
        -> (waveform (n_shift * (T_feats - 1),) on spc's device in spc's dtype, fs)."""
        if not isinstance(spc, torch.Tensor):
            spc = torch.as_tensor(np.asarray(spc))
        if spc.dim() != 2:
            raise ValueError(f"spc (T, D) expected, got {tuple(spc.shape)}")
        ys, _, fs = self.decode_batch(spc.unsqueeze(0), None, init_phase=None if init_phase is None else torch.as_tensor(init_phase)[None],
                                      seed=seed, pad_mode=pad_mode)
        return ys[0], fs
