"""Launchers and host-side tables of the log-mel spectrogram kernels (csrc/melspec.hip; C ABI in include/s2svc_hip.h): forward, fused L1
loss, backward.  GPU tensors only, fp32; every argument after the host-side table build is device-resident, so a sequence of these
launches is capturable.  The autograd Functions live with the module (urhythmic/dataset.py)."""
import numpy as np
import torch

from .. import _lib
from .fft_tables import dense_from_segments, segment_tables  # noqa: F401  (imported from here by the module, tests and tools)
from .kernels import _f32c, _need_cuda, ptr, stream
from .kernels_griffin_lim import tables as fft_tables

N_FFT = 1024
MAX_MELS = 128
EPS = 1e-5
_TABLES = {}


def _hz_to_mel(f):
    f = np.asarray(f, dtype=float)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    big = f >= min_log_hz
    return np.where(big, min_log_mel + np.log(np.where(big, f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=float)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None):
    """Slaney-scale, Slaney-normalised triangular filters (torchaudio.functional.melscale_fbanks(norm="slaney", mel_scale="slaney"))
    -> (n_fft // 2 + 1, n_mels) float64.  The caller rounds it once to fp32."""
    f_max = sample_rate / 2 if f_max is None else f_max
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sample_rate)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(f_min), _hz_to_mel(f_max), n_mels + 2))
    fb = np.zeros((len(freqs), n_mels))
    for i in range(n_mels):
        lo, ce, hi = pts[i], pts[i + 1], pts[i + 2]
        fb[:, i] = np.clip(np.minimum((freqs - lo) / (ce - lo), (hi - freqs) / (hi - ce)), 0, None) * (2.0 / (hi - lo))
    return fb


def melspec_supported(n_fft, win_length, n_mels):
    """What the kernels transform: n_fft = 1024 with a window of n_fft points, n_mels <= 128 (no GPU needed: the library answers)."""
    return bool(_lib.lib().s2svc_melspec_supported(int(n_fft), int(win_length), int(n_mels)))


def geometry(n_samples, n_fft, win_length, hop_length):
    """-> (pad, T) of a row of n_samples: pad = (win_length - hop_length) // 2 on both sides, T = (N + 2 pad - n_fft) // hop + 1."""
    pad = (win_length - hop_length) // 2
    if n_samples <= pad:
        raise ValueError(f"a reflect pad of {pad} samples needs more than {pad} samples, got {n_samples}")
    T = (n_samples + 2 * pad - n_fft) // hop_length + 1
    if T < 1:
        raise ValueError(f"{n_samples} samples (+ 2 x {pad} of padding) do not fill one frame of {n_fft}")
    return pad, T


def tables(device, sample_rate, n_fft, n_mels):
    """Device tables of one configuration: (fft table (twiddles and window: the Griffin-Lim table), seg_lo, seg_len, wud, bin_seg)."""
    key = (str(device), sample_rate, n_fft, n_mels)
    if key not in _TABLES:
        seg = segment_tables(mel_filterbank(sample_rate, n_fft, n_mels).astype(np.float32))
        if seg is None:
            raise NotImplementedError("the mel basis must have at most two non-zero weights per bin, in neighbouring filters")
        _TABLES[key] = (fft_tables(device, n_fft),) + tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in seg)
    return _TABLES[key]


def melspec_fwd(wav, tab, hop, pad, n_mels, tgt=None, mel=None, logmel=None):
    """wav (B, N) -> (mel, logmel (B, n_mels, T), partials [B T] double or None): partials[b T + t] = sum_m |logmel - tgt| with tgt."""
    _need_cuda(wav, tgt, mel, logmel, *tab)
    B, N = wav.shape
    _f32c(wav, (B, N), "melspec_fwd wav")
    T = (N + 2 * pad - N_FFT) // hop + 1
    if mel is None:
        mel = torch.empty(B, n_mels, T, dtype=torch.float32, device=wav.device)
    if logmel is None:
        logmel = torch.empty(B, n_mels, T, dtype=torch.float32, device=wav.device)
    _f32c(mel, (B, n_mels, T), "melspec_fwd mel")
    _f32c(logmel, (B, n_mels, T), "melspec_fwd logmel")
    partials = None
    if tgt is not None:
        _f32c(tgt, (B, n_mels, T), "melspec_fwd tgt")
        partials = torch.empty(B * T, dtype=torch.float64, device=wav.device)
    fft, seg_lo, seg_len, wud, _ = tab
    _lib.check(_lib.lib().s2svc_melspec_fwd(B, N, T, hop, pad, n_mels, ptr(wav), ptr(fft), ptr(seg_lo), ptr(seg_len), ptr(wud), EPS, ptr(mel),
                                            ptr(logmel), ptr(tgt), ptr(partials), stream()), "melspec_fwd")
    return mel, logmel, partials


def melspec_loss_finish(partials, count, loss=None):
    """partials [n] double -> loss [1] fp32 = the ascending sum in double / count, rounded once."""
    _need_cuda(partials, loss)
    if partials.dtype != torch.float64 or not partials.is_contiguous() or partials.dim() != 1:
        raise ValueError("melspec_loss_finish: a contiguous 1-D float64 tensor of partial sums expected")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=partials.device)
    _f32c(loss, (1,), "melspec_loss_finish loss")
    _lib.check(_lib.lib().s2svc_melspec_loss_finish(partials.numel(), ptr(partials), 1.0 / float(count), ptr(loss), stream()),
               "melspec_loss_finish")
    return loss


def melspec_bwd_frames(wav, tab, hop, pad, mel, g_logmel=None, logmel=None, tgt=None, gout=None, gscale=1.0, frames=None):
    """-> frames (B, T, 1024): the gradient of every windowed frame.  g_logmel (B, n_mels, T), or the fused loss: logmel, tgt and the
    incoming scalar gradient gout [1], g = sign(logmel - tgt) * gscale * gout."""
    _need_cuda(wav, mel, g_logmel, logmel, tgt, gout, frames, *tab)
    B, N = wav.shape
    _, n_mels, T = mel.shape
    _f32c(wav, (B, N), "melspec_bwd_frames wav")
    _f32c(mel, (B, n_mels, T), "melspec_bwd_frames mel")
    if g_logmel is not None:
        _f32c(g_logmel, (B, n_mels, T), "melspec_bwd_frames g_logmel")
    else:
        if logmel is None or tgt is None or gout is None:
            raise ValueError("melspec_bwd_frames: g_logmel, or logmel, tgt and gout of the fused loss")
        _f32c(logmel, (B, n_mels, T), "melspec_bwd_frames logmel")
        _f32c(tgt, (B, n_mels, T), "melspec_bwd_frames tgt")
        if gout.dtype != torch.float32 or gout.numel() != 1:
            raise ValueError("melspec_bwd_frames gout: one fp32 value expected")
    if frames is None:
        frames = torch.empty(B, T, N_FFT, dtype=torch.float32, device=wav.device)
    _f32c(frames, (B, T, N_FFT), "melspec_bwd_frames frames")
    fft, _, _, wud, bin_seg = tab
    _lib.check(_lib.lib().s2svc_melspec_bwd_frames(B, N, T, hop, pad, n_mels, ptr(wav), ptr(fft), ptr(wud), ptr(bin_seg), EPS, ptr(mel),
                                                   ptr(g_logmel), ptr(logmel), ptr(tgt), ptr(gout), float(gscale), ptr(frames), stream()),
               "melspec_bwd_frames")
    return frames


def melspec_bwd_ola(frames, n_samples, hop, pad, dwav=None):
    """frames (B, T, 1024) -> dwav (B, N): overlap-add and the adjoint of the reflect pad."""
    _need_cuda(frames, dwav)
    B, T = frames.shape[:2]
    _f32c(frames, (B, T, N_FFT), "melspec_bwd_ola frames")
    if dwav is None:
        dwav = torch.empty(B, n_samples, dtype=torch.float32, device=frames.device)
    _f32c(dwav, (B, n_samples), "melspec_bwd_ola dwav")
    _lib.check(_lib.lib().s2svc_melspec_bwd_ola(B, n_samples, T, hop, pad, ptr(frames), ptr(dwav), stream()), "melspec_bwd_ola")
    return dwav
