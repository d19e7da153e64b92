"""LogMelSpectrogram of the vocoder fine-tuning loop on HIP (reference urhythmic/dataset.py:23-50), differentiable, with the L1 loss the
loop takes of it fused in (urhythmic_fine_tune_vocoder.py:191-222).  MelDataset (audio file I/O) is not part of this package.

    melspectrogram = LogMelSpectrogram()
    mels_ = melspectrogram(wavs_)                         # 1 launch; under grad mode one autograd node, backward 2 launches
    loss_mel, mels_ = melspectrogram.l1_loss(wavs_, tgts) # F.l1_loss(melspectrogram(wavs_), tgts) as one node: 2 launches + 2

PARITY UNPINNED against torchaudio itself: the reference delegates the arithmetic to torchaudio.transforms.MelSpectrogram (not
installed here), which builds its filterbank with an fp32 linspace; this one is built in float64 and rounded once, so the two may
differ in the last bits.  The yardstick is the plain-torch restatement in tests/mel_loss_ref.py."""
import numpy as np
import torch

from ..ops import kernels_melspec as KM


def _rows(wav, what):
    """(B, 1, N) or (B, N) -> (B, N) contiguous, and whether the channel axis was there."""
    if wav.dim() == 3 and wav.shape[1] == 1:
        return wav.reshape(wav.shape[0], wav.shape[2]).contiguous(), True
    if wav.dim() == 2:
        return wav.contiguous(), False
    raise ValueError(f"{what}: (B, 1, N) or (B, N) expected, got {tuple(wav.shape)}")


class _LogMelFunction(torch.autograd.Function):
    """wav -> log-mel as ONE autograd node: forward 1 launch (mel kept for the backward), backward 2."""

    @staticmethod
    def forward(ctx, wav, mod):
        x, chan = _rows(wav, "LogMelSpectrogram")
        tab = KM.tables(x.device, mod.sample_rate, mod.n_fft, mod.n_mels)
        mel, logmel, _ = KM.melspec_fwd(x, tab, mod.hop_length, mod.pad, mod.n_mels)
        ctx.mod, ctx.tab, ctx.wav_shape = mod, tab, wav.shape
        ctx.save_for_backward(x, mel)
        return logmel.unsqueeze(1) if chan else logmel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, mel = ctx.saved_tensors
        mod = ctx.mod
        g = g.reshape(mel.shape).contiguous()
        frames = KM.melspec_bwd_frames(x, ctx.tab, mod.hop_length, mod.pad, mel, g_logmel=g)
        return KM.melspec_bwd_ola(frames, x.shape[1], mod.hop_length, mod.pad).view(ctx.wav_shape), None


class _MelL1Function(torch.autograd.Function):
    """(wav, tgt) -> (mean |logmel - tgt|, logmel) as ONE autograd node: forward 2 launches, backward 2."""

    @staticmethod
    def forward(ctx, wav, tgt, mod):
        x, _ = _rows(wav, "LogMelSpectrogram.l1_loss")
        tab = KM.tables(x.device, mod.sample_rate, mod.n_fft, mod.n_mels)
        B, T = x.shape[0], mod.output_shape(wav.shape)[-1]
        tg = tgt.reshape(B, mod.n_mels, T).contiguous()
        mel, logmel, partials = KM.melspec_fwd(x, tab, mod.hop_length, mod.pad, mod.n_mels, tgt=tg)
        loss = KM.melspec_loss_finish(partials, logmel.numel())
        ctx.mod, ctx.tab, ctx.wav_shape = mod, tab, wav.shape
        ctx.save_for_backward(x, mel, logmel, tg)
        out = logmel.unsqueeze(1)
        ctx.mark_non_differentiable(out)
        return loss.view(()), out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_logmel):
        x, mel, logmel, tg = ctx.saved_tensors
        mod = ctx.mod
        frames = KM.melspec_bwd_frames(x, ctx.tab, mod.hop_length, mod.pad, mel, logmel=logmel, tgt=tg, gout=g_loss.reshape(1),
                                       gscale=1.0 / logmel.numel())
        return KM.melspec_bwd_ola(frames, x.shape[1], mod.hop_length, mod.pad).view(ctx.wav_shape), None, None


class LogMelSpectrogram(torch.nn.Module):
    """log(clamp(mel, min=1e-5)), mel = fb^T |STFT(reflect_pad(wav, pad))|, pad = (win_length - hop_length) // 2, STFT with center=False,
    a periodic Hann window and power 1; Slaney-scale, Slaney-normalised filters from 0 to sample_rate / 2.
    wav (B, 1, N) or (B, N), fp32, on the GPU -> (B, 1, n_mels, T) or (B, n_mels, T), T = (N + 2 pad - n_fft) // hop_length + 1."""

    def __init__(self, sample_rate: int = 16000, n_fft: int = 1024, win_length: int = 1024, hop_length: int = 320, n_mels: int = 80):
        super().__init__()
        if n_fft != KM.N_FFT:
            raise NotImplementedError(f"n_fft must be {KM.N_FFT} (csrc/melspec.hip), got {n_fft}")
        if win_length != n_fft:
            raise NotImplementedError(f"win_length must equal n_fft, got {win_length}")
        if not 1 <= n_mels <= KM.MAX_MELS:
            raise NotImplementedError(f"n_mels must be in 1 .. {KM.MAX_MELS}, got {n_mels}")
        if not 1 <= hop_length <= win_length:
            raise ValueError(f"hop_length must be in 1 .. win_length, got {hop_length}")
        self.sample_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels = sample_rate, n_fft, win_length, hop_length, n_mels
        self.pad = (win_length - hop_length) // 2
        fb = KM.mel_filterbank(sample_rate, n_fft, n_mels).astype(np.float32)        # float64, rounded once
        if KM.segment_tables(fb) is None:
            raise NotImplementedError("the mel filterbank must have at most two non-zero weights per bin, in neighbouring filters")
        self.register_buffer("fb", torch.from_numpy(fb), persistent=False)

    def output_shape(self, wav_shape):
        """The shape forward() gives for an input of this shape; ValueError where torch's reflect pad or the framing would refuse."""
        wav_shape = tuple(wav_shape)
        if not (len(wav_shape) == 2 or (len(wav_shape) == 3 and wav_shape[1] == 1)):
            raise ValueError(f"LogMelSpectrogram: (B, 1, N) or (B, N) expected, got {wav_shape}")
        _, T = KM.geometry(wav_shape[-1], self.n_fft, self.win_length, self.hop_length)
        return wav_shape[:-1] + (self.n_mels, T)

    def _check(self, wav, tgt=None):
        """Shapes and dtypes first (ValueError), then the device (RuntimeError), as the launchers do."""
        want = self.output_shape(wav.shape)
        if wav.dtype != torch.float32:
            raise ValueError(f"LogMelSpectrogram: fp32 waveforms only, got {wav.dtype}")
        if tgt is not None:
            if tuple(tgt.shape) != want:
                raise ValueError(f"l1_loss: the target must have the shape of forward(wav), {want}; got {tuple(tgt.shape)}")
            if tgt.dtype != torch.float32:
                raise ValueError(f"l1_loss: fp32 targets only, got {tgt.dtype}")
            if tgt.requires_grad:
                raise NotImplementedError("l1_loss: the target gets no gradient")
        if not wav.is_cuda or (tgt is not None and not tgt.is_cuda):
            raise RuntimeError("seq2seq_vc_amd kernels need GPU tensors (there is no CPU path)")

    def forward(self, wav: torch.Tensor) -> torch.Tensor:
        self._check(wav)
        return _LogMelFunction.apply(wav, self)

    def l1_loss(self, wav: torch.Tensor, tgt: torch.Tensor):
        """-> (F.l1_loss(self(wav), tgt) as a 0-d tensor, the (B, 1, n_mels, T) log-mel).  tgt has the shape of forward(wav) and gets no
        gradient; the log-mel returned beside the loss is for logging and validation and carries none either."""
        self._check(wav, tgt)
        return _MelL1Function.apply(wav, tgt, self)
