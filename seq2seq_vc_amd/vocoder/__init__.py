"""Vocoders on the HIP path: the HiFi-GAN generator (mel -> waveform) with the decode wrapper of the reference's Vocoder, and the
Griffin-Lim vocoder the reference builds when no checkpoint is configured."""
from .hifigan import HifiganGenerator, HifiganVocoder, ResBlock  # noqa: F401
from .griffin_lim import Spectrogram2Waveform, griffin_lim, istft, logmel2linear  # noqa: F401
