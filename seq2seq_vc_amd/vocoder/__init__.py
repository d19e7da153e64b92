"""Vocoders on the HIP path: the HiFi-GAN generator (mel -> waveform) and the decode wrapper of the reference's Vocoder."""
from .hifigan import HifiganGenerator, HifiganVocoder, ResBlock  # noqa: F401
