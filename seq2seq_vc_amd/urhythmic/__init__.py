"""Urhythmic on HIP: segmenter, rhythm model, time stretchers and the conversion that chains them with the HiFi-GAN generator."""
from .dataset import LogMelSpectrogram
from .vocoder import MultiPeriodDiscriminator, PeriodDiscriminator
from .hubert import Hubert, HubertSoft
from .model import UrhythmicFine, convert_wavs, encode, encode_batch
from .rhythm_model import RhythmModelFineGrained, segment_rate, transform
from .segmenter import Segmenter, cluster_merge, segment
from .stretcher import TimeStretcherFineGrained, TimeStretcherGlobal
from .utils import OBSTRUENT, SILENCE, SONORANT, SoundType

__all__ = ["Hubert", "HubertSoft", "encode", "encode_batch", "convert_wavs", "LogMelSpectrogram", "MultiPeriodDiscriminator", "PeriodDiscriminator", "UrhythmicFine", "RhythmModelFineGrained", "segment_rate", "transform", "Segmenter", "cluster_merge", "segment",
           "TimeStretcherFineGrained", "TimeStretcherGlobal", "OBSTRUENT", "SILENCE", "SONORANT", "SoundType"]
