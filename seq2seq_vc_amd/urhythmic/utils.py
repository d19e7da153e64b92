"""Sound types of urhythmic (reference urhythmic/utils.py:17-28): six phone classes as flags and the three groups the segmenter tells apart."""
from enum import Flag, auto


class SoundType(Flag):
    VOWEL = auto()
    APPROXIMANT = auto()
    NASAL = auto()
    FRICATIVE = auto()
    STOP = auto()
    SILENCE = auto()


SONORANT = SoundType.VOWEL | SoundType.APPROXIMANT | SoundType.NASAL
OBSTRUENT = SoundType.FRICATIVE | SoundType.STOP
SILENCE = SoundType.SILENCE
