"""Urhythmic rhythm model, fine-grained (reference urhythmic/rhythm_model.py): a gamma distribution over the duration of each sound
type for the source and the target speaker; a source duration is mapped through the source CDF and the target quantile function.
Host code on scipy (imported on first use): the same calls as the reference, hence the same durations, Python's round included.
duration_table holds the same durations for every (sound type, segment length): what the stretch plan on the device reads."""
import numpy as np

from .utils import SILENCE, SONORANT

SHORT_SILENCE = 3            # silences of at most this many frames are ignored (and dropped by the time stretcher)
UNMAPPED = -2**31            # duration_table: no duration for this (sound type, length); __call__ raises there


def _stats():
    import scipy.stats as stats
    return stats


def transform(source, target, sample):
    return target.ppf(source.cdf(sample))


def segment_rate(codes, boundaries, sonorant=SONORANT, silence=SILENCE, unit_rate=0.02):
    """Sonorant segments per second of non-silent speech."""
    times = np.round(np.array(boundaries) * unit_rate, 2)
    voiced = [(code, t0, tn) for code, t0, tn in zip(codes, times[:-1], times[1:]) if code not in silence]
    return len([code for code, _, _ in voiced if code in sonorant]) / sum([tn - t0 for _, t0, tn in voiced])


class RhythmModelFineGrained:
    """Rhythm modeling block (fine-grained): estimates the duration distribution of each sound type."""

    def __init__(self, hop_length: int = 320, sample_rate: int = 16000):
        self.hop_rate = hop_length / sample_rate
        self.source = None
        self.target = None
        self._table = None       # duration_table's cache, one entry: ((max_frames, sound types), table, sound types)

    def _tally_durations(self, utterances):
        tally = {}
        for clusters, boundaries in utterances:
            for cluster, duration in zip(clusters, np.diff(boundaries)):
                if cluster.value == SILENCE.value and duration <= SHORT_SILENCE:
                    continue
                tally.setdefault(cluster, []).append(self.hop_rate * duration)
        return {cluster: np.array(durations) for cluster, durations in tally.items()}

    def state_dict(self):
        state = {}
        for side in ("source", "target"):
            dists = getattr(self, side)
            if dists:
                state[side] = {cluster: (dist.args[0], dist.kwds["scale"]) for cluster, dist in dists.items()}
        return state

    def load_state_dict(self, state_dict):
        """{"source": {SoundType: (a, loc, scale)}, "target": {..}}: the dictionaries the reference's training script saves."""
        gamma = _stats().gamma
        for side in ("source", "target"):
            if side in state_dict:
                setattr(self, side, {cluster.value: gamma(a, scale=scale) for cluster, (a, _, scale) in state_dict[side].items()})
        self._table = None

    def _fit(self, utterances):
        gamma = _stats().gamma
        return {cluster: gamma.fit(durations, floc=0) for cluster, durations in self._tally_durations(utterances).items()}

    def _frozen(self, utterances):
        gamma = _stats().gamma
        return {cluster: gamma(a, scale=scale) for cluster, (a, _, scale) in self._fit(utterances).items()}

    def fit_source(self, utterances):
        """Fit the duration model of the source speaker from segmented utterances [(sound types, boundaries)]."""
        self.source = self._frozen(utterances)
        self._table = None

    def fit_target(self, utterances):
        """Fit the duration model of the target speaker from segmented utterances [(sound types, boundaries)]."""
        self.target = self._frozen(utterances)
        self._table = None

    def __call__(self, clusters, boundaries):
        """Sound types (N,) and boundaries (N + 1,) -> target durations in frames, one per segment that is not a short silence."""
        durations = self.hop_rate * np.diff(boundaries)
        mapped = [transform(self.source[cluster.value], self.target[cluster.value], duration)
                  for cluster, duration in zip(clusters, durations)
                  if not cluster.value == SILENCE.value or duration > SHORT_SILENCE * self.hop_rate]
        return [round(duration / self.hop_rate) for duration in mapped]

    # -----------------------------------------------------------------------------------------------------------------------
    # the same durations as a table: the mapped duration depends on the sound type and the integer segment length only
    # -----------------------------------------------------------------------------------------------------------------------
    def _scalar_duration(self, sound_type, n):
        """What __call__ computes for ONE segment of n frames, exceptions included (KeyError: no distribution; OverflowError /
        ValueError: the mapped duration is not finite)."""
        return round(transform(self.source[sound_type.value], self.target[sound_type.value], self.hop_rate * np.int64(n)) / self.hop_rate)

    def duration_table(self, sound_types, max_frames):
        """sound_types: the segmenter's {cluster id: SoundType}; -> int32 (n_clusters, max_frames + 1), read-only: entry [c, n] is the
        duration __call__ gives a segment of n frames of sound_types[c], or UNMAPPED where __call__ raises (the mapped value is not
        finite, or source / target has no distribution of that type; ids without a sound type too).  One vectorised cdf / ppf call per
        sound type: for frozen scipy distributions it returns the bits of the per-element calls.  The last table built is kept
        until the distributions change or another (sound_types, max_frames) is asked for.  ValueError if for this hop rate
        __call__'s float filter of short silences and the stretcher's integer filter disagree at some n <= max_frames (the host
        path pairs segments and durations wrongly then)."""
        max_frames = int(max_frames)
        if max_frames < 0 or any(int(c) != c or c < 0 for c in sound_types):
            raise ValueError("duration_table: max_frames >= 0 and cluster ids 0, 1, .. expected")
        key = (max_frames, tuple(sorted((int(c), t.value) for c, t in sound_types.items())))
        if self._table is not None and self._table[0] == key:
            return self._table[1]
        frames = np.arange(max_frames + 1)
        seconds = self.hop_rate * frames                          # int64 array times a Python float, as hop_rate * np.diff(boundaries)
        disagree = np.flatnonzero((seconds > SHORT_SILENCE * self.hop_rate) != (frames > SHORT_SILENCE))
        if disagree.size:
            raise ValueError(f"duration_table: at hop rate {self.hop_rate} the duration filter of short silences and the frame-count "
                             f"filter of the time stretcher disagree at {int(disagree[0])} frames")
        table = np.full((max(sound_types, default=-1) + 1, max_frames + 1), UNMAPPED, np.int32)
        for c, sound_type in sound_types.items():
            src, tgt = (self.source or {}).get(sound_type.value), (self.target or {}).get(sound_type.value)
            if src is None or tgt is None:
                continue
            mapped = transform(src, tgt, seconds)
            for n in np.flatnonzero(np.isfinite(mapped)):
                d = round(mapped[n] / self.hop_rate)              # Python's round of a float64, as in __call__
                if -2**31 < d < 2**31:                            # beyond int32 (never a real duration): left to the scalar path
                    table[c, n] = d
        table.setflags(write=False)
        self._table = (key, table, dict(sound_types))
        return table

    def durations_from_table(self, table, clusters, boundaries):
        """The list __call__ returns for [sound_types[c] for c in clusters], from the table duration_table returned last (that very
        array: it stands for the distributions and sound types it was built from) and the integer cluster ids.  Where the table has no entry for a segment that is kept (UNMAPPED, or a length beyond the table), the scalar path runs
        for that one segment, so the exception is __call__'s own."""
        if self._table is None or self._table[1] is not table:
            raise ValueError("durations_from_table: not the table this model's duration_table returned last (the distributions may have changed since)")
        sound_types = self._table[2]
        out = []
        for c, t0, tn in zip(clusters, boundaries[:-1], boundaries[1:]):
            sound_type, n = sound_types[c], tn - t0
            if sound_type.value == SILENCE.value and n <= SHORT_SILENCE:
                continue
            d = int(table[c, n]) if 0 <= n < table.shape[1] else UNMAPPED
            out.append(d if d != UNMAPPED else self._scalar_duration(sound_type, n))
        return out
