"""Urhythmic rhythm model, fine-grained (reference urhythmic/rhythm_model.py): a gamma distribution over the duration of each sound
type for the source and the target speaker; a source duration is mapped through the source CDF and the target quantile function.
Host code on scipy (imported on first use): the same calls as the reference, hence the same durations, Python's round included."""
import numpy as np

from .utils import SILENCE, SONORANT

SHORT_SILENCE = 3            # silences of at most this many frames are ignored (and dropped by the time stretcher)


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

    def _fit(self, utterances):
        gamma = _stats().gamma
        return {cluster: gamma.fit(durations, floc=0) for cluster, durations in self._tally_durations(utterances).items()}

    def _frozen(self, utterances):
        gamma = _stats().gamma
        return {cluster: gamma(a, scale=scale) for cluster, (a, _, scale) in self._fit(utterances).items()}

    def fit_source(self, utterances):
        """Fit the duration model of the source speaker from segmented utterances [(sound types, boundaries)]."""
        self.source = self._frozen(utterances)

    def fit_target(self, utterances):
        """Fit the duration model of the target speaker from segmented utterances [(sound types, boundaries)]."""
        self.target = self._frozen(utterances)

    def __call__(self, clusters, boundaries):
        """Sound types (N,) and boundaries (N + 1,) -> target durations in frames, one per segment that is not a short silence."""
        durations = self.hop_rate * np.diff(boundaries)
        mapped = [transform(self.source[cluster.value], self.target[cluster.value], duration)
                  for cluster, duration in zip(clusters, durations)
                  if not cluster.value == SILENCE.value or duration > SHORT_SILENCE * self.hop_rate]
        return [round(duration / self.hop_rate) for duration in mapped]
