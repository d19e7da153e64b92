"""Urhythmic segmenter on the kernels of csrc/urhythmic.hip (reference urhythmic/segmenter.py).

The search the reference runs per utterance on the host (numba-JIT, a dense (T, T, K) table) is two launches here for a whole batch:
span scores, then one wave per utterance for the dynamic programme, the backtrack and the cluster merge.  Class name, constructor,
return structures and the six state_dict keys are the reference's.  Clustering of the codebook (sklearn) and the identification of
the clusters are host code, as there.  There is no CPU path for the search."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import torch

from ..ops import kernels_urhythmic as KU
from .utils import OBSTRUENT, SILENCE, SONORANT


def _device_log_probs(log_probs, device=None):
    """numpy array or tensor on any device, (T, K) or (B, T, K) -> contiguous fp32 tensor on the GPU"""
    t = torch.from_numpy(np.ascontiguousarray(log_probs)) if isinstance(log_probs, np.ndarray) else log_probs.detach()
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("the segmentation search needs a GPU (there is no CPU path)")
        t = t.to(device if device is not None else "cuda")
    return t.float().contiguous()


def segment(log_probs, gamma):
    """log_probs (T, K) -> (codes (T,) int32: the unit of every frame, boundaries (N + 1,) ascending from 0), as numpy arrays."""
    lp = _device_log_probs(log_probs)
    if lp.dim() != 2:
        raise ValueError(f"segment: log_probs (T, K) expected, got {tuple(lp.shape)}")
    T = lp.shape[0]
    lens = torch.tensor([T], dtype=torch.int32).to(lp.device)
    out = KU.useg_segment(lp.unsqueeze(0), lens, gamma)
    flat = torch.cat([out["nseg"], out["codes"].view(-1), out["boundaries"].view(-1)]).cpu().numpy()
    n = int(flat[0])
    return flat[1:1 + T].astype(np.int32), flat[1 + T:2 + T + n].astype(np.int64)


def cluster_merge(clustering, segments, boundaries):
    """Adjacent segments whose units fall in the same cluster become one: (clusters (M,), cluster boundaries (M + 1,))."""
    clusters = np.asarray(clustering.labels_)[np.asarray(segments)]
    boundaries = np.asarray(boundaries)
    opens = np.flatnonzero(np.diff(clusters, prepend=-1, append=-1))     # a cluster opens at every change, and the end closes the last
    return clusters[opens[:-1]], boundaries[opens]


class Segmenter:
    """Segmentation and clustering block: groups similar speech units into short segments, then merges the segments into coarser
    groups approximating sonorants, obstruents and silences."""

    def __init__(self, num_clusters: int = 3, gamma: float = 2):
        self.gamma = gamma
        self.clustering = SimpleNamespace(n_clusters=num_clusters)     # receives sklearn's fitted attributes (cluster / load_state_dict)
        self.sound_types = dict()
        self._labels = {}

    def state_dict(self):
        c = self.clustering
        return {"n_clusters_": c.n_clusters_, "labels_": torch.from_numpy(np.asarray(c.labels_)), "n_leaves_": c.n_leaves_,
                "n_features_in_": c.n_features_in_, "children_": torch.from_numpy(np.asarray(c.children_)), "sound_types": self.sound_types}

    def load_state_dict(self, state_dict):
        if self.clustering.n_clusters != state_dict["n_clusters_"]:
            raise RuntimeError(f"Error in loading state_dict for {self.__class__.__name__}")
        c = self.clustering
        c.n_clusters_ = state_dict["n_clusters_"]
        c.labels_ = state_dict["labels_"].numpy()
        c.n_leaves_ = state_dict["n_leaves_"]
        c.n_features_in_ = state_dict["n_features_in_"]
        c.children_ = state_dict["children_"].numpy()
        self.sound_types = state_dict["sound_types"]
        self._labels = {}

    def cluster(self, codebook):
        """Fit the hierarchical clustering from the codebook of discrete units (K, D)."""
        from sklearn.cluster import AgglomerativeClustering
        fitted = AgglomerativeClustering(n_clusters=self.clustering.n_clusters).fit(codebook)
        for name in ("n_clusters_", "labels_", "n_leaves_", "n_features_in_", "children_"):
            setattr(self.clustering, name, getattr(fitted, name))
        self._labels = {}

    def identify(self, utterances):
        """Which cluster is silence, which sonorant, which obstruent (num_clusters = 3 only).  utterances: (segments, boundaries,
        silence flags, voiced flags) per utterance.  The cluster that overlaps marked silence most (relative to its frames) is silence,
        of the other two the more voiced one is the sonorant."""
        if self.clustering.n_clusters_ != 3:
            raise ValueError("Cluster identification is only implemented for num_clusters = 3.")
        silent, voiced, total = Counter(), Counter(), Counter()
        for segments, boundaries, silences, voiced_flags in utterances:
            for code, a, b in zip(segments, boundaries[:-1], boundaries[1:]):
                silent[code] += np.count_nonzero(silences[a:b + 1])
                voiced[code] += np.count_nonzero(voiced_flags[a:b + 1])
                total[code] += b - a + 1
        left = {0, 1, 2}
        silence = max(((k, v / total[k]) for k, v in silent.items()), key=lambda kv: kv[1])[0]
        left.remove(silence)
        sonorant = max(((k, v / total[k]) for k, v in voiced.items() if k in left), key=lambda kv: kv[1])[0]
        left.remove(sonorant)
        self.sound_types = {silence: SILENCE, sonorant: SONORANT, left.pop(): OBSTRUENT}
        return self.sound_types

    def _device_labels(self, device):
        key = str(device)
        if key not in self._labels:
            self._labels[key] = torch.from_numpy(np.asarray(self.clustering.labels_).astype(np.int32)).to(device)
        return self._labels[key]

    def segment_tables(self, log_probs, lens):
        """log_probs (B, Tmax, K) fp32 and lens (B) int32 on the device -> the device tensors of ops.kernels_urhythmic.useg_segment with
        the clustering's labels (clusters, cboundaries, ncl, ..).  Two launches whatever B is, and no host read: what
        ops.kernels_urhythmic.useg_plan takes."""
        KU.check_segment_args(log_probs, lens)
        labels = np.asarray(self.clustering.labels_)
        if labels.shape != (log_probs.shape[2],):
            raise ValueError(f"the clustering knows {labels.shape[0]} units, log_probs has {log_probs.shape[2]}")
        return KU.useg_segment(log_probs, lens, self.gamma, labels=self._device_labels(log_probs.device))

    def segment_batch(self, log_probs, lens, want_tables=False):
        """log_probs (B, Tmax, K) fp32 and lens (B) int32 on the device -> (tables, rows).  tables: the device tensors of
        ops.kernels_urhythmic.useg_segment (clusters, cboundaries, ncl, codes, boundaries, nseg, ..); rows: per utterance
        (clusters: list of int, boundaries: list of int), read back with ONE device-to-host copy.  Two launches whatever B is."""
        KU.check_segment_args(log_probs, lens)
        labels = np.asarray(self.clustering.labels_)
        if labels.shape != (log_probs.shape[2],):
            raise ValueError(f"the clustering knows {labels.shape[0]} units, log_probs has {log_probs.shape[2]}")
        tables = KU.useg_segment(log_probs, lens, self.gamma, labels=self._device_labels(log_probs.device), want_tables=want_tables)
        B, Tmax = log_probs.shape[:2]
        host = tables["packed"].cpu().numpy()
        ncl, cl, cb = host[:B], host[B:B + B * Tmax].reshape(B, Tmax), host[B + B * Tmax:].reshape(B, Tmax + 1)
        rows = [(cl[b, :ncl[b]].tolist(), cb[b, :ncl[b] + 1].tolist()) for b in range(B)]
        return tables, rows

    def _segment(self, log_probs):
        lp = _device_log_probs(log_probs)
        if lp.dim() != 2:
            raise ValueError(f"Segmenter: log_probs (T, K) expected, got {tuple(lp.shape)}")
        lens = torch.tensor([lp.shape[0]], dtype=torch.int32).to(lp.device)
        return self.segment_batch(lp.unsqueeze(0), lens)[1][0]

    def __call__(self, log_probs):
        """log_probs (T, K), a numpy array or a tensor on any device -> (sound type of every segment (N,), boundaries (N + 1,))."""
        segments, boundaries = self._segment(log_probs)
        return [self.sound_types[cluster] for cluster in segments], boundaries
