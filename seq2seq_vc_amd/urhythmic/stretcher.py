"""Urhythmic time stretchers (reference urhythmic/stretcher.py) on the resampling kernel of csrc/urhythmic.hip: every segment is
linearly resampled to its target duration on its own (F.interpolate(mode="linear"), no neighbour across a boundary) and the pieces
stand side by side.  One launch for a whole batch; the bookkeeping (which segments survive, where they land) is host code
(stretch_batch) or the plan kernel's (stretch_planned: ops.kernels_urhythmic.useg_plan, the same two filters on the device)."""
import math

import numpy as np
import torch

from ..ops import kernels_urhythmic as KU
from .rhythm_model import SHORT_SILENCE
from .utils import SILENCE


def stretch_plan(clusters, boundaries, tgt_durations):
    """The reference's two filters as a table: silences of at most 3 frames are dropped, the remaining segments pair up with the
    target durations in order, and a pair whose duration is <= 0 is dropped -> [(source start, source length, target length)]."""
    kept = [(t0, tn - t0) for cluster, t0, tn in zip(clusters, boundaries[:-1], boundaries[1:])
            if not cluster.value == SILENCE.value or tn - t0 > SHORT_SILENCE]
    return [(int(t0), int(n), int(d)) for (t0, n), d in zip(kept, tgt_durations) if d > 0]


def segment_table(plans, device):
    """[[(start, length, target)]] per row -> (seg (B, Smax, 4) int32 with the exclusive prefix sum of the targets in column 3, nsegs (B)
    int32, both on `device`; output frames of every row)."""
    smax = max(1, max((len(p) for p in plans), default=1))
    seg = np.zeros((len(plans), smax, 4), np.int32)
    totals = []
    for b, plan in enumerate(plans):
        off = 0
        for j, (start, length, target) in enumerate(plan):
            seg[b, j] = (start, length, target, off)
            off += target
        totals.append(off)
    nsegs = np.array([len(p) for p in plans], np.int32)
    return torch.from_numpy(seg).to(device), torch.from_numpy(nsegs).to(device), totals


def _check_units(units):
    if units.dim() != 3:
        raise ValueError(f"units (B, D, T) expected, got {tuple(units.shape)}")


class TimeStretcherFineGrained:
    """Time stretching block (fine-grained): up/down samples the speech units to match the target rhythm."""

    def stretch_batch(self, units, rows):
        """units (B, D, Tmax), any strides (fp32 / bf16); rows: (sound types, boundaries, target durations) per utterance ->
        (stretched (B, Nmax, D) fp32 channel-last, zero past each row's own frames -- what HifiganGenerator.forward_batch takes --,
        output frames of every row).  One launch whatever B is."""
        _check_units(units)
        if len(rows) != units.shape[0]:
            raise ValueError("stretch_batch: one (sound types, boundaries, target durations) per row of units")
        plans = [stretch_plan(*row) for row in rows]
        for plan in plans:
            if any(start < 0 or length < 1 or start + length > units.shape[2] for start, length, _ in plan):
                raise ValueError("stretch_batch: a segment lies outside the units")
        seg, nsegs, totals = segment_table(plans, units.device)
        return KU.useg_stretch(units, seg, nsegs, max(totals, default=0), channel_dim=1), totals

    def stretch_planned(self, units, plan, n_out):
        """units (B, D, Tmax) as for stretch_batch; plan: what ops.kernels_urhythmic.useg_plan returned for the segmentation of these
        units (its segment table stays on the device); n_out: the largest of the plan's totals -> stretched (B, n_out, D) fp32
        channel-last, zero past each row's own frames.  One launch whatever B is."""
        _check_units(units)
        seg = plan["seg"]
        if seg.dim() != 3 or seg.shape[0] != units.shape[0] or seg.shape[1] != units.shape[2]:
            raise ValueError(f"stretch_planned: a plan of {units.shape[0]} rows of {units.shape[2]} frames expected, got seg {tuple(seg.shape)}")
        return KU.useg_stretch(units, seg, plan["nsegs"], int(n_out), channel_dim=1)

    def __call__(self, units, clusters, boundaries, tgt_duartations):
        """units (1, D, T), sound types (N,), boundaries (N + 1,), target durations -> up/down sampled units (1, D, T')."""
        _check_units(units)
        if units.shape[0] != 1:
            raise ValueError("TimeStretcherFineGrained: one utterance per call (stretch_batch takes a batch)")
        out, totals = self.stretch_batch(units, [(clusters, boundaries, tgt_duartations)])
        if totals[0] == 0:
            raise ValueError("TimeStretcherFineGrained: no segment is left after the filters")
        return out.transpose(1, 2)


class TimeStretcherGlobal:
    """Time stretching block (global): up/down samples the speech units to match the target speaking rate."""

    def __call__(self, units, ratio: float):
        """units (B, D, T), ratio between the source and target speaking rates -> (B, D, floor(T * ratio)), as
        F.interpolate(units, scale_factor=ratio, mode="linear") (the source step is 1 / ratio, not T / output length)."""
        _check_units(units)
        B, _, T = units.shape
        n = int(math.floor(float(T) * float(ratio)))
        if ratio <= 0 or n < 1:
            raise ValueError(f"TimeStretcherGlobal: ratio {ratio} leaves no frame of {T}")
        seg, nsegs, _ = segment_table([[(0, T, n)]] * B, units.device)
        return KU.useg_stretch(units, seg, nsegs, n, channel_dim=1, scale=1.0 / float(ratio)).transpose(1, 2)
