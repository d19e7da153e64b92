"""Urhythmic (fine-grained) conversion inside the package (reference urhythmic/model.py): segmenter -> rhythm model -> time stretcher
-> vocoder, single and batched."""
import torch
from torch import nn

from .rhythm_model import RhythmModelFineGrained
from .segmenter import Segmenter, _device_log_probs
from .stretcher import TimeStretcherFineGrained


class UrhythmicFine(nn.Module):
    """Voice and rhythm conversion that needs neither text nor parallel data.  segmenter: groups the units into segments of three
    sound types; rhythm_model: maps every segment's duration to the target speaker's; time_stretcher: resamples the units to these
    durations; vocoder (vocoder.HifiganGenerator with in_channels = unit width): units -> waveform."""

    def __init__(self, segmenter: Segmenter, rhythm_model: RhythmModelFineGrained, time_stretcher: TimeStretcherFineGrained, vocoder):
        super().__init__()
        self.segmenter = segmenter
        self.rhythm_model = rhythm_model
        self.time_stretcher = time_stretcher
        self.vocoder = vocoder

    @torch.inference_mode()
    def forward(self, units: torch.Tensor, log_probs: torch.Tensor) -> torch.Tensor:
        """units (1, D, N), log_probs (1, N, K) -> the converted waveform (1, 1, T)."""
        clusters, boundaries = self.segmenter(log_probs.squeeze(0))
        tgt_durations = self.rhythm_model(clusters, boundaries)
        units = self.time_stretcher(units, clusters, boundaries, tgt_durations)
        return self.vocoder(units)

    @torch.inference_mode()
    def convert_batch(self, units, log_probs, lens):
        """units (B, D, Nmax) (any strides), log_probs (B, Nmax, K), lens (B) frames of every row (list, CPU or device tensor) ->
        list of B waveforms (1-D), each bit-equal to forward() of its own row.

        Launches: 2 (span scores, search) + 1 (stretch) + the vocoder's (79 in its default configuration), whatever B is.  One
        device-to-host read: the segment tables.  The target durations are computed on the host (scipy) from them."""
        lp = _device_log_probs(log_probs, units.device if units.is_cuda else None)
        if lp.dim() != 3 or units.dim() != 3 or units.shape[0] != lp.shape[0] or units.shape[2] != lp.shape[1]:
            raise ValueError(f"convert_batch: units (B, D, Nmax) and log_probs (B, Nmax, K) expected, got {tuple(units.shape)}, {tuple(lp.shape)}")
        if isinstance(lens, torch.Tensor) and lens.is_cuda:
            lens_d = lens.to(torch.int32).contiguous()
        else:
            lens_d = torch.as_tensor(lens, dtype=torch.int32).to(lp.device)
        _, rows = self.segmenter.segment_batch(lp, lens_d)
        plan_rows = []
        for clusters, boundaries in rows:
            types = [self.segmenter.sound_types[c] for c in clusters]
            plan_rows.append((types, boundaries, self.rhythm_model(types, boundaries) if types else []))
        stretched, totals = self.time_stretcher.stretch_batch(units.to(lp.device), plan_rows)
        if stretched.shape[1] == 0:
            return [stretched.new_zeros(0) for _ in totals]
        out_lens = torch.tensor(totals, dtype=torch.int32).to(lp.device)
        return self.vocoder.forward_batch(stretched, out_lens, host_lens=totals)
