"""Urhythmic (fine-grained) conversion inside the package (reference urhythmic/model.py): segmenter -> rhythm model -> time stretcher
-> vocoder, single and batched; and the step before it, encode / encode_batch: waveform -> soft units and unit log-probs."""
import torch
from torch import nn

from ..ops import kernels_hubert as KH
from .hubert import HubertSoft, _host_lens, _inference_only, _wav2
from .rhythm_model import RhythmModelFineGrained
from .segmenter import Segmenter, _device_log_probs
from .stretcher import TimeStretcherFineGrained


def _need_hubert(hubert):
    if not isinstance(hubert, HubertSoft):
        raise TypeError("encode: a seq2seq_vc_amd.urhythmic.hubert.HubertSoft expected (load the hub checkpoint's state_dict into one: "
                        "INTEGRATION.md); there is no path through another implementation")


@torch.inference_mode()
def encode(hubert: HubertSoft, wav: torch.Tensor):
    """Encode a waveform into soft speech units and the log probabilities of the associated discrete units (reference
    urhythmic/model.py:22-36).  wav (B, 1, T), every row T samples -> units (B, D, N) fp32, log_probs (B, N, K) fp32."""
    _need_hubert(hubert)
    units = hubert.units(wav)
    log_probs = KH.hubert_logits(units, hubert.label_embedding.weight)
    return units.transpose(1, 2), log_probs


@torch.inference_mode()
def encode_batch(hubert: HubertSoft, wavs: torch.Tensor, lens):
    """wavs (B, 1, Tmax), lens (B) samples of every row (list or CPU tensor) -> units (B, D, Nmax), log_probs (B, Nmax, K), frame_lens (B)
    int32 on the CPU: what UrhythmicFine.convert_batch takes.  Every row is computed from its own samples only; units and log_probs are
    zero beyond a row's frames."""
    _need_hubert(hubert)
    _inference_only(hubert, wavs, grad_ok=True)
    units, frame_lens, frame_lens_dev = hubert._units(_wav2(wavs), _host_lens(lens), True)
    log_probs = KH.hubert_logits(units, hubert.label_embedding.weight, lens=frame_lens_dev)
    return units.transpose(1, 2), log_probs, torch.tensor(frame_lens, dtype=torch.int32)


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
