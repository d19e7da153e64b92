"""Urhythmic (fine-grained) conversion inside the package (reference urhythmic/model.py): segmenter -> rhythm model -> time stretcher
-> vocoder, single and batched; the step before it, encode / encode_batch: waveform -> soft units and unit log-probs; and the two
chained, convert_wavs."""
import torch
from torch import nn

from .. import audio
from ..ops import kernels_hubert as KH
from ..ops import kernels_urhythmic as KU
from .hubert import HubertSoft, _host_lens, _inference_only, _wav2
from .rhythm_model import SHORT_SILENCE, RhythmModelFineGrained
from .segmenter import Segmenter, _device_log_probs
from .stretcher import TimeStretcherFineGrained
from .utils import SILENCE

SAMPLING_RATE = 16000        # what HuBERT-Soft takes (urhythmic_convert.py: SAMPLING_RATE)

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
        self._tables = {}        # device -> (the rhythm model's duration table, its copy on that device)

    @torch.inference_mode()
    def forward(self, units: torch.Tensor, log_probs: torch.Tensor) -> torch.Tensor:
        """units (1, D, N), log_probs (1, N, K) -> the converted waveform (1, 1, T)."""
        clusters, boundaries = self.segmenter(log_probs.squeeze(0))
        tgt_durations = self.rhythm_model(clusters, boundaries)
        units = self.time_stretcher(units, clusters, boundaries, tgt_durations)
        return self.vocoder(units)

    def _device_table(self, device):
        """(duration table of the rhythm model on `device`, cluster id of silence): uploaded once per device and table."""
        sound_types = self.segmenter.sound_types
        table = self.rhythm_model.duration_table(sound_types, KU.MAX_T)
        silences = [c for c, t in sound_types.items() if t.value == SILENCE.value]
        if table.shape[0] < 1 or len(silences) > 1:
            raise ValueError("convert_batch: plan=\"device\" (and only that plan) needs sound types that name at least one cluster and at most one "
                             "silence cluster: the plan kernel takes a single silence id; plan=\"host\" and plan=\"table\" have no such limit")
        key = str(device)
        if key not in self._tables or self._tables[key][0] is not table:
            self._tables[key] = (table, torch.from_numpy(table.copy()).to(device))
        return self._tables[key][1], silences[0] if silences else -1

    def _refuse_plan(self, tables, status):
        """A row the plan kernel flagged: raise what the host path raises for it (error path: reads that row's tables back).  Only
        the FIRST flagged row is looked at, and within a row the kernel ranks malformed (2) above unmapped (1): with tables the search
        kernel never writes (a malformed row before or beside an unmapped one) this is a ValueError where the host path would fail in
        its own way.  Status 2 / 3: ValueError naming the row; status 1 on a row the host path maps after all: RuntimeError."""
        b = int(status.nonzero()[0][0])
        if status[b] != 1:
            raise ValueError(f"convert_batch: row {b}: " + ("the output frames add up to more than 2^31 - 1" if status[b] == 3 else
                                                           "the segment tables are malformed (a segment longer than the duration table, or an unknown cluster)"))
        n = int(tables["ncl"][b])
        clusters, boundaries = tables["clusters"][b, :n].tolist(), tables["cboundaries"][b, :n + 1].tolist()
        self.rhythm_model([self.segmenter.sound_types[c] for c in clusters], boundaries)
        raise RuntimeError(f"convert_batch: row {b}: the duration table has no entry for a segment the rhythm model maps: the two paths disagree")

    def _convert_planned(self, units, lp, lens_d):
        tables = self.segmenter.segment_tables(lp, lens_d)
        table, silence = self._device_table(lp.device)
        plan = KU.useg_plan(tables["clusters"], tables["cboundaries"], tables["ncl"], table, silence, SHORT_SILENCE)
        _, totals, status = plan["packed"].cpu().numpy()             # the one host read: 3 B ints
        if status.any():
            self._refuse_plan(tables, status)
        totals = totals.tolist()
        stretched = self.time_stretcher.stretch_planned(units.to(lp.device), plan, max(totals, default=0))
        if stretched.shape[1] == 0:
            return [stretched.new_zeros(0) for _ in totals]
        return self.vocoder.forward_batch(stretched, plan["totals"], host_lens=totals)

    @torch.inference_mode()
    def convert_batch(self, units, log_probs, lens, plan="host"):
        """units (B, D, Nmax) (any strides), log_probs (B, Nmax, K), lens (B) frames of every row (list, CPU or device tensor) ->
        list of B waveforms (1-D), each bit-equal to forward() of its own row, whatever `plan` is.

        plan "host": 2 launches (span scores, search) + 1 (stretch) + the vocoder's (79 in its default configuration), whatever B is.
        One device-to-host read: the segment tables.  The target durations are computed on the host (scipy) from them, two calls
        per segment.  plan "table": the same with the rhythm model's duration table in place of the scipy calls.  plan "device":
        2 (search) + 1 (ops.kernels_urhythmic.useg_plan: duration table -> segment table) + 1 (stretch) + the vocoder's; the segment
        tables stay on the device and the one host read is 3 B ints (segments, output frames and status of every row).  A segment
        length the rhythm model cannot map raises what plan "host" raises.  Plan "device" alone needs at most one silence cluster
        among the segmenter's sound types (ValueError otherwise): the plan kernel takes a single silence id."""
        if plan not in ("host", "table", "device"):
            raise ValueError(f"convert_batch: plan is \"host\", \"table\" or \"device\", got {plan!r}")
        lp = _device_log_probs(log_probs, units.device if units.is_cuda else None)
        if lp.dim() != 3 or units.dim() != 3 or units.shape[0] != lp.shape[0] or units.shape[2] != lp.shape[1]:
            raise ValueError(f"convert_batch: units (B, D, Nmax) and log_probs (B, Nmax, K) expected, got {tuple(units.shape)}, {tuple(lp.shape)}")
        if isinstance(lens, torch.Tensor) and lens.is_cuda:
            lens_d = lens.to(torch.int32).contiguous()
        else:
            lens_d = torch.as_tensor(lens, dtype=torch.int32).to(lp.device)
        if plan == "device":
            return self._convert_planned(units, lp, lens_d)
        table = self.rhythm_model.duration_table(self.segmenter.sound_types, KU.MAX_T) if plan == "table" else None
        _, rows = self.segmenter.segment_batch(lp, lens_d)
        plan_rows = []
        for clusters, boundaries in rows:
            types = [self.segmenter.sound_types[c] for c in clusters]
            if table is None:
                plan_rows.append((types, boundaries, self.rhythm_model(types, boundaries) if types else []))
            else:
                plan_rows.append((types, boundaries, self.rhythm_model.durations_from_table(table, clusters, boundaries)))
        stretched, totals = self.time_stretcher.stretch_batch(units.to(lp.device), plan_rows)
        if stretched.shape[1] == 0:
            return [stretched.new_zeros(0) for _ in totals]
        out_lens = torch.tensor(totals, dtype=torch.int32).to(lp.device)
        return self.vocoder.forward_batch(stretched, out_lens, host_lens=totals)


@torch.inference_mode()
def convert_wavs(hubert: HubertSoft, model: UrhythmicFine, wavs: torch.Tensor, lens, plan="device", sample_rate=SAMPLING_RATE, trim=None):
    """Waveform to waveform: encode_batch, then model.convert_batch.  wavs (B, 1, Tmax), lens (B) samples of every row (list or CPU
    tensor) -> list of B converted waveforms (1-D).  Launches: HuBERT-Soft's + 4 of the search, plan and stretch + the vocoder's
    (plan "device"), whatever B is; one device-to-host read (3 B ints).

    sample_rate other than 16000 and / or trim = dict(top_db=, frame_length=, hop_length=[, pad_mode=]): the waveforms are conditioned
    first as urhythmic_convert.py:160-171 does on the host (audio.condition_batch: resample to 16 kHz, then trim the silence): one
    launch for the resampling, three and one more host read (2 B ints) for the trim.  With the defaults nothing is added."""
    if sample_rate != SAMPLING_RATE or trim is not None:
        config = dict(sampling_rate=SAMPLING_RATE, trim_silence=trim is not None)
        if trim is not None:
            trim = audio._trim_keys(trim)
            config.update(trim_threshold_in_db=trim["top_db"], trim_frame_size=trim["frame_length"], trim_hop_size=trim["hop_length"],
                          trim_pad_mode=trim.get("pad_mode", "constant"))
        wavs, lens = audio.condition_batch(wavs, lens, sample_rate, config)
    units, log_probs, frame_lens = encode_batch(hubert, wavs, lens)
    return model.convert_batch(units, log_probs, frame_lens, plan=plan)
