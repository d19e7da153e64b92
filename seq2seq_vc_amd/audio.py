"""Waveform conditioning on HIP: what the reference's scripts do on the host, one utterance at a time, before either pipeline sees a
waveform (urhythmic_convert.py:160-171, urhythmic_encode.py:122-133, urhythmic_resample.py:27-31, bin/preprocess.py:207-221, :250):
resample, trim the silence, apply the global gain.  Here: padded batches with per-row lengths, GPU tensors, fp32, inference only.

resample / resample_batch: torchaudio.functional.resample(wav, orig_freq, new_freq) at its defaults (sinc_interp_hann,
lowpass_filter_width = 6, rolloff = 0.99), the filter built in float64 and rounded once to fp32.  This is NOT librosa.resample's
soxr filter: a recipe that resampled with librosa gets slightly different samples.
trim_batch: librosa.effects.trim(y, top_db, frame_length, hop_length), pad_mode "constant" (librosa >= 0.10) or "reflect" (0.9).
Every row of a batch equals its own B = 1 call bit for bit; samples beyond lens[b] are never read."""
import torch

from .ops import kernels_audio as KA


def _host_lens(lens):
    if isinstance(lens, torch.Tensor):
        if lens.is_cuda:
            raise ValueError("lens: a list or a CPU tensor expected (the output lengths are computed on the host, without a device read)")
        return [int(n) for n in lens.tolist()]
    return [int(n) for n in lens]


def _wav2(wavs):
    if wavs.dim() != 3 or wavs.shape[1] != 1:
        raise ValueError(f"wavs: (B, 1, Nmax) expected, got {tuple(wavs.shape)}")
    if wavs.dtype != torch.float32:
        raise ValueError(f"wavs: float32 expected, got {wavs.dtype}")
    if not wavs.is_cuda:
        raise RuntimeError("seq2seq_vc_amd.audio needs GPU tensors (there is no CPU path)")
    return wavs[:, 0].contiguous()


def _trim_keys(trim):
    if set(trim) != {"top_db", "frame_length", "hop_length"} and set(trim) != {"top_db", "frame_length", "hop_length", "pad_mode"}:
        raise ValueError(f"trim: dict(top_db=, frame_length=, hop_length=[, pad_mode=]) expected, got keys {sorted(trim)}")
    return dict(trim)


@torch.inference_mode()
def resample(wav, orig_freq, new_freq):
    """torchaudio.functional.resample(wav, orig_freq, new_freq): wav (..., N) fp32 on the GPU, every row N samples ->
    (..., ceil(new N / orig)).  orig_freq == new_freq returns wav itself.  One launch."""
    orig, new = KA.reduced(orig_freq, new_freq)
    if wav.dim() < 1 or wav.dtype != torch.float32:
        raise ValueError(f"wav: float32 (..., N) expected, got {wav.dtype} {tuple(wav.shape)}")
    if not wav.is_cuda:
        raise RuntimeError("seq2seq_vc_amd.audio needs GPU tensors (there is no CPU path)")
    if orig == new:
        return wav
    flat = wav.reshape(-1, wav.shape[-1]).contiguous()
    out, _ = KA.resample_poly(flat, [flat.shape[1]] * flat.shape[0], KA.poly_table(orig, new, wav.device))
    return out.view(*wav.shape[:-1], out.shape[1])


@torch.inference_mode()
def resample_batch(wavs, lens, orig_freq, new_freq):
    """wavs (B, 1, Nmax) fp32, lens (B) samples of every row (list or CPU tensor) -> (out (B, 1, Mmax), out_lens): out_lens a host list,
    ceil(new n / orig) per row, no device read; rows are zero beyond their length.  orig_freq == new_freq returns (wavs, lens) with
    no launch.  One launch whatever B is."""
    orig, new = KA.reduced(orig_freq, new_freq)
    w = _wav2(wavs)
    lens = KA.check_lens(_host_lens(lens), w.shape[0], w.shape[1])
    if orig == new:
        return wavs, lens
    out, out_lens = KA.resample_poly(w, lens, KA.poly_table(orig, new, wavs.device))
    return out.unsqueeze(1), out_lens


def _trim(w, lens, top_db, frame_length, hop_length, pad_mode, gain):
    frame_length, hop_length = KA.check_trim_args(top_db, frame_length, hop_length, pad_mode)
    B = w.shape[0]
    if B == 0:
        return w.new_zeros(0, 1, 0), [], torch.zeros(0, 2, dtype=torch.int32)
    lens_d = torch.tensor(lens, dtype=torch.int32).to(w.device)
    iv_d = KA.trim_intervals(w, lens_d, 1 + max(lens) // hop_length, top_db, frame_length, hop_length, pad_mode)
    intervals = iv_d.cpu()                                          # the one host read: 2 B ints
    out_lens = (intervals[:, 1] - intervals[:, 0]).tolist()
    out = KA.wav_gather_rows(w, iv_d, max(out_lens), gain)
    return out.unsqueeze(1), out_lens, intervals


@torch.inference_mode()
def trim_batch(wavs, lens, top_db=60, frame_length=2048, hop_length=512, pad_mode="constant"):
    """librosa.effects.trim per row: wavs (B, 1, Nmax) fp32, lens (B) (list or CPU tensor) -> (out (B, 1, Mmax): every row's
    non-silent interval moved to offset 0, zero beyond it; out_lens: host list; intervals: CPU int32 (B, 2) of (start, end), (0, 0)
    for a row without a non-silent frame).  Three launches whatever B is (two when every interval is empty: there is nothing to
    gather), one device-to-host read of 2 B ints."""
    w = _wav2(wavs)
    lens = KA.check_lens(_host_lens(lens), w.shape[0], w.shape[1])
    return _trim(w, lens, top_db, frame_length, hop_length, pad_mode, 1.0)


def _config(fs, config):
    target = config["sampling_rate"]
    KA.reduced(fs, target)
    trim = None
    if config.get("trim_silence", False):
        trim = dict(top_db=config["trim_threshold_in_db"], frame_length=config["trim_frame_size"], hop_length=config["trim_hop_size"],
                    pad_mode=config.get("trim_pad_mode", "constant"))
        KA.check_trim_args(**trim)
    gain = float(config.get("global_gain_scale", 0.0))
    return int(target), trim, (gain if gain > 0.0 else 1.0)


@torch.inference_mode()
def condition_batch(wavs, lens, fs, config):
    """The reference's order (bin/preprocess.py:207-221, :250): resample fs -> config["sampling_rate"] if they differ, trim if
    config["trim_silence"] (trim_threshold_in_db, trim_frame_size, trim_hop_size; optional trim_pad_mode), then the gain
    config["global_gain_scale"] where it is > 0 (applied by the trim's gather; without a trim, by one gather of its own).
    -> (out (B, 1, Mmax), out_lens: host list), what urhythmic.encode_batch and frontend.logmelfilterbank_batch(..., lengths=) take."""
    target, trim, gain = _config(fs, config)
    w = _wav2(wavs)
    lens = KA.check_lens(_host_lens(lens), w.shape[0], w.shape[1])
    orig, new = KA.reduced(fs, target)
    if orig != new:
        w, lens = KA.resample_poly(w, lens, KA.poly_table(orig, new, wavs.device))
    if trim is not None:
        out, out_lens, _ = _trim(w, lens, gain=gain, **trim)
        return out, out_lens
    if gain != 1.0 and w.shape[0] > 0:
        iv = torch.tensor([[0, n] for n in lens], dtype=torch.int32).to(w.device)
        w = KA.wav_gather_rows(w, iv, max(lens), gain)
    return w.unsqueeze(1), lens


def launch_plan(what="condition", fs=None, config=None, orig_freq=None, new_freq=None):
    """The launches of one call, in order, whatever B is.  what: "resample" (orig_freq, new_freq), "trim", or "condition" (fs, config)."""
    if what == "resample":
        return [] if KA.reduced(orig_freq, new_freq)[0] == KA.reduced(orig_freq, new_freq)[1] else ["s2svc_resample_poly"]
    if what == "trim":
        return ["s2svc_trim_frames", "s2svc_trim_intervals", "s2svc_wav_gather_rows"]
    if what != "condition":
        raise ValueError(f"launch_plan: what is \"resample\", \"trim\" or \"condition\", got {what!r}")
    target, trim, gain = _config(fs, config)
    plan = launch_plan("resample", orig_freq=fs, new_freq=target)
    if trim is not None:
        return plan + launch_plan("trim")
    return plan + (["s2svc_wav_gather_rows"] if gain != 1.0 else [])
