"""Launchers of the waveform-conditioning kernels (csrc/audio.hip; C ABI in include/s2svc_hip.h): banded polyphase resampling
(torchaudio.functional.resample at its defaults) and silence trimming (librosa.effects.trim) of padded batches with per-row lengths.
fp32, non-differentiable, GPU tensors only; no launcher waits for the device."""
import math
from collections import namedtuple

import numpy as np
import torch

from .. import _lib
from .kernels import _need_cuda, ptr, stream

TILE = 1024                  # outputs per workgroup of the resampler (s2svc_resample_tile)
MAX_SPAN = 12288             # input samples a workgroup may stage: 48 KiB of LDS (s2svc_resample_max_span)
MAX_TABLE = 1 << 20          # taps (Kb * new) a table may hold: 4 MiB
MAX_LEN = 2**31 - 1
MAX_B = 65535
AMIN = 1e-10                 # librosa's floor under the frame POWER (amplitude_to_db's amin = 1e-5, squared)
LAUNCHES = 0                 # launches queued by this module since import (tests and the bench read the difference around a call)

# taps (Kb, new) fp32 and first (new) int32 on the device; orig / new after division by their gcd; fmin / fmax: the range of first
PolyTable = namedtuple("PolyTable", "taps first orig new width Kb fmin fmax")
_TABLES = {}


def _count():
    global LAUNCHES
    LAUNCHES += 1


def reduced(orig_freq, new_freq):
    """(orig, new) divided by their gcd; ValueError unless both are positive integers."""
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"resample: positive integer frequencies expected, got {orig_freq!r}, {new_freq!r}")
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def out_length(n, orig, new):
    """Samples torchaudio keeps of a row of n: ceil(new n / orig), in integers."""
    return -((-int(new) * int(n)) // int(orig))


def span_of(orig, new, Kb, fmin, fmax):
    """Input samples one workgroup stages (the formula of s2svc_resample_poly)."""
    return ((new + TILE - 2) // new) * orig + (fmax - fmin) + Kb


def banded_taps(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The windowed-sinc kernel of torchaudio's _get_sinc_resample_kernel (sinc_interp_hann) in float64, banded: per phase the taps
    whose argument stayed inside the clamp.  -> (taps (Kb, new) fp32, every dropped or absent entry 0; first (new) int32; orig, new, width)."""
    orig, new = reduced(orig_freq, new_freq)
    lpw = int(lowpass_filter_width)
    if lpw < 1 or not 0.0 < float(rolloff) <= 1.0:
        raise ValueError("resample: lowpass_filter_width >= 1 and 0 < rolloff <= 1 expected")
    base = min(orig, new) * float(rolloff)
    width = int(math.ceil(lpw * orig / base))
    if (2 * width + orig) * new > 64 * MAX_TABLE:
        raise ValueError(f"resample: {orig_freq} -> {new_freq} Hz needs a dense kernel of {(2 * width + orig) * new} taps; reduce the ratio")
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -lpw, lpw)
    window = np.cos(t * math.pi / lpw / 2) ** 2
    tp = t * math.pi
    safe = np.where(tp == 0, 1.0, tp)
    dense = np.where(tp == 0, 1.0, np.sin(safe) / safe) * window * (base / orig)
    inside = np.abs(t) < lpw
    counts = inside.sum(1)
    if counts.min() < 1:
        raise ValueError("resample: a phase without a tap inside the window")
    first = inside.argmax(1).astype(np.int32)
    Kb = int(counts.max())
    cols = first[:, None].astype(np.int64) + np.arange(Kb)[None, :]                   # (new, Kb)
    ok = (cols < dense.shape[1])
    cols_c = np.minimum(cols, dense.shape[1] - 1)
    band = np.where(ok & np.take_along_axis(inside, cols_c, 1), np.take_along_axis(dense, cols_c, 1), 0.0)
    return np.ascontiguousarray(band.T.astype(np.float32)), first, orig, new, width


def make_table(taps, first, orig, new, width, device):
    """A PolyTable from host arrays: taps (Kb, new) (any values: the tests pass integers), first (new).  ValueError beyond the caps."""
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float32))
    first = np.ascontiguousarray(np.asarray(first, dtype=np.int32))
    if taps.ndim != 2 or taps.shape[1] != new or taps.shape[0] < 1 or first.shape != (new,):
        raise ValueError(f"resample table: taps (Kb, {new}) and first ({new}) expected, got {taps.shape}, {first.shape}")
    Kb, fmin, fmax = taps.shape[0], int(first.min()), int(first.max())
    if fmin < 0 or fmax > 2 * width + orig:
        raise ValueError(f"resample table: first tap indices outside [0, 2 width + orig = {2 * width + orig}]")
    if Kb * new > MAX_TABLE:
        raise ValueError(f"resample table: {Kb} x {new} taps exceed the cap of {MAX_TABLE}")
    if span_of(orig, new, Kb, fmin, fmax) > MAX_SPAN:
        raise ValueError(f"resample: {orig} / {new} makes one workgroup stage {span_of(orig, new, Kb, fmin, fmax)} samples, above the cap of {MAX_SPAN}")
    return PolyTable(torch.from_numpy(taps).to(device), torch.from_numpy(first).to(device), int(orig), int(new), int(width), Kb, fmin, fmax)


def poly_table(orig_freq, new_freq, device, lowpass_filter_width=6, rolloff=0.99):
    """The cached device table of a rate pair: built once per (orig, new, lowpass_filter_width, rolloff, device)."""
    orig, new = reduced(orig_freq, new_freq)
    key = (orig, new, int(lowpass_filter_width), float(rolloff), str(torch.device(device)))
    if key not in _TABLES:
        taps, first, orig, new, width = banded_taps(orig, new, lowpass_filter_width, rolloff)
        _TABLES[key] = make_table(taps, first, orig, new, width, device)
    return _TABLES[key]


def _wavs2(wavs, name="wavs"):
    if wavs.dim() != 2 or wavs.dtype != torch.float32 or not wavs.is_contiguous():
        raise ValueError(f"{name}: a contiguous fp32 (B, Nmax) batch expected, got {wavs.dtype} {tuple(wavs.shape)}")
    if wavs.shape[0] > MAX_B:
        raise ValueError(f"{name}: up to {MAX_B} rows, got {wavs.shape[0]}")
    if wavs.shape[1] > MAX_LEN:
        raise ValueError(f"{name}: rows of up to 2^31 - 1 samples, got {wavs.shape[1]}")
    return wavs.shape


def check_lens(lens, B, Nmax):
    lens = [int(n) for n in lens]
    if len(lens) != B or any(n < 0 or n > Nmax for n in lens):
        raise ValueError(f"lens: {B} lengths in [0, {Nmax}] expected, got {lens}")
    return lens


def resample_poly(wavs, lens, table, out=None):
    """wavs (B, Nmax) fp32, lens: B host ints, table: a PolyTable -> (out (B, Mmax) fp32, out_lens: host list, ceil(new n / orig)),
    Mmax = max(out_lens); rows are +0 beyond their length.  `out` (tests): a (B, Mmax) buffer to write instead.  One launch
    whatever B is; the lengths travel to the device, nothing travels back."""
    B, Nmax = _wavs2(wavs)
    lens = check_lens(lens, B, Nmax)
    out_lens = [out_length(n, table.orig, table.new) for n in lens]
    Mmax = max(out_lens, default=0)
    if Mmax > MAX_LEN:
        raise ValueError(f"resample: an output row of {Mmax} samples exceeds 2^31 - 1")
    if (tuple(table.taps.shape) != (table.Kb, table.new) or table.taps.dtype != torch.float32 or not table.taps.is_contiguous()
            or tuple(table.first.shape) != (table.new,) or table.first.dtype != torch.int32 or not table.first.is_contiguous()):
        raise ValueError("resample table: taps (Kb, new) fp32 and first (new) int32 expected, as make_table builds them")
    _need_cuda(wavs, table.taps, table.first, out)
    if out is None:
        out = torch.empty(B, Mmax, dtype=torch.float32, device=wavs.device)
    elif tuple(out.shape) != (B, Mmax) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out: contiguous fp32 {(B, Mmax)} expected, got {out.dtype} {tuple(out.shape)}")
    if B == 0 or Mmax == 0:
        return out, out_lens
    both = torch.tensor([lens, out_lens], dtype=torch.int32).to(wavs.device)
    _lib.check(_lib.lib().s2svc_resample_poly(B, Nmax, Mmax, table.orig, table.new, table.width, table.Kb, table.fmin, table.fmax, ptr(wavs),
                                              ptr(both[0]), ptr(both[1]), ptr(table.taps), ptr(table.first), ptr(out), stream()), "resample_poly")
    _count()
    return out, out_lens


def check_trim_args(top_db, frame_length, hop_length, pad_mode):
    if int(frame_length) != frame_length or int(hop_length) != hop_length or frame_length < 1 or hop_length < 1:
        raise ValueError(f"trim: positive integer frame_length and hop_length expected, got {frame_length!r}, {hop_length!r}")
    if not float(top_db) >= 0.0:
        raise ValueError(f"trim: top_db must not be negative, got {top_db!r}")
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"trim: pad_mode is \"constant\" or \"reflect\", got {pad_mode!r}")
    return int(frame_length), int(hop_length)


def trim_intervals(wavs, lens_d, nfmax, top_db=60, frame_length=2048, hop_length=512, pad_mode="constant"):
    """wavs (B, Nmax) fp32, lens_d (B) int32 on the device, nfmax = 1 + max(lens) // hop_length -> intervals (B, 2) int32 on the
    device: (start, end) of librosa.effects.trim per row, (0, 0) for a row without a non-silent frame.  Two launches whatever B is."""
    B, Nmax = _wavs2(wavs)
    frame_length, hop_length = check_trim_args(top_db, frame_length, hop_length, pad_mode)
    if lens_d.dtype != torch.int32 or not lens_d.is_contiguous() or lens_d.numel() != B:
        raise ValueError(f"lens_d: a contiguous int32 tensor of {B} values expected, got {lens_d.dtype} {tuple(lens_d.shape)}")
    nfmax = int(nfmax)
    if not 1 <= nfmax <= 1 + Nmax // hop_length:
        raise ValueError(f"nfmax: 1 .. 1 + Nmax // hop_length = {1 + Nmax // hop_length} expected, got {nfmax}")
    _need_cuda(wavs, lens_d)
    intervals = torch.empty(B, 2, dtype=torch.int32, device=wavs.device)
    if B == 0:
        return intervals
    power = torch.empty(B, nfmax, dtype=torch.float64, device=wavs.device)
    L = _lib.lib()
    _lib.check(L.s2svc_trim_frames(B, Nmax, nfmax, frame_length, hop_length, int(pad_mode == "reflect"), ptr(wavs), ptr(lens_d), ptr(power),
                                   stream()), "trim_frames")
    _count()
    _lib.check(L.s2svc_trim_intervals(B, Nmax, nfmax, hop_length, AMIN, 10.0 ** (-float(top_db) / 10.0), ptr(lens_d), ptr(power),
                                      ptr(intervals), stream()), "trim_intervals")
    _count()
    return intervals


def wav_gather_rows(wavs, intervals, Mmax, gain=1.0):
    """out (B, Mmax)[b, i] = wavs[b, start_b + i] * gain for i < end_b - start_b, +0 beyond; intervals (B, 2) int32 on the device.
    One launch whatever B is."""
    B, Nmax = _wavs2(wavs)
    if intervals.dtype != torch.int32 or not intervals.is_contiguous() or tuple(intervals.shape) != (B, 2):
        raise ValueError(f"intervals: a contiguous int32 ({B}, 2) tensor expected, got {intervals.dtype} {tuple(intervals.shape)}")
    Mmax = int(Mmax)
    if not 0 <= Mmax <= MAX_LEN:
        raise ValueError(f"Mmax: 0 .. 2^31 - 1 expected, got {Mmax}")
    _need_cuda(wavs, intervals)
    out = torch.empty(B, Mmax, dtype=torch.float32, device=wavs.device)
    if B == 0 or Mmax == 0:
        return out
    _lib.check(_lib.lib().s2svc_wav_gather_rows(B, Nmax, Mmax, float(gain), ptr(wavs), ptr(intervals), ptr(out), stream()), "wav_gather_rows")
    _count()
    return out
