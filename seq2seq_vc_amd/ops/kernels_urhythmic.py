"""Launchers of the urhythmic kernels (csrc/urhythmic.hip; C ABI in include/s2svc_hip.h): segmentation search, stretch plan and
segment-wise linear resampling.  Non-differentiable, GPU tensors only; every argument is device-resident, so no launcher waits for the device."""
import torch

from .. import _lib
from .kernels import _need_cuda, ptr, stream

MAX_K = 256                  # units (the hub model has 100)
MAX_T = 4096                 # frames per utterance
LAUNCHES = 0                 # launches queued by this module since import (tests and the bench read the difference around a call)


def _count():
    global LAUNCHES
    LAUNCHES += 1


def _i32c(t, n, name):
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{name}: a contiguous int32 tensor of {n} values expected, got {t.dtype} {tuple(t.shape)}")


def check_segment_args(log_probs, lens, labels=None):
    """Shape / dtype / limit checks of useg_segment (ValueError), before any device work."""
    if log_probs.dim() != 3:
        raise ValueError(f"log_probs: (B, Tmax, K) expected, got {tuple(log_probs.shape)}")
    B, Tmax, K = log_probs.shape
    if log_probs.dtype != torch.float32 or not log_probs.is_contiguous():
        raise ValueError(f"log_probs: contiguous fp32 expected, got {log_probs.dtype}")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"the segmentation search supports 1 .. {MAX_K} units, got K = {K}")
    if not 1 <= Tmax <= MAX_T:
        raise ValueError(f"the segmentation search supports 1 .. {MAX_T} frames, got Tmax = {Tmax}")
    _i32c(lens, B, "lens")
    if labels is not None:
        _i32c(labels, K, "labels")
    return B, Tmax, K


def useg_segment(log_probs, lens, gamma, labels=None, want_tables=False):
    """log_probs (B, Tmax, K) fp32, lens (B) int32 -> dict of device tensors: codes (B, Tmax), boundaries (B, Tmax + 1), nseg (B);
    with labels ((K) int32, unit -> cluster) also clusters (B, Tmax), cboundaries (B, Tmax + 1), ncl (B) and `packed`, the one flat
    int32 buffer [ncl | clusters | cboundaries] these three are views of (one device-to-host copy fetches all of them);
    want_tables: alpha (B, Tmax + 1) fp32 and P (B, Tmax + 1, 2) int32.  Two launches whatever B is."""
    B, Tmax, K = check_segment_args(log_probs, lens, labels)
    _need_cuda(log_probs, lens, labels)
    dev = log_probs.device
    L = _lib.lib()
    ws = torch.empty(L.s2svc_useg_ws_bytes(B, Tmax, K) // 8 + 1, dtype=torch.int64, device=dev)
    out = dict(codes=torch.empty(B, Tmax, dtype=torch.int32, device=dev), boundaries=torch.empty(B, Tmax + 1, dtype=torch.int32, device=dev),
               nseg=torch.empty(B, dtype=torch.int32, device=dev), alpha=None, P=None, clusters=None, cboundaries=None, ncl=None, packed=None)
    if want_tables:
        out["alpha"] = torch.empty(B, Tmax + 1, dtype=torch.float32, device=dev)
        out["P"] = torch.empty(B, Tmax + 1, 2, dtype=torch.int32, device=dev)
    if labels is not None:
        packed = torch.empty(B * (2 * Tmax + 2), dtype=torch.int32, device=dev)
        out.update(packed=packed, ncl=packed[:B], clusters=packed[B:B + B * Tmax].view(B, Tmax), cboundaries=packed[B + B * Tmax:].view(B, Tmax + 1))
    _lib.check(L.s2svc_useg_spans(B, Tmax, K, ptr(log_probs), ptr(lens), ptr(ws), stream()), "useg_spans")
    _count()
    _lib.check(L.s2svc_useg_search(B, Tmax, float(gamma), ptr(lens), ptr(ws), ptr(labels), ptr(out["codes"]), ptr(out["boundaries"]),
                                   ptr(out["nseg"]), ptr(out["alpha"]), ptr(out["P"]), ptr(out["clusters"]), ptr(out["cboundaries"]),
                                   ptr(out["ncl"]), stream()), "useg_search")
    _count()
    return out


def check_stretch_args(units, seg, nsegs, n_out, channel_dim=1):
    if units.dim() != 3:
        raise ValueError(f"units: three dimensions expected, got {tuple(units.shape)}")
    if channel_dim not in (1, 2):
        raise ValueError("channel_dim is 1 ((B, C, N), the reference's layout) or 2 ((B, N, C))")
    if units.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"units: float32 or bfloat16 expected, got {units.dtype}")
    B = units.shape[0]
    C, N = units.shape[channel_dim], units.shape[3 - channel_dim]
    if C < 1 or N < 1:
        raise ValueError("units: at least one channel and one frame")
    if seg.dim() != 3 or seg.shape[0] != B or seg.shape[2] != 4 or seg.shape[1] < 1 or seg.dtype != torch.int32 or not seg.is_contiguous():
        raise ValueError(f"seg: a contiguous int32 (B, Smax, 4) table expected, got {seg.dtype} {tuple(seg.shape)}")
    _i32c(nsegs, B, "nsegs")
    if int(n_out) < 0:
        raise ValueError("n_out must not be negative")
    return B, N, C


def useg_stretch(units, seg, nsegs, n_out, channel_dim=1, scale=0.0):
    """units (B, C, N) (channel_dim = 1) or (B, N, C) (channel_dim = 2), any strides, fp32 / bf16; seg (B, Smax, 4) int32 rows of
    (source start, source length, target length, exclusive prefix sum of the target lengths); nsegs (B) int32
    -> (B, n_out, C) fp32 channel-last, zero past every row's own frames.  One launch whatever B is."""
    B, N, C = check_stretch_args(units, seg, nsegs, n_out, channel_dim)
    _need_cuda(units, seg, nsegs)
    out = torch.empty(B, int(n_out), C, dtype=torch.float32, device=units.device)
    if B == 0 or n_out == 0:
        return out
    st, sc = units.stride(3 - channel_dim), units.stride(channel_dim)
    _lib.check(_lib.lib().s2svc_useg_stretch(0 if units.dtype == torch.float32 else 1, B, N, C, ptr(units), units.stride(0), st, sc, ptr(seg),
                                             ptr(nsegs), seg.shape[1], int(n_out), float(scale), ptr(out), stream()), "useg_stretch")
    _count()
    return out


def check_plan_args(clusters, cboundaries, ncl, table):
    """Shape / dtype / limit checks of useg_plan (ValueError), before any device work."""
    if clusters.dim() != 2 or clusters.dtype != torch.int32 or not clusters.is_contiguous():
        raise ValueError(f"clusters: a contiguous int32 (B, Tmax) table expected, got {clusters.dtype} {tuple(clusters.shape)}")
    B, Tmax = clusters.shape
    if not 1 <= Tmax <= MAX_T:
        raise ValueError(f"the stretch plan supports 1 .. {MAX_T} frames, got Tmax = {Tmax}")
    if B > 65535:
        raise ValueError(f"the stretch plan supports up to 65535 rows, got B = {B}")
    if cboundaries.dim() != 2 or tuple(cboundaries.shape) != (B, Tmax + 1):
        raise ValueError(f"cboundaries: (B, Tmax + 1) = ({B}, {Tmax + 1}) expected, got {tuple(cboundaries.shape)}")
    _i32c(cboundaries, B * (Tmax + 1), "cboundaries")
    _i32c(ncl, B, "ncl")
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 1 or table.dtype != torch.int32 or not table.is_contiguous():
        raise ValueError(f"table: a contiguous int32 (n_clusters, Lmax + 1) duration table expected, got {table.dtype} {tuple(table.shape)}")
    return B, Tmax


def useg_plan(clusters, cboundaries, ncl, table, silence_cluster, short_silence=3):
    """The stretch plan on the device.  clusters (B, Tmax), cboundaries (B, Tmax + 1), ncl (B): the merged clusters of useg_segment;
    table (n_clusters, Lmax + 1) int32: RhythmModelFineGrained.duration_table -> dict of device tensors: seg (B, Tmax, 4), what
    useg_stretch reads with Smax = Tmax, and nsegs, totals (output frames), status (0 ok, 1 unmapped length, 2 malformed input,
    3 total above INT32_MAX), each (B) and a view of the one (3, B) int32 buffer `packed` (one device-to-host copy fetches all three).
    A row whose status is not 0 has nsegs = totals = 0.  One launch whatever B is."""
    B, Tmax = check_plan_args(clusters, cboundaries, ncl, table)
    _need_cuda(clusters, cboundaries, ncl, table)
    dev = clusters.device
    seg = torch.empty(B, Tmax, 4, dtype=torch.int32, device=dev)
    packed = torch.empty(3, B, dtype=torch.int32, device=dev)
    out = dict(seg=seg, nsegs=packed[0], totals=packed[1], status=packed[2], packed=packed)
    if B == 0:
        return out
    _lib.check(_lib.lib().s2svc_useg_plan(B, Tmax, table.shape[0], table.shape[1] - 1, ptr(clusters), ptr(cboundaries), ptr(ncl), ptr(table),
                                          int(silence_cluster), int(short_silence), ptr(seg), ptr(out["nsegs"]), ptr(out["totals"]),
                                          ptr(out["status"]), stream()), "useg_plan")
    _count()
    return out
