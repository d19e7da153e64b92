"""Launchers of the GAN-loss kernels (csrc/gan_loss.hip; C ABI in include/s2svc_hip.h) and the host tables that drive them.
Non-differentiable, GPU tensors only, fp32.  An entry is one mean over one tensor (pair); all entries of a call share one launch.

The index model (plain Python, no device): `chunk_prefix` cuts every entry into chunks of CHUNK elements of its physical storage and
numbers the workgroups; `locate` is what a workgroup does with that table; `chunk_range` is the element range it then walks."""
import ctypes

import torch

from .. import _lib
from .kernels import _need_cuda, ptr, stream

CHUNK = 8192        # elements per workgroup; the library states the same number (gan_loss_chunk)
MAX_ENTRIES = 64    # entries per call (gan_loss_max)
KIND_ONE_MINUS_SQ, KIND_SQ, KIND_ABS_DIFF = 0, 1, 2


def chunk_prefix(numels, chunk=CHUNK):
    """[first workgroup of entry e] + [the grid]: entry e owns ceil(numel_e / chunk) consecutive workgroups."""
    prefix = [0]
    for n in numels:
        if n < 1:
            raise ValueError("chunk_prefix: every entry has at least one element")
        prefix.append(prefix[-1] + -(-int(n) // chunk))
    return prefix


def locate(prefix, block):
    """(entry, chunk) of a workgroup: the last entry whose first workgroup is <= block (the kernels' binary search)."""
    if not 0 <= block < prefix[-1]:
        raise ValueError(f"locate: workgroup {block} outside the grid of {prefix[-1]}")
    lo, hi = 0, len(prefix) - 2
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if prefix[mid] <= block:
            lo = mid
        else:
            hi = mid - 1
    return lo, block - prefix[lo]


def chunk_range(numel, c, chunk=CHUNK):
    """[lo, hi) of chunk c of an entry of numel elements"""
    return c * chunk, min(numel, (c + 1) * chunk)


def dense_like(t):
    """Is t non-overlapping and dense (a permutation of a contiguous block), so that its numel elements are the numel values behind
    data_ptr()?"""
    dims = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1)
    want = 1
    for st, sz in dims:
        if st != want:
            return False
        want *= sz
    return True


def same_layout(a, b):
    return a.shape == b.shape and all(sa == sb for sa, sb, sz in zip(a.stride(), b.stride(), a.shape) if sz != 1)


def _check(name, t):
    if t.dtype in (torch.bfloat16, torch.float16):
        raise NotImplementedError(f"{name}: fp32 only (the discriminators run in fp32 only, DESIGN.md section 8)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: float32 tensors")
    if t.numel() < 1:
        raise ValueError(f"{name}: empty tensor")


def _tables(name, rows):
    """rows [(a, b, grad_a, grad_b, numel, kind)] -> (n, the int64 table, the int32 prefix table, the grid)"""
    n = len(rows)
    if not 1 <= n <= MAX_ENTRIES:
        raise ValueError(f"{name}: 1 .. {MAX_ENTRIES} entries per call, got {n}")
    flat = []
    for a, b, ga, gb, numel, kind in rows:
        flat += [ptr(a) or 0, ptr(b) or 0, ptr(ga) or 0, ptr(gb) or 0, int(numel), int(kind)]
    prefix = chunk_prefix([r[4] for r in rows], int(_lib.lib().s2svc_gan_loss_chunk()))
    return n, (ctypes.c_int64 * len(flat))(*flat), (ctypes.c_int32 * len(prefix))(*prefix), prefix[-1]


def _forward(name, fn, rows, device):
    n, table, prefix, grid = _tables(name, rows)
    partials = torch.empty(grid, dtype=torch.float64, device=device)
    out = torch.empty(n + 1, dtype=torch.float32, device=device)
    _lib.check(fn(n, table, prefix, ptr(partials), ptr(out), stream()), name)
    return out


def feature_loss_fwd(pairs):
    """pairs [(a, b)]: dense fp32 tensors, a and b of a pair in the same layout -> out (n + 1): the n means of |a - b| and their sum.
    2 launches (chunk sums, finish)."""
    rows = []
    for a, b in pairs:
        _need_cuda(a, b)
        _check("feature_loss", a)
        _check("feature_loss", b)
        if not (dense_like(a) and same_layout(a, b)):
            raise ValueError("feature_loss_fwd: every pair is dense and equally strided (copy it first)")
        rows.append((a, b, None, None, a.numel(), KIND_ABS_DIFF))
    return _forward("gan_feature_loss", _lib.lib().s2svc_gan_feature_loss, rows, pairs[0][0].device)


def _grad_like(name, t, out):
    """The gradient buffer of t: a new tensor in t's physical layout, or the caller's (same shape, strides, fp32, on the device)"""
    if out is None:
        return torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device=t.device)
    _need_cuda(out)
    if out.dtype != torch.float32 or out.shape != t.shape or not same_layout(out, t):
        raise ValueError(f"{name}: a caller's gradient buffer has the input's shape and strides, fp32")
    return out


def feature_loss_bwd(pairs, upstream, need_a, need_b, out_a=None, out_b=None):
    """-> ([grad_a or None], [grad_b or None]) in the pairs' own physical layout; upstream: one fp32 value on the device.  1 launch.
    out_a / out_b: lists of caller's buffers (or None per pair) to write into."""
    _need_cuda(upstream)
    if upstream.dtype != torch.float32 or upstream.numel() != 1:
        raise ValueError("feature_loss_bwd: the upstream gradient is one fp32 value")
    rows, gas, gbs = [], [], []
    for i, ((a, b), na, nb) in enumerate(zip(pairs, need_a, need_b)):
        ga = _grad_like("feature_loss_bwd", a, None if out_a is None else out_a[i]) if na else None
        gb = _grad_like("feature_loss_bwd", b, None if out_b is None else out_b[i]) if nb else None
        gas.append(ga)
        gbs.append(gb)
        if na or nb:
            rows.append((a, b, ga, gb, a.numel(), KIND_ABS_DIFF))
    if rows:
        n, table, prefix, _ = _tables("gan_feature_loss_bwd", rows)
        _lib.check(_lib.lib().s2svc_gan_feature_loss_bwd(n, table, prefix, ptr(upstream), stream()), "gan_feature_loss_bwd")
    return gas, gbs


def score_loss_fwd(entries):
    """entries [(x, kind)], kind 0: mean((1 - x)^2), kind 1: mean(x^2); x dense fp32 -> out (n + 1): the means and their sum.  2 launches."""
    rows = []
    for x, kind in entries:
        _need_cuda(x)
        _check("score_loss", x)
        if kind not in (KIND_ONE_MINUS_SQ, KIND_SQ) or not dense_like(x):
            raise ValueError("score_loss_fwd: dense tensors, kind 0 or 1")
        rows.append((x, None, None, None, x.numel(), kind))
    return _forward("gan_score_loss", _lib.lib().s2svc_gan_score_loss, rows, entries[0][0].device)


def score_loss_bwd(entries, upstream, need, out=None):
    """-> [grad_x or None] in x's own physical layout.  1 launch.  out: a list of caller's buffers (or None per tensor)."""
    _need_cuda(upstream)
    if upstream.dtype != torch.float32 or upstream.numel() != 1:
        raise ValueError("score_loss_bwd: the upstream gradient is one fp32 value")
    rows, grads = [], []
    for i, ((x, kind), nd) in enumerate(zip(entries, need)):
        g = _grad_like("score_loss_bwd", x, None if out is None else out[i]) if nd else None
        grads.append(g)
        if nd:
            rows.append((x, None, g, None, x.numel(), kind))
    if rows:
        n, table, prefix, _ = _tables("gan_score_loss_bwd", rows)
        _lib.check(_lib.lib().s2svc_gan_score_loss_bwd(n, table, prefix, ptr(upstream), stream()), "gan_score_loss_bwd")
    return grads
