"""Attention cores (QK^T -> masked softmax -> PV), plain and relative-position, as autograd nodes over the HIP kernels.
Reference: modules/transformer/attention.py:63-111, :262-305.

Four nodes: `_Attn` (the core on q, k, v in one of three packings, see `_views`), `_AttnBlock` (input projection + core +
out-projection of the short-sequence path), `_RelAttnCore` and `_RelAttnPacked` (relative-position attention on separate and on
packed projections).  The core binds to one of three kernel families by length (`_attn_fwd_views` / `_attn_common_bwd`).
"""
import math

import torch
from torch.autograd import Function

from . import kernels as K
from . import kernels_attn as KAT
from .functional import _c, _linear_bwd, _reduce_to, _slotted, _wcast
from .schedule import _side_run


# ================================================================================================
# operands and the three batched products
# ================================================================================================
def _bop(t, dk, layout=K.KC, bs0=None):
    """GEMM operand over a (B, T, H*dk) activation that may be a column slice of a packed (B, T, n*D) tensor:
    row stride and batch stride come from the view, heads are the second batch level."""
    assert t.stride(-1) == 1
    return K.operand(t, t.stride(1), layout=layout, bs0=t.stride(0) if bs0 is None else bs0, bs1=dk)


def _pad8(n):
    return (n + 7) // 8 * 8


def _qk(q, k, B, H, T1, T2, dk, D, dtype, bs0_b=None):
    """fp32 scores (B, H, T1, ld) with ld = T2 rounded up to 8 (16-byte rows for the bf16 consumers)."""
    ld = _pad8(T2)
    scores = torch.empty((B, H, T1, ld), dtype=torch.float32, device=q.device)
    K.gemm(_bop(q, dk), _bop(k, dk, bs0=bs0_b), T1, T2, dk, scores, in_dtype=dtype, nb0=B, nb1=H, ldc=ld, cbs=(H * T1 * ld, T1 * ld))
    return scores


def _into(out, A, Bop, M, N, Kd, dk, dtype, B, H, group=None):
    """Batched (b, h) GEMM writing head h of batch b into columns [h*dk, (h+1)*dk) of the (B, T, .) view `out`.
    group: a list that collects the problem instead of launching it (K.launch_group_batched)."""
    K.gemm(A, Bop, M, N, Kd, out, in_dtype=dtype, nb0=B, nb1=H, ldc=out.stride(1), cbs=(out.stride(0), dk), group=group)
    return out


def _pop(pm, T1, H, layout=K.KC):
    """Operand over a padded probability-like tensor (B, H, T1, ld): the maps, dS, and the (B, H, T, Lq) dbd of the
    relative-position term."""
    ld = pm.shape[-1]
    return K.operand(pm, ld, layout=layout, bs0=H * T1 * ld, bs1=T1 * ld, zero_padded=True)


def _pv(pm, v, B, H, T1, T2, dk, D, dtype):
    ctxv = torch.empty((B, T1, D), dtype=dtype, device=v.device)
    return _into(ctxv, _pop(pm, T1, H), _bop(v, dk, K.RC), T1, dk, T2, dk, dtype, B, H)


def _pad_like(dattn, ref):
    """External gradient wrt the (B,H,T1,T2) attention view -> the padded (B,H,T1,ld) layout of `ref`."""
    if dattn is None:
        return None
    if dattn.shape[-1] == ref.shape[-1]:
        return _c(dattn)
    out = torch.zeros_like(ref)
    out[..., : dattn.shape[-1]].copy_(dattn)
    return out


# ================================================================================================
# the core, forward and backward, on q / k / v views
# ================================================================================================
def _attn_common_bwd(dctx, dattn, attn, pm, q, k, v, H, scale, p, seed, Lp=0, rel_mode=0, outs=None, ldb=None, groups=None):
    """Backward of softmax(QK^T)V.  attn/pm: padded (B,H,T1,ld) tensors; q/k/v may be column slices of packed
    tensors; `outs` = (dq, dk, dv) views to write into (e.g. slices of a packed gradient), allocated when None.
    The three batched products behind the softmax backward are launched as two grids (dQ = dS K | dV = P^T dctx, dK = dS^T Q:
    one grid per operand-kind pair, K.launch_group_batched); groups = (kc, rc, keep): two lists the caller launches itself
    after adding its own products (relative-position attention: d qv, d pos), and a list that keeps the operands of the queued
    products alive until then (a descriptor holds raw pointers: a temporary freed before the launch is the next allocation)."""
    B, T1, D = q.shape
    T2 = k.shape[1]
    dk = D // H
    dtype = q.dtype
    dctx = _c(dctx) if dctx is not None else torch.zeros((B, T1, D), dtype=dtype, device=q.device)
    if outs is None:
        outs = (torch.empty((B, T1, D), dtype=dtype, device=q.device), torch.empty((B, T2, D), dtype=dtype, device=q.device),
                torch.empty((B, T2, D), dtype=dtype, device=q.device))
    dq, dkk, dv = outs
    if pm is None:      # forward ran the fused kernel (no dropped copy was stored): one launch, masks regenerated
        KAT.fused_bwd(q, k, v, dctx, attn, _pad_like(dattn, attn), H, scale, p, seed, dq, dkk, dv)
        return dq, dkk, dv, None
    gkc, grc, keep = groups if groups is not None else ([], [], [])
    dq_fused = False
    rel_ok = not Lp or (rel_mode == 1 and T1 == T2 and Lp == 2 * T1 - 1 and ldb is not None and ldb % 8 == 0)
    if rel_ok and attn.is_contiguous() and KAT.map_supported(dctx, v, H):
        # up to 512 keys, bf16: dP = dctx . v^T, the softmax backward and (rel-pos) the un-shift in ONE launch, dP never in memory,
        # no zero fill of dbd (csrc/attn_map.hip)
        # ... and, for d_k in {64, 96, 128}, dq = dS . k as the same launch's second product
        dq_fused = dq.stride(2) == 1 and KAT.map_product_ok(k, H)
        ds, dbd = KAT.map_bwd(dctx, v, attn, _pad_like(dattn, attn), H, scale, p, seed, ldb=ldb if Lp else 0,
                              k=k if dq_fused else None, dq=dq if dq_fused else None)
    else:
        # dP[b,h,i,j] = sum_d dctx[b,i,hd] v[b,j,hd]
        dp = _qk(dctx, v, B, H, T1, T2, dk, D, dtype)
        ds, dbd = K.attn_softmax_bwd(attn, dp, scale, p=p, seed=seed, Lp=Lp, rel_mode=rel_mode, dattn=_pad_like(dattn, attn), T2=T2,
                                     ldb=ldb)
    # dV[b,j,hd] = sum_i pm[b,h,i,j] dctx[b,i,hd]
    _into(dv, _pop(pm, T1, H, K.RC), _bop(dctx, dk, K.RC), T2, dk, T1, dk, dtype, B, H, group=grc)
    # dQ[b,i,hd] = sum_j dS[b,h,i,j] k[b,j,hd]
    if not dq_fused:
        _into(dq, _pop(ds, T1, H), _bop(k, dk, K.RC), T1, dk, T2, dk, dtype, B, H, group=gkc)
    # dK[b,j,hd] = sum_i dS[b,h,i,j] q[b,i,hd]
    _into(dkk, _pop(ds, T1, H, K.RC), _bop(q, dk, K.RC), T2, dk, T1, dk, dtype, B, H, group=grc)
    keep += [dctx, ds, dbd, pm, q, k, v]
    if groups is None:
        K.launch_group_batched(gkc)
        K.launch_group_batched(grc)
    return dq, dkk, dv, dbd


_FUSED = object()        # stands in for `pdrop` when the fused kernel ran: nothing but the attention map was stored


def _split_pdrop(ctx, pdrop):
    ctx.fused = pdrop is _FUSED
    return None if ctx.fused else pdrop


def _pm(ctx, attn, pdrop):
    """The (dropped) probabilities the unfused backward multiplies with; None = run the fused backward kernel."""
    return None if ctx.fused else (pdrop if pdrop is not None else attn)


def _scale_seed(dk, p, device):
    """1/sqrt(d_k) and the dropout seed of one attention call (no seed is drawn without dropout: the streams do not shift)."""
    return 1.0 / math.sqrt(dk), (K.new_seed(device) if p > 0.0 else (None, 0))


def _attn_fwd_views(q, k, v, klen, causal, H, p):
    B, T1, D = q.shape
    T2 = k.shape[1]
    dk = D // H
    dtype = q.dtype
    scale, seed = _scale_seed(dk, p, q.device)
    if KAT.supported(q, k, v, H):       # short sequences, bf16: scores + mask + softmax + dropout + P.V in ONE launch
        out, attn = KAT.fused_fwd(q, k, v, klen, causal, H, scale, p, seed)
        return out, attn, _FUSED, scale, seed
    if KAT.map_supported(q, k, H):      # up to 512 keys, bf16: scores + mask + softmax + dropout in ONE launch (csrc/attn_map.hip)
        # ... and, for d_k in {64, 96, 128}, the context (dropped map) . v as the same launch's second product
        attn, pdrop, out = KAT.map_fwd(q, k, klen, causal, H, scale, p, seed, v=v if KAT.map_product_ok(v, H) else None)
        if out is not None:
            return out, attn, pdrop, scale, seed
    else:
        scores = _qk(q, k, B, H, T1, T2, dk, D, dtype)
        attn, pdrop = K.attn_softmax_fwd(scores, dtype, scale, klen=klen, causal=causal, p=p, seed=seed, T2=T2)
    out = _pv(pdrop if pdrop is not None else attn, v, B, H, T1, T2, dk, D, dtype)
    return out, attn, pdrop, scale, seed


def _user_attn(attn, T2):
    """The (B,H,T1,T2) view handed to callers (`self.attn`); the padded tensor stays the saved one."""
    return attn if attn.shape[-1] == T2 else attn[..., :T2]


# ================================================================================================
# column blocks of one packed tensor, their gradient written in place
# ================================================================================================
class _GradSink:
    """The gradient of a tensor that split_cols cut into column blocks, allocated once and written IN PLACE by the consumers of
    the blocks (the source-attention blocks of all decoder layers write dK | dV of their (B, T, 2D) block straight into the
    (B, T, L * 2D) gradient of the batched projection): the backward pass of split_cols then has nothing to concatenate (one
    18 us torch.cat of 18.6 MB on the VTN chain per step)."""
    __slots__ = ("shape", "dtype", "device", "W", "buf", "claimed")

    def __init__(self, shape, dtype, device, W):
        self.shape, self.dtype, self.device, self.W, self.buf, self.claimed = shape, dtype, device, W, None, set()

    def part(self, i):
        """Block i of the buffer for its ONE consumer.  A block that feeds a second consumer gets a fresh tensor instead: two
        consumers writing the same view would leave autograd summing two aliases of one buffer (2 g2 instead of g1 + g2); with
        the fresh tensor autograd's sum is a new tensor, holds() fails and _SplitCols concatenates the correct sums."""
        if i in self.claimed:
            return torch.empty(self.shape[:-1] + (self.W,), dtype=self.dtype, device=self.device)
        self.claimed.add(i)
        if self.buf is None:
            self.buf = torch.empty(self.shape, dtype=self.dtype, device=self.device)
        return self.buf[..., i * self.W:(i + 1) * self.W]

    def holds(self, grads):
        """True if `grads` are exactly the blocks of the buffer, in order (every consumer wrote its block in place)."""
        if self.buf is None:
            return False
        base, es = self.buf.data_ptr(), self.buf.element_size()
        return all(g is not None and g.data_ptr() == base + i * self.W * es and g.shape == self.buf.shape[:-1] + (self.W,)
                   and g.stride() == self.buf.stride() and g.dtype == self.dtype for i, g in enumerate(grads))


class _SplitCols(Function):
    """(..., n*W) -> n column blocks (..., W) as VIEWS (no copy); the backward pass returns the sink's buffer if every consumer wrote
    its block's gradient in place (_GradSink), else it concatenates the n gradients with one kernel.
    (Plain slicing would make autograd build n zero-padded full-width gradients and n-1 adds.)"""

    @staticmethod
    def forward(ctx, x, n, sink):
        W = x.shape[-1] // n
        ctx.n, ctx.W, ctx.sink = n, W, sink
        ctx.meta = (x.shape, x.dtype, x.device)
        ctx.set_materialize_grads(False)
        return tuple(x[..., i * W:(i + 1) * W] for i in range(n))

    @staticmethod
    def backward(ctx, *grads):
        shape, dtype, device = ctx.meta
        if all(g is None for g in grads):
            return None, None, None
        sink = ctx.sink
        if sink is not None and sink.holds(grads):
            buf, sink.buf = sink.buf, None
            sink.claimed.clear()
            return buf, None, None
        if sink is not None:
            sink.buf = None
            sink.claimed.clear()
        blk = shape[:-1] + (ctx.W,)
        parts = [g if g is not None else torch.zeros(blk, dtype=dtype, device=device) for g in grads]
        return torch.cat(parts, dim=-1), None, None


def split_cols(x, n):
    sink = _GradSink(tuple(x.shape), x.dtype, x.device, x.shape[-1] // n) if (x.requires_grad and x.is_contiguous()) else None
    parts = _SplitCols.apply(x, n, sink)
    if sink is not None:
        for i, t in enumerate(parts):
            t._s2s_gsink = (sink, i)
    return parts


# ================================================================================================
# the three packings ("forms") of q, k, v and the one node that runs the core on any of them
# ================================================================================================
def _views(form, ts, D):
    """(q, k, v) as views of the form's tensors -- "q_k_v": three tensors; "q_kv": q and ONE packed projection kv (B, T2, 2D) of
    the memory; "qkv": ONE packed projection (B, T, 3D) (fused Q/K/V GEMM).  The gradients come back in the same packing, so the
    same call over `_grads(...)` gives the (dq, dk, dv) views the backward kernels write."""
    if form == "qkv":
        t = ts[0]
        return t[..., :D], t[..., D:2 * D], t[..., 2 * D:]
    if form == "q_kv":
        kv = ts[1]
        return ts[0], kv[..., :D], kv[..., D:]
    return ts


def _inputs(form, ts, H):
    """The form's tensors as the kernels can read them, and the gradient sink of a kv block that is used in place."""
    if form != "q_kv":
        return tuple(_c(t) for t in ts), None
    q, kv = _c(ts[0]), ts[1]
    D = q.shape[-1]
    # a column slice of the decoder's batched K/V projection (split_cols) is used in place when the kernels that take row and
    # batch strides run (the one-launch kernel of short sequences; the attention-map kernel of medium ones, whose neighbours are
    # GEMM descriptors with strides of their own); everything else wants a dense (B, T2, 2D) tensor
    in_place = kv.stride(-1) == 1 and (KAT.supported(q, kv[..., :D], kv[..., D:], H)
                                       or (KAT.map_supported(q, kv[..., :D], H) and KAT.view_ok(kv[..., D:])))
    if not in_place:
        return (q, _c(kv)), None
    # a column block of split_cols whose gradient can be written in place (see _GradSink): on the same paths (their backward
    # kernels / descriptors take row and batch strides for dK and dV)
    return (q, kv), getattr(kv, "_s2s_gsink", None)


def _grads(form, ts, gsink, main):
    """Fresh gradient tensors in the packing of `ts`; the kv block of a split_cols tensor is this block of the packed gradient,
    written where split_cols wants it, when a sink exists and the main gradient `main` is present."""
    if form != "q_kv":
        return tuple(torch.empty_like(t) for t in ts)
    q, kv = ts
    if gsink is not None and main is not None:
        return torch.empty_like(q), gsink[0].part(gsink[1])
    return torch.empty_like(q), torch.empty(kv.shape, dtype=kv.dtype, device=kv.device)


class _Attn(Function):
    """The attention core on q, k, v in the packing `form` (see _views); returns the gradients in the same packing."""

    @staticmethod
    def forward(ctx, form, klen, causal, H, p, *ts):
        ts, ctx.gsink = _inputs(form, ts, H)
        D = ts[0].shape[-1] // 3 if form == "qkv" else ts[0].shape[-1]
        q, k, v = _views(form, ts, D)
        out, attn, pdrop, scale, seed = _attn_fwd_views(q, k, v, klen, causal, H, p)
        ctx.meta = (form, H, scale, p, seed, D)
        ctx.save_for_backward(*ts, attn, _split_pdrop(ctx, pdrop))
        ctx.set_materialize_grads(False)
        return out, _user_attn(attn, k.shape[1])

    @staticmethod
    def backward(ctx, dctx, dattn):
        *ts, attn, pdrop = ctx.saved_tensors
        form, H, scale, p, seed, D = ctx.meta
        grads = _grads(form, ts, ctx.gsink, dctx)
        _attn_common_bwd(dctx, dattn, attn, _pm(ctx, attn, pdrop), *_views(form, ts, D), H, scale, p, seed,
                         outs=_views(form, grads, D))
        return (None, None, None, None, None) + grads


def attention_core(q, k, v, klen, causal, H, p=0.0):
    """(context (B,T1,D), attn (B,H,T1,T2)); klen: int32 device tensor (B,) of valid key counts or None."""
    return _Attn.apply("q_k_v", klen, causal, H, p, q, k, v)


def attention_packed_qkv(qkv, klen, causal, H, p=0.0):
    return _Attn.apply("qkv", klen, causal, H, p, qkv)


def attention_packed_kv(q, kv, klen, causal, H, p=0.0):
    return _Attn.apply("q_kv", klen, causal, H, p, q, kv)


# ------------------------------------------------------------------------------------------------
# Whole attention blocks of the short-sequence path (bf16, T <= 64): input projection + fused core + out-projection as ONE autograd
# node.  The values are those of Fn.linear -> attention_packed_* -> Fn.linear; what the node buys is the backward pass: the core's
# kernel takes the gradient of the out-projection's OUTPUT and computes its own head's columns of dctx = dY W_o in its prologue
# (KAT.proj_bwd: no workgroup needs another's data, nothing is replicated), so the out-projection's data-gradient GEMM -- one
# dependent launch per block on the chain -- is gone and dctx is never stored.
# ------------------------------------------------------------------------------------------------
def attn_block_ok(query, T2, kv, H, w_o):
    """The one-node blocks run where the fused short-sequence kernels do and the optimiser keeps W_o^T (FlatAdam's `_s2s_bf16_t`);
    training only (decode / eval keep the separate nodes)."""
    if not (torch.is_grad_enabled() and query.dim() == 3 and getattr(w_o, "_s2s_bf16_t", None) is not None):
        return False
    D = query.shape[-1]
    if not KAT.proj_bwd_supported(query.dtype, query.shape[1], T2, D // H, D) or D % 8:
        return False
    return kv is None or (kv.dtype == query.dtype and kv.stride(-1) == 1 and KAT.view_ok(kv[..., :D]) and KAT.view_ok(kv[..., D:]))


def _block_project(x, weight, bias):
    """x (B, T, D) -> (x2, the compute-dtype weight, x W^T + b as (B, T, N)): the forward of Fn.linear."""
    dtype = x.dtype
    x2 = _c(x).view(-1, x.shape[-1])
    M, Kd = x2.shape
    N = weight.shape[0]
    w = _wcast(weight, dtype)
    y = torch.empty((M, N), dtype=dtype, device=x.device)
    K.gemm(K.operand(x2, Kd), K.operand(w, Kd), M, N, Kd, y, in_dtype=dtype, bias=bias)
    return x2, w, y.view(*x.shape[:-1], N)


def _block_core_bwd(ctx, dy, dattn, attn, cv, wo, q, k, v, outs):
    """Out-projection and core of a block, backward: W_o's weight / bias gradient as _Linear queues it, then dq | dk | dv into
    `outs` -- from dy with the data gradient folded into the core's launch, or through the separate GEMM where that is switched
    off or does not apply.  -> (dw_o, db_o)."""
    _, H, scale, p, seed, D = ctx.meta
    w_o, b_o = ctx.out_params
    if dy is None:                     # only the attention map was used
        _attn_common_bwd(None, dattn, attn, None, q, k, v, H, scale, p, seed, outs=outs)
        return None, None
    dy = _c(dy)
    wot = getattr(w_o, "_s2s_bf16_t", None)
    # (B T1 > 64: the rows at which the separate GEMM runs its tile kernels, whose K order the prologue repeats -- the same bits;
    # below, the skinny kernel sums K in four quarters)
    fold = (wot is not None and dy.shape[0] * dy.shape[1] > 64 and all(t.stride(-1) == 1 for t in outs)
            and KAT.proj_bwd_ok(q, k, v, dy, wot, H))
    dctx, dwo, dbo = _linear_bwd(cv.view(-1, D), wo, None, None, w_o, b_o, b_o is not None, dy, None, not fold)
    if fold:
        KAT.proj_bwd(q, k, v, dy, wot, attn, _pad_like(dattn, attn), H, scale, p, seed, *outs)
    else:
        _attn_common_bwd(dctx.view(cv.shape), dattn, attn, None, q, k, v, H, scale, p, seed, outs=outs)
    return dwo, dbo


class _AttnBlock(Function):
    """One attention block.  kv None: self-attention on the packed (3D, D) projection of x (form "qkv").  Else source attention
    (form "q_kv"): the Q projection of x, and the packed K|V projection `kv` (B, T2, 2D) of the memory computed by the caller
    (used in place: a column block of the decoder's batched projection, its gradient written into the block's _GradSink)."""

    @staticmethod
    def forward(ctx, x, w_in, b_in, kv, w_o, b_o, klen, causal, H, p, passthrough):
        D = x.shape[-1]
        x2, wi, proj = _block_project(x, w_in, b_in)
        form, ts = ("qkv", (proj,)) if kv is None else ("q_kv", (proj, kv))
        q, k, v = _views(form, ts, D)
        cv, attn, pdrop, scale, seed = _attn_fwd_views(q, k, v, klen, causal, H, p)
        assert pdrop is _FUSED
        _, wo, y = _block_project(cv, w_o, b_o)
        ctx.meta = (form, H, scale, p, seed, D)
        ctx.in_params, ctx.out_params, ctx.xshape = (w_in, b_in), (w_o, b_o), x.shape
        ctx.gsink = None if kv is None else getattr(kv, "_s2s_gsink", None)
        ctx.save_for_backward(x2, wi, *ts, attn, cv, wo)
        ctx.set_materialize_grads(False)
        if passthrough:
            return y, _user_attn(attn, k.shape[1]), x.view_as(x)
        return y, _user_attn(attn, k.shape[1])

    @staticmethod
    def backward(ctx, dy, dattn, g_pass=None):
        if dy is None and dattn is None:
            return (g_pass,) + (None,) * 10
        x2, wi, *ts, attn, cv, wo = ctx.saved_tensors
        form, D = ctx.meta[0], ctx.meta[5]
        grads = _grads(form, ts, ctx.gsink, dy)
        dwo, dbo = _block_core_bwd(ctx, dy, dattn, attn, cv, wo, *_views(form, ts, D), _views(form, grads, D))
        w_in, b_in = ctx.in_params
        dx, dw, db = _linear_bwd(x2, wi, None, None, w_in, b_in, b_in is not None, grads[0], g_pass, ctx.needs_input_grad[0])
        dkv = grads[1] if form == "q_kv" else None
        return (None if dx is None else dx.view(ctx.xshape)), dw, db, dkv, dwo, dbo, None, None, None, None, None


def attention_block_qkv(x, w_qkv, b_qkv, w_o, b_o, klen, causal, H, p=0.0, passthrough=False):
    """(out, attn[, alias of x]): see _AttnBlock; the caller checks attn_block_ok."""
    return _AttnBlock.apply(x, w_qkv, b_qkv, None, w_o, b_o, klen, causal, H, p, passthrough)


def attention_block_kv(x, w_q, b_q, kv, w_o, b_o, klen, causal, H, p=0.0, passthrough=False):
    return _AttnBlock.apply(x, w_q, b_q, kv, w_o, b_o, klen, causal, H, p, passthrough)


# ================================================================================================
# relative-position attention: scores = (qu.k^T + rel_shift(qv.pos^T)) / sqrt(dk)
# rel_mode 1 = new (pos (1,2T-1,D)), 2 = legacy (pos (1,T,D))
# ================================================================================================
def _rel_scores(qu, qv, k, pos, klen, H, scale, p, seed, rel_mode):
    """The separate kernels: both score terms as batched GEMMs, then the softmax kernel with the shift as index arithmetic.
    -> (attn, pdrop)."""
    B, T, D = qu.shape
    dk = D // H
    L = pos.shape[1]
    dtype = qu.dtype
    ac = _qk(qu, k, B, H, T, T, dk, D, dtype)
    Lq = _pad8(L)                 # bd / dbd rows padded to 16 bytes (2T-1 is odd) so the backward GEMMs vectorise
    bd = torch.empty((B, H, T, Lq), dtype=torch.float32, device=qu.device)
    K.gemm(K.operand(qv, D, bs0=T * D, bs1=dk), K.operand(pos, D, bs0=0, bs1=dk), T, L, dk, bd, in_dtype=dtype, nb0=B, nb1=H,
           ldc=Lq, cbs=(H * T * Lq, T * Lq))
    return K.attn_softmax_fwd(ac, dtype, scale, klen=klen, causal=False, bd=bd, rel_mode=rel_mode, p=p, seed=seed, T2=T, Lp=L)


def _rel_pos_bwd(dbd, qv, pos, H, gkc=None, grc=None):
    """Gradients of the position term from dbd (B, H, T, Lq) -> (d qv, d pos).  gkc / grc: the lists of queued batched products
    the two GEMMs join (see _attn_common_bwd), launched here as two grids; None = each GEMM launches at once."""
    B, T, D = qv.shape
    dk = D // H
    L = pos.shape[1]
    dtype = qv.dtype
    # dQv[b,i,hd] = sum_c dbd[b,h,i,c] pos[c,hd]
    dqv = torch.empty((B, T, D), dtype=dtype, device=qv.device)
    K.gemm(_pop(dbd, T, H), K.operand(pos, D, layout=K.RC, bs0=0, bs1=dk), T, dk, L, dqv, in_dtype=dtype, nb0=B, nb1=H, ldc=D,
           cbs=(T * D, dk), group=gkc)
    # dPos[c,hd] = sum_{b,i} dbd[b,h,i,c] qv[b,i,hd]  (per-batch partials, then a deterministic sum over b)
    part = torch.empty((B, L, D), dtype=dtype, device=qv.device)
    K.gemm(_pop(dbd, T, H, K.RC), K.operand(qv, D, layout=K.RC, bs0=T * D, bs1=dk), L, dk, T, part, in_dtype=dtype, nb0=B, nb1=H,
           ldc=D, cbs=(L * D, dk), group=grc)
    if gkc is not None:
        K.launch_group_batched(gkc)
        K.launch_group_batched(grc)
    dpos, _ = K.colreduce(0, part.view(B, L * D))
    return dqv, K.cast(dpos.view(1, L, D), dtype)


class _RelAttnCore(Function):
    @staticmethod
    def forward(ctx, qu, qv, k, v, pos, klen, H, p, rel_mode):
        qu, qv, k, v, pos = _c(qu), _c(qv), _c(k), _c(v), _c(pos)
        B, T, D = qu.shape
        dk = D // H
        scale, seed = _scale_seed(dk, p, qu.device)
        attn, pdrop = _rel_scores(qu, qv, k, pos, klen, H, scale, p, seed, rel_mode)
        out = _pv(pdrop if pdrop is not None else attn, v, B, H, T, T, dk, D, qu.dtype)
        ctx.meta = (H, scale, p, seed, rel_mode)
        ctx.save_for_backward(qu, qv, k, v, pos, attn, pdrop)
        ctx.set_materialize_grads(False)
        return out, _user_attn(attn, T)

    @staticmethod
    def backward(ctx, dctx, dattn):
        qu, qv, k, v, pos, attn, pdrop = ctx.saved_tensors
        H, scale, p, seed, rel_mode = ctx.meta
        L = pos.shape[1]
        pm = pdrop if pdrop is not None else attn
        dqu, dkk, dv, dbd = _attn_common_bwd(dctx, dattn, attn, pm, qu, k, v, H, scale, p, seed, Lp=L, rel_mode=rel_mode, ldb=_pad8(L))
        dqv, dpos = _rel_pos_bwd(dbd, qv, pos, H)
        return dqu, dqv, dkk, dv, dpos, None, None, None, None


def rel_attention_core(qu, qv, k, v, pos, klen, H, p=0.0, rel_mode=1):
    return _RelAttnCore.apply(qu, qv, k, v, pos, klen, H, p, rel_mode)


def _head_bias_grads(u, v, dqu, dqv):
    """d pos_bias_u = sum over (batch, time) of dQu, likewise v.  With flat-gradient slots the two reductions are queued and
    join the grouped column reductions of the batch (two launches for up to 24 of them) instead of six launches per layer."""
    if not u.requires_grad:
        return None, None
    D = dqu.shape[-1]
    a, b = dqu.view(-1, D), dqv.view(-1, D)
    if _slotted(u, v):
        _side_run(lambda: (_reduce_to(u, None, 0, a), _reduce_to(v, None, 0, b)), keep=(a, b))
        return None, None
    su, _ = K.colreduce(0, a)
    sv, _ = K.colreduce(0, b)
    return su.view(u.shape), sv.view(v.shape)


class _RelAttnPacked(Function):
    """Relative-position self-attention on ONE packed projection qkv (B, T, 3D) (the Q | K | V GEMM of the layer):
    qu = q + pos_bias_u, qv = q + pos_bias_v, then _RelAttnCore's arithmetic with k, v read in place as column blocks.
    The gradient comes back packed, so the three projections also share ONE data-gradient and ONE weight-gradient GEMM
    (K = 3D instead of three products and two additions)."""

    @staticmethod
    def forward(ctx, qkv, pos, u, v, klen, H, p, rel_mode):
        qkv, pos = _c(qkv), _c(pos)
        B, T, D3 = qkv.shape
        D = D3 // 3
        dk = D // H
        q, k, vv = _views("qkv", (qkv,), D)
        scale, seed = _scale_seed(dk, p, qkv.device)
        ub, vb = u.detach().reshape(-1), v.detach().reshape(-1)
        ctx.fused_rel = KAT.rel_supported(q, k, vv, pos, H, rel_mode)
        if ctx.fused_rel:       # T <= 256, bf16: head bias + both score terms + shift + softmax + dropout in ONE launch (csrc/relattn.hip)
            attn, pdrop, qu, qv = KAT.rel_fwd(q, k, pos, ub, vb, klen, H, scale, p, seed)
        else:
            qu, qv = K.add_head_bias_view(q, ub, vb)
            attn, pdrop = _rel_scores(qu, qv, k, pos, klen, H, scale, p, seed, rel_mode)
        out = _pv(pdrop if pdrop is not None else attn, vv, B, H, T, T, dk, D, qkv.dtype)
        ctx.meta = (H, scale, p, seed, rel_mode, D)
        ctx.params = (u, v)
        ctx.save_for_backward(qkv, qu, qv, pos, attn, pdrop)
        ctx.set_materialize_grads(False)
        return out, _user_attn(attn, T)

    @staticmethod
    def backward(ctx, dctx, dattn):
        qkv, qu, qv, pos, attn, pdrop = ctx.saved_tensors
        H, scale, p, seed, rel_mode, D = ctx.meta
        u, v = ctx.params
        L = pos.shape[1]
        _, k, vv = _views("qkv", (qkv,), D)
        pm = pdrop if pdrop is not None else attn
        dqkv = torch.empty_like(qkv)
        dq, dkk, dvv = _views("qkv", (dqkv,), D)
        dqu = torch.empty_like(qu)
        gkc, grc, keep = [], [], []      # the five batched products behind the softmax backward: two grids (K.launch_group_batched)
        _, _, _, dbd = _attn_common_bwd(dctx, dattn, attn, pm, qu, k, vv, H, scale, p, seed, Lp=L, rel_mode=rel_mode, ldb=_pad8(L),
                                        outs=(dqu, dkk, dvv), groups=(gkc, grc, keep))
        dqv, dpos = _rel_pos_bwd(dbd, qv, pos, H, gkc, grc)
        del keep
        K.add_rows(dqu, dqv, dq)
        du, dv = _head_bias_grads(u, v, dqu, dqv)
        return dqkv, dpos, du, dv, None, None, None, None


def rel_attention_packed(qkv, pos, u, v, klen, H, p=0.0, rel_mode=1):
    return _RelAttnPacked.apply(qkv, pos, u, v, klen, H, p, rel_mode)


class _HeadBias(Function):
    """qu = q + pos_bias_u, qv = q + pos_bias_v   (attention.py:283-286)."""

    @staticmethod
    def forward(ctx, q, u, v):
        q = _c(q)
        ctx.params = (u, v)
        return K.add_head_bias(q, u.detach().reshape(-1), v.detach().reshape(-1))

    @staticmethod
    def backward(ctx, dqu, dqv):
        u, v = ctx.params
        dqu, dqv = _c(dqu), _c(dqv)
        dq = K.axpby(1.0, dqu, 1.0, dqv)
        du, dv = _head_bias_grads(u, v, dqu, dqv)
        return dq, du, dv


def add_head_bias(q, u, v):
    return _HeadBias.apply(q, u, v)
