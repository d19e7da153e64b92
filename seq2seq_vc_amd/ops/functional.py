"""Differentiable ops of the hot path: torch.autograd.Function wrappers whose forward AND backward
are hand-written HIP kernels (seq2seq_vc_amd/csrc) reached through the C ABI.

Conventions
  * activations are (B, T, D) channel-last, contiguous, in the compute dtype (fp32 = parity mode,
    bf16 = benchmark mode); parameters stay fp32 in the reference's torch layouts;
  * masks are never materialised: ops take int32 length vectors that live on the device;
  * weight gradients are fp32.  If a parameter carries `_s2s_grad` (a view into the model's flat
    gradient buffer, see optim.FlatAdam) the wgrad kernel accumulates straight into it and autograd
    gets no tensor for that input.
"""
import torch
from torch.autograd import Function

from . import kernels as K
# where and when the parameter-gradient closures run is ops.schedule; the names its users call through this module stay here
from .schedule import _Side, _side_flush, _side_run, _zero_scalar, enable_side_streams, grad_cuts, root_backward, side_join  # noqa: F401

_STATE = {"dtype": torch.float32}


def set_compute_dtype(dtype):
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("compute dtype must be float32 or bfloat16")
    _STATE["dtype"] = dtype


def compute_dtype():
    return _STATE["dtype"]


def to_compute(x):
    """Cast an input tensor to the compute dtype with the HIP cast kernel."""
    return K.cast(x.contiguous(), _STATE["dtype"])


def _c(x):
    return x if x.is_contiguous() else K.dense_rows(x)


def _wcast(w, dtype):
    """fp32 master weight -> compute-dtype operand (uses the optimiser's bf16 shadow when present)."""
    if dtype == torch.float32:
        return w
    sh = getattr(w, "_s2s_bf16", None)
    if sh is not None:
        return sh
    return K.cast(w.detach(), dtype)


def _dgrad_operand(weight, w, n_out, n_in, dtype):
    """The weight as B operand of dX[M, n_in] = dY[M, n_out] . W[n_out, n_in]  (B(row = k', red = n') = W[n', k']).
    With the optimiser's transposed bf16 shadow (FlatAdam, `_s2s_bf16_t` = W^T (n_in, n_out)) that operand is
    K-contiguous and the GEMM runs on the all-DMA kernel; otherwise W is read row-contiguous (register transposes).
    The transposed shadow is always current: FlatAdam.step() and refresh_shadow() rewrite it in line (refresh_derived)."""
    wt = getattr(weight, "_s2s_bf16_t", None) if dtype == torch.bfloat16 else None
    if wt is not None:
        return K.operand(wt, n_out)
    return K.operand(w, n_in, layout=K.RC)


def _emit_wgrad(param, shape, writer):
    """Run `writer(out, accumulate)` into the flat-grad slot of `param` if it has one (returns None so
    autograd skips it), else into a fresh fp32 tensor (returned to autograd)."""
    slot = getattr(param, "_s2s_grad", None)
    if slot is not None:
        writer(slot.view(shape), True)
        return None
    out = torch.empty(shape, dtype=torch.float32, device=param.device)
    writer(out, False)
    return out


def _emit_vgrad(param, value):
    """Same for small vector gradients already computed in fp32 (`value`)."""
    slot = getattr(param, "_s2s_grad", None)
    if slot is not None:
        K.axpby(1.0, slot.view(-1), 1.0, value.reshape(-1), out=slot.view(-1))
        return None
    return value.view(param.shape)


def _emit_permuted(param, dwp, n, A, Bn):
    """The weight gradient `dwp` (n, A, Bn) as its GEMM left it -> the parameter's (n, Bn, A) layout, accumulated into the flat-gradient
    slot if the parameter has one: ONE launch through LDS (K.permute_inner) instead of an element-wise gather + an axpby."""
    if K.permute_inner_ok(A, Bn):
        slot = getattr(param, "_s2s_grad", None)
        if slot is not None:
            K.permute_inner(dwp, n, A, Bn, out=slot, accumulate=True)
            return None
        return K.permute_inner(dwp, n, A, Bn).view(param.shape)
    return _emit_vgrad(param, K.gather3(dwp, (n, Bn, A), (A * Bn, 1, Bn), 0, torch.float32))


def _slotted(*params):
    return all(p is None or getattr(p, "_s2s_grad", None) is not None for p in params)


def _bias_sink(bias, n):
    """Where a wgrad GEMM should put the fused bias gradient: (buffer, accumulate, value_for_autograd)."""
    if bias is None or not bias.requires_grad:
        return None, False, None
    slot = getattr(bias, "_s2s_grad", None)
    if slot is not None:
        return slot.view(-1), True, None
    buf = torch.empty(n, dtype=torch.float32, device=bias.device)
    return buf, False, buf.view(bias.shape)


def _reduce_to(p_sum, p_dot, mode, dy, x=None, mean=None, rstd=None):
    """Column reduction whose results are the gradients of `p_sum` (sum_r dy) and `p_dot` (sum_r dy*xhat): written
    (accumulated) straight into their flat-gradient slots when they have them -> (None, None) for autograd."""
    s_slot = getattr(p_sum, "_s2s_grad", None)
    d_slot = getattr(p_dot, "_s2s_grad", None) if p_dot is not None else None
    if s_slot is not None and (p_dot is None or d_slot is not None):
        K.colreduce(mode, dy, x, mean, rstd, want_dot=p_dot is not None, out_sum=s_slot.view(-1),
                    out_dot=None if d_slot is None else d_slot.view(-1), accumulate=True)
        return None, None
    s, d = K.colreduce(mode, dy, x, mean, rstd, want_dot=p_dot is not None)
    return s.view(p_sum.shape), (None if d is None else d.view(p_dot.shape))


# ================================================================================================
# Linear (+bias, +activation)          reference: torch.nn.Linear call sites of the hot path
# ================================================================================================


class _Linear(Function):
    """y = act(x W^T + b).  passthrough=True additionally returns an alias of x: a post-LN residual that takes x from there
    sends its gradient back through this node, where it rides in the epilogue of the data-gradient GEMM (dX = dY W + g_pass)
    instead of costing an element-wise add on the main chain."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, passthrough=False):
        dtype = x.dtype
        x2 = _c(x).view(-1, x.shape[-1])
        M, Kd = x2.shape
        N = weight.shape[0]
        w = _wcast(weight, dtype)
        y = torch.empty((M, N), dtype=dtype, device=x.device)
        K.gemm(K.operand(x2, Kd), K.operand(w, Kd), M, N, Kd, y, in_dtype=dtype, bias=bias, act=act)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)
        ctx.save_for_backward(x2, w, y if act else None)
        ctx.xshape = x.shape
        if passthrough:
            ctx.set_materialize_grads(False)
            return y.view(*x.shape[:-1], N), x.view_as(x)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy, g_pass=None):
        if dy is None:                 # only the pass-through output was used
            return g_pass, None, None, None, None
        x2, w, y = ctx.saved_tensors
        weight, bias = ctx.params
        dx, dw, db = _linear_bwd(x2, w, y, ctx.act, weight, bias, ctx.has_bias, dy, g_pass, ctx.needs_input_grad[0])
        return (None if dx is None else dx.view(ctx.xshape)), dw, db, None, None


def _linear_bwd(x2, w, y, act, weight, bias, has_bias, dy, g_pass, want_dx):
    """Backward of y = act(x2 W^T + b) for x2 (M, Kd): -> (dx (M, Kd) = dY W + g_pass, or None without want_dx; dw; db).  The
    weight / bias gradient goes to the flat-gradient slots on a side stream when the parameters have them (dw = db = None)."""
    M, Kd = x2.shape
    N = w.shape[0]
    dtype = x2.dtype
    dy2 = _c(dy).view(M, N)
    if act:
        dy2 = K.act_dropout_bwd(dy2, y, act=act)
    ldy, zp, dy_rows = N, False, dy2
    if dtype == torch.float32 and N % 4 and dy2.is_cuda:
        # rows of N fp32 values with N % 4 != 0 (the 29 spline parameters of a ConvFlow) keep both gradient GEMMs on the
        # element-wise fallback kernel (19 + 37 us per flow): a zero-padded copy with rows of a whole number of 16-byte vectors
        # puts them on the vectorised kernels (the pad columns contribute zeros to the reductions and are never stored)
        ldy, zp = (N + 3) // 4 * 4, True
        dy2 = K.pad_cols(dy2, ldy)
    dx = None
    if want_dx:
        dx = torch.empty((M, Kd), dtype=dtype, device=dy.device)
        res = _c(g_pass).view(M, Kd).to(dtype) if g_pass is not None else None
        K.gemm(K.operand(dy2, ldy, zero_padded=zp), _dgrad_operand(weight, w, N, Kd, dtype), M, Kd, N, dx, in_dtype=dtype, res=res)
    dw = db = None
    if weight.requires_grad:
        tile, sk = K.plan_gemm(N, Kd, M, dtype=dtype)
        rs, racc, db = _bias_sink(bias, N)     # bias gradient = row sums of dY^T, fused into the wgrad GEMM

        def wr(out, acc):
            K.gemm(K.operand(dy2, ldy, layout=K.RC, zero_padded=zp), K.operand(x2, Kd, layout=K.RC), N, Kd, M, out, in_dtype=dtype,
                   splitk=sk, tile=tile, accumulate=acc, a_rowsum=rs, a_rowsum_accumulate=racc)
        if _slotted(weight, bias if has_bias else None):
            _side_run(lambda: _emit_wgrad(weight, (N, Kd), wr), keep=(dy2, x2))
        else:
            dw = _emit_wgrad(weight, (N, Kd), wr)
            if dw is not None:
                dw = dw.view(weight.shape)  # 1x1 Conv1d weights (N, K, 1) are accepted as Linear weights
    elif has_bias and bias.requires_grad:
        db, _ = _reduce_to(bias, None, 0, dy_rows)
    return dx, dw, db


def linear(x, weight, bias=None, act=None, passthrough=False):
    """passthrough=True -> (y, x_alias), see _Linear."""
    return _Linear.apply(x, weight, bias, act, passthrough)


class _FFNRelu(Function):
    """w_2(dropout(act(w_1 x)))  (positionwise_feed_forward.py:30-32), act = relu (Transformer) or swish (Conformer), as two
    GEMMs forward and four backward: activation and dropout mask ride in the first GEMM's epilogue, and the dgrad GEMM
    through w_2 applies dropmask * act' in its epilogue -- relu: (h > 0 <=> active and kept) read off the stored output;
    swish: swish'(u) of the pre-activation u, which the first GEMM writes as a second output -- so no element-wise pass
    over the (rows, hidden) tensor remains."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, p, passthrough=False, act="relu"):
        dtype = x.dtype
        x2 = _c(x).view(-1, x.shape[-1])
        M, Kd = x2.shape
        Hd, N = w1.shape[0], w2.shape[0]
        w1c, w2c = _wcast(w1, dtype), _wcast(w2, dtype)
        seed = K.new_seed(x.device) if p > 0.0 else (None, 0)
        h = torch.empty((M, Hd), dtype=dtype, device=x.device)
        u = torch.empty((M, Hd), dtype=dtype, device=x.device) if act != "relu" else None
        K.gemm(K.operand(x2, Kd), K.operand(w1c, Kd), M, Hd, Kd, h, in_dtype=dtype, bias=b1, act=act, drop_p=p, seed=seed, pre_out=u)
        y = torch.empty((M, N), dtype=dtype, device=x.device)
        K.gemm(K.operand(h, Hd), K.operand(w2c, Hd), M, N, Hd, y, in_dtype=dtype, bias=b2)
        ctx.params = (w1, b1, w2, b2)
        ctx.meta = (p, seed, x.shape)
        ctx.save_for_backward(x2, h, w1c, w2c, u)
        if passthrough:                # (y, alias of x): see _Linear
            ctx.set_materialize_grads(False)
            return y.view(*x.shape[:-1], N), x.view_as(x)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy, g_pass=None):
        if dy is None:
            return g_pass, None, None, None, None, None, None, None
        x2, h, w1c, w2c, u = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        p, seed, xshape = ctx.meta
        M, Kd = x2.shape
        Hd, N = w1c.shape[0], w2c.shape[0]
        dtype = x2.dtype
        dy2 = _c(dy).view(M, N)
        # du = (dY W2) * dropmask * relu'(u): gradient at the pre-activation, straight out of the GEMM
        du = torch.empty((M, Hd), dtype=dtype, device=dy.device)
        K.gemm(K.operand(dy2, N), _dgrad_operand(w2, w2c, N, Hd, dtype), M, Hd, N, du, in_dtype=dtype, emask=h if u is None else u,
               emask_mode=0 if u is None else 1, drop_p=p, seed=seed)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, Kd), dtype=dtype, device=dy.device)
            res = _c(g_pass).view(M, Kd).to(dtype) if g_pass is not None else None
            K.gemm(K.operand(du, Hd), _dgrad_operand(w1, w1c, Hd, Kd, dtype), M, Kd, Hd, dx, in_dtype=dtype, res=res)
            dx = dx.view(xshape)

        def wgrad(weight, bias, g, a, n_out, n_in):
            tile, sk = K.plan_gemm(n_out, n_in, M, dtype=dtype)
            rs, racc, db = _bias_sink(bias, n_out)

            def wr(out, acc):
                K.gemm(K.operand(g, n_out, layout=K.RC), K.operand(a, n_in, layout=K.RC), n_out, n_in, M, out, in_dtype=dtype,
                       splitk=sk, tile=tile, accumulate=acc, a_rowsum=rs, a_rowsum_accumulate=racc)
            if _slotted(weight, bias):
                _side_run(lambda: _emit_wgrad(weight, (n_out, n_in), wr), keep=(g, a))
                return None, None
            dw = _emit_wgrad(weight, (n_out, n_in), wr)
            return (dw.view(weight.shape) if dw is not None else None), db
        dw2, db2 = wgrad(w2, b2, dy2, h, N, Hd) if w2.requires_grad else (None, None)
        dw1, db1 = wgrad(w1, b1, du, x2, Hd, Kd) if w1.requires_grad else (None, None)
        return dx, dw1, db1, dw2, db2, None, None, None


def ffn_relu(x, w1, b1, w2, b2, p=0.0, passthrough=False):
    return _FFNRelu.apply(x, w1, b1, w2, b2, p, passthrough, "relu")


def ffn_act(x, w1, b1, w2, b2, act, p=0.0, passthrough=False):
    """The same block with `act` in ("relu", "swish")."""
    return _FFNRelu.apply(x, w1, b1, w2, b2, p, passthrough, act)


class _Embedding(Function):
    """Token embedding lookup (models/transformer_tts.py:63-77) in the compute dtype; deterministic weight gradient."""

    @staticmethod
    def forward(ctx, idx, weight, padding_idx):
        idx = idx.contiguous()
        ctx.weight, ctx.padding_idx = weight, padding_idx
        ctx.save_for_backward(idx)
        return K.embedding_fwd(idx, weight.detach(), compute_dtype())

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        weight = ctx.weight
        dw = None
        if weight.requires_grad:
            dw = _emit_wgrad(weight, tuple(weight.shape),
                             lambda out, acc: K.embedding_bwd(idx, _c(dy), weight.shape[0], ctx.padding_idx, out=out, accumulate=acc))
        return None, dw, None


def embedding(idx, weight, padding_idx=None):
    return _Embedding.apply(idx, weight, padding_idx)


# ================================================================================================
# LayerNorm, optionally fused with "s = res + hscale * dropout(h)"
# reference: modules/transformer/layer_norm.py:12-42 + residual/dropout lines of the layer classes
# ================================================================================================
class _AddLayerNorm(Function):
    @staticmethod
    def forward(ctx, h, res, gamma, beta, eps, p, hscale):
        seed = K.new_seed(h.device) if p > 0.0 else (None, 0)
        h = _c(h)
        res = _c(res) if res is not None else None
        y, s, mean, rstd = K.layernorm_fwd(h, gamma, beta, eps, res=res, p=p, seed=seed, hscale=hscale)
        ctx.meta = (eps, p, seed, hscale, res is not None)
        ctx.params = (gamma, beta)
        ctx.save_for_backward(s if res is not None else h, mean, rstd)
        ctx.set_materialize_grads(False)
        if res is None:
            return y
        return y, s

    @staticmethod
    def backward(ctx, dy, ds_direct=None):
        s, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.params
        eps, p, seed, hscale, fused = ctx.meta
        dy = _c(dy) if dy is not None else torch.zeros_like(s)
        extra = _c(ds_direct) if (fused and ds_direct is not None) else None
        slotted = gamma.requires_grad and _slotted(gamma, beta)
        ds, dh, part = K.layernorm_bwd(dy, s, mean, rstd, gamma, ds_extra=extra, p=p, seed=seed,
                                       want_dh=fused and (p > 0.0 or hscale != 1.0), hscale=hscale, want_partials=True, partials_ok=slotted)
        dgamma = dbeta = None
        if gamma.requires_grad:
            if part is not None:
                # the backward kernel left the first reduction stage of d gamma / d beta (big sites: dy and the LayerNorm input are not
                # read a second time); the second stage joins the batch's grouped column reductions
                ws, chunks = part
                b_slot, g_slot = beta._s2s_grad.view(-1), gamma._s2s_grad.view(-1)
                _side_run(lambda: K.colreduce_partials(ws, chunks, s.shape[-1], b_slot, g_slot), keep=(ws,))
            elif _slotted(gamma, beta):
                _side_run(lambda: _reduce_to(beta, gamma, 1, dy, s, mean, rstd), keep=(dy, s, mean, rstd))
            else:
                dbeta, dgamma = _reduce_to(beta, gamma, 1, dy, s, mean, rstd)
        if fused:
            return (dh if dh is not None else ds), ds, dgamma, dbeta, None, None, None
        return ds, None, dgamma, dbeta, None, None, None


class _LayerNormPass(Function):
    """(LayerNorm(x), alias of x): a pre-LN layer feeds x to its first norm AND to the residual behind the first sub-layer.  With the
    residual taken from the alias both gradients meet inside the LayerNorm backward kernel (its `ds_extra` operand) instead of in an
    element-wise add of autograd's accumulation (8 x 7 us on the chain of an AAS-VC step: profiles/r05_aasvc_train_bf16_timeline.txt)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = _c(x)
        y, _, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps)
        ctx.params = (gamma, beta)
        ctx.save_for_backward(x, mean, rstd)
        ctx.set_materialize_grads(False)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dx_pass=None):
        x, mean, rstd = ctx.saved_tensors
        gamma, beta = ctx.params
        if dy is None:                                  # only the alias was used
            return dx_pass, None, None, None
        dy = _c(dy)
        slotted = gamma.requires_grad and _slotted(gamma, beta)
        ds, _, part = K.layernorm_bwd(dy, x, mean, rstd, gamma, ds_extra=_c(dx_pass) if dx_pass is not None else None,
                                      want_partials=True, partials_ok=slotted)
        dgamma = dbeta = None
        if gamma.requires_grad:
            if part is not None:
                ws, chunks = part
                b_slot, g_slot = beta._s2s_grad.view(-1), gamma._s2s_grad.view(-1)
                _side_run(lambda: K.colreduce_partials(ws, chunks, x.shape[-1], b_slot, g_slot), keep=(ws,))
            elif _slotted(gamma, beta):
                _side_run(lambda: _reduce_to(beta, gamma, 1, dy, x, mean, rstd), keep=(dy, x, mean, rstd))
            else:
                dbeta, dgamma = _reduce_to(beta, gamma, 1, dy, x, mean, rstd)
        return ds, dgamma, dbeta, None


def layer_norm(x, gamma, beta, eps=1e-12, passthrough=False):
    """passthrough=True -> (LayerNorm(x), alias of x): take a residual that starts at x from the alias (see _LayerNormPass)."""
    if passthrough and torch.is_grad_enabled() and x.requires_grad:
        return _LayerNormPass.apply(x, gamma, beta, eps)
    y = _AddLayerNorm.apply(x, None, gamma, beta, eps, 0.0, 1.0)
    return (y, x) if passthrough else y


class _FanOut(Function):
    """n aliases of x for n consumers: their gradients arrive at ONE autograd node and are summed by one launch of s2svc_add_n (two
    when n > 4) instead of by n - 1 element-wise adds of autograd's accumulation."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [_c(g) for g in grads if g is not None]
        if not gs:
            return None, None
        while len(gs) > 1:
            gs = [K.add_n(gs[:4])] + gs[4:]
        return gs[0], None


def fan_out(x, n):
    """x for n consumers (see _FanOut); plain copies of the reference when no gradient is recorded."""
    if n < 2 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * n
    return _FanOut.apply(x, n)


def add_dropout_layer_norm(res, h, gamma, beta, eps=1e-12, p=0.0, hscale=1.0):
    """s = res + hscale*dropout(h, p); y = LayerNorm(s).  Returns (y, s)."""
    return _AddLayerNorm.apply(h, res, gamma, beta, eps, p, hscale)


class _AddDropout(Function):
    """s = res + hscale * dropout(h)   (a residual that is not followed by a LayerNorm)."""

    @staticmethod
    def forward(ctx, h, res, p, hscale):
        seed = K.new_seed(h.device) if p > 0.0 else (None, 0)
        hd = K.act_dropout_fwd(_c(h), p=p, seed=seed) if p > 0.0 else _c(h)
        ctx.meta = (p, seed, hscale)
        return K.axpby(1.0, _c(res), hscale, hd)

    @staticmethod
    def backward(ctx, ds):
        p, seed, hscale = ctx.meta
        ds = _c(ds)
        dh = ds
        if p > 0.0:
            dh = K.act_dropout_bwd(ds, ds, act=None, p=p, seed=seed)
        if hscale != 1.0:
            dh = K.axpby(hscale, dh)
        return dh, ds, None, None


def add_dropout(res, h, p=0.0, hscale=1.0):
    return _AddDropout.apply(h, res, p, hscale)


# ================================================================================================
# dropout / activations
# ================================================================================================
class _ActDropout(Function):
    @staticmethod
    def forward(ctx, x, act, p):
        seed = K.new_seed(x.device) if p > 0.0 else (None, 0)
        x = _c(x)
        y = K.act_dropout_fwd(x, act=act, p=p, seed=seed)
        ctx.meta = (act, p, seed)
        ctx.save_for_backward(x if act in ("swish", "gelu") else y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (saved,) = ctx.saved_tensors
        act, p, seed = ctx.meta
        return K.act_dropout_bwd(_c(dy), saved, act=act, p=p, seed=seed), None, None


def act_dropout(x, act=None, p=0.0):
    if act is None and p <= 0.0:
        return x
    return _ActDropout.apply(x, act, p)


def dropout(x, p, training=True):
    return act_dropout(x, None, p if training else 0.0)


class _Glu(Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.save_for_backward(x)
        return K.glu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return K.glu_bwd(x, _c(dy))


def glu(x):
    return _Glu.apply(x)


# ================================================================================================
# positional encodings          reference: layers/positional_encoding.py
# ================================================================================================
class _PosEnc(Function):
    @staticmethod
    def forward(ctx, x, alpha, pe, xscale, p):
        seed = K.new_seed(x.device) if p > 0.0 else (None, 0)
        x = _c(x)
        y = K.posenc_fwd(x, xscale, alpha, pe, p=p, seed=seed)
        ctx.meta = (xscale, p, seed)
        ctx.alpha = alpha
        ctx.save_for_backward(pe)
        return y

    @staticmethod
    def backward(ctx, dy):
        (pe,) = ctx.saved_tensors
        xscale, p, seed = ctx.meta
        alpha = ctx.alpha
        want = alpha is not None and alpha.requires_grad
        dx, dalpha = K.posenc_bwd(_c(dy), xscale, pe, p=p, seed=seed, want_dalpha=want)
        if want:
            dalpha = _emit_vgrad(alpha, dalpha)
        return dx, dalpha, None, None, None


def posenc(x, pe, alpha=None, xscale=1.0, p=0.0):
    """y = dropout(x*xscale + alpha*pe[:T])  (pe None -> scaling only)."""
    return _PosEnc.apply(x, alpha, pe, xscale, p)


# ================================================================================================
# Conv1d (stride 1, 'same' padding, channel-last activations) as an implicit GEMM
# reference: Postnet / AlignmentModule / DurationPredictor / FFN Conv1d call sites
# ================================================================================================


class _Conv1d(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act):
        x = _c(x)
        B, T, Cin = x.shape
        Cout, _, ks = weight.shape
        pad = (ks - 1) // 2
        dtype = x.dtype
        wp = K.gather3_cached(weight, (Cout, ks, Cin), (Cin * ks, 1, ks), 0, dtype)  # (O, k, I)
        y = torch.empty((B, T, Cout), dtype=dtype, device=x.device)
        K.gemm(K.operand(x, Cin, mode=K.CONV1D, C=Cin, T=T, pad=pad), K.operand(wp, ks * Cin), B * T, Cout, ks * Cin, y,
               in_dtype=dtype, bias=bias, act=act)
        ctx.act = act
        ctx.params = (weight, bias)
        ctx.save_for_backward(x, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight, bias = ctx.params
        B, T, Cin = x.shape
        Cout, _, ks = weight.shape
        pad = (ks - 1) // 2
        dtype = x.dtype
        dy = _c(dy)
        if ctx.act:
            dy = K.act_dropout_bwd(dy, y, act=ctx.act)
        dx = None
        if ctx.needs_input_grad[0]:
            wd = K.gather3_cached(weight, (Cin, ks, Cout), (ks, -1, Cin * ks), ks - 1, dtype)  # (I, k flipped, O)
            dx = torch.empty((B, T, Cin), dtype=dtype, device=x.device)
            K.gemm(K.operand(dy, Cout, mode=K.CONV1D, C=Cout, T=T, pad=pad), K.operand(wd, ks * Cout), B * T, Cin, ks * Cout, dx,
                   in_dtype=dtype)
        dw = db = None
        if weight.requires_grad:
            def work():
                # forked gradient batches (VTN, Transformer-TTS): the batch's eligible layers share ONE capped launch that adds into
                # the (Cout, Cin, ks) slots (csrc/conv1d_wgrad.hip) instead of split-K GEMM + reduction + permutation per layer
                if (K.in_capped_batch() and _slotted(weight) and K.conv1d_wgrad_enabled()
                        and K.conv1d_wgrad_supported(Cout, Cin, ks, dtype, bias) and K.conv1d_wgrad_queue(dy, x, weight._s2s_grad)):
                    return None, None
                dwp = torch.empty((Cout, ks * Cin), dtype=torch.float32, device=x.device)
                rs, racc, dbv = _bias_sink(bias, Cout)
                tile, sk = K.plan_gemm(Cout, ks * Cin, B * T)
                # wgrad=True: big bf16 outputs (the aligner's 1536 x 4608 over 4096 frames) run on the ragged 8-wave weight-gradient kernel
                # with the implicit im2col B operand (csrc/gemm_8ph.hip "w8_conv" kind 1); everything else as before
                K.gemm(K.operand(dy, Cout, layout=K.RC), K.operand(x, Cin, layout=K.RC, mode=K.CONV1D, C=Cin, T=T, pad=pad),
                       Cout, ks * Cin, B * T, dwp, in_dtype=dtype, splitk=sk, tile=tile, a_rowsum=rs, a_rowsum_accumulate=racc,
                       wgrad=True)
                return _emit_permuted(weight, dwp, Cout, ks, Cin), dbv
            if _slotted(weight, bias):
                _side_run(work, keep=(dy, x))
            else:
                dw, db = work()
        elif bias is not None and bias.requires_grad:
            db, _ = _reduce_to(bias, None, 0, dy.view(B * T, Cout))
        return dx, dw, db, None


class _CropRows(Function):
    """Rows t >= vlens[b] of a (B, T, C) tensor are ABSENT (a captured training step on a batch shorter than its padded shape,
    modules.Lens.crop): zero on the way in -- what a 'same'-padded convolution behind this op reads where the reference's cropped
    tensor ends (models/vtn.py:208-214) -- and zero on the way back, so that no gradient leaves a frame the reference does not have."""

    @staticmethod
    def forward(ctx, x, vlens):
        from . import kernels_sdp as KS
        ctx.vlens = vlens
        return KS.mask_rows(_c(x), vlens)

    @staticmethod
    def backward(ctx, dy):
        from . import kernels_sdp as KS
        return KS.mask_rows(_c(dy), ctx.vlens), None


def crop_rows(x, vlens):
    """Identity when vlens is None (every row present)."""
    return x if vlens is None else _CropRows.apply(x, vlens)


def conv1d(x, weight, bias=None, act=None, vlens=None):
    """x (B,T,Cin) channel-last; weight (Cout,Cin,k) torch layout; returns (B,T,Cout).
    vlens (B int32, device; captured steps only): input frames t >= vlens[b] are absent -- read as zero padding (k > 1), and no
    gradient flows back into them.  The OUTPUT frames beyond vlens are not cleared: whoever mixes along time next does that."""
    if vlens is not None and weight.shape[-1] > 1:
        x = crop_rows(x, vlens)
    return _Conv1d.apply(x, weight, bias, act)


# ================================================================================================
# Conv2d 3x3 stride 2 (+ReLU) on NHWC activations         reference: subsampling.py:58-63
# ================================================================================================
#                                                                    (189 vs 190 us), so the plain launches stay the default




class _Conv2dS2(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, grad_premasked=False, input_is_relu=False):
        x = _c(x)
        ctx.grad_premasked = grad_premasked
        ctx.input_is_relu = input_is_relu
        B, T1, F1, C = x.shape
        O = weight.shape[0]
        T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
        dtype = x.dtype
        wp = K.gather3_cached(weight, (O, 9, C), (C * 9, 1, 9), 0, dtype)  # (O, tap, C)
        y = torch.empty((B, T2, F2, O), dtype=dtype, device=x.device)
        K.gemm(K.operand(x, C, mode=K.CONV2D_S2, C=C, T1=T1, F1=F1, T2=T2, F2=F2), K.operand(wp, 9 * C), B * T2 * F2, O, 9 * C, y,
               in_dtype=dtype, bias=bias, act="relu")
        ctx.params = (weight, bias)
        ctx.save_for_backward(x, y, wp)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, wp = ctx.saved_tensors
        weight, bias = ctx.params
        B, T1, F1, C = x.shape
        O = weight.shape[0]
        T2, F2 = y.shape[1], y.shape[2]
        M2 = B * T2 * F2
        dtype = x.dtype
        # the consumer may already have applied relu' in its dgrad epilogue (linear_fc_permuted(..., input_is_relu=True))
        dy = _c(dy) if ctx.grad_premasked else K.act_dropout_bwd(_c(dy), y, act="relu")
        dw = db = None
        if weight.requires_grad:
            def work():
                dwp = torch.empty((O, 9 * C), dtype=torch.float32, device=x.device)
                rs, racc, dbv = _bias_sink(bias, O)
                tile, sk = K.plan_gemm(O, 9 * C, M2)
                # bf16, C % 128 == 0: the ragged 8-wave weight-gradient kernel with the implicit im2col B operand (wgrad=True;
                # csrc/gemm_8ph.hip "w8_conv"), otherwise the 4-wave split-K kernel
                K.gemm(K.operand(dy, O, layout=K.RC),
                       K.operand(x, C, layout=K.RC, mode=K.CONV2D_S2, C=C, T1=T1, F1=F1, T2=T2, F2=F2), O, 9 * C, M2, dwp,
                       in_dtype=dtype, splitk=sk, tile=tile, a_rowsum=rs, a_rowsum_accumulate=racc, wgrad=True)
                return _emit_permuted(weight, dwp, O, 9, C), dbv
            if _slotted(weight, bias):
                # queued AND forked before the data-gradient GEMM below: this is the last big layer of the backward pass,
                # its weight gradient would otherwise run alone after the main chain has ended.  (Sending the batch queued so
                # far to ANOTHER stream first -- so that its grouped weight gradients do not wait behind this 150-280 us GEMM --
                # was measured: 4.24 vs 4.20 ms per VTN step, the extra concurrent work slows the transposed convolution on the
                # main stream, which is the critical path.  Issuing it AFTER the data-gradient GEMMs instead: 4.33 ms.)
                _side_run(work, keep=(dy, x))
                _side_flush()
            else:
                dw, db = work()
        dx = None
        if ctx.needs_input_grad[0] and dtype == torch.bfloat16 and O % 8 == 0 and O >= 64 and C % 8 == 0:
            # transposed convolution as four implicit GEMMs, one per parity class (t1 % 2, f1 % 2) of input pixels: each
            # gathers its 4 / 2 / 2 / 1 taps of dY straight from HBM and stores into its pixels of dX (no dcols, no col2im)
            wts = K.tconv2d_weights_cached(weight)       # a managed weight: kept fresh by the optimiser, nothing launched here
            dx = torch.empty((B, T1, F1, C), dtype=dtype, device=x.device)
            mask = x if ctx.input_is_relu else None     # x = relu(u): the GEMMs hand back dL/du (mask rows follow the c_map)
            for cls, wt in enumerate(wts):
                pt, pf = cls >> 1, cls & 1
                Tc, Fc = (T1 - pt + 1) // 2, (F1 - pf + 1) // 2
                if Tc <= 0 or Fc <= 0:
                    continue
                Kc = wt.shape[1]
                K.gemm(K.operand(dy, O, mode=K.TCONV2D_S2, C=O, T1=Tc, F1=Fc, T2=T2, F2=F2, pad=cls), K.operand(wt, Kc),
                       B * Tc * Fc, C, Kc, dx, in_dtype=dtype, c_map=(T1, F1, Tc, Fc, pt, pf), emask=mask)
        elif ctx.needs_input_grad[0]:
            dcols = torch.empty((M2, 9 * C), dtype=dtype, device=x.device)
            K.gemm(K.operand(dy, O), K.operand(wp, 9 * C, layout=K.RC), M2, 9 * C, O, dcols, in_dtype=dtype)
            dx = K.col2im_s2(dcols, B, T1, F1, C, T2, F2)
            if ctx.input_is_relu:
                dx = K.act_dropout_bwd(dx, x, act="relu")
        if not weight.requires_grad and bias is not None and bias.requires_grad:
            db, _ = _reduce_to(bias, None, 0, dy.view(M2, O))
        return dx, dw, db, None, None


def conv2d_s2_relu(x_nhwc, weight, bias, grad_premasked=False, input_is_relu=False):
    """grad_premasked=True: the ONLY consumer of the result hands back a gradient that already carries relu'
    (see linear_fc_permuted(input_is_relu=True)); the backward then skips its own mask pass.
    input_is_relu=True: x_nhwc is a ReLU output whose producer wants dL/d(pre-activation) back (conv_in1_relu(grad_premasked=True)):
    relu'(x) is applied in the epilogue of the data-gradient GEMMs."""
    return _Conv2dS2.apply(x_nhwc, weight, bias, grad_premasked, input_is_relu)


class _ConvIn1(Function):
    """Conv2d(1 -> O, 3x3, stride 2) + ReLU straight on the (B, T, F) mel batch (subsampling.py:58-60)."""

    @staticmethod
    def forward(ctx, x, weight, bias, grad_premasked=False):
        x = _c(x)
        y = K.conv_in1_fwd(x, weight.detach(), bias.detach() if bias is not None else None)
        ctx.params = (weight, bias)
        ctx.grad_premasked = grad_premasked
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight, bias = ctx.params
        # relu' is applied inside the wgrad kernel (y > 0: no mask pass over 60 M values) -- unless the consumer's data-gradient
        # GEMM already did it in its epilogue (conv2d_s2_relu(input_is_relu=True)): then the kernel reads dy only (122 instead of
        # 244 MB at VTN's shapes -- this kernel is the very end of the backward pass)
        dy = _c(dy)
        ym = None if ctx.grad_premasked else y
        wslot, bslot = getattr(weight, "_s2s_grad", None), getattr(bias, "_s2s_grad", None) if bias is not None else None
        if wslot is not None and (bias is None or bslot is not None):
            # its own fork: the last closure of the backward pass must not queue behind the batch it would otherwise end
            _side_run(lambda: K.conv_in1_wgrad(x, dy, wslot, bslot, True, y=ym), keep=(x, dy, y), solo=True)
            return None, None, None, None
        dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
        db = torch.empty(bias.shape, dtype=torch.float32, device=x.device) if bias is not None else None
        K.conv_in1_wgrad(x, dy, dw, db, False, y=ym)
        return None, dw, db, None


def conv_in1_relu(x, weight, bias, grad_premasked=False):
    """grad_premasked=True: the ONLY consumer hands back a gradient that already carries relu' of this layer's output."""
    return _ConvIn1.apply(x, weight, bias, grad_premasked)




class _LinearPermuted(Function):
    """y = x2d . Wp^T + b where Wp[d, f*C + c] = W[d, c*F + f]: the Linear after the conv2d front-end
    (subsampling.py:64-70 flattens (c, f); our activations are (f, c) channel-last)."""

    @staticmethod
    def forward(ctx, x, weight, bias, C, Fd, input_is_relu=False):
        x = _c(x)
        ctx.input_is_relu = input_is_relu
        dtype = x.dtype
        D = weight.shape[0]
        M = x.numel() // (C * Fd)
        wp = K.gather3_cached(weight, (D, Fd, C), (C * Fd, 1, Fd), 0, dtype)
        y = torch.empty((M, D), dtype=dtype, device=x.device)
        K.gemm(K.operand(x, C * Fd), K.operand(wp, C * Fd), M, D, C * Fd, y, in_dtype=dtype, bias=bias)
        ctx.params = (weight, bias)
        ctx.meta = (C, Fd)
        ctx.save_for_backward(x, wp)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wp = ctx.saved_tensors
        weight, bias = ctx.params
        C, Fd = ctx.meta
        D = weight.shape[0]
        Kd = C * Fd
        M = x.numel() // Kd
        dtype = x.dtype
        dy = _c(dy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, Kd), dtype=dtype, device=x.device)
            mask = x.view(M, Kd) if ctx.input_is_relu else None              # x = relu(u): hand back dL/du
            if dtype == torch.bfloat16:
                # the permuted weight once more, TRANSPOSED ((f, c) rows of D values: a cached copy the optimiser keeps fresh):
                # both operands K-contiguous, so the 2016 x 7296 x 384 product runs on the 8-wave kernel instead of the 4-wave
                # kernel's transposing fragment reads (65 -> ~25 us at the end of VTN's backward chain)
                wd = K.gather3_cached(weight, (Fd, C, D), (1, Fd, C * Fd), 0, dtype)
                K.gemm(K.operand(dy, D), K.operand(wd, D), M, Kd, D, dx, in_dtype=dtype, emask=mask)
            else:
                K.gemm(K.operand(dy, D), K.operand(wp, Kd, layout=K.RC), M, Kd, D, dx, in_dtype=dtype, emask=mask)
            dx = dx.view(x.shape)
        dw = db = None
        if weight.requires_grad:
            def work():
                dwp = torch.empty((D, Kd), dtype=torch.float32, device=x.device)
                rs, racc, dbv = _bias_sink(bias, D)
                tile, sk = K.plan_gemm(D, Kd, M)
                K.gemm(K.operand(dy, D, layout=K.RC), K.operand(x, Kd, layout=K.RC), D, Kd, M, dwp, in_dtype=dtype,
                       splitk=sk, tile=tile, a_rowsum=rs, a_rowsum_accumulate=racc, wgrad=True)
                return _emit_permuted(weight, dwp, D, Fd, C), dbv
            if _slotted(weight, bias):
                _side_run(work, keep=(dy, x))
            else:
                dw, db = work()
        elif bias is not None and bias.requires_grad:
            db, _ = _reduce_to(bias, None, 0, dy)
        return dx, dw, db, None, None, None


def linear_fc_permuted(x, weight, bias, C, Fd, input_is_relu=False):
    return _LinearPermuted.apply(x, weight, bias, C, Fd, input_is_relu)


# ================================================================================================
# BatchNorm1d over (B*T) rows, channel-last, fused with activation + dropout
# reference: pre_postnets.py:108-165, conformer/convolution.py:73-75
# ================================================================================================
class _BatchNormAct(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, num_batches, training, act, p, eps, momentum, vlens=None):
        x = _c(x)
        C = x.shape[-1]
        rows = x.numel() // C
        seed = K.new_seed(x.device) if p > 0.0 else (None, 0)
        if not training:
            vlens = None
        Tn = x.shape[-2] if vlens is not None else 0       # absent rows (include/s2svc_hip.h): out of the statistics, zero in y and dx
        ctx.vl = (vlens, Tn)
        ctx.vec = training and K.bn_vec_ok(x)
        if ctx.vec:     # bf16: 16-byte kernels; the backward pass recomputes the activation / dropout derivative (csrc/batchnorm.hip)
            mean, rstd = K.bn_stats_vec(x, rows, C, eps, momentum, run_mean, run_var, num_batches, vlens=vlens, Tn=Tn)
            need_pre = act in ("swish", "gelu")
            y, pre = K.bn_act_apply_vec(x, mean, rstd, gamma.detach(), beta.detach(), act=act, p=p, seed=seed, want_pre=need_pre,
                                        vlens=vlens, Tn=Tn)
            ctx.meta = (training, act, p, seed)
            ctx.params = (gamma, beta)
            ctx.save_for_backward(x, mean, rstd, (pre if need_pre else y) if (act or p > 0.0) else None)
            return y
        if training:
            if x.dtype == torch.bfloat16:      # one pass over x: mean and E[x^2] together (fp32 sums of bf16 values)
                mean, rstd = K.bn_stats(x, rows, C, eps, momentum, run_mean, run_var, num_batches, vlens=vlens, Tn=Tn)
            else:                              # parity mode: the two-pass variance torch computes
                sc = 1.0 / rows if vlens is None else -1.0          # < 0: 1 / (number of present rows), on the device
                mean, _ = K.colreduce(0, x.view(rows, C), scale=sc, vlens=vlens, Tn=Tn)
                var, _ = K.colreduce(3, None, x=x.view(rows, C), mean=mean, scale=sc, rows=rows, D=C, vlens=vlens, Tn=Tn)
                rstd = K.bn_finalize(mean, var, rows, eps, momentum, run_mean, run_var, num_batches, vlens=vlens, Tn=Tn)
        else:
            mean = run_mean
            rstd = K.rstd_from_var(run_var, eps)
        need_pre = act in ("swish", "gelu")
        y, pre = K.bn_apply(x, mean, rstd, gamma, beta, act=act, p=p, seed=seed, want_pre=need_pre, vlens=vlens, Tn=Tn)
        ctx.meta = (training, act, p, seed)
        ctx.params = (gamma, beta)
        ctx.save_for_backward(x, mean, rstd, pre if need_pre else y)
        return y

    @staticmethod
    def backward(ctx, dz):
        x, mean, rstd, saved = ctx.saved_tensors
        gamma, beta = ctx.params
        training, act, p, seed = ctx.meta
        C = x.shape[-1]
        rows = x.numel() // C
        dy = _c(dz)
        vlens, Tn = ctx.vl
        if ctx.vec:
            g_slot = getattr(gamma, "_s2s_grad", None) if gamma.requires_grad else None
            b_slot = getattr(beta, "_s2s_grad", None) if beta.requires_grad else None
            both = g_slot is not None and b_slot is not None
            dx, sdy, sdyx = K.bn_act_bwd_vec(dy, saved, x, mean, rstd, gamma.detach(), act=act, p=p, seed=seed,
                                             dgamma_acc=g_slot.view(-1) if both else None, dbeta_acc=b_slot.view(-1) if both else None,
                                             vlens=vlens, Tn=Tn)
            dgamma = dbeta = None
            if gamma.requires_grad and not both:
                dgamma, dbeta = _emit_vgrad(gamma, sdyx), _emit_vgrad(beta, sdy)
            return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None
        if act or p > 0.0:
            dy = K.act_dropout_bwd(dy, saved, act=act, p=p, seed=seed)
        sdy, sdyx = K.colreduce(2, dy.view(rows, C), x.view(rows, C), mean, rstd, want_dot=True, vlens=vlens, Tn=Tn)
        dx = K.bn_bwd(dy, x, mean, rstd, gamma, sdy, sdyx, use_batch_stats=training, vlens=vlens, Tn=Tn)
        dgamma = dbeta = None
        if gamma.requires_grad:
            if _slotted(gamma, beta):      # the two accumulations into the gradient slots leave the data-gradient chain
                _side_run(lambda: (_emit_vgrad(gamma, sdyx), _emit_vgrad(beta, sdy)), keep=(sdy, sdyx))
            else:
                dgamma, dbeta = _emit_vgrad(gamma, sdyx), _emit_vgrad(beta, sdy)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, run_mean, run_var, num_batches, training, act=None, p=0.0, eps=1e-5, momentum=0.1, vlens=None):
    """vlens (B int32, device; x must be (B, T, C)): frames t >= vlens[b] are absent -- not in the batch statistics, zero in the
    output and in the data gradient (captured steps on batches shorter than their padded shape; include/s2svc_hip.h)."""
    return _BatchNormAct.apply(x, gamma, beta, run_mean, run_var, num_batches, training, act, p, eps, momentum, vlens)


# ================================================================================================
# losses
# ================================================================================================


class _WeightedSum(Function):
    """sum_i w_i * sum(x_i) of fp32 tensors (scalars or small vectors) as ONE launch each way: the training loss from its parts
    (trainers/ar_vc.py:86-97, trainers/aas_vc.py:100-139) without a chain of 0-dim ATen adds / muls and their autograd nodes."""

    @staticmethod
    def forward(ctx, weights, *xs):
        xs = [_c(x.float()) for x in xs]
        ctx.meta = ([tuple(x.shape) for x in xs], list(weights))
        return K.weighted_sum(list(zip(xs, weights)))

    @staticmethod
    def backward(ctx, g):
        shapes, weights = ctx.meta
        outs = K.weighted_sum_bwd(_c(g.float()), list(zip(shapes, weights)), g.device)
        return (None,) + tuple(outs)


def weighted_sum(terms):
    """terms: [(tensor, weight)] (at most 8) -> 0-dim fp32 tensor sum_i weight_i * tensor_i.sum()."""
    return _WeightedSum.apply(tuple(float(w) for _, w in terms), *[t for t, _ in terms])


class _SeqLoss(Function):
    @staticmethod
    def forward(ctx, after, before, logits, ys, labels, olens_i32, pos_weight):
        after = _c(after) if after is not None else None
        before = _c(before)
        logits = _c(logits) if logits is not None else None
        ys = _c(ys.float())
        labels = _c(labels.float()) if labels is not None else None
        out = K.seq_loss_fwd(after, before, logits, ys, labels, olens_i32, pos_weight)
        ctx.pos_weight = pos_weight
        ctx.save_for_backward(after, before, logits, ys, labels, olens_i32, out)
        ctx.set_materialize_grads(False)          # an unused loss (bce of the L1-only criterion) arrives as None, not as a zeros launch
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_l1, g_bce):
        after, before, logits, ys, labels, olens_i32, out = ctx.saved_tensors
        g1 = _c(g_l1.float()) if g_l1 is not None else None
        g2 = _c(g_bce.float()) if g_bce is not None else None
        if g1 is None:
            g1 = _zero_scalar(before.device)
        if g2 is None:
            g2 = _zero_scalar(before.device)
        da, db, dl = K.seq_loss_bwd(after, before, logits, ys, labels, olens_i32, ctx.pos_weight, out, g1, g2)
        return da, db, dl, None, None, None, None


def seq2seq_loss(after, before, logits, ys, labels, olens_i32, pos_weight=10.0):
    """(l1, bce): losses/seq2seq_loss.py:30-59; `logits`/`labels` None -> l1 only (losses/l1_loss.py)."""
    return _SeqLoss.apply(after, before, logits, ys, labels, olens_i32, pos_weight)


class _GuidedAttnLoss(Function):
    @staticmethod
    def forward(ctx, att, ilens_i32, olens_i32, sigma, alpha):
        att = _c(att)
        out = K.guided_attn_loss_fwd(att, ilens_i32, olens_i32, sigma, alpha)
        ctx.meta = (att.shape, att.dtype, sigma, alpha)
        ctx.save_for_backward(ilens_i32, olens_i32, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        ilens_i32, olens_i32, out = ctx.saved_tensors
        shape, dtype, sigma, alpha = ctx.meta
        return K.guided_attn_loss_bwd(shape, dtype, g.device, ilens_i32, olens_i32, sigma, alpha, out, _c(g.float())), None, None, None, None


def guided_attention_loss(att, ilens_i32, olens_i32, sigma=0.4, alpha=1.0):
    return _GuidedAttnLoss.apply(att, ilens_i32, olens_i32, sigma, alpha)


# ================================================================================================
# monotonic alignment search + binarisation loss     reference: modules/alignments.py:281-310
# ================================================================================================
class _Viterbi(Function):
    @staticmethod
    def forward(ctx, log_p_attn, text_lens_i32, feat_lens_i32):
        lp = _c(log_p_attn.float())
        ds, path, binmean = K.mas(lp, text_lens_i32, feat_lens_i32)
        B = lp.shape[0]
        bin_loss = K.weighted_sum([(binmean, -1.0 / B)])          # -(sum_b mean_t log p[b, t, path]) / B, one launch
        ctx.save_for_backward(path, feat_lens_i32)
        ctx.shape = lp.shape
        ctx.in_dtype = log_p_attn.dtype
        ctx.mark_non_differentiable(ds, path)
        ctx.set_materialize_grads(False)
        return ds, bin_loss, path

    @staticmethod
    def backward(ctx, _dds, g, _dpath):
        if g is None:
            return None, None, None
        path, feat_lens_i32 = ctx.saved_tensors
        dlogp = K.zeros(ctx.shape, torch.float32, g.device)
        K.mas_binloss_bwd(path, feat_lens_i32, _c(g.float()), dlogp)
        return dlogp.to(ctx.in_dtype), None, None


def viterbi_decode(log_p_attn, text_lens_i32, feat_lens_i32):
    """-> (ds (B,T_text) fp32, bin_loss scalar (differentiable), path (B,T_feats) int32)."""
    return _Viterbi.apply(log_p_attn, text_lens_i32, feat_lens_i32)
