"""Launchers of the HiFi-GAN generator kernels (csrc/hifigan.hip; C ABI in include/s2svc_hip.h).  Non-differentiable, GPU tensors
only, channel-last activations (B, T, C) -- see kernels.py for the conventions."""
import torch

from .. import _lib
from .kernels import _need_cuda, dt, ptr, stream, zeros

KC = 32                      # input channels per reduction step of the implicit GEMM (s2svc_hifigan_cin_padded)


def cin_padded(c):
    return (c + KC - 1) // KC * KC


def _check_act(x, B, T, C, name):
    if x.dim() != 3 or tuple(x.shape) != (B, T, C) or not x.is_contiguous():
        raise ValueError(f"{name}: contiguous (B, T, C) = {(B, T, C)} expected, got {tuple(x.shape)}")


def _out_act(name, out, like, B, T, C, accumulate=False):
    """The output of a convolution launch: `out` (required when it is accumulated into), or a new tensor in `like`'s dtype; checked to be
    contiguous (B, T, C) in that dtype -- the kernels store like's element size."""
    if out is None:
        if accumulate:
            raise ValueError(f"{name}: accumulate needs out")
        out = torch.empty(B, T, C, dtype=like.dtype, device=like.device)
    _check_act(out, B, T, C, f"{name} out")
    if out.dtype != like.dtype:
        raise TypeError(f"{name}: out dtype")
    return out


def hifigan_conv1d(x, w_op, bias, k, dil, cout, slope=0.0, res=None, accumulate=False, scale=1.0, tanh=False, out=None, vlens=None,
                   vmul=1):
    """out = (accumulate ? out : 0) + scale * (conv1d(leaky_relu(x, slope)) + bias (+ res)), optional tanh; x (B, T, C_in)."""
    _need_cuda(x, w_op, bias, res, out, vlens)
    B, T, cin = x.shape
    _check_act(x, B, T, cin, "hifigan_conv1d x")
    if w_op.dtype != x.dtype or w_op.numel() != cout * k * cin_padded(cin):
        raise ValueError("hifigan_conv1d: operand does not match (C_out, k, C_in padded) in the activation dtype")
    out = _out_act("hifigan_conv1d", out, x, B, T, cout, accumulate)
    if res is not None:
        _check_act(res, B, T, cout, "hifigan_conv1d res")
        if res.dtype != x.dtype:
            raise TypeError("hifigan_conv1d: res dtype")
    _lib.check(_lib.lib().s2svc_hifigan_conv1d(dt(x), B, T, cin, cout, k, dil, ptr(x), ptr(w_op), ptr(bias), float(slope), ptr(res),
                                               int(accumulate), float(scale), int(tanh), ptr(out), ptr(vlens), int(vmul), stream()),
               "hifigan_conv1d")
    return out


def hifigan_tconv1d(x, w_op, bias, k, u, cout, slope=0.0, out=None, vlens=None, vmul=1):
    """out (B, u T, C_out) = conv_transpose1d(leaky_relu(x, slope), stride u, padding (k - u) / 2) + bias; x (B, T, C_in)."""
    _need_cuda(x, w_op, bias, out, vlens)
    B, T, cin = x.shape
    _check_act(x, B, T, cin, "hifigan_tconv1d x")
    ntaps = (k + u - 1) // u
    if w_op.dtype != x.dtype or w_op.numel() != u * cout * ntaps * cin_padded(cin):
        raise ValueError("hifigan_tconv1d: operand does not match (u C_out, ceil(k / u), C_in padded) in the activation dtype")
    out = _out_act("hifigan_tconv1d", out, x, B, u * T, cout)
    _lib.check(_lib.lib().s2svc_hifigan_tconv1d(dt(x), B, T, cin, cout, k, u, ptr(x), ptr(w_op), ptr(bias), float(slope), ptr(out),
                                                ptr(vlens), int(vmul), stream()), "hifigan_tconv1d")
    return out


def hifigan_conv_out(x, w, bias, k, slope=0.0, tanh=True, want_pre=False, vlens=None, vmul=1):
    """y (B, T) fp32 = tanh(conv1d(leaky_relu(x, slope), C -> 1) + bias) (+ the value before tanh); w fp32 [k][C]."""
    _need_cuda(x, w, bias, vlens)
    B, T, C = x.shape
    _check_act(x, B, T, C, "hifigan_conv_out x")
    if w.dtype != torch.float32 or w.numel() != k * C:
        raise ValueError("hifigan_conv_out: w is fp32 [k][C]")
    y = torch.empty(B, T, dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if want_pre else None
    _lib.check(_lib.lib().s2svc_hifigan_conv_out(dt(x), B, T, C, k, ptr(x), ptr(w), ptr(bias), float(slope), int(tanh), ptr(y), ptr(pre),
                                                 ptr(vlens), int(vmul), stream()), "hifigan_conv_out")
    return y, pre


def hifigan_input(x, B, T, C, strides, out_dtype, a=None, b=None, vlens=None):
    """out (B, T, C) in out_dtype = a[c] * x[b, t, c] + b[c]; `strides` = element strides of x for (b, t, c)."""
    _need_cuda(x, a, b, vlens)
    out = torch.empty(B, T, C, dtype=out_dtype, device=x.device)
    _lib.check(_lib.lib().s2svc_hifigan_input(dt(x), dt(out_dtype), B, T, C, ptr(x), int(strides[0]), int(strides[1]), int(strides[2]),
                                              ptr(a), ptr(b), ptr(out), ptr(vlens), stream()), "hifigan_input")
    return out


def hifigan_fold(mode, v, g, op_dtype, u=1, want_w32=True, want_op=True):
    """Weight-norm fold: v (D0, D1, k) fp32, g (D0, 1, 1) or None -> (w fp32 in v's layout, operand of the kernels).
    mode 0: Conv1d, 1: ConvTranspose1d (stride u), 2: the output convolution (operand fp32).  want_w32 / want_op: which of the two to produce."""
    _need_cuda(v, g)
    if v.dtype != torch.float32 or v.dim() != 3 or not v.is_contiguous() or (g is not None and (g.dtype != torch.float32 or g.numel() != v.shape[0])):
        raise ValueError("hifigan_fold: v fp32 contiguous (D0, D1, k), g fp32 with D0 values")
    D0, D1, k = v.shape
    if mode == 0:
        shape = (D0, k * cin_padded(D1))
    elif mode == 1:
        shape = (u * D1, (k + u - 1) // u * cin_padded(D0))
    else:
        shape, op_dtype = (k, D1), torch.float32
    op = zeros(shape, op_dtype, v.device) if want_op else None
    w32 = torch.empty_like(v) if want_w32 else None
    _lib.check(_lib.lib().s2svc_hifigan_fold(mode, D0, D1, k, u, ptr(None if g is None else g.contiguous()), ptr(v), ptr(w32), dt(op_dtype),
                                             ptr(op), stream()), "hifigan_fold")
    return w32, op


# ---------------------------------------------------------------------------------------------------------------------------
# backward with respect to the parameters (csrc/hifigan_bwd.hip)
# ---------------------------------------------------------------------------------------------------------------------------
WGRAD_STEP = 32              # frames per reduction step of the weight-gradient kernel: chunk edges are multiples of it
OUT_BWD_CHUNK = 256          # frames per partial of hifigan_conv_out_bwd


def wgrad_rows(kind, T, k, u=1):
    """Rows per utterance of the weight-gradient reduction: T (Conv1d) or the transposed convolution's GEMM rows T + ceil(pad / u)."""
    return T if kind == 0 else T + -(-((k - u) // 2) // u)


def wgrad_plan(B, rows, chunk=None):
    """The chunks of the weight-gradient reduction, in the order the finish launch sums them: [(utterance, first row, end row)].
    They depend on the shapes only.  Every utterance is cut on its own (no chunk spans two utterances): 128 rows per chunk up
    to 1024 rows, 512 above (the partials of a long stage stay a small fraction of its activations)."""
    if B < 1 or rows < 1:
        raise ValueError("wgrad_plan: B, rows >= 1")
    if chunk is None:
        chunk = 128 if rows <= 1024 else 512
    if chunk < WGRAD_STEP or chunk % WGRAD_STEP:
        raise ValueError("wgrad_plan: chunk is a positive multiple of 32 rows")
    return [(b, r, min(r + chunk, rows)) for b in range(B) for r in range(0, rows, chunk)]


def _plan_chunk(plan):
    return plan[0][2] - plan[0][1] if len(plan) > 1 and plan[1][0] == plan[0][0] else -(-plan[0][2] // WGRAD_STEP) * WGRAD_STEP


def hifigan_fold_bwd(mode, w32, op_dtype, u=1):
    """Operand of the data gradient from the folded fp32 weight (hifigan_fold's first result): mode 0 Conv1d (O, C, k) ->
    [C][k * O padded], taps flipped, (o, c) transposed; mode 1 ConvTranspose1d (C, O, k) -> [C][ceil(k / u) * (u O) padded]."""
    _need_cuda(w32)
    if mode not in (0, 1) or w32.dtype != torch.float32 or w32.dim() != 3 or not w32.is_contiguous():
        raise ValueError("hifigan_fold_bwd: mode 0 / 1, w32 fp32 contiguous (D0, D1, k)")
    D0, D1, k = w32.shape
    if mode == 1 and k < u:
        raise ValueError("hifigan_fold_bwd: ConvTranspose1d k >= u")
    shape = (D1, k * cin_padded(D0)) if mode == 0 else (D0, (k + u - 1) // u * cin_padded(u * D1))
    op = zeros(shape, op_dtype, w32.device)
    _lib.check(_lib.lib().s2svc_hifigan_fold_bwd(mode, D0, D1, k, u, ptr(w32), dt(op_dtype), ptr(op), stream()), "hifigan_fold_bwd")
    return op


def _check_same(name, t, like):
    if t is not None and (tuple(t.shape) != tuple(like.shape) or t.dtype != like.dtype or not t.is_contiguous()):
        raise ValueError(f"{name}: contiguous {tuple(like.shape)} in {like.dtype} expected")


def hifigan_conv1d_dgrad(dy, w_opT, k, dil, cin, mask_src=None, slope=0.0, res=None, accumulate=False, scale=1.0, out=None):
    """dx (B, T, C_in) = (accumulate ? out : 0) + scale * (lrelu'(mask_src, slope) * conv(dy, w flipped / transposed) (+ res))."""
    _need_cuda(dy, w_opT, mask_src, res, out)
    B, T, cout = dy.shape
    _check_act(dy, B, T, cout, "hifigan_conv1d_dgrad dy")
    if w_opT.dtype != dy.dtype or w_opT.numel() != cin * k * cin_padded(cout) or not w_opT.is_contiguous():
        raise ValueError("hifigan_conv1d_dgrad: operand does not match (C_in, k, C_out padded) in the gradient's dtype")
    out = _out_act("hifigan_conv1d_dgrad", out, dy, B, T, cin, accumulate)
    _check_same("hifigan_conv1d_dgrad mask_src", mask_src, out)
    _check_same("hifigan_conv1d_dgrad res", res, out)
    _lib.check(_lib.lib().s2svc_hifigan_conv1d_dgrad(dt(dy), B, T, cin, cout, k, dil, ptr(dy), ptr(w_opT), ptr(mask_src), float(slope),
                                                     ptr(res), int(accumulate), float(scale), ptr(out), stream()), "hifigan_conv1d_dgrad")
    return out


def hifigan_tconv1d_dgrad(dy, w_opT, k, u, cin, mask_src=None, slope=0.0, scale=1.0, out=None):
    """dx (B, T, C_in) of the transposed convolution from dy (B, u T, C_out): scale * lrelu'(mask_src, slope) * (the forward's GEMM, transposed)."""
    _need_cuda(dy, w_opT, mask_src)
    B, Tu, cout = dy.shape
    _check_act(dy, B, Tu, cout, "hifigan_tconv1d_dgrad dy")
    if u < 1 or Tu % u or k < u or (k - u) % 2:
        raise ValueError("hifigan_tconv1d_dgrad: dy has u * T frames; k >= u, (k - u) even")
    T = Tu // u
    if w_opT.dtype != dy.dtype or w_opT.numel() != cin * ((k + u - 1) // u) * cin_padded(u * cout) or not w_opT.is_contiguous():
        raise ValueError("hifigan_tconv1d_dgrad: operand does not match (C_in, ceil(k / u), u C_out padded) in the gradient's dtype")
    _need_cuda(out)
    out = _out_act("hifigan_tconv1d_dgrad", out, dy, B, T, cin)
    _check_same("hifigan_tconv1d_dgrad mask_src", mask_src, out)
    _lib.check(_lib.lib().s2svc_hifigan_tconv1d_dgrad(dt(dy), B, T, cin, cout, k, u, ptr(dy), ptr(w_opT), ptr(mask_src), float(slope),
                                                      float(scale), ptr(out), stream()), "hifigan_tconv1d_dgrad")
    return out


def hifigan_wgrad(kind, dy, x, k, dil_or_u, slope=0.0, plan=None, wpart=None, bpart=None):
    """Partials of the weight and bias gradients of one layer over the chunks of `plan` (wgrad_plan of the layer's rows).
    kind 0: Conv1d, dy (B, T, C_out), x (B, T, C_in), dil_or_u = dilation -> wpart (chunks, C_out, k, C_in), bpart (chunks, C_out);
    kind 1: ConvTranspose1d, dy (B, u T, C_out), dil_or_u = u -> wpart (chunks, u C_out, ceil(k / u), C_in), bpart (chunks, u C_out)."""
    _need_cuda(dy, x, wpart, bpart)
    B, T, cin = x.shape
    _check_act(x, B, T, cin, "hifigan_wgrad x")
    u = dil_or_u if kind == 1 else 1
    if kind not in (0, 1) or dy.dim() != 3 or dy.dtype != x.dtype or (kind == 1 and (k < u or (k - u) % 2)):
        raise ValueError("hifigan_wgrad: kind 0 / 1, dy (B, T', C_out) in x's dtype; ConvTranspose1d k >= u, (k - u) even")
    cout = dy.shape[2]
    _check_act(dy, B, T * u, cout, "hifigan_wgrad dy")
    rows = wgrad_rows(kind, T, k, u)
    plan = wgrad_plan(B, rows) if plan is None else plan
    chunk = _plan_chunk(plan)
    if plan != wgrad_plan(B, rows, chunk):
        raise ValueError("hifigan_wgrad: plan is not wgrad_plan(B, rows, chunk) of this layer")
    na, ntaps = (cout, k) if kind == 0 else (u * cout, (k + u - 1) // u)
    if wpart is None:
        wpart = torch.empty(len(plan), na, ntaps, cin, dtype=torch.float32, device=x.device)
    if bpart is None:
        bpart = torch.empty(len(plan), na, dtype=torch.float32, device=x.device)
    if (tuple(wpart.shape) != (len(plan), na, ntaps, cin) or tuple(bpart.shape) != (len(plan), na) or wpart.dtype != torch.float32
            or bpart.dtype != torch.float32 or not wpart.is_contiguous() or not bpart.is_contiguous()):
        raise ValueError("hifigan_wgrad: wpart (chunks, Na, taps, C_in) / bpart (chunks, Na) fp32 contiguous")
    _lib.check(_lib.lib().s2svc_hifigan_wgrad(dt(x), kind, B, T, cin, cout, k, dil_or_u, chunk, ptr(dy), ptr(x), float(slope), ptr(wpart),
                                              ptr(bpart), stream()), "hifigan_wgrad")
    return wpart, bpart


def hifigan_wgrad_finish(mode, wpart, bpart, v, g=None, u=1, want_bias=True, out=None):
    """Partials -> (grad_weight or grad_v in v's shape, grad_g or None, grad_bias): the sum in ascending chunk order, the
    parameter's layout, and with g the weight-norm backward.  Modes as hifigan_fold; v (D0, D1, k) fp32 is the live parameter."""
    _need_cuda(wpart, bpart, v, g)
    if v.dtype != torch.float32 or v.dim() != 3 or not v.is_contiguous() or (g is not None and (g.dtype != torch.float32 or g.numel() != v.shape[0])):
        raise ValueError("hifigan_wgrad_finish: v fp32 contiguous (D0, D1, k), g fp32 with D0 values")
    D0, D1, k = v.shape
    nparts = wpart.shape[0]
    if mode == 0:
        shape, bshape, nbias = (nparts, D0, k, D1), (nparts, D0), D0
    elif mode == 1:
        if k < u:
            raise ValueError("hifigan_wgrad_finish: ConvTranspose1d k >= u")
        shape, bshape, nbias = (nparts, u * D1, (k + u - 1) // u, D0), (nparts, u * D1), D1
    elif mode == 2 and D0 == 1:
        shape, bshape, nbias = (nparts, k, D1), (nparts,), 1
    else:
        raise ValueError("hifigan_wgrad_finish: mode 0 / 1 / 2 (one output channel)")
    if (tuple(wpart.shape) != shape or tuple(bpart.shape) != bshape or wpart.dtype != torch.float32 or bpart.dtype != torch.float32
            or not wpart.is_contiguous() or not bpart.is_contiguous() or nparts < 1):
        raise ValueError(f"hifigan_wgrad_finish: partials {shape} / {bshape} fp32 contiguous expected")
    gw = torch.empty_like(v)
    gg = None if g is None else torch.empty(D0, 1, 1, dtype=torch.float32, device=v.device)
    gb = torch.empty(nbias, dtype=torch.float32, device=v.device) if want_bias else None
    if out is not None:                                   # caller-provided (grad_w, grad_g, grad_bias) of exactly these shapes
        for mine, theirs in zip((gw, gg, gb), out):
            if (mine is None) != (theirs is None) or (mine is not None and (tuple(theirs.shape) != tuple(mine.shape) or theirs.dtype != torch.float32
                                                                             or not theirs.is_contiguous() or not theirs.is_cuda)):
                raise ValueError("hifigan_wgrad_finish: out = (grad_w, grad_g, grad_bias) fp32 contiguous in the parameters' shapes")
        gw, gg, gb = out
    _lib.check(_lib.lib().s2svc_hifigan_wgrad_finish(mode, D0, D1, k, u, nparts, ptr(wpart), ptr(bpart), ptr(None if g is None else g.contiguous()),
                                                     ptr(v), ptr(gw), ptr(gg), ptr(gb), stream()), "hifigan_wgrad_finish")
    return gw, gg, gb


def hifigan_conv_out_bwd(x, w, y, dy, k, slope=0.0, scale=1.0, out=None):
    """Backward of hifigan_conv_out (with tanh): x (B, T, C), w fp32 [k][C], y / dy (B, T) fp32 -> (dx (B, T, C) in x's dtype =
    scale * lrelu'(x) * data gradient, wpart (chunks, k, C), bpart (chunks)), chunks = B * ceil(T / OUT_BWD_CHUNK)."""
    _need_cuda(x, w, y, dy)
    B, T, C = x.shape
    _check_act(x, B, T, C, "hifigan_conv_out_bwd x")
    if w.dtype != torch.float32 or w.numel() != k * C or not w.is_contiguous():
        raise ValueError("hifigan_conv_out_bwd: w is fp32 [k][C]")
    for name, t in (("y", y), ("dy", dy)):
        if t.dtype != torch.float32 or t.numel() != B * T or not t.is_contiguous():
            raise ValueError(f"hifigan_conv_out_bwd: {name} is fp32 contiguous with B * T values")
    nch = B * (-(-T // OUT_BWD_CHUNK))
    dx = torch.empty_like(x)
    wpart = torch.empty(nch, k, C, dtype=torch.float32, device=x.device)
    bpart = torch.empty(nch, dtype=torch.float32, device=x.device)
    if out is not None:                                   # caller-provided (dx, wpart, bpart) of exactly these shapes
        for mine, theirs in zip((dx, wpart, bpart), out):
            if tuple(theirs.shape) != tuple(mine.shape) or theirs.dtype != mine.dtype or not theirs.is_contiguous() or not theirs.is_cuda:
                raise ValueError("hifigan_conv_out_bwd: out = (dx like x, wpart (chunks, k, C), bpart (chunks)) contiguous")
        dx, wpart, bpart = out
    _lib.check(_lib.lib().s2svc_hifigan_conv_out_bwd(dt(x), B, T, C, k, OUT_BWD_CHUNK, ptr(x), ptr(w), ptr(y), ptr(dy), float(slope), float(scale),
                                                     ptr(dx), ptr(wpart), ptr(bpart), stream()), "hifigan_conv_out_bwd")
    return dx, wpart, bpart
