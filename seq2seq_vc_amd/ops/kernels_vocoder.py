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


def hifigan_conv1d(x, w_op, bias, k, dil, cout, slope=0.0, res=None, accumulate=False, scale=1.0, tanh=False, out=None, vlens=None,
                   vmul=1):
    """out = (accumulate ? out : 0) + scale * (conv1d(leaky_relu(x, slope)) + bias (+ res)), optional tanh; x (B, T, C_in)."""
    _need_cuda(x, w_op, bias, res, out, vlens)
    B, T, cin = x.shape
    _check_act(x, B, T, cin, "hifigan_conv1d x")
    if w_op.dtype != x.dtype or w_op.numel() != cout * k * cin_padded(cin):
        raise ValueError("hifigan_conv1d: operand does not match (C_out, k, C_in padded) in the activation dtype")
    if out is None:
        if accumulate:
            raise ValueError("hifigan_conv1d: accumulate needs out")
        out = torch.empty(B, T, cout, dtype=x.dtype, device=x.device)
    _check_act(out, B, T, cout, "hifigan_conv1d out")
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
    if out is None:
        out = torch.empty(B, u * T, cout, dtype=x.dtype, device=x.device)
    _check_act(out, B, u * T, cout, "hifigan_tconv1d out")
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
