"""Launchers of the HiFi-GAN multi-scale discriminator kernels (csrc/hifigan_msd.hip; C ABI in include/s2svc_hip.h).
Non-differentiable, GPU tensors only, fp32.  Activations are channel-last (B, L, C) and hold the post-activation values.  The forward
operand of a grouped convolution is the generator's hifigan_fold mode 0 of the weight (C_out, C_in / groups, 41); the finish of its
weight gradients is hifigan_wgrad_finish mode 0 (kernels_vocoder.py).  Layer 6 and conv_post are the multi-period discriminator's
launchers at p = 1 (kernels_disc.py)."""
import torch

from .. import _lib
from .kernels import _need_cuda, ptr, stream
from .kernels_disc import check_f32, check_flat, out_or_empty
from .kernels_vocoder import cin_padded

TAPS, PAD = 41, 20                         # kernel size and padding of the grouped convolutions convs[1..5]
IN_TAPS, IN_PAD, C_FIRST = 15, 7, 128      # the input layer convs[0]: 1 -> 128
IN_CHUNK = 256                             # rows (b, t) per partial of the input layer's weight gradient
SN_EPS = 1e-12


def pool_len(T):
    """Samples after AvgPool1d(4, 2, padding=2)."""
    return T // 2 + 1


def out_len(L, stride):
    """Rows after a convolution with padding (k - 1) // 2 and this stride."""
    return (L - 1) // stride + 1


def gconv_chunk(Lo):
    """Output rows per partial of msd_gconv_wgrad (every utterance is cut on its own): max(256, 32 * ceil(Lo / 256)), as the library states it."""
    return int(_lib.lib().s2svc_hifigan_msd_gconv_chunk(int(Lo)))


def gconv_chunks(B, Lo):
    return B * -(-Lo // gconv_chunk(Lo))


def msd_pool(x, out=None):
    """x (B, T) -> (B, T // 2 + 1): AvgPool1d(4, 2, padding=2), the padding counted."""
    _need_cuda(x)
    if x.dim() != 2:
        raise ValueError("msd_pool: x (B, T)")
    B, T = check_f32("msd_pool x", x).shape
    y = out_or_empty("msd_pool", out, (B, pool_len(T)), x)
    _lib.check(_lib.lib().s2svc_hifigan_msd_pool(B, T, ptr(x), ptr(y), stream()), "hifigan_msd_pool")
    return y


def msd_pool_bwd(dy, T, out=None):
    """dx (B, T) from dy (B, T // 2 + 1): the adjoint of msd_pool."""
    _need_cuda(dy)
    if dy.dim() != 2:
        raise ValueError("msd_pool_bwd: dy (B, T // 2 + 1)")
    B = dy.shape[0]
    check_f32("msd_pool_bwd dy", dy, (B, pool_len(T)))
    dx = out_or_empty("msd_pool_bwd", out, (B, T), dy)
    _lib.check(_lib.lib().s2svc_hifigan_msd_pool_bwd(B, T, ptr(dy), ptr(dx), stream()), "hifigan_msd_pool_bwd")
    return dx


def msd_input(x, w32, bias, slope=0.1, out=None):
    """x (B, T) -> (B, T, 128) = leaky_relu(conv k 15, padding 7 + bias); w32 (128, 1, 15)."""
    _need_cuda(x, w32, bias)
    if x.dim() != 2:
        raise ValueError("msd_input: x (B, T)")
    B, T = check_f32("msd_input x", x).shape
    check_flat("msd_input w32", w32, C_FIRST * IN_TAPS)
    check_f32("msd_input bias", bias, (C_FIRST,))
    out = out_or_empty("msd_input", out, (B, T, C_FIRST), x)
    _lib.check(_lib.lib().s2svc_hifigan_msd_input(B, T, ptr(x), ptr(w32), ptr(bias), float(slope), ptr(out), stream()), "hifigan_msd_input")
    return out


def msd_input_wgrad(dy, x, out=None):
    """Partials of the input layer: dy (B, T, 128), x (B, T) -> (wpart (chunks, 128, 15, 1), bpart (chunks, 128)), chunks of 256 rows."""
    _need_cuda(dy, x)
    B, T = check_f32("msd_input_wgrad x", x).shape
    check_f32("msd_input_wgrad dy", dy, (B, T, C_FIRST))
    nch = -(-B * T // IN_CHUNK)
    shapes = ((nch, C_FIRST, IN_TAPS, 1), (nch, C_FIRST))
    outs = [out_or_empty("msd_input_wgrad", None if out is None else out[i], shapes[i], x) for i in range(2)]
    _lib.check(_lib.lib().s2svc_hifigan_msd_input_wgrad(B, T, ptr(dy), ptr(x), ptr(outs[0]), ptr(outs[1]), stream()), "hifigan_msd_input_wgrad")
    return tuple(outs)


def msd_input_dgrad(dy, w32, out=None):
    """dx (B, T) of the input layer from dy (B, T, 128)."""
    _need_cuda(dy, w32)
    if dy.dim() != 3:
        raise ValueError("msd_input_dgrad: dy (B, T, 128)")
    B, T = dy.shape[:2]
    check_f32("msd_input_dgrad dy", dy, (B, T, C_FIRST))
    check_flat("msd_input_dgrad w32", w32, C_FIRST * IN_TAPS)
    dx = out_or_empty("msd_input_dgrad", out, (B, T), dy)
    _lib.check(_lib.lib().s2svc_hifigan_msd_input_dgrad(B, T, ptr(dy), ptr(w32), ptr(dx), stream()), "hifigan_msd_input_dgrad")
    return dx


def _gshape(name, cin, cout, groups, stride):
    if groups < 1 or cin % groups or cout % groups or stride not in (1, 2, 4):
        raise ValueError(f"{name}: channels divisible by the groups, stride 1, 2 or 4")
    cg, og = cin // groups, cout // groups
    if cg % 4 or og % 4 or cg > 64 or og > 64:
        raise ValueError(f"{name}: channels per group multiples of 4, at most 64 (got {cg} -> {og})")
    return cg, og


def msd_gconv(x, w_op, bias, cout, groups, stride, slope=0.1, out=None):
    """x (B, L, C_in) -> (B, (L - 1) // stride + 1, C_out) = leaky_relu(grouped conv k 41 + bias); w_op [C_out][41 * (C_in / groups padded)]."""
    _need_cuda(x, w_op, bias)
    if x.dim() != 3:
        raise ValueError("msd_gconv: x (B, L, C_in)")
    B, L, cin = check_f32("msd_gconv x", x).shape
    cg, _ = _gshape("msd_gconv", cin, cout, groups, stride)
    check_flat("msd_gconv w_op", w_op, cout * TAPS * cin_padded(cg))
    check_f32("msd_gconv bias", bias, (cout,))
    out = out_or_empty("msd_gconv", out, (B, out_len(L, stride), cout), x)
    _lib.check(_lib.lib().s2svc_hifigan_msd_gconv(B, L, cin, cout, groups, stride, ptr(x), ptr(w_op), ptr(bias), float(slope), ptr(out), stream()),
               "hifigan_msd_gconv")
    return out


def msd_fold_bwd(w32, groups, out=None):
    """Operand of msd_gconv_dgrad from the folded weight w32 (C_out, C_in / groups, 41): [C_in][41 * (C_out / groups padded)]."""
    _need_cuda(w32)
    if w32.dim() != 3 or w32.shape[2] != TAPS:
        raise ValueError("msd_fold_bwd: w32 (C_out, C_in / groups, 41)")
    cout, cg, _ = check_f32("msd_fold_bwd w32", w32).shape
    if groups < 1 or cout % groups:
        raise ValueError("msd_fold_bwd: C_out divisible by the groups")
    op = out_or_empty("msd_fold_bwd", out, (cg * groups, TAPS * cin_padded(cout // groups)), w32)
    _lib.check(_lib.lib().s2svc_hifigan_msd_fold_bwd(cg * groups, cout, groups, ptr(w32), ptr(op), stream()), "hifigan_msd_fold_bwd")
    return op


def msd_gconv_dgrad(dy, w_opT, L, cin, groups, stride, mask_src=None, add=None, slope=0.1, out=None):
    """dx (B, L, C_in) = leaky_relu'(mask_src) * (add + conv^T(dy)); dy (B, (L - 1) // stride + 1, C_out); w_opT = msd_fold_bwd."""
    _need_cuda(dy, w_opT, mask_src, add)
    if dy.dim() != 3:
        raise ValueError("msd_gconv_dgrad: dy (B, Lo, C_out)")
    B, Lo, cout = check_f32("msd_gconv_dgrad dy", dy).shape
    if Lo != out_len(L, stride):
        raise ValueError(f"msd_gconv_dgrad: dy has {Lo} rows, the convolution of {L} rows gives {out_len(L, stride)}")
    _, og = _gshape("msd_gconv_dgrad", cin, cout, groups, stride)
    check_flat("msd_gconv_dgrad w_opT", w_opT, cin * TAPS * cin_padded(og))
    for name, t in (("mask_src", mask_src), ("add", add)):
        if t is not None:
            check_f32("msd_gconv_dgrad " + name, t, (B, L, cin))
    dx = out_or_empty("msd_gconv_dgrad", out, (B, L, cin), dy)
    _lib.check(_lib.lib().s2svc_hifigan_msd_gconv_dgrad(B, L, cin, cout, groups, stride, ptr(dy), ptr(w_opT), ptr(mask_src), ptr(add), float(slope),
                                                        ptr(dx), stream()), "hifigan_msd_gconv_dgrad")
    return dx


def msd_gconv_wgrad(dy, x, groups, stride, out=None):
    """Partials of the weight / bias gradients of msd_gconv: dy (B, Lo, C_out) gradient of the pre-activation, x (B, L, C_in) ->
    (wpart (chunks, C_out, 41, C_in / groups), bpart (chunks, C_out)), chunks = B * ceil(Lo / gconv_chunk(Lo)) in (utterance, chunk) order."""
    _need_cuda(dy, x)
    if x.dim() != 3 or dy.dim() != 3:
        raise ValueError("msd_gconv_wgrad: dy (B, Lo, C_out), x (B, L, C_in)")
    B, L, cin = check_f32("msd_gconv_wgrad x", x).shape
    cout = dy.shape[-1]
    cg, _ = _gshape("msd_gconv_wgrad", cin, cout, groups, stride)
    Lo = out_len(L, stride)
    check_f32("msd_gconv_wgrad dy", dy, (B, Lo, cout))
    nch = gconv_chunks(B, Lo)
    shapes = ((nch, cout, TAPS, cg), (nch, cout))
    outs = [out_or_empty("msd_gconv_wgrad", None if out is None else out[i], shapes[i], x) for i in range(2)]
    _lib.check(_lib.lib().s2svc_hifigan_msd_gconv_wgrad(B, L, cin, cout, groups, stride, gconv_chunk(Lo), ptr(dy), ptr(x), ptr(outs[0]), ptr(outs[1]),
                                                        stream()), "hifigan_msd_gconv_wgrad")
    return tuple(outs)


def _sn_args(name, W, u, v):
    _need_cuda(W, u, v)
    if W.dim() < 2:
        raise ValueError(f"{name}: W (O, ...)")
    O = W.shape[0]
    K = W.numel() // O
    check_f32(name + " W", W)
    check_f32(name + " u", u, (O,))
    check_f32(name + " v", v, (K,))
    return O, K


def msd_sn_power(W, u, v, iterate, eps=SN_EPS, out=None):
    """One power iteration of spectral norm on W (O, ...) viewed (O, K): with `iterate`, v and u are updated IN PLACE; -> sigma (1,) on the
    device (= u . W v), no host read.  iterate False leaves u and v untouched."""
    O, K = _sn_args("msd_sn_power", W, u, v)
    sigma = out_or_empty("msd_sn_power", out, (1,), W)
    ws = torch.empty(O + K, dtype=torch.float64, device=W.device)
    _lib.check(_lib.lib().s2svc_hifigan_msd_sn_power(O, K, int(bool(iterate)), float(eps), ptr(W), ptr(u), ptr(v), ptr(sigma), ptr(ws), stream()),
               "hifigan_msd_sn_power")
    return sigma


def msd_sn_scale(W, sigma, out=None):
    """W / sigma in W's shape."""
    _need_cuda(W, sigma)
    check_f32("msd_sn_scale W", W)
    check_f32("msd_sn_scale sigma", sigma, (1,))
    w = out_or_empty("msd_sn_scale", out, tuple(W.shape), W)
    _lib.check(_lib.lib().s2svc_hifigan_msd_sn_scale(W.numel(), ptr(W), ptr(sigma), ptr(w), stream()), "hifigan_msd_sn_scale")
    return w


def msd_sn_finish(dW, W, u, v, sigma, out=None):
    """grad of weight_orig from dW = the gradient of W / sigma (u, v constants): dW / sigma - (sum(dW * W) / sigma^2) u v^T, in W's shape."""
    O, K = _sn_args("msd_sn_finish", W, u, v)
    _need_cuda(dW, sigma)
    check_f32("msd_sn_finish dW", dW, tuple(W.shape))
    check_f32("msd_sn_finish sigma", sigma, (1,))
    grad = out_or_empty("msd_sn_finish", out, tuple(W.shape), W)
    ws = torch.empty(O, dtype=torch.float64, device=W.device)
    _lib.check(_lib.lib().s2svc_hifigan_msd_sn_finish(O, K, ptr(dW), ptr(W), ptr(u), ptr(v), ptr(sigma), ptr(grad), ptr(ws), stream()),
               "hifigan_msd_sn_finish")
    return grad
