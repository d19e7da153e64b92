"""Launchers of the HiFi-GAN multi-period discriminator kernels (csrc/hifigan_disc.hip; C ABI in include/s2svc_hip.h).
Non-differentiable, GPU tensors only, fp32.  Activations are channel-last (B, L, p, C) and hold the post-activation values; the weight
norm fold, the data-gradient operand and the finish of the weight gradients are the generator's launchers (kernels_vocoder.py:
hifigan_fold mode 0 / 2, hifigan_fold_bwd mode 0, hifigan_wgrad_finish mode 0 / 2)."""
import torch

from .. import _lib
from .kernels import _need_cuda, ptr, stream
from .kernels_vocoder import cin_padded

TAPS, STRIDE, POST_TAPS = 5, 3, 3          # kernel size and stride along L of convs[0..3] (convs[4]: stride 1); conv_post's kernel size
C_FIRST = 32                               # output channels of the input layer
CHUNK = 256                                # rows (b, l, w) per partial of every weight-gradient launch


def folded_len(T, p):
    """(L0, pad): rows of the (L0, p) view of T samples and the reflect padding that completes the last row."""
    if p < 1 or T < p:
        raise ValueError(f"period {p} needs at least {p} samples (reflect padding of up to p - 1), got {T}")
    pad = (p - T % p) % p
    return (T + pad) // p, pad


def out_len(L, stride):
    """Rows along L after Conv2d((5, 1), (stride, 1), padding (2, 0))."""
    return (L - 1) // stride + 1


def reflect_index(t, T):
    """Sample of x that the padded position t >= 0 holds (F.pad(x, (0, n), "reflect"))."""
    return t if t < T else 2 * (T - 1) - t


def chunks(rows):
    return -(-rows // CHUNK)


def check_f32(name, t, shape=None):
    if t.dtype != torch.float32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name}: contiguous fp32 {'' if shape is None else tuple(shape)} expected, got {t.dtype} {tuple(t.shape)}")
    return t


def check_flat(name, t, n):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{name}: contiguous fp32 with {n} values expected, got {t.dtype} {tuple(t.shape)}")
    return t


def out_or_empty(name, out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    _need_cuda(out)
    return check_f32(name + " out", out, shape)


def disc_input(x, w32, bias, p, slope=0.1, out=None):
    """x (B, T) -> (B, L1, p, 32) = leaky_relu(conv(reflect-padded x viewed (L0, p), k 5, stride 3) + bias); w32 (32, 1, 5) folded."""
    _need_cuda(x, w32, bias)
    B, T = check_f32("disc_input x", x).shape
    L0, _ = folded_len(T, p)
    check_flat("disc_input w32", w32, C_FIRST * TAPS)
    check_f32("disc_input bias", bias, (C_FIRST,))
    out = out_or_empty("disc_input", out, (B, out_len(L0, STRIDE), p, C_FIRST), x)
    _lib.check(_lib.lib().s2svc_hifigan_disc_input(B, T, p, ptr(x), ptr(w32), ptr(bias), float(slope), ptr(out), stream()), "hifigan_disc_input")
    return out


def disc_conv(x, w_op, bias, cout, stride, slope=0.1, out=None):
    """x (B, L, p, C_in) -> (B, (L - 1) // stride + 1, p, C_out) = leaky_relu(conv k 5 + bias); w_op [C_out][5 * C_in padded]."""
    _need_cuda(x, w_op, bias)
    if x.dim() != 4:
        raise ValueError("disc_conv: x (B, L, p, C_in)")
    B, L, p, cin = check_f32("disc_conv x", x).shape
    check_flat("disc_conv w_op", w_op, cout * TAPS * cin_padded(cin))
    check_f32("disc_conv bias", bias, (cout,))
    out = out_or_empty("disc_conv", out, (B, out_len(L, stride), p, cout), x)
    _lib.check(_lib.lib().s2svc_hifigan_disc_conv(B, L, p, cin, cout, stride, ptr(x), ptr(w_op), ptr(bias), float(slope), ptr(out), stream()),
               "hifigan_disc_conv")
    return out


def disc_post(x, w, bias, out=None):
    """x (B, L, p, C) -> y (B, L * p), conv_post C -> 1 (k 3, padding 1, no activation); w fp32 [3][C]."""
    _need_cuda(x, w, bias)
    if x.dim() != 4:
        raise ValueError("disc_post: x (B, L, p, C)")
    B, L, p, C = check_f32("disc_post x", x).shape
    check_flat("disc_post w", w, POST_TAPS * C)
    check_f32("disc_post bias", bias, (1,))
    y = out_or_empty("disc_post", out, (B, L * p), x)
    _lib.check(_lib.lib().s2svc_hifigan_disc_post(B, L, p, C, ptr(x), ptr(w), ptr(bias), ptr(y), stream()), "hifigan_disc_post")
    return y


def disc_post_bwd(x, w, dy1=None, dy2=None, add=None, slope=0.1, out=None):
    """Backward of disc_post: d = dy1 + dy2 ((B, L * p) each or None) -> (dx (B, L, p, C) = leaky_relu'(x) * (add + data gradient),
    wpart (chunks, 3, C), bpart (chunks,)); add = the gradient of the feature x itself, or None."""
    _need_cuda(x, w, dy1, dy2, add)
    B, L, p, C = check_f32("disc_post_bwd x", x).shape
    check_flat("disc_post_bwd w", w, POST_TAPS * C)
    for name, t in (("dy1", dy1), ("dy2", dy2)):
        if t is not None:
            check_flat("disc_post_bwd " + name, t, B * L * p)
    if add is not None:
        check_f32("disc_post_bwd add", add, x.shape)
    nch = chunks(B * L * p)
    shapes = (tuple(x.shape), (nch, POST_TAPS, C), (nch,))
    outs = [out_or_empty("disc_post_bwd", None if out is None else out[i], shapes[i], x) for i in range(3)]
    _lib.check(_lib.lib().s2svc_hifigan_disc_post_bwd(B, L, p, C, ptr(x), ptr(w), ptr(dy1), ptr(dy2), ptr(add), float(slope), ptr(outs[0]),
                                                      ptr(outs[1]), ptr(outs[2]), stream()), "hifigan_disc_post_bwd")
    return tuple(outs)


def disc_wgrad(dy, x, stride, out=None):
    """Partials of the weight / bias gradients of disc_conv: dy (B, Lo, p, C_out) gradient of the pre-activation, x (B, L, p, C_in) ->
    (wpart (chunks, C_out, 5, C_in), bpart (chunks, C_out)), chunks of 256 rows of B * Lo * p in ascending order."""
    _need_cuda(dy, x)
    B, L, p, cin = check_f32("disc_wgrad x", x).shape
    cout = dy.shape[-1]
    Lo = out_len(L, stride)
    check_f32("disc_wgrad dy", dy, (B, Lo, p, cout))
    nch = chunks(B * Lo * p)
    shapes = ((nch, cout, TAPS, cin), (nch, cout))
    outs = [out_or_empty("disc_wgrad", None if out is None else out[i], shapes[i], x) for i in range(2)]
    _lib.check(_lib.lib().s2svc_hifigan_disc_wgrad(B, L, p, cin, cout, stride, ptr(dy), ptr(x), ptr(outs[0]), ptr(outs[1]), stream()),
               "hifigan_disc_wgrad")
    return tuple(outs)


def disc_dgrad(dy, w_opT, L, cin, stride, mask_src=None, add=None, slope=0.1, out=None):
    """dx (B, L, p, C_in) = leaky_relu'(mask_src) * (add + conv^T(dy)); dy (B, (L - 1) // stride + 1, p, C_out); w_opT =
    hifigan_fold_bwd mode 0 of the folded weight: [C_in][5 * C_out padded]."""
    _need_cuda(dy, w_opT, mask_src, add)
    if dy.dim() != 4:
        raise ValueError("disc_dgrad: dy (B, Lo, p, C_out)")
    B, Lo, p, cout = check_f32("disc_dgrad dy", dy).shape
    if Lo != out_len(L, stride):
        raise ValueError(f"disc_dgrad: dy has {Lo} rows along L, the convolution of {L} rows gives {out_len(L, stride)}")
    check_flat("disc_dgrad w_opT", w_opT, cin * TAPS * cin_padded(cout))
    for name, t in (("mask_src", mask_src), ("add", add)):
        if t is not None:
            check_f32("disc_dgrad " + name, t, (B, L, p, cin))
    dx = out_or_empty("disc_dgrad", out, (B, L, p, cin), dy)
    _lib.check(_lib.lib().s2svc_hifigan_disc_dgrad(B, L, p, cin, cout, stride, ptr(dy), ptr(w_opT), ptr(mask_src), ptr(add), float(slope),
                                                   ptr(dx), stream()), "hifigan_disc_dgrad")
    return dx


def disc_input_wgrad(dy, x, p, out=None):
    """Partials of the input layer: dy (B, L1, p, 32), x (B, T) -> (wpart (chunks, 32, 5, 1), bpart (chunks, 32))."""
    _need_cuda(dy, x)
    B, T = check_f32("disc_input_wgrad x", x).shape
    L1 = out_len(folded_len(T, p)[0], STRIDE)
    check_f32("disc_input_wgrad dy", dy, (B, L1, p, C_FIRST))
    nch = chunks(B * L1 * p)
    shapes = ((nch, C_FIRST, TAPS, 1), (nch, C_FIRST))
    outs = [out_or_empty("disc_input_wgrad", None if out is None else out[i], shapes[i], x) for i in range(2)]
    _lib.check(_lib.lib().s2svc_hifigan_disc_input_wgrad(B, T, p, ptr(dy), ptr(x), ptr(outs[0]), ptr(outs[1]), stream()),
               "hifigan_disc_input_wgrad")
    return tuple(outs)


def disc_input_dgrad(dy, w32, T, p, out=None):
    """dx (B, T) of the input layer from dy (B, L1, p, 32): own position plus the mirror image where the reflect pad copied the sample."""
    _need_cuda(dy, w32)
    L1 = out_len(folded_len(T, p)[0], STRIDE)
    if dy.dim() != 4:
        raise ValueError("disc_input_dgrad: dy (B, L1, p, 32)")
    B = dy.shape[0]
    check_f32("disc_input_dgrad dy", dy, (B, L1, p, C_FIRST))
    check_flat("disc_input_dgrad w32", w32, C_FIRST * TAPS)
    dx = out_or_empty("disc_input_dgrad", out, (B, T), dy)
    _lib.check(_lib.lib().s2svc_hifigan_disc_input_dgrad(B, T, p, ptr(dy), ptr(w32), ptr(dx), stream()), "hifigan_disc_input_dgrad")
    return dx
