"""Yardstick of the HiFi-GAN generator's backward pass: torch autograd over tests/vocoder_ref.generator_forward in float64, float64
restatements of the single-layer formulas the kernels implement (csrc/hifigan_bwd.hip), the view / operand functions of the
transposed convolution's backward, and a table of PLANTS -- the generator with one deliberate error in its backward -- that shows
the tests' bars can see each of them.  Test infrastructure: the product never imports it."""
import torch
import torch.nn.functional as F

import vocoder_ref as VR

LRELU_SLOPE = VR.LRELU_SLOPE
POST_SLOPE = 0.01
GRAD_SEED = 1021             # tools/gen_golden_vocoder_grads.py: the first seed >= 1000 whose leaky-relu inputs keep a margin from zero
R_SEED = 4242


def grad_input():
    """The committed model-level input: x (2, 80, 5) for TINY_CFG, rounded to fp32 (chosen by the tool, see `margin`)."""
    return torch.randn(2, 80, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(GRAD_SEED)).float()


def loss_weights(shape):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(R_SEED)).float()


def loss_fn(y, r):
    """mean(y * r) + 1/2 mean(y^2)"""
    return (y * r.to(y.dtype)).mean() + 0.5 * (y * y).mean()


# ---------------------------------------------------------------------------------------------------------------------------
# the generator with every leaky-relu input exposed, and with plants
# ---------------------------------------------------------------------------------------------------------------------------
def lrelu_grad(x, slope):
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, slope))


def conv1d_backward(x, w, dy, dil, slope, flip=True, transpose=True, mask="before", neighbour_halo=False, y=None):
    """Float64 restatement of the three formulas of one convolution y = conv(lrelu(x, s), w) + b, channel-first x (B, C, T),
    w (O, C, k), dy (B, O, T) -> (dx, dw, db).  The keyword arguments plant errors (defaults: none)."""
    B, C, T = x.shape
    O, _, k = w.shape
    half = (k - 1) // 2
    a = F.leaky_relu(x, slope) if slope else x
    db = dy.sum((0, 2))
    P = half * dil
    if neighbour_halo:                       # the halo of an utterance read from its neighbours in the batch
        flat = a.transpose(0, 1).reshape(C, B * T)
        ap = F.pad(flat, (P, P)).unsqueeze(0)
        ap = torch.stack([ap[0, :, b * T:b * T + T + 2 * P] for b in range(B)])
    else:
        ap = F.pad(a, (P, P))
    dw = torch.stack([torch.einsum("bot,bct->oc", dy, ap[:, :, j * dil:j * dil + T]) for j in range(k)], dim=2)
    wd = w.flip(2) if flip else w
    wd = wd.transpose(0, 1) if transpose else wd         # (C, O, k): a convolution from O channels to C
    dx = F.conv1d(dy, wd, None, dilation=dil, padding=P)
    if mask == "before":
        dx = dx * lrelu_grad(x, slope)
    elif mask == "after":                    # the mask taken from the layer's OUTPUT side tensor instead of its input
        dx = dx * lrelu_grad(y, slope)
    return dx, dw, db


def weight_norm_backward(v, g, dw, v_term=True):
    """w = g v / ||v|| (norm over all dims but 0): (dg, dv) from dw."""
    n = v.flatten(1).norm(dim=1).view(-1, 1, 1)
    dot = (dw * v).flatten(1).sum(1).view(-1, 1, 1)
    dv = (g / n) * dw
    if v_term:
        dv = dv - (g * dot / n ** 3) * v
    return dot / n, dv


class _Conv(torch.autograd.Function):
    """conv(lrelu(x, slope), w) + b whose backward is conv1d_backward with the given plant."""

    @staticmethod
    def forward(ctx, x, w, b, dil, slope, plant):
        k = w.shape[2]
        y = F.conv1d(F.leaky_relu(x, slope) if slope else x, w, b, dilation=dil, padding=(k - 1) // 2 * dil)
        ctx.save_for_backward(x, w, y)
        ctx.cfg = (dil, slope, plant)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dil, slope, plant = ctx.cfg
        kw = {}
        if plant == "taps not flipped":
            kw["flip"] = False
        elif plant == "(o, c) not transposed" and w.shape[0] == w.shape[1]:
            kw["transpose"] = False
        elif plant == "mask dropped":
            kw["mask"] = None
        elif plant == "mask after the activation" and w.shape[0] == w.shape[1]:
            kw.update(mask="after", y=y)
        elif plant == "halo from the neighbouring utterance":
            kw["neighbour_halo"] = True
        dx, dw, db = conv1d_backward(x, w, dy, dil, slope, **kw)
        return dx, dw, db, None, None, None


class _Scale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s, planted):
        ctx.s = 1.0 if planted else s
        return x * s

    @staticmethod
    def backward(ctx, dy):
        return dy * ctx.s, None, None


class _Tanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, planted):
        y = torch.tanh(x)
        ctx.save_for_backward(y)
        ctx.planted = planted
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return (dy if ctx.planted else dy * (1 - y * y)), None


class _WeightNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, g, planted):
        ctx.save_for_backward(v, g)
        ctx.planted = planted
        return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))

    @staticmethod
    def backward(ctx, dw):
        v, g = ctx.saved_tensors
        dg, dv = weight_norm_backward(v, g, dw, v_term=not ctx.planted)
        return dv, dg, None


PLANTS = ("taps not flipped", "(o, c) not transposed", "mask dropped", "mask after the activation", "1/nk missing",
          "halo from the neighbouring utterance", "v term of the weight-norm backward missing", "tanh derivative missing")


def generator_forward_explicit(sd, cfg, x, lrelu_inputs=None, plant=None):
    """tests/vocoder_ref.generator_forward with every Conv1d, the MRF scale, tanh and the weight norm as explicit autograd
    Functions over the formulas above (`plant`: one of PLANTS, or None for the correct backward).  lrelu_inputs (list) receives
    every tensor that passes through a leaky_relu.  The transposed convolutions stay F.conv_transpose1d."""
    cfg = VR.full_cfg(cfg)
    nk = len(cfg["resblock_kernel_sizes"])

    def weight(name):
        if name + ".weight" in sd:
            return sd[name + ".weight"]
        return _WeightNorm.apply(sd[name + ".weight_v"], sd[name + ".weight_g"], plant == "v term of the weight-norm backward missing")

    def seen(v):
        if lrelu_inputs is not None:
            lrelu_inputs.append(v)
        return v

    def conv(name, v, dil, slope):
        if slope:
            seen(v)
        return _Conv.apply(v, weight(name), sd[name + ".bias"], dil, slope, plant)

    out = conv("conv_pre", x, 1, 0.0)
    for i, (u, k) in enumerate(zip(cfg["upsample_factors"], cfg["upsample_kernel_sizes"])):
        out = F.conv_transpose1d(F.leaky_relu(seen(out), LRELU_SLOPE), weight(f"ups.{i}"), sd[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        z_sum = None
        for j, (rk, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            rb = f"resblocks.{i * nk + j}"
            xr = out
            for q, d in enumerate(dils):
                xt = conv(f"{rb}.convs1.{q}", xr, d, LRELU_SLOPE)
                xt = conv(f"{rb}.convs2.{q}", xt, 1, LRELU_SLOPE)
                xr = xt + xr
            z_sum = xr if z_sum is None else z_sum + xr
        out = _Scale.apply(z_sum, 1.0 / nk, plant == "1/nk missing")
    out = conv("conv_post", out, 1, POST_SLOPE)
    return _Tanh.apply(out, plant == "tanh derivative missing")


def generator_grads(sd, cfg, x, r=None, dtype=torch.float64, forward=VR.generator_forward, autocast=False, **kw):
    """(y, loss, {parameter: gradient}) of loss_fn over `forward` with torch autograd on the CPU, the state dict's entries as leaves."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xin = x.to(dtype)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y = forward(leaves, cfg, xin, **kw).float()
    else:
        y = forward(leaves, cfg, xin, **kw)
    r = loss_weights(y.shape) if r is None else r
    loss = loss_fn(y, r)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return y.detach(), loss.detach(), dict(zip(leaves, grads))


def margin(sd, cfg, x):
    """(m, e, count): m = the smallest |v| / rms(tensor) over every leaky-relu input of the float64 run; e = the largest
    |v32 - v64| / rms(tensor) of stock torch's fp32 run at the same tensors.  A mask can only flip where |v| is within the forward
    error of zero: the model-level input is chosen with m >= 4 e."""
    t64, t32 = [], []
    with torch.no_grad():
        generator_forward_explicit({k: v.double() for k, v in sd.items()}, cfg, x.double(), lrelu_inputs=t64)
        generator_forward_explicit({k: v.float() for k, v in sd.items()}, cfg, x.float(), lrelu_inputs=t32)
    m = min(float(a.abs().min() / a.pow(2).mean().sqrt()) for a in t64)
    e = max(float((b.double() - a).abs().max() / a.pow(2).mean().sqrt()) for a, b in zip(t64, t32))
    return m, e, sum(a.numel() for a in t64)


# ---------------------------------------------------------------------------------------------------------------------------
# the transposed convolution's backward in the forward's own GEMM view
# ---------------------------------------------------------------------------------------------------------------------------
def tconv_geometry(k, u):
    pad = (k - u) // 2
    return pad, -(-k // u), -(-pad // u)             # (pad, taps per phase, extra rows)


def tconv_dy_view(dy, k, u, rows):
    """dy (B, u T, C_out) channel-last -> (B, rows, u * C_out): element (i, p * C_out + o) is dy[u i + p - pad, o], i.e. the flat
    tensor read at an offset of -pad * C_out elements; zero outside the utterance."""
    B, Tu, C = dy.shape
    pad = (k - u) // 2
    flat = dy.reshape(B, Tu * C)
    need = rows * u * C
    flat = F.pad(flat, (pad * C, max(0, need - pad * C - Tu * C)))[:, :need]
    return flat.reshape(B, rows, u * C)


def tconv_operand(w, u):
    """w (C_in, C_out, k) -> op (u * C_out, ntaps, C_in): op[p * C_out + o][n][c] = w[c, o, p + u n] (zero where p + u n >= k)."""
    cin, cout, k = w.shape
    ntaps = -(-k // u)
    op = w.new_zeros(u, cout, ntaps, cin)
    for p in range(u):
        for n in range(ntaps):
            if p + u * n < k:
                op[p, :, n, :] = w[:, :, p + u * n].t()
    return op.reshape(u * cout, ntaps, cin)


def tconv_backward(x, w, dy, u, slope):
    """Channel-last x (B, T, C_in), w (C_in, C_out, k), dy (B, u T, C_out) -> (dx, dw, db) through the view:
    dx[i, c] = lrelu'(x) * sum_n sum_(p,o) dy'[i + n, (p,o)] op[(p,o)][n][c];  dop[(p,o)][n][c] = sum_i dy'[i, (p,o)] a[i - n, c]."""
    B, T, cin = x.shape
    _, cout, k = w.shape
    pad, ntaps, extra = tconv_geometry(k, u)
    rows = T + extra
    dv = tconv_dy_view(dy, k, u, rows + ntaps)        # rows past `rows` are zero: they only make the slices below uniform
    op = tconv_operand(w, u)
    a = F.leaky_relu(x, slope) if slope else x
    dx = sum(torch.einsum("bim,mc->bic", dv[:, n:n + T], op[:, n]) for n in range(ntaps))
    if slope:
        dx = dx * lrelu_grad(x, slope)
    ap = F.pad(a, (0, 0, ntaps - 1, rows - T))        # frames -(ntaps-1) .. rows-1
    dop = torch.stack([torch.einsum("bim,bic->mc", dv[:, :rows], ap[:, ntaps - 1 - n:ntaps - 1 - n + rows]) for n in range(ntaps)], dim=1)
    dop = dop.reshape(u, cout, ntaps, cin)
    dw = torch.zeros_like(w)
    for p in range(u):
        for n in range(ntaps):
            if p + u * n < k:                          # the zero-filled slots p + u n >= k are dropped
                dw[:, :, p + u * n] = dop[p, :, n].t()
    return dx, dw, dy.sum((0, 1))
