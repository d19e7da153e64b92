"""Functional restatement of the HiFi-GAN generator over a state_dict (reference: seq2seq_vc/urhythmic/vocoder.py:87-106, 195-202)
with stock torch operators, any dtype.  It is the yardstick where the reference does not exist (the GPU tests) and is itself pinned
to tests/golden/hifigan_tiny.npz on the CPU (tests/test_vocoder_host.py).  Test infrastructure: the product never imports it."""
import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.1
TINY_CFG = dict(in_channels=80, upsample_channels=64, upsample_factors=(4, 4, 2, 2), upsample_kernel_sizes=(8, 8, 4, 4))
DEFAULT_CFG = dict(in_channels=256, resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), resblock_kernel_sizes=(3, 7, 11),
                   upsample_kernel_sizes=(20, 16, 4, 4), upsample_channels=512, upsample_factors=(10, 8, 2, 2), sample_rate=16000)


def full_cfg(cfg):
    out = dict(DEFAULT_CFG)
    out.update(cfg)
    return out


def weight(sd, name, dtype=None):
    """The convolution weight of layer `name` in either checkpoint form (torch._weight_norm over dim 0, as weight_norm does)."""
    if name + ".weight" in sd:
        w = sd[name + ".weight"]
    else:
        w = torch._weight_norm(sd[name + ".weight_v"], sd[name + ".weight_g"], 0)
    return w if dtype is None else w.to(dtype)


def generator_forward(sd, cfg, x, taps=None):
    """x (B, in_channels, N) -> (B, 1, N * prod(factors)); taps (dict) receives conv_pre, ups.i, stage.i, conv_post (before tanh),
    all channel-first as torch computes them.  Runs in x's dtype and on x's device (autocast applies if the caller enabled it)."""
    cfg = full_cfg(cfg)
    sd = {k: v.to(device=x.device, dtype=x.dtype) for k, v in sd.items()}
    nk = len(cfg["resblock_kernel_sizes"])

    def keep(name, v):
        if taps is not None:
            taps[name] = v
        return v

    out = keep("conv_pre", F.conv1d(x, weight(sd, "conv_pre"), sd["conv_pre.bias"], padding=2))
    for i, (u, k) in enumerate(zip(cfg["upsample_factors"], cfg["upsample_kernel_sizes"])):
        out = F.leaky_relu(out, LRELU_SLOPE)
        out = keep(f"ups.{i}", F.conv_transpose1d(out, weight(sd, f"ups.{i}"), sd[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2))
        z_sum = None
        for j, (rk, dils) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            rb = f"resblocks.{i * nk + j}"
            xr = out
            for q, d in enumerate(dils):
                xt = F.leaky_relu(xr, LRELU_SLOPE)
                xt = F.conv1d(xt, weight(sd, f"{rb}.convs1.{q}"), sd[f"{rb}.convs1.{q}.bias"], dilation=d, padding=(rk * d - d) // 2)
                xt = F.leaky_relu(xt, LRELU_SLOPE)
                xt = F.conv1d(xt, weight(sd, f"{rb}.convs2.{q}"), sd[f"{rb}.convs2.{q}.bias"], padding=(rk - 1) // 2)
                xr = xt + xr
            z_sum = xr if z_sum is None else z_sum + xr
        out = keep(f"stage.{i}", z_sum / nk)
    out = F.leaky_relu(out)                                   # torch's default slope 0.01 (vocoder.py:103)
    out = keep("conv_post", F.conv1d(out, weight(sd, "conv_post"), sd["conv_post.bias"], padding=3))
    return torch.tanh(out)


def tap_names(cfg):
    n = len(full_cfg(cfg)["upsample_factors"])
    return ["conv_pre"] + [f"ups.{i}" for i in range(n)] + [f"stage.{i}" for i in range(n)] + ["conv_post"]


G_SCALE = {"conv_pre": 1.0, "convs1": 1.0, "convs2": 0.7, "ups": 2.0, "conv_post": 0.25}


def seed_state_dict(sd, seed):
    """Weights that make the generator's output alive and unsaturated (a freshly constructed one is almost constant):
    weight_v ~ N(0, 1), bias ~ 0.1 N(0, 1), weight_g = c U(0.75, 1.25) with c by layer kind (G_SCALE).  sd: a weight-normed state_dict
    (shapes are taken from it); returns a new fp32 state_dict."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_v"):
            out[k] = torch.randn(v.shape, generator=g)
        elif k.endswith("bias"):
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("weight_g"):
            kind = next(n for n in ("convs1", "convs2", "ups", "conv_pre", "conv_post") if n in k)
            out[k] = G_SCALE[kind] * (0.75 + 0.5 * torch.rand(v.shape, generator=g))
        else:
            raise KeyError(f"not a weight-normed generator key: {k}")
    return out


def alive(y, taps, cfg):
    """The conditions a fixture must meet: std of y >= 0.1, no |y| > 0.99, every stage's RMS within [0.25, 4]."""
    n = len(full_cfg(cfg)["upsample_factors"])
    rms = [float(taps[f"stage.{i}"].double().pow(2).mean().sqrt()) for i in range(n)]
    ok = float(y.std()) >= 0.1 and float(y.abs().max()) <= 0.99 and all(0.25 <= r <= 4 for r in rms)
    return ok, f"std {float(y.std()):.3f}, max |y| {float(y.abs().max()):.3f}, stage RMS {[round(r, 3) for r in rms]}"


def load_fixture():
    """tests/golden/hifigan_tiny.npz (+ _taps): (cfg, weight-normed state_dict in the reference's key order, x, y, taps)."""
    import json
    import os

    import numpy as np
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = np.load(os.path.join(gold, "hifigan_tiny.npz"))
    cfg = json.loads(bytes(z["__cfg__"]).decode())
    sd = {str(k): torch.from_numpy(z["sd/" + str(k)]) for k in z["keys"]}
    zt = np.load(os.path.join(gold, "hifigan_tiny_taps.npz"))
    taps = {k[4:]: torch.from_numpy(zt[k]) for k in zt.files}
    return cfg, sd, torch.from_numpy(z["x"]), torch.from_numpy(z["y"]), taps
