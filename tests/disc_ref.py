"""Plain-torch restatement of the HiFi-GAN multi-period discriminator over a state_dict, any dtype, on the CPU, written from the
description of the operation (not from the reference's text):

  a period discriminator of period p pads x (B, 1, T) on the right by reflection to a multiple of p, views it (B, 1, L0, p) and runs
  five weight-normed convolutions along L only (kernel (5, 1), padding (2, 0), strides 3, 3, 3, 3, 1, channels 1 -> 32 -> 128 -> 512
  -> 1024 -> 1024), each followed by leaky_relu(0.1) and recorded as a feature, then conv_post (1024 -> 1, kernel (3, 1), padding
  (1, 0), no activation), which is the sixth feature; the score is its flattening.  The multi-period discriminator runs periods
  2, 3, 5, 7, 11 and returns the two lists.

It is the yardstick of the GPU tests (float64 = the truth, float32 = what stock arithmetic costs) and is itself pinned to the
reference by tests/golden/hifigan_mpd.npz (tools/gen_golden_disc.py, tests/test_disc_host.py).  The weights of every test come from a
seeded numpy rule (41 M values are not stored).  Test infrastructure: no GPU, nothing of seq2seq_vc_amd.ops; the product never imports it."""
import os

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.1
PERIODS = (2, 3, 5, 7, 11)
CHANNELS = (1, 32, 128, 512, 1024, 1024)
STRIDES = (3, 3, 3, 3, 1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hifigan_mpd.npz")


# ---------------------------------------------------------------------------------------------------------------------------
# shapes and index maps
# ---------------------------------------------------------------------------------------------------------------------------
def state_dict_shapes(channels=CHANNELS):
    """[(key, shape)] of MultiPeriodDiscriminator.state_dict() in order."""
    out = []
    for i in range(len(PERIODS)):
        layers = [(f"discriminators.{i}.convs.{j}", channels[j + 1], channels[j], 5) for j in range(len(STRIDES))]
        layers.append((f"discriminators.{i}.conv_post", 1, channels[-1], 3))
        for name, o, c, k in layers:
            out += [(name + ".bias", (o,)), (name + ".weight_g", (o, 1, 1, 1)), (name + ".weight_v", (o, c, k, 1))]
    return out


def reflect_map(T, p):
    """Sample of x under every position of the padded signal: t for t < T, then T - 2, T - 3, .. (the mirror image about T - 1)."""
    pad = (p - T % p) % p
    assert pad < T, "reflection needs pad < T"
    return [t if t < T else 2 * (T - 1) - t for t in range(T + pad)]


def length_chain(T, p):
    """[L0 .. L5]: L0 = ceil(T / p), then L -> floor((L - 1) / s) + 1 per convolution"""
    L = [-(-T // p)]
    for s in STRIDES:
        L.append((L[-1] - 1) // s + 1)
    return L


# ---------------------------------------------------------------------------------------------------------------------------
# seeded weights
# ---------------------------------------------------------------------------------------------------------------------------
def seeded_state_dict(seed, channels=CHANNELS):
    """weight_v ~ N(0, 1), weight_g = 1.5 U(0.8, 1.2) (a unit-norm row over unit-variance inputs keeps the scale; 1.5 makes up for
    what leaky_relu removes), bias ~ 0.05 N(0, 1).  One numpy Generator per key, seeded with (seed, index of the key)."""
    out = {}
    for n, (key, shape) in enumerate(state_dict_shapes(channels)):
        rng = np.random.default_rng([seed, n])
        if key.endswith("weight_v"):
            a = rng.standard_normal(shape, dtype=np.float32)
        elif key.endswith("weight_g"):
            a = (1.5 * (0.8 + 0.4 * rng.random(shape, dtype=np.float32))).astype(np.float32)
        else:
            a = (0.05 * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
        out[key] = torch.from_numpy(a)
    return out


def alive(x, feats):
    """Every feature's mean |.| lies within two decades of the input's."""
    ref = float(x.detach().abs().mean())
    m = [[float(f.detach().abs().mean()) for f in fl] for fl in feats]
    ok = all(ref / 100 <= v <= ref * 100 for fl in m for v in fl)
    return ok, f"input mean |x| {ref:.3e}; features " + "; ".join(" ".join(f"{v:.2e}" for v in fl) for fl in m)


# ---------------------------------------------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------------------------------------------
def folded(x, p):
    B, C, T = x.shape
    idx = torch.tensor(reflect_map(T, p), dtype=torch.long)
    return x[:, :, idx].reshape(B, C, -1, p)


def normed_weight(v, g):
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))


def period_forward(sd, i, x, drop_tap=None):
    """Discriminator i of the state_dict on x (B, 1, T) -> (score, [6 features]).  drop_tap = (layer, tap): that tap's weights are
    zeroed (a planted error for the tests of the tests)."""
    p = PERIODS[i]
    h = folded(x, p)
    feats = []
    for j, s in enumerate(STRIDES):
        pre = f"discriminators.{i}.convs.{j}"
        w = normed_weight(sd[pre + ".weight_v"], sd[pre + ".weight_g"])
        if drop_tap is not None and drop_tap[0] == j:
            w = w.clone()
            w[:, :, drop_tap[1]] = 0
        h = F.leaky_relu(F.conv2d(h, w, sd[pre + ".bias"], stride=(s, 1), padding=(2, 0)), SLOPE)
        feats.append(h)
    pre = f"discriminators.{i}.conv_post"
    h = F.conv2d(h, normed_weight(sd[pre + ".weight_v"], sd[pre + ".weight_g"]), sd[pre + ".bias"], padding=(1, 0))
    feats.append(h)
    return h.flatten(1), feats


def mpd_forward(sd, x, periods=range(len(PERIODS))):
    scores, feats = [], []
    for i in periods:
        s, f = period_forward(sd, i, x)
        scores.append(s)
        feats.append(f)
    return scores, feats


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed scalar loss: the three losses of the fine-tuning step, summed
# ---------------------------------------------------------------------------------------------------------------------------
def total_loss(scores_r, feats_r, scores_g, feats_g):
    """feature loss (sum over features of mean |real - generated|) + discriminator loss (sum of mean (1 - real)^2 + mean generated^2)
    + generator loss (sum of mean (1 - generated)^2)"""
    loss = 0
    for fr, fg in zip(feats_r, feats_g):
        for a, b in zip(fr, fg):
            loss = loss + torch.mean(torch.abs(a - b))
    for r, g in zip(scores_r, scores_g):
        loss = loss + torch.mean((1 - r) ** 2) + torch.mean(g ** 2)
    for g in scores_g:
        loss = loss + torch.mean((1 - g) ** 2)
    return loss


def run(sd, xr, xg, dtype, periods=range(len(PERIODS))):
    """The whole computation in `dtype`: D(xr), D(xg), the loss, its gradients.  -> dict(scores, feats (of xg), scores_r, loss, dxg, dxr,
    grads {key: gradient})."""
    keys = [k for k in sd if int(k.split(".")[1]) in set(periods)]
    prm = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in keys}        # clones: the caller's tensors stay as they are
    xr, xg = xr.detach().to(dtype).clone().requires_grad_(True), xg.detach().to(dtype).clone().requires_grad_(True)
    sr, fr = mpd_forward(prm, xr, periods)
    sg, fg = mpd_forward(prm, xg, periods)
    loss = total_loss(sr, fr, sg, fg)
    grads = torch.autograd.grad(loss, [xr, xg] + [prm[k] for k in keys])
    return dict(scores=[s.detach() for s in sg], feats=[[f.detach() for f in fl] for fl in fg], scores_r=[s.detach() for s in sr],
                loss=loss.detach(), dxr=grads[0], dxg=grads[1], grads=dict(zip(keys, grads[2:])))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the tests (shared by the host tests, the fixture and the GPU cases)
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 11
SAMPLE = 64           # elements of a tensor the fixture records (fixed positions)


def inputs(T, B=2, seed=3, scale=0.3):
    g = torch.Generator().manual_seed(seed * 1000 + T)
    return scale * torch.randn(B, 1, T, generator=g), scale * torch.randn(B, 1, T, generator=g)


def sample_positions(numel, n=SAMPLE):
    """n fixed flat positions of a tensor with `numel` elements: evenly spread, first and last included"""
    if numel <= n:
        return np.arange(numel)
    return np.unique(np.round(np.linspace(0, numel - 1, n)).astype(np.int64))


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' index arithmetic, stated once in plain Python on one small sequence (tests/test_disc_host.py holds each against stock
# torch, and shows that the planted error beside it is caught)
# ---------------------------------------------------------------------------------------------------------------------------
DGRAD_PHASES = {0: ((0, 2),), 1: ((0, 3), (1, 0)), 2: ((0, 4), (1, 1))}       # l mod 3 -> ((offset of the output row from l // 3, tap j), ..)


def dgrad_phase_model(dy, w, L, plant=False):
    """Data gradient of the stride-3 convolution of ONE sequence: dy (Lo, C_out), w (C_out, C_in, 5) -> dx (L, C_in).  Input row l
    receives only the taps j = l + 2 (mod 3), from output rows l // 3 (+ 1).  plant: the table of phase r is used for phase r + 1."""
    Lo = dy.shape[0]
    dx = torch.zeros(L, w.shape[1], dtype=dy.dtype)
    for l in range(L):
        g, r = divmod(l, 3)
        for off, j in DGRAD_PHASES[(r + 1) % 3 if plant else r]:
            if g + off < Lo:
                dx[l] += dy[g + off] @ w[:, :, j]
    return dx


def dx_gather_model(gpad, T, mirror=True):
    """dx (T) from the gradient of the reflect-padded signal gpad (T + pad): own position plus the mirror image 2 (T - 1) - t where the
    pad copied the sample.  mirror=False is the planted error."""
    Tp = gpad.shape[0]
    dx = gpad[:T].clone()
    if mirror:
        for t in range(T):
            tm = 2 * (T - 1) - t
            if T <= tm < Tp:
                dx[t] += gpad[tm]
    return dx


def flat_row_conv_model(x, w, stride, leak=False):
    """The strided convolution over channel-last rows (b, l, w) flattened to i = (b * L + l) * p + w: x (B, L, p, C_in),
    w (C_out, C_in, 5) -> (B, Lo, p, C_out).  Output row (b, lo, w) reads row (b, stride * lo + j - 2, w) when that l lies in [0, L).
    leak=True bounds the FLAT index over the whole batch instead (the planted error: a tap that leaves an utterance at its start or
    end lands in the neighbouring utterance's rows)."""
    B, L, p, cin = x.shape
    Lo = (L - 1) // stride + 1
    xf = x.reshape(B * L * p, cin)
    out = torch.zeros(B, Lo, p, w.shape[0], dtype=x.dtype)
    for b in range(B):
        for lo in range(Lo):
            for ww in range(p):
                for j in range(5):
                    l = stride * lo + j - 2
                    flat = (b * L + l) * p + ww
                    inside = (0 <= flat < B * L * p) if leak else (0 <= l < L)
                    if inside:
                        out[b, lo, ww] += w[:, :, j] @ xf[flat]
    return out
