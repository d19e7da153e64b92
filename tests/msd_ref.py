"""Plain-torch restatement of the HiFi-GAN multi-scale discriminator over a state_dict, any dtype, on the CPU, written from the
description of the operation (not from the reference's text):

  three scale discriminators see x (B, 1, T), pool(x) and pool(pool(x)), pool = the average of 4 samples at stride 2 with 2 zeros of
  padding on either side, the padding counted (T -> T // 2 + 1).  A scale discriminator runs Conv1d 1 -> 128 (15 taps), five grouped
  convolutions of 41 taps (128 -> 128 stride 2 groups 4, 128 -> 256 stride 2 groups 16, 256 -> 512 stride 4 groups 16, 512 -> 1024
  stride 4 groups 16, 1024 -> 1024 stride 1 groups 16) and Conv1d 1024 -> 1024 (5 taps), each with padding (k - 1) / 2, followed by
  leaky_relu(0.1) and recorded as a feature, then conv_post (1024 -> 1, 3 taps, no activation), the eighth feature; the score is its
  flattening.  Scales 1 and 2 are weight-normed.  Scale 0 is spectrally normed: with W = weight_orig viewed (O, -1), a call in train()
  mode first runs v <- W^T u / max(|W^T u|, eps), u <- W v / max(|W v|, eps) (written back to the buffers), every call uses
  sigma = u . (W v) and the weight weight_orig / sigma, with u and v constants for autograd.

It is the yardstick of the GPU tests (float64 = the truth, float32 = what stock arithmetic costs) and is itself pinned to the
reference by tests/golden/hifigan_msd.npz (tools/gen_golden_msd.py, tests/test_msd_host.py).  The weights of every test come from a
seeded numpy rule (30 M values are not stored).  Test infrastructure: no GPU, nothing of seq2seq_vc_amd.ops; the product never imports it."""
import os

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.1
EPS = 1e-12
# convs[j]: (C_in, C_out, kernel size, stride, groups); the last entry is conv_post
LAYERS = ((1, 128, 15, 1, 1), (128, 128, 41, 2, 4), (128, 256, 41, 2, 16), (256, 512, 41, 4, 16), (512, 1024, 41, 4, 16),
          (1024, 1024, 41, 1, 16), (1024, 1024, 5, 1, 1), (1024, 1, 3, 1, 1))
SCALES = 3
SPECTRAL = (True, False, False)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hifigan_msd.npz")


# ---------------------------------------------------------------------------------------------------------------------------
# shapes and index maps
# ---------------------------------------------------------------------------------------------------------------------------
def layer_name(j):
    return f"convs.{j}" if j < len(LAYERS) - 1 else "conv_post"


def state_dict_shapes():
    """[(key, shape)] of MultiScaleDiscriminator.state_dict() in order: 80 keys, 29 637 357 values."""
    out = []
    for i in range(SCALES):
        for j, (cin, cout, k, _, g) in enumerate(LAYERS):
            name = f"discriminators.{i}.{layer_name(j)}"
            if SPECTRAL[i]:
                out += [(name + ".bias", (cout,)), (name + ".weight_orig", (cout, cin // g, k)), (name + ".weight_u", (cout,)),
                        (name + ".weight_v", (cin // g * k,))]
            else:
                out += [(name + ".bias", (cout,)), (name + ".weight_g", (cout, 1, 1)), (name + ".weight_v", (cout, cin // g, k))]
    return out


def is_buffer(key):
    return SPECTRAL[int(key.split(".")[1])] and key.rsplit(".", 1)[1] in ("weight_u", "weight_v")


def pool_len(T):
    return T // 2 + 1


def conv_len(L, s):
    return (L - 1) // s + 1


def length_chain(T):
    """[[L of the 8 features] per scale] for x of T samples"""
    out = []
    for i in range(SCALES):
        if i:
            T = pool_len(T)
        L, row = T, []
        for _, _, _, s, _ in LAYERS:
            L = conv_len(L, s)
            row.append(L)
        out.append(row)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# seeded weights
# ---------------------------------------------------------------------------------------------------------------------------
def _orthonormal_rows(O, K, rng):
    """(O, K) float64 with orthonormal rows (O <= K) or columns (O > K): rows of the DCT-II matrix of max(O, K) points at
    frequencies 1 .. min(O, K), its columns shuffled and given random signs -- a closed form, the same on every machine."""
    n, m = max(O, K), min(O, K)
    pos = rng.permutation(n).astype(np.float64)
    sign = rng.integers(0, 2, n).astype(np.float64) * 2 - 1
    c = np.sqrt(2.0 / n) * np.cos(np.pi * (pos[None, :] + 0.5) * np.arange(1, m + 1, dtype=np.float64)[:, None] / n) * sign[None, :]
    return c if O <= K else np.ascontiguousarray(c.T)


def seeded_state_dict(seed):
    """Weight norm (scales 1, 2): weight_v ~ N(0, 1), weight_g = 1.5 U(0.8, 1.2) (a unit-norm row over unit-variance inputs keeps the
    scale; 1.5 makes up for what leaky_relu removes).  Spectral norm (scale 0): weight / sigma does not depend on the scale of
    weight_orig, and an i.i.d. Gaussian (O, K) matrix has sigma = sqrt(O) + sqrt(K) against rows of norm sqrt(K): every layer would
    lose a factor 2 to 4 and the eighth feature would be bias alone.  So weight_orig = 0.7 (Q + 0.1 G / sqrt(K)), Q with orthonormal
    rows (sigma = row norm = 1: nothing lost but leaky_relu's share) and G ~ N(0, 1), which keeps the power iteration away from its
    fixed point.  u, v: normalised N(0, 1) draws.  bias ~ 0.05 N(0, 1).  One numpy Generator per key, seeded with (seed, index)."""
    out = {}
    for n, (key, shape) in enumerate(state_dict_shapes()):
        rng = np.random.default_rng([seed, n])
        leaf = key.rsplit(".", 1)[1]
        if leaf == "weight_orig":
            O, K = shape[0], shape[1] * shape[2]
            a = (0.7 * (_orthonormal_rows(O, K, rng) + 0.1 * rng.standard_normal((O, K)) / np.sqrt(K))).reshape(shape).astype(np.float32)
        elif leaf == "weight_g":
            a = (1.5 * (0.8 + 0.4 * rng.random(shape, dtype=np.float32))).astype(np.float32)
        elif leaf == "bias":
            a = (0.05 * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
        elif is_buffer(key):
            d = rng.standard_normal(shape)
            a = (d / np.linalg.norm(d)).astype(np.float32)
        else:
            a = rng.standard_normal(shape, dtype=np.float32)
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
def pool(x):
    """(B, 1, T) -> (B, 1, T // 2 + 1): y[t] = 0.25 (x[2t - 2] + x[2t - 1] + x[2t] + x[2t + 1]), zeros outside"""
    T = x.shape[-1]
    To = pool_len(T)
    xp = F.pad(x, (2, 2 * To + 2 - T))
    return 0.25 * (xp[..., 0:2 * To:2] + xp[..., 1:2 * To + 1:2] + xp[..., 2:2 * To + 2:2] + xp[..., 3:2 * To + 3:2])


def weight_normed(v, g):
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))


def power_iteration(W, u, v, train):
    """-> (u, v), detached: after one iteration when `train`, the stored u, v otherwise (the caller forms sigma = u . (W v))"""
    Wm = W.detach().flatten(1)
    u, v = u.detach(), v.detach()
    if train:
        t = Wm.t() @ u
        v = t / t.norm().clamp_min(EPS)
        s = Wm @ v
        u = s / s.norm().clamp_min(EPS)
    return u, v


def scale_forward(sd, i, x, train=True, drop_tap=None, buffers=None):
    """Discriminator i of the state_dict on x (B, 1, T) -> (score, [8 features]).  buffers (a dict) receives the updated u, v of a
    spectrally normed scale.  drop_tap = (layer, tap): that tap's weights are zeroed (a planted error for the tests of the tests)."""
    h, feats = x, []
    for j, (cin, cout, k, s, g) in enumerate(LAYERS):
        pre = f"discriminators.{i}.{layer_name(j)}"
        if SPECTRAL[i]:
            W = sd[pre + ".weight_orig"]
            u, v = power_iteration(W, sd[pre + ".weight_u"].to(W.dtype), sd[pre + ".weight_v"].to(W.dtype), train)
            if buffers is not None:
                buffers[pre + ".weight_u"], buffers[pre + ".weight_v"] = u, v
            w = W / torch.dot(u, W.flatten(1) @ v)
        else:
            w = weight_normed(sd[pre + ".weight_v"], sd[pre + ".weight_g"])
        if drop_tap is not None and drop_tap[0] == j:
            w = w.clone()
            w[:, :, drop_tap[1]] = 0
        h = F.conv1d(h, w, sd[pre + ".bias"], stride=s, padding=(k - 1) // 2, groups=g)
        if j < len(LAYERS) - 1:
            h = F.leaky_relu(h, SLOPE)
        feats.append(h)
    return h.flatten(1), feats


def msd_forward(sd, x, train=True, buffers=None):
    scores, feats = [], []
    for i in range(SCALES):
        if i:
            x = pool(x)
        s, f = scale_forward(sd, i, x, train, buffers=buffers)
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


def run(sd, xr, xg, dtype, train=True):
    """The whole computation in `dtype`: D(xr), then D(xg) from the buffers the first call left (two power iterations in train mode),
    the loss, its gradients.  -> dict(scores, feats (of xg), scores_r, loss, dxg, dxr, grads {key: gradient}, buffers {key: u or v after
    both calls})."""
    keys = [k for k in sd if not is_buffer(k)]
    prm = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in keys}        # clones: the caller's tensors stay as they are
    bufs = {k: sd[k].detach().to(dtype).clone() for k in sd if is_buffer(k)}
    xr, xg = xr.detach().to(dtype).clone().requires_grad_(True), xg.detach().to(dtype).clone().requires_grad_(True)
    after = {}
    sr, fr = msd_forward({**prm, **bufs}, xr, train, after)
    sg, fg = msd_forward({**prm, **bufs, **after}, xg, train, after)
    loss = total_loss(sr, fr, sg, fg)
    grads = torch.autograd.grad(loss, [xr, xg] + [prm[k] for k in keys])
    return dict(scores=[s.detach() for s in sg], feats=[[f.detach() for f in fl] for fl in fg], scores_r=[s.detach() for s in sr],
                loss=loss.detach(), dxr=grads[0], dxg=grads[1], grads=dict(zip(keys, grads[2:])), buffers={k: v.detach() for k, v in after.items()})


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the tests (shared by the host tests, the fixture and the GPU cases)
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 13
SAMPLE = 64           # elements of a tensor the fixture records (fixed positions)


def inputs(T, B=2, seed=5, scale=0.3):
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
# the kernels' index arithmetic, stated once in plain Python on one small sequence (tests/test_msd_host.py holds each against stock
# torch, and shows that the planted error beside it is caught)
# ---------------------------------------------------------------------------------------------------------------------------
TAPS, PAD = 41, 20


def dgrad_phase_table(stride, ph):
    """[(offset of the output row from l // stride, tap j)] of input rows l = stride * q + ph: the taps j = l + 20 (mod stride);
    tap j pairs row l with the output row lo of stride * lo + j - 20 = l"""
    j0 = (ph + PAD) % stride
    return [((ph + PAD - j) // stride, j) for j in range(j0, TAPS, stride)]


def dgrad_phase_model(dy, w, L, stride, plant=False):
    """Data gradient of the stride-s, 41-tap convolution of ONE sequence and ONE group: dy (Lo, C_out), w (C_out, C_in, 41) ->
    dx (L, C_in).  plant: the table of phase r + 1 is used for phase r."""
    Lo = dy.shape[0]
    dx = torch.zeros(L, w.shape[1], dtype=dy.dtype)
    for l in range(L):
        q, r = divmod(l, stride)
        for off, j in dgrad_phase_table(stride, (r + 1) % stride if plant else r):
            if 0 <= q + off < Lo:
                dx[l] += dy[q + off] @ w[:, :, j]
    return dx


def grouped_conv_model(x, w, groups, stride, neighbour=False, leak=False):
    """The grouped strided convolution over channel-last rows flattened to i = b * L + l: x (B, L, C_in), w (C_out, C_in / groups, 41)
    -> (B, Lo, C_out).  Output channel o of group g = o // (C_out / groups) reads channels [g Cg, g Cg + Cg) of row (b, stride * lo +
    j - 20) when that l lies in [0, L).  neighbour=True reads the NEXT group's channels (the planted error at the group boundary);
    leak=True bounds the FLAT row index over the whole batch instead (a tap that leaves an utterance lands in the next one)."""
    B, L, cin = x.shape
    cout, cg, k = w.shape
    og = cout // groups
    Lo = conv_len(L, stride)
    xf = x.reshape(B * L, cin)
    out = torch.zeros(B, Lo, cout, dtype=x.dtype)
    for b in range(B):
        for lo in range(Lo):
            for j in range(k):
                l = stride * lo + j - PAD
                flat = b * L + l
                if not ((0 <= flat < B * L) if leak else (0 <= l < L)):
                    continue
                for g in range(groups):
                    gs = (g + 1) % groups if neighbour else g
                    out[b, lo, g * og:(g + 1) * og] += w[g * og:(g + 1) * og, :, j] @ xf[flat, gs * cg:(gs + 1) * cg]
    return out


def pool_adjoint_model(dy, T, plant=None):
    """dx (T) from dy (T // 2 + 1): sample i is summand j of output t whenever 2 t - 2 + j = i, j < 4.  plant "right": the last output
    is forgotten (it reads x[T - 2 ..] or x[T - 1 ..] and padding); plant "left": output 0 is forgotten (it reads padding, x[0], x[1])."""
    To = dy.shape[0]
    dx = torch.zeros(T, dtype=dy.dtype)
    for i in range(T):
        for j in range(4):
            num = i + 2 - j
            if num >= 0 and num % 2 == 0 and (1 if plant == "left" else 0) <= num // 2 < (To - 1 if plant == "right" else To):
                dx[i] += 0.25 * dy[num // 2]
    return dx


def spectral_grad(dW, W, u, v, sigma):
    """Gradient of weight_orig from dW = the gradient of W / sigma, sigma = u . (W v) with u, v constants"""
    return dW / sigma - (dW * W).sum() / sigma ** 2 * torch.outer(u, v).view_as(W)
