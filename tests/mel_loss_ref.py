"""Plain-torch restatement of the reference's LogMelSpectrogram (urhythmic/dataset.py:23-50) and of the L1 loss the fine-tuning loop takes of
it (urhythmic_fine_tune_vocoder.py:191-222), the case table and inputs the host test and the GPU checks share, and an explicit
(hand-written) backward with switches for the errors the comparison rule must be able to see.  Test infrastructure: it needs no GPU,
imports nothing of seq2seq_vc_amd.ops, and the product never imports it.

PARITY UNPINNED against torchaudio itself (not installed here): torchaudio builds its filterbank with an fp32 linspace; this one is
oracle/logmel.py's float64 construction, cast to the dtype of the run.

`dt` = torch.float64 gives `ref64` (the truth), torch.float32 the `yard` (the same formula as stock torch computes it in float32);
gradients come from torch autograd on these.  The comparison rule is step_kernels_ref.compare, unchanged:
|got - ref64| <= 4 d + ulp_out at every element, d = max |yard - ref64|.  Nothing here is fitted to what the kernels return."""
import functools

import torch
import torch.nn.functional as F

from oracle import logmel as OL

F32, F64 = torch.float32, torch.float64
EPS = 1e-5
DEFAULT = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop_length=320, n_mels=80)
OTHER = dict(sample_rate=22050, n_fft=1024, win_length=1024, hop_length=256, n_mels=40)

# name -> (B, N, cfg, T, {row: (first sample of the tail, factor on the tail)}, clamped log-mel elements).  A factor of 0 sets the tail to
# exactly 0.  In the silent frames |X| = 0 stops the gradient whatever the clamp does, so a dropped clamp mask is invisible there:
# `quiet_frame` has one frame below the clamp value with |X| != 0 (mel ~ 1e-9), where only the mask makes the gradient zero.
CASES = {
    "one_frame": (2, 353, DEFAULT, 1, {}, 0),               # smallest legal N: left and right mirrors overlap on the same samples
    "ragged_tail": (2, 677, DEFAULT, 2, {}, 0),             # N no multiple of hop: tail samples reached through the mirror or not at all
    "silence": (2, 1600, DEFAULT, 5, {1: (700, 0.0)}, 80),  # one wholly silent frame: |X| = 0 in every bin
    "finetune": (3, 8320, DEFAULT, 26, {1: (4000, 0.0)}, 960),  # the reference's segment length
    "other_cfg": (2, 1100, OTHER, 4, {}, 0),                # no constant of the default configuration is baked in
    "quiet_frame": (2, 1600, DEFAULT, 5, {1: (700, 1e-8)}, 80),   # one frame clamped with a non-zero spectrum: the clamp mask alone acts
}


def filterbank64(cfg):
    """(bins, n_mels) float64: Slaney scale, Slaney norm, 0 .. sample_rate / 2"""
    sr = cfg["sample_rate"]
    return torch.from_numpy(OL.mel_filterbank64(sr, cfg["n_fft"], cfg["n_mels"], 0, sr / 2).T.copy())


def geometry(N, cfg):
    pad = (cfg["win_length"] - cfg["hop_length"]) // 2
    return pad, (N + 2 * pad - cfg["n_fft"]) // cfg["hop_length"] + 1


def constants(cfg, dt, device="cpu"):
    """(filterbank (bins, n_mels), window) in dt on `device`: what a caller that runs the restatement many times builds once"""
    cfg = {**DEFAULT, **cfg}
    return filterbank64(cfg).to(dt).to(device), torch.hann_window(cfg["win_length"], periodic=True, dtype=dt, device=device)


def mel(wav, dt, consts=None, **cfg):
    """wav (B, N) -> linear mel (B, n_mels, T) in dt"""
    cfg = {**DEFAULT, **cfg}
    pad, _ = geometry(wav.shape[-1], cfg)
    fb, win = constants(cfg, dt, wav.device) if consts is None else consts
    x = F.pad(wav.to(dt).unsqueeze(1), (pad, pad), "reflect").squeeze(1)
    spec = torch.stft(x, cfg["n_fft"], hop_length=cfg["hop_length"], win_length=cfg["win_length"], window=win, center=False,
                      return_complex=True).abs()
    return torch.matmul(spec.transpose(-1, -2), fb).transpose(-1, -2)


def logmel(wav, dt, consts=None, **cfg):
    """wav (B, N) -> (B, n_mels, T) in dt: log(clamp(mel, min=1e-5))"""
    return torch.log(torch.clamp(mel(wav, dt, consts, **cfg), min=EPS))


def l1(wav, tgt, dt, consts=None, **cfg):
    """F.l1_loss(logmel(wav), tgt) in dt"""
    return F.l1_loss(logmel(wav, dt, consts, **cfg), tgt.to(dt))


def logmel_grad(wav, g_logmel, dt, **cfg):
    """-> (logmel, dwav) by autograd: the gradient of sum(logmel * g_logmel)"""
    x = wav.to(dt).clone().requires_grad_(True)
    y = logmel(x, dt, **cfg)
    y.backward(g_logmel.to(dt))
    return y.detach(), x.grad


def l1_grad(wav, tgt, dt, g_out=1.0, **cfg):
    """-> (loss, dwav) by autograd: the gradient of g_out * loss"""
    x = wav.to(dt).clone().requires_grad_(True)
    loss = l1(x, tgt, dt, **cfg)
    loss.backward(torch.tensor(g_out, dtype=dt))
    return loss.detach(), x.grad


# ---------------------------------------------------------------------------------------------------------------------------
# the same chain with a hand-written backward, and planted errors
# ---------------------------------------------------------------------------------------------------------------------------
PLANTS = ("no_clamp_mask", "no_left_mirror", "no_right_mirror", "interior_doubled", "hop256", "no_nmels", "nan_phase")


def explicit(wav, dt, g_logmel=None, tgt=None, plant=None, **cfg):
    """-> (logmel, loss or None, dwav): forward and backward written out step by step -- clamp mask (ties pass), X / |X| with 0 where
    |X| = 0, the one-sided adjoint of the real FFT as N irfft(H) with H[0] = Re G[0], H[k] = G[k] / 2, H[N/2] = Re G[N/2], overlap-add,
    the adjoint of the reflect pad.  Exactly one of g_logmel / tgt.  plant: one of PLANTS, the error to commit."""
    cfg = {**DEFAULT, **cfg}
    n_fft, hop, n_mels = cfg["n_fft"], cfg["hop_length"], cfg["n_mels"]
    B, N = wav.shape
    pad, T = geometry(N, cfg)
    fhop = 256 if plant == "hop256" else hop                # the framing step only: pad and T stay
    fb = filterbank64(cfg).to(dt)
    win = torch.hann_window(cfg["win_length"], periodic=True, dtype=dt)
    xp = F.pad(wav.to(dt).unsqueeze(1), (pad, pad), "reflect").squeeze(1)
    fr = torch.stack([xp[:, t * fhop:t * fhop + n_fft] for t in range(T)], 1)       # (B, T, n_fft)
    X = torch.fft.rfft(fr * win)
    mag = X.abs()
    ml = mag @ fb                                             # (B, T, n_mels)
    lm = torch.log(torch.clamp(ml, min=EPS)).transpose(1, 2)
    loss = None
    if tgt is not None:
        diff = lm - tgt.to(dt)
        loss = diff.abs().sum() / (B * T * (1 if plant == "no_nmels" else n_mels))
        g = torch.sign(diff) / (B * T * (1 if plant == "no_nmels" else n_mels))
    else:
        g = g_logmel.to(dt)
    gmel = g.transpose(1, 2) / torch.clamp(ml, min=EPS)
    if plant != "no_clamp_mask":
        gmel = gmel * (ml >= EPS).to(dt)
    gmag = gmel @ fb.t()
    unit = X / mag if plant == "nan_phase" else torch.where(mag > 0, X / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.zeros_like(X))
    G = gmag * unit
    Hh = G.clone()
    if plant != "interior_doubled":
        Hh[..., 1:-1] = Hh[..., 1:-1] * 0.5
    Hh[..., 0] = G[..., 0].real.to(G.dtype)
    Hh[..., -1] = G[..., -1].real.to(G.dtype)
    gfr = n_fft * torch.fft.irfft(Hh, n=n_fft) * win
    gp = torch.zeros(B, N + 2 * pad, dtype=dt)
    for t in range(T):
        gp[:, t * fhop:t * fhop + n_fft] += gfr[:, t]
    dwav = gp[:, pad:pad + N].clone()
    if plant != "no_left_mirror":
        for j in range(1, pad + 1):
            dwav[:, j] += gp[:, pad - j]
    if plant != "no_right_mirror":
        for j in range(N - 1 - pad, N - 1):
            dwav[:, j] += gp[:, pad + 2 * (N - 1) - j]
    return lm, loss, dwav


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and references of the case table, computed once and shared (callers must not modify them)
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(wav (B, N) fp32, tgt, g_logmel (B, n_mels, T) fp32, cfg, pad, T)"""
    B, N, cfg, T, tails, _ = CASES[name]
    seed = 1000 + 10 * list(CASES).index(name)
    wav = (0.3 * torch.randn(B, N, generator=_gen(seed))).to(F32)
    for row, (start, factor) in tails.items():
        wav[row, start:] = wav[row, start:] * factor if factor else 0.0
    pad, T_ = geometry(N, cfg)
    assert T_ == T, (name, T_, T)
    lm64 = logmel(wav, F64, **cfg)
    u = torch.rand(lm64.shape, generator=_gen(seed + 1), dtype=F64) * 0.95 + 0.05
    s = torch.randint(0, 2, lm64.shape, generator=_gen(seed + 2)).to(F64) * 2 - 1
    tgt = (lm64 + s * u).to(F32).contiguous()
    g = torch.randn(lm64.shape, generator=_gen(seed + 3)).to(F32)
    return dict(wav=wav, tgt=tgt, g_logmel=g, cfg=cfg, pad=pad, T=T)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict of (ref64, yard) pairs: logmel, dwav (generic path, g_logmel of inputs()), loss and dwav_l1 (fused path, g_out = 1)"""
    inp = inputs(name)
    out = {}
    per = {}
    for dt in (F64, F32):
        lm, dw = logmel_grad(inp["wav"], inp["g_logmel"], dt, **inp["cfg"])
        loss, dwl = l1_grad(inp["wav"], inp["tgt"], dt, **inp["cfg"])
        per[dt] = dict(logmel=lm, dwav=dw, loss=loss.reshape(1), dwav_l1=dwl)
    for k in per[F64]:
        out[k] = (per[F64][k], per[F32][k])
    out["mel64"] = mel(inp["wav"], F64, **inp["cfg"])
    return out


def loss_bound(name):
    """The scalar loss: |got - ref64| <= 4 d_logmel + ulp32(max |ref64_logmel - tgt|) + ulp32(loss64) -- the element rule plus one final
    rounding, given that the partial sums are taken in double."""
    import step_kernels_ref as R
    ref, inp = reference(name), inputs(name)
    lm64, lm32 = ref["logmel"]
    d = float((lm32.double() - lm64).abs().max())
    top = (lm64 - inp["tgt"].double()).abs().max().reshape(1)
    return R.MARGIN * d + float(R.ulp_out(top, F32)) + float(R.ulp_out(ref["loss"][0], F32))
