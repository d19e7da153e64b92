"""Float64 restatements and shared problems for AASVC.inference_batch (tests/test_aasvc_batch_host.py pins them to stock torch and to the
reference's rule; tests/gpu_aasvc_batch_check.py compares the kernels with them).  Test infrastructure: needs no GPU, imports nothing
of seq2seq_vc_amd, and the product never imports it."""
import json
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("aasvc_tiny_inference_batch", "aasvc_det_tiny_inference_batch")
MAX_DP_OUTPUT = 10

# (B, Tn, C, ks), vlens (None: every row is full).  70 and 130 cross the 64-frame tile of the kernel, vlens 1 / 9 are shorter than the
# half width of the taps, C = 32 does not fill the 64-channel tile, C = 128 takes two of them; the last case is the kernel's run-time-ks
# route (every ks other than 7 / 15 / 31) at a C that is a multiple of 8 only.
CONVMOD_CASES = [
    ((3, 70, 32, 7), [70, 1, 37]),
    ((2, 130, 128, 15), [130, 65]),
    ((2, 33, 64, 31), [33, 9]),
    ((2, 130, 128, 15), None),
    ((2, 70, 40, 5), [70, 3]),
]


def convmod_problem(shape, seed):
    """Inputs of one case, fp32 on the CPU: y2 (B,Tn,2C), depthwise weight (C,1,ks) / bias, BatchNorm running statistics and affine."""
    B, Tn, C, ks = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(y2=r(B, Tn, 2 * C), w=r(C, 1, ks) * (1.0 / ks ** 0.5), bias=r(C) * 0.1, mean=r(C) * 0.2, var=torch.rand(C, generator=g) + 0.5,
                gamma=1.0 + 0.2 * r(C), beta=0.1 * r(C), eps=1e-5)


def convmod_infer_ref(y2, w, bias, mean, var, gamma, beta, eps, vlens=None):
    """out[b,t,c] = swish(bn_eval(bias[c] + sum_j w[c,j] g[b,t+j-(ks-1)/2,c])) for t < vlens[b], 0 beyond; g = glu(y2) inside the row, 0
    outside.  Float64, written from the definition (explicit taps; frames >= vlens[b] of y2 are never touched)."""
    y2, w, mean, var, gamma, beta = (torch.as_tensor(t).double() for t in (y2, w, mean, var, gamma, beta))
    B, Tn, C2 = y2.shape
    C, ks = C2 // 2, w.shape[-1]
    pad = (ks - 1) // 2
    out = torch.zeros(B, Tn, C, dtype=torch.float64)
    for b in range(B):
        L = Tn if vlens is None else int(vlens[b])
        g = torch.zeros(L + 2 * pad, C, dtype=torch.float64)
        g[pad:pad + L] = y2[b, :L, :C] / (1.0 + torch.exp(-y2[b, :L, C:]))
        acc = torch.zeros(L, C, dtype=torch.float64) if bias is None else torch.as_tensor(bias).double().expand(L, C).clone()
        for j in range(ks):
            acc += w[:, 0, j] * g[j:j + L]
        z = (acc - mean) / torch.sqrt(var + eps) * gamma + beta
        out[b, :L] = z / (1.0 + torch.exp(-z))
    return out


def durations_finalize_ref(d, text_lens, dmax=MAX_DP_OUTPUT):
    """-> (d_outs in d's dtype: min(d, dmax), 0 at entries >= text_lens[b]; ds float32: d_outs, a row whose valid entries sum to 0 gets 1 in
    every valid entry; total int32: row sums of ds)."""
    d = np.asarray(d)
    B, Tx = d.shape
    d_outs = np.zeros_like(d)
    ds = np.zeros((B, Tx), np.float32)
    for b in range(B):
        L = int(text_lens[b])
        d_outs[b, :L] = np.minimum(d[b, :L], dmax)
        ds[b, :L] = d_outs[b, :L]
        if ds[b, :L].sum() == 0:
            ds[b, :L] = 1
    return d_outs, ds, ds.sum(1).astype(np.int32)


def interp_rows_ref(x, Tout, lens_in, lens_out):
    """Row b: F.interpolate (nearest) of its own lens_in[b] frames to lens_out[b] frames; zero beyond."""
    x = torch.as_tensor(x)
    out = torch.zeros(x.shape[0], Tout, x.shape[2], dtype=x.dtype)
    for b in range(x.shape[0]):
        li, lo = int(lens_in[b]), int(lens_out[b])
        out[b, :lo] = torch.nn.functional.interpolate(x[b, :li].t()[None], size=lo)[0].t()
    return out


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = json.loads(bytes(z["__cfg__"]).decode())
    return cfg, z


def state_dict_of(cfg):
    """The batch fixtures hold inputs and outputs only; their weights are the ones of the single-utterance fixture named in the config."""
    z = np.load(os.path.join(GOLD, cfg["__sd_from__"] + ".npz"))
    return {k[3:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("sd.")}


def fixture_conditions(cfg, z):
    """The lengths are the test (tools/gen_golden_aasvc_batch.py): [(ok, message)]."""
    T, ol, d = z["in.ilens"].tolist(), z["out.olens"].tolist(), z["out.d_outs"]
    pr = cfg.get("post_encoder_reduction_factor", 1)
    tx = [t // pr for t in T]
    cross = [L for L in ol if L > 64 and L % 64 != 0]
    res = [(z["in.xs"].shape[1] == max(T) and T.count(max(T)) == 1, f"one row fills the batch: T {T}"),
           (pr == 1 or any(t % pr for t in T), f"a row with T % {pr} != 0: T {T}"),
           (any(t <= 3 for t in tx), f"a row with at most 3 encoder frames: Tx {tx}"),
           (bool(cross) and any(ol.count(L) == 1 for L in cross), f"an output length beyond 64 that is no multiple of 64 and unlike the others: olens {ol}"),
           (d.shape == (len(T), max(tx)) and all((d[b, tx[b]:] == 0).all() for b in range(len(T))), f"d_outs {d.shape} padded with zeros"),
           ([int(np.minimum(d[b, :tx[b]], MAX_DP_OUTPUT).sum()) for b in range(len(T))] == ol, "olens are the row sums of the durations"),
           (z["out.outs"].shape == (len(T), max(ol), cfg["odim"]) and all((z["out.outs"][b, ol[b]:] == 0).all() for b in range(len(T))),
            f"outs {z['out.outs'].shape} zero beyond olens")]
    if "in.sdp_noise" in z.files:
        n = z["in.sdp_noise"]
        res.append((n.shape == (len(T), 2, max(tx)) and all((n[b, :, tx[b]:] == 0).all() for b in range(len(T))), f"noise {n.shape} zero-padded"))
    return res


def cmp(name, got, ref, atol, l1_tol=None):
    """The comparison of tests/gpu_model_check.py: max |got - ref| <= atol (NaN fails), optionally mean |.| <= l1_tol."""
    got = torch.as_tensor(got).detach().double().cpu()
    ref = torch.as_tensor(np.asarray(ref)).double()
    if got.shape != ref.shape:
        return False, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    mx = float(err.max()) if err.numel() else 0.0
    l1 = float(err.mean()) if err.numel() else 0.0
    ok = bool((err <= atol).all()) and (l1_tol is None or l1 <= l1_tol)
    return ok, f"{name}: max_err={mx:.3e} mean_abs_err={l1:.3e} (atol {atol:g}" + (f", mean {l1_tol:g})" if l1_tol is not None else ")")
