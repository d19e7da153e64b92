"""How much of a bf16 gradient's distance to float64 is leaky-relu masks flipped by the bf16 FORWARD (CPU only, no GPU).

    python tools/vocoder_mask_flips.py

On the tests' tiny generator and committed input: runs tests/vocoder_ref.generator_forward under torch.autocast("cpu", bfloat16),
records every leaky-relu mask, then repeats the computation in float64 with those recorded masks in place of its own.  Prints the
number of flipped masks and the per-tensor relL2 to the float64 gradient of (a) autocast and (b) float64 arithmetic over autocast's
masks.  (b) ~ (a) is why a trainable generator keeps fp32 activations in bf16 mode (profiles/AB_LOG.md)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vocoder_bwd_ref as VB  # noqa: E402
import vocoder_ref as VR  # noqa: E402

cfg, sd, *_ = VR.load_fixture()
x = VB.grad_input()
orig = F.leaky_relu
masks = []
def rec(v, slope=0.01, *a, **k):
    masks.append((v > 0).detach().clone()); return orig(v, slope)
it = None
def replay(v, slope=0.01, *a, **k):
    m = next(it); return v * torch.where(m, torch.ones_like(v), torch.full_like(v, slope))
def rel(a, b): return float((a.double()-b.double()).norm() / b.double().norm().clamp_min(1e-30))
_, _, g64 = VB.generator_grads(sd, cfg, x)
F.leaky_relu = rec
_, _, gamp = VB.generator_grads(sd, cfg, x, dtype=torch.float32, autocast=True)
F.leaky_relu = replay; it = iter(masks)
_, _, gflip = VB.generator_grads(sd, cfg, x)     # float64 arithmetic, the bf16 run's masks
F.leaky_relu = orig
nflip = 0
chk = []
F.leaky_relu = lambda v, slope=0.01, *a, **k: (chk.append(v > 0), orig(v, slope))[1]
VB.generator_grads(sd, cfg, x); F.leaky_relu = orig
nflip = sum(int((a != b).sum()) for a, b in zip(masks, chk)); tot = sum(a.numel() for a in chk)
ra = [rel(gamp[k], g64[k]) for k in g64]; rf = [rel(gflip[k], g64[k]) for k in g64]
print(f"masks flipped in the autocast forward: {nflip} of {tot}")
print(f"median relL2 vs f64: autocast {statistics.median(ra):.2e}; f64 arithmetic with autocast's masks {statistics.median(rf):.2e}")
share = sorted(f / max(a, 1e-30) for a, f in zip(ra, rf))
print(f"flip-only / total per tensor: min {share[0]:.2f} median {statistics.median(share):.2f} max {share[-1]:.2f}")
print(f"autocast vs (f64 with its own masks), median relL2: {statistics.median(rel(gamp[k], gflip[k]) for k in g64):.2e}")
