"""Plain torch-CPU restatement of what csrc/attn_fused.hip's attn_proj_bwd_kernel stands in for -- the out-projection's data gradient
dctx = dY . W_o followed by the attention backward of tests/attn_kernels_ref.py -- with the case table and the inputs of
tests/gpu_attn_proj_kernel_check.py (tests/test_attn_proj_host.py runs its power check on the very same tensors).

Roundings to bf16 (`bf16=True`, the yard): dctx, once, after the fp32 sum over D (the kernel's header comment: the values the GEMM
stores); then those of attn_kernels_ref.attn_bwd (dS, the dropped map, the outputs).

Planted errors (`plant`), each of which the comparison rule must reject on the GPU cases' own inputs:
  "head+1"        the weight rows of the next head
  "untransposed"  W_o read as if it were W_o^T (dctx = dY . W_o^T)
  "k_short"       the sum over D stops one 32-step early"""
import torch

import attn_kernels_ref as A
import step_kernels_ref as R
from step_kernels_ref import BF16, F32, F64, bf16_round

PLANTS = ("head+1", "untransposed", "k_short")
B_ = 3
P_DROP = 0.3

# (D, H, dk, kind, T1, T2, causal).  kind "self": q | k | v are the column blocks of a packed (B, T, 3D) tensor and dq | dk | dv those of
# the packed gradient; "source": q is dense, k | v a column block of a (B, T2, L 2D) tensor, dk | dv written into that block of the gradient.
# D = 64 / 256 / 384: 2 / 4 / 6 chunks of 64 columns (the kernel's compiled variants; D = 64 leaves the second chunk of its variant empty);
# T 1 / 15 / 17 / 33 / 63 / 64: a single row, waves without a valid row, rows that end inside a 16-row tile, full tiles.
CASES = [(64, 2, 32, "self", 1, 1, True), (64, 2, 32, "self", 17, 17, True),
         (384, 4, 96, "self", 63, 63, False), (384, 4, 96, "self", 64, 64, True),
         (384, 4, 96, "source", 33, 63, False), (384, 4, 96, "source", 64, 15, False), (384, 4, 96, "source", 1, 33, False),
         (256, 2, 128, "self", 17, 17, True), (256, 2, 128, "self", 64, 64, False)]


def dctx_of(dy, w_o, H, dt, bf16=False, plant=None):
    """dctx[b, i, c] = sum_n dY[b, i, n] W_o[n, c]  (the data gradient of y = ctx W_o^T + b_o), (B, T1, D)."""
    D = w_o.shape[0]
    w = w_o.to(dt)
    if plant == "untransposed":
        w = w.t()
    if plant == "head+1":
        dk = D // H
        w = torch.roll(w, -dk, dims=1)              # head h reads columns (h + 1) dk ..
    y = dy.to(dt)
    if plant == "k_short":
        y, w = y[..., :D - 32], w[:D - 32]
    d = torch.matmul(y, w)
    return bf16_round(d) if bf16 else d


def proj_bwd(pmap, dy, w_o, v, k, q, scale, H, dt, dattn=None, keep=None, bf16=False, plant=None):
    """-> (dS, dq, dk, dv) of attn_kernels_ref.attn_bwd on dctx = dY . W_o."""
    return A.attn_bwd(pmap, dctx_of(dy, w_o, H, dt, bf16, plant), v, k, q, scale, H, dt, dattn=dattn, keep=keep, bf16=bf16)


def inputs(case):
    """The tensors of one case: those of attn_kernels_ref.plain_inputs (q, k, v, dattn, klen, scale; its dctx is not used), dy (B, T1, D)
    bf16 of unit scale and W_o (D, D) bf16 of scale 1 / sqrt(D), so that dctx has unit scale like the dctx of the attention cases."""
    D, H, dk, kind, T1, T2, causal = case
    seed = 5000 + 11 * CASES.index(case)
    inp = A.plain_inputs(T1, T2, dk, causal, seed, B=B_, H=H)
    inp["dy"] = R.randn(B_, T1, D, seed=seed + 5, dtype=BF16)
    inp["w_o"] = R.randn(D, D, seed=seed + 6, scale=D ** -0.5, dtype=BF16)
    return inp
