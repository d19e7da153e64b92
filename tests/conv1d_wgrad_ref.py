"""Plain torch-CPU restatement of the Conv1d weight gradient that csrc/conv1d_wgrad.hip computes, the shapes and inputs the host test and
the GPU cases share, and four planted errors.  Test infrastructure: it needs no GPU, imports nothing of seq2seq_vc_amd.ops, and the product
never imports it.

  dw[o][i][j] = pre[o][i][j] + sum_{b,t} dy[b,t,o] * x[b, t + j - pad, i],   pad = (ks - 1) / 2,

taps outside [0, T) of the same utterance counting as zero; dy (B, T, Cout) and x (B, T, Cin) channel-last, dw in torch's (Cout, Cin, ks).
`dt` = torch.float64 gives ref64 (bf16 inputs upcast exactly), torch.float32 the yard of tests/step_kernels_ref.py: compare.
tests/test_conv1d_wgrad_host.py pins the restatement, in float64, to torch.autograd of F.conv1d and shows that every plant breaks the
rule on every case's own inputs."""
import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

# (B, T, Cin, Cout, ks)
CASES = [
    (2, 37, 80, 256, 5),     # Cin tail of 16; an utterance edge inside a reduction step
    (2, 37, 256, 80, 5),     # Cout tail
    (3, 5, 16, 16, 5),       # T equal to ks
    (1, 3, 16, 32, 5),       # T below ks: some taps see nothing
    (2, 64, 64, 64, 5),      # whole blocks only
]
# T % 64 == 0 and a reduction long enough for the split-K plan of the launches the kernel replaces to cut it (11 K tiles in runs of 4 / 4 / 3,
# 14 in runs of 5 / 5 / 4 with two steps per utterance and a Cin tail; Cout > 64 and Cin >= 64 keep those launches on the tile kernel): the
# kernel sums in the same runs and keeps their bits
SPLIT_CASES = [
    (11, 64, 64, 80, 5),
    (7, 128, 80, 80, 5),
]
EDGE = {"normal": 100.0, "exact": 64.0}     # what the first and the last frame of every utterance carry, times the rest
PLANTS = ("flip", "pad", "edge", "layout")
SLACK_VALUE = 1.0                           # plant "edge": what lies in front of the first and behind the last row of the tensor


def name_of(c):
    return "B %d, T %d, Cin %d, Cout %d, ks %d" % c


def inputs(c, regime, salt=0):
    """-> dy (B, T, Cout) bf16, x (B, T, Cin) bf16, pre (Cout, Cin, ks) fp32, all on the CPU.  regime "normal": normal values; "exact":
    integers of magnitude <= 3 (pre: <= 7), so that every product and every partial sum is an integer below 2^24 (exact_ok).  The rows at
    the utterance edges carry EDGE[regime] times the rest: a tap that leaks across an edge moves the result by orders of magnitude more
    than the rule allows."""
    B, T, Cin, Cout, ks = c
    g = torch.Generator(device="cpu").manual_seed(1000 * (CASES + SPLIT_CASES).index(c) + 17 * salt + (1 if regime == "exact" else 2))
    if regime == "exact":
        dy = torch.randint(-3, 4, (B, T, Cout), generator=g).to(F32)
        x = torch.randint(-3, 4, (B, T, Cin), generator=g).to(F32)
        pre = torch.randint(-7, 8, (Cout, Cin, ks), generator=g).to(F32)
    else:
        dy = torch.randn(B, T, Cout, generator=g)
        x = torch.randn(B, T, Cin, generator=g)
        pre = torch.randn(Cout, Cin, ks, generator=g)
    for t in (dy, x):
        t[:, 0] *= EDGE[regime]
        if T > 1:
            t[:, T - 1] *= EDGE[regime]
    dy, x = dy.to(BF16), x.to(BF16)
    if regime == "exact":
        assert exact_ok(dy, x, pre), c
    return dy, x, pre


def exact_ok(dy, x, pre):
    """Every partial sum of every output stays an integer below 2^24 in magnitude: float32 (in any order) and float64 agree bit for bit."""
    ints = all(bool((t.to(F64) == t.to(F64).round()).all()) for t in (dy, x, pre))
    bound = torch.einsum("bo,bi->oi", dy.to(F64).abs().sum(1), x.to(F64).abs().amax(1))       # >= sum_{b,t} |dy| |x shifted|
    return ints and float(bound.max()) + float(pre.abs().max()) < 2.0 ** 24


def _shifted(x, sh, plant):
    """xs[b, t] = x[b, t + sh], zero where t + sh leaves [0, T).  plant "edge": the frames are read from the flat (B T) sequence
    instead -- the neighbouring utterance's, and SLACK_VALUE in front of the first and behind the last row."""
    B, T, C = x.shape
    if plant == "edge":
        flat = x.reshape(B * T, C)
        n = abs(sh)
        ext = torch.cat([torch.full((n, C), SLACK_VALUE, dtype=x.dtype), flat, torch.full((n, C), SLACK_VALUE, dtype=x.dtype)])
        return ext[n + sh:n + sh + B * T].reshape(B, T, C)
    xs = torch.zeros_like(x)
    lo, hi = max(0, -sh), min(T, T - sh)
    if hi > lo:
        xs[:, lo:hi] = x[:, lo + sh:hi + sh]
    return xs


def wgrad(dy, x, ks, dt, pre=None, plant=None):
    """-> (Cout, Cin, ks) in `dt`.  plant: None or one of PLANTS -- "flip": tap j takes tap ks - 1 - j's frames; "pad": pad + 1;
    "edge": see _shifted; "layout": the taps are stored (ks, Cin) per output channel instead of (Cin, ks)."""
    assert plant is None or plant in PLANTS
    dy, x = dy.to(dt), x.to(dt)
    Cout, Cin = dy.shape[2], x.shape[2]
    pad = (ks - 1) // 2 + (1 if plant == "pad" else 0)
    dw = torch.zeros(Cout, Cin, ks, dtype=dt)
    for j in range(ks):
        jj = ks - 1 - j if plant == "flip" else j
        dw[:, :, j] = torch.einsum("bto,bti->oi", dy, _shifted(x, jj - pad, plant))
    if plant == "layout":
        dw = dw.permute(0, 2, 1).contiguous().view(Cout, Cin, ks)
    return dw if pre is None else pre.to(dt) + dw
