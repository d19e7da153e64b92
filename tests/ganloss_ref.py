"""What the tests of the GAN losses, MultiAdamW and the fine-tuning step share: float64 restatements of the three losses (reference
urhythmic/vocoder.py:428-465) and of torch.optim.AdamW, the case tables, and checkers of the two host index models (the (pair, chunk)
prefix table of csrc/gan_loss.hip and the pointer table of csrc/adamw_multi.hip).  Plain torch on the CPU; nothing here is fitted to
what the kernels return."""
import torch

F32, F64 = torch.float32, torch.float64
KIND_ONE_MINUS_SQ, KIND_SQ = 0, 1
CHUNK = 8192                         # elements per workgroup of the loss kernels (the library states the same number)


# ---------------------------------------------------------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------------------------------------------------------
def feature_loss(pairs, dtype=F64):
    """-> ([mean(|r - g|) per pair], their sum) in `dtype`, evaluated on the tensors' own (fp32) values"""
    means = [torch.mean(torch.abs(r.to(dtype) - g.to(dtype))) for r, g in pairs]
    return means, sum(means)


def score_losses(entries, dtype=F64):
    """entries [(x, kind)] -> ([mean((1 - x)^2) or mean(x^2)], their sum)"""
    means = [torch.mean((1 - x.to(dtype)) ** 2) if kind == KIND_ONE_MINUS_SQ else torch.mean(x.to(dtype) ** 2) for x, kind in entries]
    return means, sum(means)


def score_grads(entries, upstream):
    """the float64 gradients 2 up (x - 1) / n and 2 up x / n"""
    return [2.0 * upstream * ((x.to(F64) - 1) if kind == KIND_ONE_MINUS_SQ else x.to(F64)) / x.numel() for x, kind in entries]


def ulp32(ref64):
    """spacing of float32 at |ref64| (elementwise, float64)"""
    a = ref64.detach().to(F64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def within_ulps(got32, ref64, n):
    """|got - ref64| <= n float32 ulp at the reference, elementwise -> (ok, worst distance in ulp)"""
    ref64 = ref64.detach().to(F64).cpu()
    err = (got32.detach().cpu().to(F64) - ref64).abs() / ulp32(ref64)
    return bool((err <= n).all()), float(err.max())


# numel of the hand-built feature pairs: 1, the wavefront edges, one chunk - 1 / exactly / + 1, two chunks + a tail
FEATURE_NUMELS = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
CHANNEL_LAST_SHAPES = ((2, 32, 7, 3), (2, 128, 5, 11), (2, 16, 33))        # (B, C, L, p) / (B, C, L) views of (B, L, p, C) / (B, L, C)


def seeded_pair(numel, seed, planted=3):
    """(r, g) fp32 with `planted` equal elements (the gradient there is a zero)"""
    gen = torch.Generator().manual_seed(seed)
    r, g = torch.randn(numel, generator=gen), torch.randn(numel, generator=gen)
    idx = torch.randperm(numel, generator=gen)[:min(planted, numel)]
    g[idx] = r[idx]
    return r, g, idx


# ---------------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------------
ADAMW_SIZES = (1, 3, 4, 5, 1023, 70001)
ADAMW_HYPER = dict(betas=(0.8, 0.99), eps=1e-8, weight_decay=1e-2)
ADAMW_LRS = (5e-5, 5e-5, 2e-5)       # the rate changes at step 3
ADAMW_NONE = (1, 3)                  # (step index, tensor index): that tensor has no gradient at step 2


def adamw_case(seed=11):
    """-> (params [fp32], grads [step][tensor or None]): seeded data gradients with exact zeros planted"""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=gen) for n in ADAMW_SIZES]
    grads = []
    for s in range(len(ADAMW_LRS)):
        row = []
        for i, n in enumerate(ADAMW_SIZES):
            g = 0.1 * torch.randn(n, generator=gen)
            g[torch.rand(n, generator=gen) < 0.1] = 0.0
            if n >= 4:
                g[1] = 0.0
            row.append(None if (s, i) == ADAMW_NONE else g)
        grads.append(row)
    return params, grads


def adamw(params, grads, lrs, betas, eps, weight_decay, dtype=F64):
    """torch.optim.AdamW's update written out, in `dtype`: -> (params, exp_avg, exp_avg_sq, steps) after len(grads) steps.  A tensor
    whose gradient is None at a step is skipped and its step count does not advance."""
    b1, b2 = betas
    p = [t.to(dtype).clone() for t in params]
    m, v, steps = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p], [0] * len(p)
    for row, lr in zip(grads, lrs):
        for i, g in enumerate(row):
            if g is None:
                continue
            g = g.to(dtype)
            steps[i] += 1
            p[i] = p[i] * (1 - lr * weight_decay)
            m[i] = m[i] + (1 - b1) * (g - m[i])
            v[i] = b2 * v[i] + (1 - b2) * g * g
            denom = v[i].sqrt() / (1 - b2 ** steps[i]) ** 0.5 + eps
            p[i] = p[i] - (lr / (1 - b1 ** steps[i])) * (m[i] / denom)
    return p, m, v, steps


def run_optimizer(make, params, grads, lrs, device="cpu", dtype=F32):
    """Step an optimiser built by make(parameter list) through the case -> (optimizer, parameters)"""
    ps = [torch.nn.Parameter(t.to(dtype).to(device).clone()) for t in params]
    opt = make(ps)
    for row, lr in zip(grads, lrs):
        for g_ in opt.param_groups:
            g_["lr"] = lr
        for p, g in zip(ps, row):
            p.grad = None if g is None else g.to(dtype).to(device).clone()
        opt.step()
    return opt, ps


# ---------------------------------------------------------------------------------------------------------------------------
# checkers of the host index models: each returns a list of complaints, empty when the table is right
# ---------------------------------------------------------------------------------------------------------------------------
def check_prefix_table(numels, prefix, chunk, locate, chunk_range):
    """Every element of every entry is walked by exactly one workgroup, and every workgroup of the grid belongs to an entry."""
    bad = []
    if len(prefix) != len(numels) + 1 or prefix[0] != 0:
        return [f"prefix has {len(prefix)} entries for {len(numels)} tensors or does not start at 0"]
    seen = [[0] * n for n in numels]
    for blk in range(prefix[-1]):
        e, c = locate(prefix, blk)
        lo, hi = chunk_range(numels[e], c, chunk)
        if not 0 <= lo < hi <= numels[e]:
            bad.append(f"workgroup {blk}: entry {e} chunk {c} walks [{lo}, {hi}) of {numels[e]} elements")
            continue
        for i in range(lo, hi):
            seen[e][i] += 1
    for e, s in enumerate(seen):
        wrong = [i for i, k in enumerate(s) if k != 1]
        if wrong:
            bad.append(f"entry {e}: {len(wrong)} of {len(s)} elements not walked exactly once, first {wrong[0]} ({s[wrong[0]]} times)")
    return bad


def check_adamw_table(numels, offsets, total, prefix, work):
    """Every element of every tensor's moment chunk is updated exactly once, vector accesses start 16-byte aligned, and nothing outside
    [offset, offset + numel) -- the gap before the neighbour, the neighbour itself -- is touched."""
    bad = []
    touched = [0] * total
    owner = [-1] * total
    for i, (o, n) in enumerate(zip(offsets, numels)):
        if o % 4:
            bad.append(f"tensor {i}: moment offset {o} is not 16-byte aligned")
        for j in range(o, min(o + n, total)):
            owner[j] = i
    if len(work) != prefix[-1]:
        bad.append(f"{len(work)} workgroups for a grid of {prefix[-1]}")
    for blk, (i, lo, hi, nvec, ntail) in enumerate(work):
        if not (prefix[i] <= blk < prefix[i + 1]):
            bad.append(f"workgroup {blk} works on tensor {i}, whose workgroups are [{prefix[i]}, {prefix[i + 1]})")
        if (offsets[i] + lo) % 4 and nvec:
            bad.append(f"workgroup {blk}: vector accesses from element {offsets[i] + lo}")
        if nvec + ntail != hi - lo:
            bad.append(f"workgroup {blk}: {nvec} + {ntail} elements for [{lo}, {hi})")
        for j in range(offsets[i] + lo, offsets[i] + lo + nvec + ntail):
            if j >= total or owner[j] != i:
                bad.append(f"workgroup {blk} of tensor {i} touches element {j}, which belongs to {'nobody' if j >= total or owner[j] < 0 else owner[j]}")
                break
            touched[j] += 1
    for j in range(total):
        if owner[j] >= 0 and touched[j] != 1:
            bad.append(f"element {j} of tensor {owner[j]} updated {touched[j]} times")
            break
    return bad
