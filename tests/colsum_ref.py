"""Restatements, case tables and inputs for the per-channel column sums of the training path: the two-stage reduction of
csrc/colsum.h as csrc/norm.hip (colreduce), csrc/batchnorm.hip (BatchNorm statistics, scalar and 16-byte) and csrc/convmod.hip (the
statistics inside the Conformer convolution module) use it.  Test infrastructure: it needs no GPU, imports nothing of seq2seq_vc_amd,
and the product never imports it.  tests/test_colsum_host.py pins it on the CPU, tests/gpu_colsum_check.py holds the kernels to it.

The scheme.  Stage 1 writes a pair of partial rows ws[chunk][2][C] per chunk of rows: wave w of a workgroup adds its rows one after
the other (rows r0 + w, r0 + w + 4, ...; in the 16-byte BatchNorm kernels a lane adds rows r0 + r8, r0 + r8 + 32, ... and the eight
lanes of a wave are joined by the xor-8 / 16 / 32 butterfly), the four waves are added as ((w0 + w1) + w2) + w3.  Stage 2 adds the
chunks in four strided groups (k = kg, kg + 4, ...) and the groups as ((g0 + g1) + g2) + g3.

Three regimes, in the manner of tests/gemm_kernels_ref.py:
  exact      non-zero integers in [-3, 3] (exact in bf16), integer `mean`, power-of-two `rstd`, scale 1, integer previous contents:
             every term and every partial sum is an integer below 2^24, float32 equals float64 in any order, and the kernel must
             return the float64 truth bit for bit (`exact_premise` asserts the premise on the tensors themselves);
  order pin  N(0, 1) inputs, outputs that are pure additions: `stage1_ordered` / `stage2_ordered` restate the order above in float32
             and the kernel must match bit for bit;
  rule       N(0, 1) inputs, every output under step_kernels_ref.compare: ref64 = the float64 restatement on the values the kernel
             reads, yard = stock torch in float32."""
import torch
import torch.nn.functional as F

import step_kernels_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
WS_CHUNKS = 64                 # partial rows a colreduce / bn_stats workspace holds (ops/kernels.py)
CR_MAX = 24                    # reductions per grouped launch (csrc/norm.hip: S2S_CR_MAX)

# ---- case tables: the smallest shapes at which each launcher can go wrong -------------------------------------------------
COLREDUCE_SHAPES = [(1, 8), (63, 40), (64, 64), (65, 72), (257, 136), (4097, 64)]    # the last: 64 chunks of 65 rows
COLREDUCE_VEC_SHAPES = [(5, 768), (300, 768), (5, 776), (300, 776)]                  # bf16, D >= 768, D % 8 == 0: 16-byte stage 1
COLREDUCE_MODES = (0, 1, 2, 3, 4, 5, 6)
MASKED_MODES = (0, 2, 3, 4, 6)
MASKED = dict(B=3, Tn=21, vlens=(21, 0, 7))                                          # 28 present rows, one empty utterance
MODE7_CHUNKS = (1, 3, 4, 5, 64)
BN_VEC_C = (8, 64, 72, 520)
BN_VEC_ROWS = (1, 63, 64, 65, 4100)                                                  # 4100 rows: 43 chunks of 96 rows
BN_SCALAR_SHAPES = [(1, 8), (65, 72), (257, 136)]
CONVMOD_SHAPES = [(1, 5, 64, 7, None), (2, 64, 64, 15, None), (3, 65, 128, 31, (65, 0, 33))]   # B, T, C, ks, vlens
RULE_SHAPES = [(63, 40), (65, 72), (257, 136), (300, 776)]                           # rows <= 300
HAS_DOT = {1, 2, 5, 6}


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def ints(*shape, seed, dtype=F32):
    """Seeded non-zero integers in [-3, 3]."""
    g = R.gen(seed)
    v = torch.randint(1, 4, shape, generator=g)
    return (v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).to(dtype)


def pow2(*shape, seed):
    """Seeded powers of two in {1, 2, 4}."""
    return torch.exp2(torch.randint(0, 3, shape, generator=R.gen(seed)).to(F32))


def colreduce_inputs(mode, rows, D, dtype, exact, seed=0):
    """-> dict(dy, x, mean, rstd) as s2svc_colreduce reads them in `mode` (None where it reads nothing)."""
    s = 1000 * mode + 7 * rows + D + seed
    mk = (lambda *sh, seed: ints(*sh, seed=seed, dtype=dtype)) if exact else (lambda *sh, seed: R.randn(*sh, seed=seed, dtype=dtype))
    per = rows if mode in (1, 5) else D
    d = dict(dy=None, x=None, mean=None, rstd=None)
    if mode not in (3, 6):
        d["dy"] = mk(rows, D, seed=s + 1)
    if mode not in (0, 5):
        d["x"] = mk(rows, D, seed=s + 2)
    if mode in (1, 2, 3, 5):
        d["mean"] = ints(per, seed=s + 3) if exact else R.randn(per, seed=s + 3, scale=0.3)
    if mode in (1, 2):
        d["rstd"] = pow2(per, seed=s + 4) if exact else R.randn(per, seed=s + 4, scale=0.2).abs() + 0.8
    return d


def colreduce_terms(mode, inp, dt):
    """The addends of the two sums of a column reduction (csrc/norm.hip, modes 0-6): (rows, D) tensors in `dt`; t1 is None in the
    modes that have one sum."""
    g = None if inp["dy"] is None else inp["dy"].to(dt)
    v = None if inp["x"] is None else inp["x"].to(dt)
    m = None if inp["mean"] is None else inp["mean"].to(dt)
    r = None if inp["rstd"] is None else inp["rstd"].to(dt)
    if mode == 0:
        return g, None
    if mode == 1:
        return g, g * (v - m[:, None]) * r[:, None]
    if mode == 2:
        return g, g * (v - m[None]) * r[None]
    if mode == 3:
        return (v - m[None]) ** 2, None
    if mode == 4:
        return g * v, None
    if mode == 5:
        return g, g * m[:, None]
    return v, v * v


def present(rows, Tn=0, vlens=None):
    """Row r = b * Tn + t is present when t < vlens[b] (csrc/common.h); vlens None: every row."""
    if vlens is None:
        return torch.ones(rows, dtype=torch.bool)
    r = torch.arange(rows)
    return (r % Tn) < torch.tensor(vlens)[r // Tn]


def present_ignoring_empty(rows, Tn, vlens):
    """PLANTED ERROR: a row mask that takes an empty utterance (vlens[b] = 0) for a full one."""
    return present(rows, Tn, tuple(v if v > 0 else Tn for v in vlens))


def n_present(rows, Tn=0, vlens=None):
    return rows if vlens is None else sum(min(max(v, 0), Tn) for v in vlens)


def colsum(terms, keep=None):
    """Plain sum over the present rows, in the dtype of `terms` (float64: the truth; float32: what stock torch gives)."""
    return (terms if keep is None else terms[keep]).sum(0)


def finish(total, scale, prev=None, dt=F32):
    """Stage 2's last step: out = (prev or 0) + total * scale, in `dt`."""
    out = total.to(dt) * torch.tensor(scale, dtype=dt)
    return out if prev is None else prev.to(dt) + out


def exact_premise(terms64):
    """The premise of the exact regime on one tensor of addends: -> (bound on every partial sum, float32 sum == float64 sum)."""
    bound = float(terms64.abs().sum(0).max())
    integral = bool((terms64 == terms64.round()).all())
    same = bool((terms64.to(F32).sum(0).to(F64) == terms64.sum(0)).all())
    return bound, integral and same


# ---- the documented order, in float32 -------------------------------------------------------------------------------------
def colreduce_chunks(rows, ws_chunks=WS_CHUNKS):
    """-> (chunks, rows per chunk) of s2svc_colreduce / s2svc_bn_stats: 64 rows per chunk until the workspace is full."""
    chunks = max(1, min((rows + 63) // 64, ws_chunks))
    return chunks, (rows + chunks - 1) // chunks


def bn_vec_chunks(rows):
    """-> (chunks, rows per chunk) of the 16-byte BatchNorm kernels: 64 rows, more (a multiple of 32) to stay within 64 chunks."""
    rpc = max(64, ((rows + 63) // 64 + 31) // 32 * 32)
    return (rows + rpc - 1) // rpc, rpc


def seq_sum(t):
    """((0 + t[0]) + t[1]) + ... along dim 0, in float32."""
    acc = torch.zeros(t.shape[1:], dtype=F32)
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def comb4(p, order=(0, 1, 2, 3)):
    return ((p[order[0]] + p[order[1]]) + p[order[2]]) + p[order[3]]


def stage1_ordered(terms, chunks, rpc, step=4, keep=None):
    """ws[chunk][C] of one of the two sums.  step 4: wave w adds rows r0 + w, r0 + w + 4, ... (colreduce, scalar and 16-byte);
    step 32: a lane adds rows r0 + r8, r0 + r8 + 32, ..., the eight lanes of wave w (r8 = 8 w + j) are joined by the xor-8 / 16 / 32
    butterfly ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) (the 16-byte BatchNorm kernels).  Absent rows are skipped."""
    terms = terms.to(F32)
    rows = terms.shape[0]
    keep = present(rows) if keep is None else keep
    ws = torch.zeros((chunks,) + tuple(terms.shape[1:]), dtype=F32)

    def lane(first, r1):
        idx = [r for r in range(first, r1, step) if keep[r]]
        return seq_sum(terms[idx])
    for k in range(chunks):
        r0, r1 = k * rpc, min(k * rpc + rpc, rows)
        if step == 4:
            waves = [lane(r0 + w, r1) for w in range(4)]
        else:
            a = [lane(r0 + r8, r1) for r8 in range(32)]
            waves = [((a[8 * w] + a[8 * w + 1]) + (a[8 * w + 2] + a[8 * w + 3])) + ((a[8 * w + 4] + a[8 * w + 5]) + (a[8 * w + 6] + a[8 * w + 7]))
                     for w in range(4)]
        ws[k] = comb4(waves)
    return ws


def stage2_ordered(ws, group_order=(0, 1, 2, 3), drop_last=False):
    """The four strided chunk groups and their combination.  group_order / drop_last: the PLANTED ERRORS (another order of the
    groups; a stage 2 that forgets the last chunk)."""
    ws = ws.to(F32)
    chunks = ws.shape[0] - (1 if drop_last else 0)
    return comb4([seq_sum(ws[kg:chunks:4]) for kg in range(4)], group_order)


def ordered_colsum(terms, chunks, rpc, step=4, keep=None, **planted):
    return stage2_ordered(stage1_ordered(terms, chunks, rpc, step, keep), **planted)


def chunked_colsum(terms, chunks, rpc, keep=None, drop_last=False):
    """Float64 sum by chunks (any order: float64 is the truth); drop_last: the PLANTED ERROR of a stage 2 that forgets a chunk."""
    rows = terms.shape[0]
    keep = present(rows) if keep is None else keep
    tot = torch.zeros(terms.shape[1:], dtype=F64)
    for k in range(chunks - (1 if drop_last else 0)):
        r0, r1 = k * rpc, min(k * rpc + rpc, rows)
        tot = tot + terms[r0:r1][keep[r0:r1]].to(F64).sum(0)
    return tot


# ---- torch.nn.BatchNorm1d's finalisation ------------------------------------------------------------------------------------
def bn_finalize(mean, var, n, eps, momentum, run_mean, run_var, dt, var_is_ex2, unbiased=True):
    """csrc/colsum.h bn_finalize_channel: biased variance (E[x^2] - mean^2 clamped at 0 when `var` holds E[x^2]) -> rstd, and the
    running statistics with the unbiased variance (n > 1).  -> (rstd, run_mean, run_var).  unbiased=False: the PLANTED ERROR."""
    m, v = mean.to(dt), var.to(dt)
    if var_is_ex2:
        v = (v - m * m).clamp_min(0)
    rstd = 1.0 / torch.sqrt(v + torch.tensor(eps, dtype=dt))
    unb = v * torch.tensor(n / (n - 1), dtype=dt) if (n > 1 and unbiased) else v
    mom = torch.tensor(momentum, dtype=dt)
    return rstd, (1 - mom) * run_mean.to(dt) + mom * m, (1 - mom) * run_var.to(dt) + mom * unb


def bn_stats64(x, eps, momentum, run_mean, run_var, keep=None):
    """The truth of a training-mode BatchNorm1d's statistics over the present rows of x (rows, C): -> (mean, rstd, run_mean, run_var)."""
    xs = (x if keep is None else x[keep]).to(F64)
    n = xs.shape[0]
    mean = xs.sum(0) / n
    rstd, rm, rv = bn_finalize(mean, ((xs - mean) ** 2).sum(0) / n, n, eps, momentum, run_mean, run_var, F64, False)
    return mean, rstd, rm, rv


def bn_stats_yard(x, eps, momentum, run_mean, run_var, keep=None):
    """The same by stock torch in float32 (F.batch_norm's running statistics, torch.var)."""
    xs = (x if keep is None else x[keep]).to(F32)
    rm, rv = run_mean.clone().to(F32), run_var.clone().to(F32)
    if xs.shape[0] > 1:
        F.batch_norm(xs, rm, rv, None, None, True, momentum, eps)
    else:                                    # F.batch_norm refuses one value per channel: its formula with the variance of one row (0)
        rm, rv = (1 - momentum) * rm + momentum * xs[0], (1 - momentum) * rv
    return xs.mean(0), 1.0 / torch.sqrt(xs.var(0, unbiased=False) + eps), rm, rv


# ---- the Conformer convolution module's statistics --------------------------------------------------------------------------
def convmod_exact_inputs(B, T, C, ks, seed):
    """y2 (B, T, 2C) bf16 = integer a | gate 30 (its sigmoid rounds to 1 in float32), a depthwise weight with a one-hot centre tap of 1
    and bias 0: z = dwconv(glu(y2)) = a exactly."""
    a = ints(B, T, C, seed=seed, dtype=BF16)
    y2 = torch.cat([a, torch.full((B, T, C), 30.0, dtype=BF16)], dim=-1)
    w = torch.zeros(C, 1, ks)
    w[:, 0, (ks - 1) // 2] = 1.0
    return y2, w, torch.zeros(C), a


def dswish(pre):
    s = torch.sigmoid(pre)
    return s * (1 + pre * (1 - s))


def convmod_bwd_stats(da, z, mean, rstd, gamma, beta, dt, keep=None):
    """csrc/convmod.hip convmod_bwd_stats: dpre = da * swish'(xhat * gamma + beta), xhat = (z - mean) * rstd;
    -> (sum dpre, sum dpre * xhat) over the present rows.  da, z: (rows, C)."""
    xh = (z.to(dt) - mean.to(dt)) * rstd.to(dt)
    d = da.to(dt) * dswish(xh * gamma.to(dt) + beta.to(dt))
    return colsum(d, keep), colsum(d * xh, keep)
