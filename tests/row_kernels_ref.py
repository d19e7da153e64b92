"""Plain torch-CPU restatements of the row-wise and element-wise operations between the GEMMs (csrc/norm.hip: LayerNorm with residual,
dropout and hscale; csrc/sdp.hip: the ln_act family of the stochastic duration predictor; csrc/elementwise.hip: activation + dropout,
positional encoding, GLU, adds and casts; csrc/batchnorm.hip: the element-wise BatchNorm kernels), the case tables, the inputs and the
restated dispatch that tests/test_row_kernels_host.py and tests/gpu_row_kernel_check.py share.  Test infrastructure: it needs no GPU,
imports nothing of seq2seq_vc_amd, and the product never imports it.

Every restatement takes `dt` as tests/step_kernels_ref.py defines it: torch.float64 gives `ref64` (the truth on exactly the values the
kernel reads), torch.float32 the `yard`.  `store` is the dtype the kernel stores its tensors in: where a kernel documents a rounding of
an INTERMEDIATE to the storage type (LayerNorm takes its statistics of the stored s) both evaluations round there; the OUTPUTS are
rounded in the yard only.  Dropout is data: `keep` holds the keep-scales (0 or 1 / (1 - p)) of every element, in flat element order.

Three regimes: exact (integer / power-of-two inputs on which a float32 evaluation equals the float64 one, `exact_premise`: the kernel
must return those bits), rule (step_kernels_ref.compare, MARGIN 4) and route equality (two routes of one launcher, same bits)."""
import math

import torch

import step_kernels_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ACTS = (None, "relu", "tanh", "swish", "gelu", "sigmoid")
SAVED_IS_OUTPUT = ("relu", "tanh", "sigmoid")       # what act_dropout_bwd / bn_act_bwd_vec read: y = dropout(act(x)); else x
LN_EPS = 1e-12                                      # modules/transformer/layer_norm.py
TAILS = (0.0, 1e-30, 4.0, 10.0, 20.0, 60.0, 87.0, 89.0, 1e4)
GUARANTEE_FROM = 88.0                               # what swish / sigmoid return for |x| >= 88


def rnd(t, store, dt):
    """An output as the yard stores it (the truth is not rounded)."""
    return R.bf16_round(t) if (store == BF16 and dt == F32) else t


def name_of(dtype):
    return "fp32" if dtype == F32 else "bf16"


# ---------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------
def act(x, a):
    if a is None:
        return x
    if a == "relu":
        return torch.relu(x)
    if a == "tanh":
        return torch.tanh(x)
    if a == "swish":
        return x * torch.sigmoid(x)
    if a == "sigmoid":
        return torch.sigmoid(x)
    if a == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    raise ValueError(a)


def act_deriv(u, a):
    """act'(u) at the pre-activation u."""
    if a is None:
        return torch.ones_like(u)
    if a == "relu":
        return (u > 0).to(u.dtype)
    if a == "tanh":
        return 1.0 - torch.tanh(u) ** 2
    sg = torch.sigmoid(u)
    if a == "swish":
        return sg * (1.0 + u * (1.0 - sg))
    if a == "sigmoid":
        return sg * (1.0 - sg)
    if a == "gelu":
        return 0.5 * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0)))) + u * torch.exp(-0.5 * u * u) * (1.0 / math.sqrt(2.0 * math.pi))
    raise ValueError(a)


def act_deriv_saved(saved, keep, a, divide=True):
    """act' from what the forward pass saved: the dropped OUTPUT y = keep * act(x) for relu / tanh / sigmoid (act(x) = y / keep, 0 where
    dropped), the pre-activation for swish / gelu.  divide=False is the planted error (the derivative taken of the dropped output)."""
    if a in ("swish", "gelu") or a is None:
        return act_deriv(saved, a)
    if a == "relu":
        return (saved > 0).to(saved.dtype)
    y = saved
    if keep is not None and divide:
        y = torch.where(keep > 0, saved / torch.where(keep > 0, keep, torch.ones_like(keep)), torch.zeros_like(saved))
    return 1.0 - y * y if a == "tanh" else y * (1.0 - y)


def drop(v, keep):
    """v * keep where the element is kept, +0 where it is dropped (never the -0 a product with a negative value would give)."""
    if keep is None:
        return v
    k = keep.to(v.dtype)
    return torch.where(k > 0, v * k, torch.zeros_like(v)) + 0.0                 # (csrc/common.h drop_mul: an fma with +0, so a kept -0 leaves as +0 too)


def act_dropout_fwd(x, a, keep, dt, store=F32):
    return rnd(drop(act(x.to(dt), a), keep), store, dt)


def act_dropout_bwd(dz, saved, a, keep, dt, store=F32, divide=True):
    k = None if keep is None else keep.to(dt)
    g = dz.to(dt) * (1.0 if k is None else k) * act_deriv_saved(saved.to(dt), k, a, divide)
    return rnd(g if k is None else torch.where(k > 0, g, torch.zeros_like(g)), store, dt)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm with residual, dropout and hscale (csrc/norm.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def row_stats(s, eps, one_pass=False, skip_tail=0):
    """mean and rstd of every row, two-pass.  one_pass / skip_tail: planted errors (E[x^2] - mean^2; the last channels left out of the sums)."""
    D = s.shape[-1]
    t = s if not skip_tail else torch.cat([s[..., :D - skip_tail], torch.zeros_like(s[..., D - skip_tail:])], -1)
    mean = t.sum(-1, keepdim=True) / D
    if one_pass:
        var = (t * t).sum(-1, keepdim=True) / D - mean * mean
    else:
        dv = s - mean
        if skip_tail:
            dv = torch.cat([dv[..., :D - skip_tail], torch.zeros_like(dv[..., D - skip_tail:])], -1)
        var = (dv * dv).sum(-1, keepdim=True) / D
    return mean, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=s.dtype))


def ln_fwd(x, res, keep, hscale, gamma, beta, eps, dt, store=F32, one_pass=False, stats_before_rounding=False, skip_tail=0,
           hscale_after=False, gamma_shift=0):
    """s = res + hscale * keep * x (s = x without res), rounded to the storage type BEFORE the statistics; y = (s - mean) rstd gamma + beta.
    -> y, s, mean (rows), rstd (rows).  The keyword switches are the planted errors of the host test."""
    s = x.to(dt)
    if res is not None:
        if keep is not None:
            s = s * keep.to(dt)
        s = (s + res.to(dt)) * hscale if hscale_after else s * hscale + res.to(dt)
    st = s if (store != BF16 or res is None or stats_before_rounding) else R.bf16_round(s)
    mean, rstd = row_stats(st, eps, one_pass, skip_tail)
    g = gamma.to(dt)
    if gamma_shift:                                   # the last lane group reads gamma one channel off
        g = torch.cat([g[:-gamma_shift], g[-gamma_shift - 1:-1]])
    y = (st - mean) * rstd * g + beta.to(dt)
    return rnd(y, store, dt), (None if res is None else rnd(s, store, dt)), mean.squeeze(-1), rstd.squeeze(-1)


def ln_bwd(dy, s, mean, rstd, gamma, ds_extra, keep, hscale, dt, store=F32, no_keep_scale=False):
    """ds = rstd (g - mean(g) - xhat mean(g xhat)) + ds_extra, g = dy gamma; dh = ds keep hscale.  mean / rstd: inputs (rows).
    -> ds, dh, and the column sums of dy and dy * xhat (what the parameter gradients are)."""
    D = s.shape[-1]
    mu, rs = mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (s.to(dt) - mu) * rs
    g = dy.to(dt) * gamma.to(dt)
    a, b = g.sum(-1, keepdim=True) / D, (g * xh).sum(-1, keepdim=True) / D
    ds = rs * (g - a - xh * b)
    if ds_extra is not None:
        ds = ds + ds_extra.to(dt)
    k = torch.ones_like(ds) if keep is None else keep.to(dt)
    if no_keep_scale:
        k = (k > 0).to(dt)
    dh = torch.where(k > 0, ds * k * hscale, torch.zeros_like(ds)) + 0.0       # (the kernels' product ends in an fma with +0: no -0 leaves it)
    return rnd(ds, store, dt), rnd(dh, store, dt), dy.to(dt).sum(0), (dy.to(dt) * xh).sum(0)


def pg_eligible(dtype, rows, D):
    """s2svc_layernorm_bwd_pg_chunks on aligned tensors: 0 or the number of partial row pairs."""
    if dtype != BF16 or D > 2048 or D % 8 or rows < 2048 or rows * D < 1500000:
        return 0
    rpw = max(1, (rows + 2047) // 2048)
    return (rows + 8 * rpw - 1) // (8 * rpw)


# ---------------------------------------------------------------------------------------------------------------------------
# the ln_act family (csrc/sdp.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def row_valid(rows, T, lens):
    """(rows) bool: row b * T + t is valid when t < lens[b]."""
    if lens is None:
        return torch.ones(rows, dtype=torch.bool)
    r = torch.arange(rows)
    return (r % T) < torch.as_tensor(lens)[r // T]


def ln_act_fwd(x, gamma, beta, eps, a, res, lens, T, keep, dt, store=F32, zero_empty=True):
    """y = valid (res + keep act(LN(x))); -> y, mean, rstd.  zero_empty=False: planted error (an utterance without frames is not zeroed)."""
    xs = x.to(dt)
    mean, rstd = row_stats(xs, eps)
    o = drop(act((xs - mean) * rstd * gamma.to(dt) + beta.to(dt), a), keep)
    if res is not None:
        o = o + res.to(dt)
    ok = row_valid(x.shape[0], T, lens)
    if not zero_empty and lens is not None:
        ok = ok | (torch.as_tensor(lens)[torch.arange(x.shape[0]) // T] == 0)
    o = torch.where(ok[:, None], o, torch.zeros_like(o))
    return rnd(o, store, dt), mean.squeeze(-1), rstd.squeeze(-1)


def ln_act_bwd(dy, x, mean, rstd, gamma, beta, a, lens, T, keep, dt, store=F32):
    """du = valid dy keep act'(u) at u = xhat gamma + beta; dx = rstd (du gamma - mean(.) - xhat mean(. xhat)); dres = valid dy."""
    D = x.shape[-1]
    ok = row_valid(x.shape[0], T, lens)[:, None]
    d = torch.where(ok, dy.to(dt), torch.zeros(1, dtype=dt))
    mu, rs = mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (x.to(dt) - mu) * rs
    du = torch.where(ok, drop(d * act_deriv(xh * gamma.to(dt) + beta.to(dt), a), keep), torch.zeros(1, dtype=dt))
    dus = rnd(du, store, dt)
    g = du * gamma.to(dt)
    dx = rs * (g - g.sum(-1, keepdim=True) / D - xh * ((g * xh).sum(-1, keepdim=True) / D))
    return dus, rnd(dx, store, dt), rnd(d, store, dt)


def dwconv(x, w, b, ks, dil, dt):
    """Depthwise Conv1d over the T frames of every utterance, channel-last: u[b, t, c] = bias[c] + sum_j w[c, j] x[b, t + (j - pad) dil, c],
    the taps clipped to [0, T)."""
    B, T, D = x.shape
    pad = (ks - 1) // 2
    xs, u = x.to(dt), (torch.zeros(B, T, D, dtype=dt) if b is None else b.to(dt).expand(B, T, D).clone())
    for j in range(ks):
        sh = (j - pad) * dil
        lo, hi = max(0, -sh), min(T, T - sh)
        if hi > lo:
            u[:, lo:hi] += w.to(dt)[:, j] * xs[:, lo + sh:hi + sh]
    return u


def dw_ln_act_fwd(x, w, b, ks, dil, gamma, beta, eps, a, dt):
    """-> u = dwconv(x), y = act(LN(u)), mean, rstd (fp32 only)."""
    B, T, D = x.shape
    u = dwconv(x, w, b, ks, dil, dt)
    y, mean, rstd = ln_act_fwd(u.reshape(B * T, D), gamma, beta, eps, a, None, None, 0, None, dt)
    return u, y.reshape(B, T, D), mean, rstd


# ---------------------------------------------------------------------------------------------------------------------------
# positional encoding, GLU, BatchNorm (element-wise part), adds and casts
# ---------------------------------------------------------------------------------------------------------------------------
def posenc_fwd(x, xscale, alpha, pe, keep, dt, store=F32):
    """y = keep (x xscale + alpha pe[t]); alpha None: 1; pe None: no table."""
    B, T, D = x.shape
    y = x.to(dt) * torch.tensor(xscale, dtype=dt)
    if pe is not None:
        y = y + (1.0 if alpha is None else alpha.to(dt)) * pe[:T].to(dt)
    return rnd(drop(y, keep), store, dt)


def posenc_bwd(dy, xscale, pe, keep, dt, store=F32):
    """dx = dy keep xscale; dalpha = sum dy keep pe[t] (a tensor of one element; None without pe)."""
    B, T, D = dy.shape
    g = drop(dy.to(dt), keep)
    dalpha = None if pe is None else (g * pe[:T].to(dt)).sum().reshape(1)
    return rnd(g * torch.tensor(xscale, dtype=dt), store, dt), dalpha


def glu_fwd(x, dt, store=F32):
    C = x.shape[-1] // 2
    return rnd(x.to(dt)[..., :C] * torch.sigmoid(x.to(dt)[..., C:]), store, dt)


def glu_bwd(x, dy, dt, store=F32):
    C = x.shape[-1] // 2
    a, sg, d = x.to(dt)[..., :C], torch.sigmoid(x.to(dt)[..., C:]), dy.to(dt)
    return rnd(torch.cat([d * sg, d * a * sg * (1.0 - sg)], -1), store, dt)


def present(rows, Tn, vlens):
    return row_valid(rows, Tn, vlens)


def bn_apply(x, mean, rstd, gamma, beta, a, keep, vlens, Tn, dt, store=F32):
    """pre = (x - mean[c]) rstd[c] gamma[c] + beta[c]; y = keep act(pre); absent rows give +0 in both.  -> y, pre"""
    pre = (x.to(dt) - mean.to(dt)) * rstd.to(dt) * gamma.to(dt) + beta.to(dt)
    y = drop(act(pre, a), keep)                       # (the kernels apply the activation to the unrounded value)
    ok = present(x.shape[0], Tn, vlens)[:, None]
    z = torch.zeros(1, dtype=dt)
    return rnd(torch.where(ok, y, z), store, dt), rnd(torch.where(ok, pre, z), store, dt)


def bn_bwd(g, x, mean, rstd, gamma, sdy, sdyx, training, vlens, Tn, dt, store=F32):
    """dx = gamma rstd (g - sdy / N - xhat sdyx / N) over the N present rows (training); gamma rstd g (eval); absent rows +0."""
    ok = present(x.shape[0], Tn, vlens)
    n = int(ok.sum())
    gs = g.to(dt)
    if training:
        inv_n = torch.tensor(1.0, dtype=dt) / torch.tensor(float(n), dtype=dt)
        xh = (x.to(dt) - mean.to(dt)) * rstd.to(dt)
        v = gamma.to(dt) * rstd.to(dt) * (gs - sdy.to(dt) * inv_n - xh * sdyx.to(dt) * inv_n)
    else:
        v = gamma.to(dt) * rstd.to(dt) * gs
    return rnd(torch.where(ok[:, None], v, torch.zeros(1, dtype=dt)), store, dt)


def add_n(xs, store, pairwise=False):
    """The documented order ((x0 + x1) + x2) + x3 in float32, the result rounded to the storage type.  pairwise: the planted other order."""
    f = [t.to(F32) for t in xs]
    if pairwise and len(f) == 4:
        v = (f[0] + f[1]) + (f[2] + f[3])
    else:
        v = f[0] + f[1]
        for t in f[2:]:
            v = v + t
    return v.to(store)


def axpby(a, x, b, y, store):
    """float32(a) x (+ float32(b) y), each product rounded to float32 before the sum unless the sum is exact anyway (the cases use a, b that
    make every product exact: powers of two)."""
    v = torch.tensor(a, dtype=F32) * x.to(F32)
    if y is not None:
        v = v + torch.tensor(b, dtype=F32) * y.to(F32)
    return v.to(store)


def add_head_bias(q, u, v, store):
    return (q.to(F32) + u).to(store), (q.to(F32) + v).to(store)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def host_keep(shape, p, seed):
    """Keep-scales for the host test (on the card they are what the standalone dropout kernel draws)."""
    if not p:
        return None
    inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    return (torch.rand(shape, generator=R.gen(seed)) >= p).to(F32) * inv


def ints(*shape, seed, lo=-3, hi=3, dtype=F32):
    return torch.randint(lo, hi + 1, shape, generator=R.gen(seed)).to(dtype)


def pow2(*shape, seed, exps=(-1, 0, 1), signed=False):
    e = torch.tensor(exps, dtype=F32)[torch.randint(0, len(exps), shape, generator=R.gen(seed))]
    v = torch.exp2(e)
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=R.gen(seed + 1)).to(F32) * 2 - 1)
    return v


def exact_gamma_beta(D):
    """Odd gamma (1, 3 alternating, the sign changing every 3 channels) and even beta in [-4, 4]: gamma differs between neighbours, and
    +-gamma + beta is never 0 (a zero would carry the sign of a rounding the float64 evaluation has and the float32 one has not)."""
    c = torch.arange(D)
    gamma = (1.0 + 2.0 * (c % 2)) * (1.0 - 2.0 * ((c // 3) % 2))
    beta = 2.0 * (c % 5) - 4.0
    return gamma.to(F32), beta.to(F32)


def balanced_rows(rows, D, seed):
    """Every row holds D / 2 values +1 and D / 2 values -1, permuted per row: mean 0, variance 1 exactly."""
    assert D % 2 == 0
    base = torch.cat([torch.ones(D // 2), -torch.ones(D // 2)])
    return torch.stack([base[torch.randperm(D, generator=R.gen(seed + r))] for r in range(rows)])


def ln_fwd_exact_inputs(rows, D, dtype, with_res, keep, hscale, seed):
    """x (and res) for which s is a balanced +-1 row under the given keep-scales (0 or 2) and hscale (1 or 0.5): res integers in [-3, 3]
    (= s where the element is dropped), x = (s - res) / (hscale keep) where kept and 7 where dropped; all exact in bf16."""
    s = balanced_rows(rows, D, seed)
    gamma, beta = exact_gamma_beta(D)
    if not with_res:
        return dict(x=s.to(dtype), res=None, gamma=gamma, beta=beta, s=s)
    k = torch.ones(rows, D) if keep is None else keep.reshape(rows, D)
    res = torch.where(k > 0, ints(rows, D, seed=seed + 1000), s)
    x = torch.where(k > 0, (s - res) / (hscale * torch.where(k > 0, k, torch.ones_like(k))), torch.full_like(s, 7.0))
    return dict(x=x.to(dtype), res=res.to(dtype), gamma=gamma, beta=beta, s=s)


def row_offsets(rows):
    """+12, -18, +24, -30, +12, ...: the per-row constants of the offset inputs."""
    r = torch.arange(rows, dtype=F32)
    return (12.0 + 6.0 * (r % 4)) * (1.0 - 2.0 * (r % 2))


def ln_rule_inputs(rows, D, dtype, with_res, seed, offset=False):
    """N(0, 1) inputs; offset: every row sits at a constant of up to +-30 with scale 0.1 (|mean| / std > 100: a one-pass variance fails
    here).  With more than one row the LAST row is constant (variance 0): rstd = 1e6 and y = beta; a single row stays an ordinary one."""
    x = R.randn(rows, D, seed=seed)
    res = R.randn(rows, D, seed=seed + 1) if with_res else None
    if offset:
        x = x * 0.1 + row_offsets(rows)[:, None]
        res = None if res is None else res * 0.1
    if rows > 1:
        x[-1] = 1.5
        if res is not None:
            res[-1] = -0.5
    gamma, beta = 1.0 + R.randn(D, seed=seed + 2, scale=0.2), R.randn(D, seed=seed + 3, scale=0.2)
    return dict(x=x.to(dtype), res=None if res is None else res.to(dtype), gamma=gamma, beta=beta)


def ln_bwd_inputs(rows, D, dtype, seed, exact, offset=False):
    """dy, s, mean, rstd, gamma, ds_extra.  exact: integer dy in [-2, 2] and s in [-3, 3], integer mean, power-of-two rstd and gamma."""
    if exact:
        return dict(dy=ints(rows, D, seed=seed, lo=-2, hi=2, dtype=dtype), s=ints(rows, D, seed=seed + 1, dtype=dtype),
                    mean=ints(rows, seed=seed + 2, lo=-1, hi=1), rstd=pow2(rows, seed=seed + 3), gamma=pow2(D, seed=seed + 4, signed=True),
                    ds_extra=ints(rows, D, seed=seed + 6, dtype=dtype))
    s = R.randn(rows, D, seed=seed + 1)
    if offset:
        s = s * 0.1 + row_offsets(rows)[:, None]
    s = s.to(dtype)
    mean, rstd = row_stats(s.to(F64), LN_EPS)
    return dict(dy=R.randn(rows, D, seed=seed, dtype=dtype), s=s, mean=mean.squeeze(-1).to(F32), rstd=rstd.squeeze(-1).to(F32),
                gamma=1.0 + R.randn(D, seed=seed + 4, scale=0.2), ds_extra=R.randn(rows, D, seed=seed + 6, dtype=dtype))


def bn_bwd_exact_inputs(rows, C, dtype, seed):
    return dict(g=ints(rows, C, seed=seed, lo=-2, hi=2, dtype=dtype), x=ints(rows, C, seed=seed + 1, dtype=dtype), mean=ints(C, seed=seed + 2, lo=-1, hi=1),
                rstd=pow2(C, seed=seed + 3), gamma=pow2(C, seed=seed + 4, signed=True), sdy=ints(C, seed=seed + 5, lo=-8, hi=8),
                sdyx=ints(C, seed=seed + 6, lo=-8, hi=8))


def tails(dtype, n_pad=0):
    """Both signs of every TAILS value, rounded to dtype (+0 and -0 included), n_pad ordinary values behind them."""
    v = torch.tensor([s * t for t in TAILS for s in (1.0, -1.0)], dtype=F32)
    if n_pad:
        v = torch.cat([v, R.randn(n_pad, seed=77)])
    return v.to(dtype)


def exact_premise(fn, what=""):
    """fn(dt) -> tensors (None allowed).  Asserts that the float32 evaluation of the restatement equals the float64 one: no operation of
    the formula rounds in float32 on these inputs, so a kernel that evaluates it in any order, fused or not, must return these bits
    (rounded once to the storage type).  LayerNorm forward: 1 + eps rounds to 1 in float32 only, so the float64 values are compared after
    their rounding to float32 (they lie within 1e-11 of the integers the float32 evaluation gives).  -> the float64 tensors."""
    a32, a64 = fn(F32), fn(F64)
    for i, (u, v) in enumerate(zip(a32, a64)):
        if u is None:
            continue
        assert R.bits_equal(u, v.to(F32)), f"exact premise broken{what}: output {i}: {int((u != v.to(F32)).sum())} values"
    return a64


# ---------------------------------------------------------------------------------------------------------------------------
# the restated dispatch and the case tables
# ---------------------------------------------------------------------------------------------------------------------------
LN_THRESH = (512, 1024)            # D <= : the NV = 8 / 16 register kernels (1 / 2 16-byte groups); above: the loop (4 groups up to LN_VEC_MAX)
LN_VEC_MAX = 2048
LN_ACT_THRESH = (256, 512)         # D <= 256 and gelu: NV 4; D <= 512: NV 8; else NV 16 (D <= LN_ACT_MAX)
LN_ACT_MAX = 1024
DW_LN_ACT_THRESH = (256,)
DW_LN_ACT_MAX = 512
ROWS = (1, 5, 9)


def _tn(dtype):
    return "float" if dtype == F32 else "bf16_t"


def ln_vec_ok(dtype, D, aligned=True):
    return dtype == BF16 and D % 8 == 0 and D <= LN_VEC_MAX and aligned


def ln_fwd_route(dtype, D, aligned=True):
    if ln_vec_ok(dtype, D, aligned):
        return "ln_fwd_vec_kernel<%d>" % (1 if D <= LN_THRESH[0] else 2 if D <= LN_THRESH[1] else 4)
    if D <= LN_THRESH[0]:
        return "ln_fwd_reg_kernel<%s, 8>" % _tn(dtype)
    if D <= LN_THRESH[1]:
        return "ln_fwd_reg_kernel<%s, 16>" % _tn(dtype)
    return "ln_fwd_kernel<%s>" % _tn(dtype)


def ln_bwd_route(dtype, D, aligned=True):
    if ln_vec_ok(dtype, D, aligned):
        return "ln_bwd_vec_kernel<%d>" % (1 if D <= LN_THRESH[0] else 2 if D <= LN_THRESH[1] else 4)
    return "ln_bwd_kernel<%s>" % _tn(dtype)


def ln_bwd_pg_route(D):
    return "ln_bwd_vec_pg_kernel<%d>" % (1 if D <= LN_THRESH[0] else 2 if D <= LN_THRESH[1] else 4)


def ln_act_route(kernel, dtype, D, a):
    assert D <= LN_ACT_MAX
    if D <= LN_ACT_THRESH[0] and a == "gelu":
        return "%s<%s, 4, S2S_ACT_GELU>" % (kernel, _tn(dtype))
    if D <= LN_ACT_THRESH[1]:
        return "%s<%s, 8%s>" % (kernel, _tn(dtype), ", S2S_ACT_GELU" if a == "gelu" else "")
    return "%s<%s, 16>" % (kernel, _tn(dtype))


def dw_ln_act_route(D, a):
    assert D <= DW_LN_ACT_MAX
    if D <= DW_LN_ACT_THRESH[0] and a == "gelu":
        return "dw_ln_act_fwd_kernel<float, 4, S2S_ACT_GELU>"
    return "dw_ln_act_fwd_kernel<float, 8%s>" % (", S2S_ACT_GELU" if a == "gelu" else "")


# (dtype, D, aligned): the smallest shapes that reach every route and sit on both sides of every threshold
LN_CASES = ([(F32, D, True) for D in (1, 50, 64, 512, 520, 1024, 1032, 2056)]
            + [(BF16, D, True) for D in (8, 504, 512, 520, 1024, 1032, 2048, 50, 1004, 1030, 2056)]
            + [(BF16, 384, False)])
LN_MISALIGN_FWD = ("x", "res", "y", "s_out", "gamma", "beta")
LN_MISALIGN_BWD = ("dy", "s", "ds", "dh", "ds_extra", "gamma")
# rows x D of the backward pass that also writes the parameter gradients' partials, and shapes its eligibility test must decline
LN_PG_SHAPES = ((2931, 512), (2048, 736), (2049, 1032))
LN_PG_DECLINED = ((2047, 1032), (2048, 728), (2931, 516))      # too few rows; rows * D < 1.5 M; D % 8
LN_ACT_D = (1, 192, 256, 264, 512, 520, 1024)
LN_ACT_ACTS = ("gelu", "tanh")
LN_ACT_LENS = dict(B=3, T=3, lens=(3, 1, 0))                   # a full, a partial and an empty utterance: 9 rows
DW_D = (200, 256, 264, 512)
DW_KS_DIL = ((3, 1), (3, 27), (5, 2))
DW_T = (1, 5, 37)
EW_N = (1, 7, 8, 4099)
EW_BIG = 2048 * 256 + 8 + 3                                    # the first size at which a thread of the capped grid takes a second element
POSENC_SHAPES = ((3, 17, 32), (5, 409, 257))                   # the second: 525 565 elements, above the block cap
BN_SCALAR_SHAPES = ((1, 8), (65, 72), (257, 136))
BN_VEC_C = (8, 72, 520)
BN_VEC_ROWS = (1, 65)
MASKED = dict(B=3, Tn=21, vlens=(21, 0, 7))


def ln_routes_covered():
    """kernel instantiation -> the smallest case of the tables that reaches it (the route table of profiles/AB_LOG.md)."""
    out = {}
    for dtype, D, al in LN_CASES:
        out.setdefault(ln_fwd_route(dtype, D, al), f"layernorm_fwd {name_of(dtype)} D {D}" + ("" if al else " misaligned"))
        out.setdefault(ln_bwd_route(dtype, D, al), f"layernorm_bwd {name_of(dtype)} D {D}" + ("" if al else " misaligned"))
    for rows, D in LN_PG_SHAPES:
        out.setdefault(ln_bwd_pg_route(D), f"layernorm_bwd_pg {rows}x{D}")
    for dtype in (F32, BF16):
        for D in LN_ACT_D:
            for a in LN_ACT_ACTS:
                out.setdefault(ln_act_route("ln_act_fwd_kernel", dtype, D, a), f"ln_act {name_of(dtype)} D {D} {a}")
                out.setdefault(ln_act_route("ln_act_bwd_kernel", dtype, D, a), f"ln_act {name_of(dtype)} D {D} {a}")
    for D in DW_D:
        for a in LN_ACT_ACTS:
            out.setdefault(dw_ln_act_route(D, a), f"dw_ln_act D {D} {a}")
    return out
