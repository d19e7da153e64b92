"""Plain torch-CPU restatement of the s2svc_gemm descriptor (include/s2svc_hip.h: operand addressing, epilogue order, row sums, row map),
the planted errors of the power check, and the problems -- operand buffers with their poison, inputs of both regimes -- that
tests/gpu_gemm_kernel_check.py and tests/test_gemm_kernels_host.py share.  Test infrastructure: it needs no GPU, imports nothing of
seq2seq_vc_amd.ops, and the product never imports it.  The comparison rule is the one of tests/step_kernels_ref.py.

`gemm_ref(p, dt)` works on what the kernel is handed: every operand is a FLAT buffer plus (offset, ld, layout, mode, C, T, pad, T1, F1, T2,
F2, bs0, bs1) exactly as s2svc_operand carries them, and element (r, k) is gathered from the address the header documents.  The buffers
are larger than the logical extents (ld > K, guard rows in front and behind) and the slack holds NaN -- the declared padding of a
`zero_padded` operand holds zeros -- so a restatement (or a kernel) that reads outside the logical extent shows a NaN in a sum.
dt = torch.float64 gives ref64, dt = torch.float32 the yard; neither rounds the output.

Two input regimes.  EXACT: operands are non-zero integers in [-3, 3], bias / residual / previous C integers in [-8, 8], alpha in {1, 0.5, 2}, act in
{none, relu}, dropout with p = 0.5 (keep-scale 2): `exact_bound(p) < 2^24` makes every partial sum in any order an exact fp32 value, so the
fp32 result must equal ref64 bit for bit and a bf16 result its bf16 rounding, whatever the K split, stage count or MFMA order.  REAL:
A ~ N(0, 1), B ~ N(0, 1) / sqrt(K), rounded to the input type; held to |got - ref64| <= 4 d + ulp_out(|ref64|) at every element,
d = max |yard - ref64| over the output.

Dropout enters as DATA: `keep` is the (M, N) tensor of 0 or 1 / (1 - p) the standalone dropout kernel draws for element index m N + n."""
import math
from types import SimpleNamespace as NS

import torch

import step_kernels_ref as R
from step_kernels_ref import BF16, F32, F64

KC, RC = 0, 1
DENSE, CONV1D, CONV2D_S2, TCONV2D_S2 = 0, 1, 2, 3
ACTS = ("none", "relu", "tanh", "swish", "sigmoid", "gelu")            # the act codes 0 .. 5 of s2svc_gemm_desc
NAN = float("nan")
SENT = -776.0                                                           # the sentinel of tests/gpu_step_kernel_check.py
BK = 64                                                                 # K tile of the LDS-DMA kernels (the unit of the K plants)

PLANTS = ("k_last_piece", "k_tile_first", "stage_wrap", "tap_across_utt", "tap_left_pad", "conv2d_f2_wrap", "tconv_class_swap", "bias_n+1",
          "alpha_after_bias", "res_before_act", "splitk_drops_remainder", "rowsum_last_row", "cmap_row_off_by_F1")


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def op_index(o, Rn, Kn, plant=None):
    """-> (element offsets relative to the operand pointer, validity), both (Rn, Kn): s2svc_operand as the header documents it."""
    r, k = torch.arange(Rn, dtype=torch.int64)[:, None], torch.arange(Kn, dtype=torch.int64)[None, :]
    one = torch.ones(Rn, Kn, dtype=torch.bool)
    if o.mode == DENSE:
        return ((r * o.ld + k) if o.layout == KC else (k * o.ld + r)).expand(Rn, Kn), one
    m, q = ((r, k) if o.layout == KC else (k, r))           # m: spatial index (b, t[, f]), q: implicit index tap * C + c
    m, q = m.expand(Rn, Kn), q.expand(Rn, Kn)
    tap, c = q // o.C, q % o.C
    if o.mode == CONV1D:                                     # taps j: x[(m + j - pad) ld + c], valid iff 0 <= t + j - pad < T
        tt = m % o.T + tap - o.pad
        lo, hi = tt >= 0, tt < o.T
        if plant == "tap_across_utt":
            hi = one
        if plant == "tap_left_pad":
            lo = one
        return (m + tap - o.pad) * o.ld + c, lo & hi
    if o.mode == CONV2D_S2:                                  # NHWC (B, T1, F1, C), 3 x 3, stride 2, no padding, m = (b, t2, f2)
        F2 = o.F2 + 1 if plant == "conv2d_f2_wrap" else o.F2
        f2, bt = m % F2, m // F2
        t2, b = bt % o.T2, bt // o.T2
        kh, kw = tap // 3, tap % 3
        return ((b * o.T1 + 2 * t2 + kh) * o.F1 + 2 * f2 + kw) * o.ld + c, one
    # TCONV2D_S2: one parity class (pt, pf), pad = 2 pt + pf; rows m = (b, i, j) over the class grid T1 x F1; tap = ta (2 - pf) + fb
    # reads pixel (i - ta, j - fb) of the (B, T2, F2, C) output gradient, zero outside
    pt, pf = o.pad >> 1, o.pad & 1
    if plant == "tconv_class_swap":
        pt, pf = pf, pt
    nf = 2 - pf
    per_b = o.T1 * o.F1
    b, rem = m // per_b, m % per_b
    i, j = rem // o.F1, rem % o.F1
    ta, fb = tap // nf, tap % nf
    ti, tj = i - ta, j - fb
    return ((b * o.T2 + ti) * o.F2 + tj) * o.ld + c, (ti >= 0) & (ti < o.T2) & (tj >= 0) & (tj < o.F2)


def expand(o, Rn, Kn, z0, z1, dt, plant=None):
    """The (Rn, Kn) matrix of batch (z0, z1) that the descriptor's operand stands for, gathered from its flat buffer."""
    idx, valid = op_index(o, Rn, Kn, plant)
    idx = idx + (o.off + z0 * o.bs0 + z1 * o.bs1)
    inside = (idx >= 0) & (idx < o.buf.numel())
    assert plant is not None or bool(inside[valid].all()), "the restatement itself reads outside an operand buffer"
    v = o.buf.to(dt)[idx.clamp(0, o.buf.numel() - 1)]
    return torch.where(valid & inside, v, torch.zeros((), dtype=dt))


def act_apply(v, act):
    if act == "relu":
        return torch.relu(v)
    if act == "tanh":
        return torch.tanh(v)
    if act == "swish":
        return v * torch.sigmoid(v)
    if act == "sigmoid":
        return torch.sigmoid(v)
    if act == "gelu":
        return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
    assert act in (None, "none"), act
    return v


def swish_grad(x):
    sg = torch.sigmoid(x)
    return sg * (1.0 + x * (1.0 - sg))


def c_rows(p, plant=None):
    """Row of C that GEMM row m is stored at: identity, or the c_map of a transposed-convolution class."""
    m = torch.arange(p.M, dtype=torch.int64)
    if p.c_map is None:
        return m
    T1, F1, Tc, Fc, pt, pf = p.c_map
    b, rem = m // (Tc * Fc), m % (Tc * Fc)
    i, j = rem // Fc, rem % Fc
    rows = (b * T1 + 2 * i + pt) * F1 + 2 * j + pf
    return rows + F1 if plant == "cmap_row_off_by_F1" else rows


def view2(x, nb0, nb1, rows, cols):
    """The logical (nb0, nb1, rows, cols) block of an output / residual buffer NS(buf, off, ld, bs0, bs1) (rows: count or index tensor)."""
    rr = torch.arange(rows, dtype=torch.int64) if isinstance(rows, int) else rows
    idx = (x.off + torch.arange(nb0)[:, None, None, None] * x.bs0 + torch.arange(nb1)[None, :, None, None] * x.bs1
           + rr[None, None, :, None] * x.ld + torch.arange(cols)[None, None, None, :])
    return x.buf[idx]


def gemm_ref(p, dt, keep=None, plant=None):
    """-> NS(C (nb0, nb1, M, N), c_pre or None, rowsum (M) or None, rows (M): the row of C each GEMM row goes to), all in dt, unrounded.
    Epilogue order: alpha A B^T + bias -> c_pre -> act -> dropout keep-scale, emask -> + res -> + previous C."""
    M, N, K = p.M, p.N, p.K
    kmask = torch.ones(K, dtype=torch.bool)
    if plant == "k_last_piece":
        kmask[K - (4 if p.dtype == F32 else 8):] = False
    if plant == "k_tile_first":
        assert K > BK
        kmask[BK] = False
    if plant == "stage_wrap":
        assert K > p.stages * BK
        kmask[p.stages * BK:(p.stages + 1) * BK] = False
    if plant == "splitk_drops_remainder":
        kt = (K + BK - 1) // BK
        assert p.splitk > 1 and kt % p.splitk
        kmask[(kt // p.splitk) * p.splitk * BK:] = False
    alpha = torch.tensor(R.f32(p.alpha), dtype=dt)
    bias = None if p.bias is None else p.bias.to(dt)
    if plant == "bias_n+1":
        bias = torch.roll(bias, -1)
    rows = c_rows(p, plant)
    C = torch.empty(p.nb0, p.nb1, M, N, dtype=dt)
    pre = torch.empty_like(C) if p.c_pre is not None else None
    res = None if p.res is None else view2(p.res, p.nb0, p.nb1, M, N).to(dt)
    prev = view2(p.Cbuf, p.nb0, p.nb1, rows, N).to(dt) if p.accumulate else None
    emask = None if p.emask is None else view2(p.emask, 1, 1, c_rows(p), N)[0, 0].to(dt)        # C's row layout: the mapped rows under a c_map
    rowsum = None
    for z0 in range(p.nb0):
        for z1 in range(p.nb1):
            A = expand(p.A, M, K, z0, z1, dt, plant) * kmask.to(dt)
            B = expand(p.B, N, K, z0, z1, dt, plant)
            acc = torch.matmul(A, B.transpose(0, 1))
            if p.a_rowsum is not None:
                rowsum = A.sum(dim=1)
                if plant == "rowsum_last_row":
                    rowsum[M - 1] = 0
                if p.a_rowsum_accumulate:
                    rowsum = rowsum + p.a_rowsum.buf[p.a_rowsum.off:p.a_rowsum.off + M].to(dt)
            if bias is None:
                v = alpha * acc
            else:
                v = alpha * (acc + bias) if plant == "alpha_after_bias" else alpha * acc + bias
            if pre is not None:
                pre[z0, z1] = v
            if plant == "res_before_act":
                v = v + res[z0, z1]
            v = act_apply(v, p.act)
            if p.drop_p > 0:
                v = v * keep.to(dt)
            if emask is not None:
                v = v * swish_grad(emask) if p.emask_mode == 1 else torch.where(emask > 0, v, torch.zeros((), dtype=dt))
            if res is not None and plant != "res_before_act":
                v = v + res[z0, z1]
            if prev is not None:
                v = v + prev[z0, z1]
            C[z0, z1] = v
    return NS(C=C, c_pre=pre, rowsum=rowsum, rows=rows)


def exact_bound(p):
    """max over (batch, m, n) of |alpha| sum_k |a| |b| + |bias| + |res| + |previous C| on the actual tensors (dropout's keep-scale 2 included):
    below 2^24 every partial sum of the exact regime, in any order, is an exact fp32 integer or half-integer."""
    worst = 0.0
    for z0 in range(p.nb0):
        for z1 in range(p.nb1):
            A, B = expand(p.A, p.M, p.K, z0, z1, F64).abs(), expand(p.B, p.N, p.K, z0, z1, F64).abs()
            v = abs(R.f32(p.alpha)) * torch.matmul(A, B.transpose(0, 1))
            if p.bias is not None:
                v = v + p.bias.to(F64).abs()
            if p.drop_p > 0:
                v = v / (1.0 - p.drop_p)
            if p.res is not None:
                v = v + view2(p.res, p.nb0, p.nb1, p.M, p.N)[z0, z1].to(F64).abs()
            if p.accumulate:
                v = v + view2(p.Cbuf, p.nb0, p.nb1, c_rows(p), p.N)[z0, z1].to(F64).abs()
            worst = max(worst, float(v.max()), float(A.sum(dim=1).max()) + (float(p.a_rowsum.buf.abs().max()) if p.a_rowsum is not None else 0.0))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# problems: buffers with poison, inputs of both regimes
# ---------------------------------------------------------------------------------------------------------------------------
def up(n, a):
    return (n + a - 1) // a * a


def _values(shape, regime, seed, dtype, scale=1.0, span=3, nonzero=False):
    if regime == "exact":
        v = torch.randint(-span, span + 1, shape, generator=R.gen(seed))
        if nonzero:                                            # operands: no zero factor, so that no dropped or foreign term goes unseen
            v = torch.where(v == 0, torch.randint(1, span + 1, shape, generator=R.gen(seed + 1000)), v)
        return v.to(dtype)
    return R.randn(*shape, seed=seed, scale=scale, dtype=dtype)


def _dense_op(vals, layout, zero_padded, misalign):
    """vals (nb0, nb1, Rn, Kn) -> operand: rows of ld > extent, one guard row (two when misaligned) in front of and behind every batch
    item, NaN in all the slack; zero_padded: zeros up to the next 16-byte multiple of the vectorised extent."""
    nb0, nb1, Rn, Kn = vals.shape
    mat = vals if layout == KC else vals.transpose(2, 3)
    rows, ext = mat.shape[2], mat.shape[3]
    vec = 16 // vals.element_size()
    ld = up(ext, vec) + 8 + (3 if misalign else 0)
    G = 2 if misalign else 1
    buf = torch.full((nb0, nb1, rows + 2 * G, ld), NAN, dtype=vals.dtype)
    sh = 1 if misalign else 0                                   # (the pointer one element past a 16-byte boundary)
    buf[:, :, G:G + rows, sh:sh + ext] = mat
    if zero_padded:
        buf[:, :, G:G + rows, sh + ext:sh + up(ext, vec)] = 0
    bs1 = (rows + 2 * G) * ld
    return NS(buf=buf.reshape(-1), off=G * ld + sh, ld=ld, layout=layout, mode=DENSE, C=0, T=0, pad=0, T1=0, F1=0, T2=0, F2=0,
              bs0=nb1 * bs1, bs1=bs1, zero_padded=1 if zero_padded else 0)


def _image_op(x, layout, mode, guard, **geo):
    """x (rows, C): the pixel / frame rows of a convolution input -> operand with ld = C + 8 and `guard` NaN rows in front and behind."""
    rows, C = x.shape
    ld = C + 8
    buf = torch.full((rows + 2 * guard, ld), NAN, dtype=x.dtype)
    buf[guard:guard + rows, :C] = x
    o = NS(buf=buf.reshape(-1), off=guard * ld, ld=ld, layout=layout, mode=mode, C=C, T=0, pad=0, T1=0, F1=0, T2=0, F2=0, bs0=0, bs1=0, zero_padded=0)
    o.__dict__.update(geo)
    return o


def _out_buf(nb0, nb1, rows, N, dtype, contiguous, fill=SENT, misalign=False):
    """An output / residual buffer: ld > N (ld = N where the descriptor demands a contiguous C), a guard row in front and behind each item."""
    ld = N if contiguous else up(N, 8) + 8 + (3 if misalign else 0)
    G = 2 if misalign else 1
    buf = torch.full((nb0, nb1, rows + 2 * G, ld), fill, dtype=dtype)
    bs1 = (rows + 2 * G) * ld
    return NS(buf=buf.reshape(-1), off=G * ld + (1 if misalign else 0), ld=ld, bs0=nb1 * bs1, bs1=bs1, rows=rows, N=N, nb0=nb0, nb1=nb1)


def _fill(x, vals):
    nb0, nb1, rows, N = vals.shape
    idx = (x.off + torch.arange(nb0)[:, None, None, None] * x.bs0 + torch.arange(nb1)[None, :, None, None] * x.bs1
           + torch.arange(rows)[None, None, :, None] * x.ld + torch.arange(N)[None, None, None, :])
    x.buf[idx] = vals


def outside_untouched(x, got_buf, rows=None):
    """True if the buffer that came back holds the sentinel bit for bit everywhere outside the logical block(s) of x (rows: mapped rows)."""
    rr = torch.arange(x.rows, dtype=torch.int64) if rows is None else rows
    idx = (x.off + torch.arange(x.nb0)[:, None, None, None] * x.bs0 + torch.arange(x.nb1)[None, :, None, None] * x.bs1
           + rr[None, None, :, None] * x.ld + torch.arange(x.N)[None, None, None, :])
    g = got_buf.detach().cpu().clone()
    g[idx.reshape(-1)] = SENT
    return R.bits_equal(g, torch.full_like(g, SENT))


_DEFAULTS = dict(dt="bf16", cdt=None, A=("dense", KC), B=("dense", KC), nb=(1, 1), alpha=1.0, bias=True, act="none", res=False, acc=False, c_pre=False,
                 emask=None, drop_p=0.0, rowsum=None, splitk=1, tile=0, p8=None, zero_padded=False, misalign=None, misalign_res=False,
                 conv=None, regimes=("exact", "real"), stages=3, shared_b=False)


def case(name, route, M, N, K, **kw):
    c = dict(_DEFAULTS, name=name, route=route, M=M, N=N, K=K)
    assert not set(kw) - set(_DEFAULTS), set(kw) - set(_DEFAULTS)
    c.update(kw)
    return NS(**c)


def _seed_of(c, regime):
    import zlib
    return zlib.crc32(f"{c.name}/{regime}".encode()) & 0x7FFFFFF


def problem(c, regime):
    """The problem of case c in one regime, entirely on the CPU: p.A / p.B (flat buffers + descriptor fields), p.Cbuf, p.res, p.emask, p.c_pre,
    p.a_rowsum, p.ws_floats and the scalar fields of s2svc_gemm_desc."""
    seed = _seed_of(c, regime)
    dtype = F32 if c.dt == "f32" else BF16
    cdt = dtype if c.cdt is None else (F32 if c.cdt == "f32" else BF16)
    M, N, K = c.M, c.N, c.K
    nb0, nb1 = c.nb
    p = NS(M=M, N=N, K=K, nb0=nb0, nb1=nb1, dtype=dtype, c_dtype=cdt, act=c.act, drop_p=c.drop_p, splitk=c.splitk, tile=c.tile, stages=c.stages,
           accumulate=c.acc, emask_mode=0 if c.emask is None else c.emask, c_map=None, name=c.name, regime=regime)
    alpha = c.alpha
    if regime == "exact":
        assert c.act in ("none", "relu") and c.alpha in (1.0, 0.5, 2.0) and c.drop_p in (0.0, 0.5) and c.emask != 1, c.name
    p.alpha = alpha
    wscale = 1.0 / math.sqrt(K)
    ops = []
    for which, (kind, layout), Rn, scale in (("A", c.A, M, 1.0), ("B", c.B, N, wscale)):
        s = seed + (1 if which == "A" else 2)
        mis = c.misalign in (which, "AB")
        if kind == "dense":
            shape = (1, 1, Rn, K) if (which == "B" and c.shared_b) else (nb0, nb1, Rn, K)
            o = _dense_op(_values(shape, regime, s, dtype, scale, nonzero=True), layout, c.zero_padded, mis)
            if which == "B" and c.shared_b:
                o.bs0 = o.bs1 = 0
        elif kind == "conv1d":
            Bu, T, ks, Cc = c.conv                                          # rows / reduction index (b, t); implicit index tap * C + c
            assert (Rn if layout == KC else K) == Bu * T and (K if layout == KC else Rn) == ks * Cc, c.name
            o = _image_op(_values((Bu * T, Cc), regime, s, dtype, scale, nonzero=True), layout, CONV1D, guard=ks // 2 + 1, T=T, pad=ks // 2)
        elif kind == "conv2d":
            Bu, T2, F2, Cc = c.conv
            T1, F1 = 2 * T2 + 1, 2 * F2 + 2                                 # (an even F1: the last input column is read by no output pixel)
            assert (Rn if layout == KC else K) == Bu * T2 * F2 and (K if layout == KC else Rn) == 9 * Cc, c.name
            o = _image_op(_values((Bu * T1 * F1, Cc), regime, s, dtype, scale, nonzero=True), layout, CONV2D_S2, guard=1, T1=T1, F1=F1, T2=T2, F2=F2)
        else:
            assert kind == "tconv2d" and which == "A" and layout == KC
            Bu, Tin, Fin, pt, pf, Oc = c.conv                               # the convolution's input is (Bu, Tin, Fin, .), its output (Bu, T2, F2, Oc)
            T2, F2 = (Tin - 3) // 2 + 1, (Fin - 3) // 2 + 1
            Tc, Fc = (Tin - pt + 1) // 2, (Fin - pf + 1) // 2
            assert M == Bu * Tc * Fc and K == (2 - pt) * (2 - pf) * Oc, (c.name, Bu * Tc * Fc, (2 - pt) * (2 - pf) * Oc)
            o = _image_op(_values((Bu * T2 * F2, Oc), regime, s, dtype, scale, nonzero=True), KC, TCONV2D_S2, guard=1, T1=Tc, F1=Fc, T2=T2, F2=F2, pad=2 * pt + pf)
            p.c_map = (Tin, Fin, Tc, Fc, pt, pf)
            p.c_rows_total = Bu * Tin * Fin
        ops.append(o)
    p.A, p.B = ops
    staged = c.drop_p > 0 or c.emask is not None
    bspan = 8
    p.bias = _values((N,), regime, seed + 3, F32, 0.5, bspan) if c.bias else None
    crow_total = p.c_rows_total if p.c_map is not None else M
    fill = SENT
    p.Cbuf = _out_buf(nb0, nb1, crow_total, N, cdt, contiguous=staged, fill=fill, misalign=c.misalign == "C")
    if c.acc:
        _fill(p.Cbuf, _values((nb0, nb1, crow_total, N), regime, seed + 4, cdt, 1.0, bspan))
    p.res = None
    if c.res:
        p.res = _out_buf(nb0, nb1, M, N, cdt, contiguous=False, fill=NAN, misalign=c.misalign_res)
        _fill(p.res, _values((nb0, nb1, M, N), regime, seed + 5, cdt, 1.0, bspan))
    p.emask = None
    if c.emask is not None:
        p.emask = _out_buf(1, 1, crow_total, N, cdt, contiguous=True, fill=NAN)
        _fill(p.emask, R.randn(1, 1, crow_total, N, seed=seed + 6, dtype=cdt))
    p.c_pre = _out_buf(nb0, nb1, M, N, cdt, contiguous=staged) if c.c_pre else None
    if p.c_pre is not None:                                                  # (the same ld and batch strides as C)
        assert (p.c_pre.ld, p.c_pre.bs0, p.c_pre.bs1) == (p.Cbuf.ld, p.Cbuf.bs0, p.Cbuf.bs1)
    p.a_rowsum, p.a_rowsum_accumulate = None, c.rowsum == "acc"
    if c.rowsum is not None:
        buf = torch.full((M + 16,), SENT, dtype=F32)
        if c.rowsum == "acc":
            buf[8:8 + M] = _values((M,), regime, seed + 7, F32, 1.0, bspan)
        p.a_rowsum = NS(buf=buf, off=8, ld=1, bs0=0, bs1=0, rows=M, N=1, nb0=1, nb1=1)
    p.ws_floats = c.splitk * nb0 * nb1 * M * N if c.splitk > 1 else 0
    return p


def host_keep(M, N, p_drop, seed):
    """A stand-in on the CPU for the dropout kernel's keep-scales (the host test has no device): 0 or 1 / (1 - p), fp32."""
    u = torch.rand(M, N, generator=R.gen(seed))
    return torch.where(u < p_drop, torch.zeros(()), torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p_drop, dtype=F32)))


def plants_of(c):
    """The planted errors that change what case c computes."""
    out = []
    akind, bkind = c.A[0], c.B[0]
    if c.K % BK:
        out.append("k_last_piece")
    if c.K > BK:
        out.append("k_tile_first")
    if c.K > c.stages * BK and c.route.startswith(("glds_dma", "glds_k2")):
        out.append("stage_wrap")
    if "conv1d" in (akind, bkind) and c.conv[2] > 1:
        out += ["tap_across_utt", "tap_left_pad"]
    if "conv2d" in (akind, bkind):
        out.append("conv2d_f2_wrap")
    if akind == "tconv2d":
        out.append("cmap_row_off_by_F1")
        if c.conv[3] != c.conv[4]:
            out.append("tconv_class_swap")
    if c.bias:
        out.append("bias_n+1")
        if c.alpha != 1.0:
            out.append("alpha_after_bias")
    if c.res and c.act != "none":
        out.append("res_before_act")
    if c.splitk > 1 and ((c.K + BK - 1) // BK) % c.splitk:
        out.append("splitk_drops_remainder")
    if c.rowsum is not None:
        out.append("rowsum_last_row")
    return out


def madds(c):
    return c.M * c.N * c.K * c.nb[0] * c.nb[1]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: (descriptor recipe, expected route).  Shapes are the smallest that reach the route through the dispatch of csrc/gemm.hip,
# gemm_skinny.hip, gemm_8ph.hip (s2svc_gemm_try_8ph), gemm_glds.hip (s2svc_gemm_try_glds) and gemm_fast.hip; the thresholds are the
# constexpr values of those files.  GROUPS maps a family to its cases: one family is one GPU test.
# ---------------------------------------------------------------------------------------------------------------------------
GROUPS = {}


def _add(group, name, route, M, N, K, **kw):
    c = case(f"{group}/{name}", route, M, N, K, **kw)
    assert all(c.name != o.name for g in GROUPS.values() for o in g), c.name
    GROUPS.setdefault(group, []).append(c)
    return c


_LAYOUTS = (("KC,KC", KC, KC), ("KC,RC", KC, RC), ("RC,KC", RC, KC), ("RC,RC", RC, RC))
_TR = {KC: "G_KC", RC: "G_TR"}


def _tables():
    # ---- skinny (M <= 64, dense K-contiguous operands, K % vector == 0): MT = ceil(M / 16); lean: MT <= 2 and the common epilogue
    for t, ks in (("bf16", (8, 40, 264, 520)), ("f32", (4, 20, 132, 260))):
        g = f"skinny_{t}"
        _add(g, "m1", f"skinny<{t},1,lean>", 1, 4, ks[0], dt=t)
        _add(g, "m17", f"skinny<{t},2,lean>", 17, 37, ks[1], dt=t, act="relu", res=True)
        _add(g, "m16_long", f"skinny<{t},1,lean>", 16, 100, ks[3], dt=t)
        _add(g, "m1_alpha", f"skinny<{t},1>", 1, 100, ks[2], dt=t, alpha=0.5)
        _add(g, "m17_acc32", f"skinny<{t},2>", 17, 4, ks[1], dt=t, cdt="f32", acc=True)             # fp32 accumulation of bf16 inputs
        _add(g, "m40", f"skinny<{t},3>", 40, 37, ks[2], dt=t, alpha=2.0, res=True)
        _add(g, "m64", f"skinny<{t},4>", 64, 100, ks[3], dt=t, act="relu")
        _add(g, "m49_k1", f"skinny<{t},4>", 49, 8, ks[0], dt=t, c_pre=True)
        _add(g, "m16_drop", f"skinny<{t},1,lean>+stage_pass", 16, 37, ks[1], dt=t, drop_p=0.5, act="relu")
        _add(g, "m33_mask", f"skinny<{t},3>+stage_pass", 33, 100, ks[0], dt=t, emask=0)
        _add(g, "m17_tanh", f"skinny<{t},2>", 17, 37, ks[2], dt=t, act="tanh", alpha=0.37, regimes=("real",))
    # ---- generic: what the fast paths refuse -- K no multiple of the vector without zero padding, a pointer off 16 bytes
    for t in ("f32", "bf16"):
        g = "generic"
        _add(g, f"{t}_k7", f"generic<{t},64,64>", 70, 37, 7, dt=t, res=True, act="relu")
        _add(g, f"{t}_k81", f"generic<{t},64,64>", 65, 64, 81, dt=t, alpha=0.5)
        _add(g, f"{t}_m63_k33", f"generic<{t},64,64>", 63, 65, 33, dt=t, A=("dense", RC), misalign="A")
        _add(g, f"{t}_misaligned", f"generic<{t},64,64>", 66, 8, 40, dt=t, misalign="B", acc=True)
        _add(g, f"{t}_rc_rc", f"generic<{t},64,64>", 64, 63, 81, dt=t, A=("dense", RC), B=("dense", RC), misalign="AB", rowsum="acc")
        _add(g, f"{t}_splitk", f"generic<{t},64,64>+splitk_reduce", 70, 37, 161, dt=t, splitk=2, rowsum="set", res=True)
        _add(g, f"{t}_splitk_mask", f"generic<{t},64,64>+splitk_reduce+stage_pass", 70, 40, 161, dt=t, splitk=3, emask=0)
        _add(g, f"{t}_drop", f"generic<{t},64,64>+stage_pass", 70, 37, 81, dt=t, drop_p=0.5, act="relu")
        _add(g, f"{t}_gelu", f"generic<{t},64,64>", 70, 37, 81, dt=t, act="gelu", alpha=0.37, regimes=("real",))
        _add(g, f"{t}_128", f"generic<{t},128,128>", 130, 130, 9, dt=t, nb=(12, 8), alpha=2.0)       # 384 tiles of 128 by batches
        _add(g, f"{t}_128_tail", f"generic<{t},128,128>", 129, 129, 33, dt=t, nb=(96, 1), B=("dense", RC), misalign="B")
    # ---- fast fp32: 64 x 64 x 64 (K < 128 or >= 128 tiles of 64 or row sums), 32 x 32 x 128, 128 x 128 x 32 (>= 256 tiles of 128);
    #      lean = dense operands and epilogue_common32_ok
    for ln, la, lb in _LAYOUTS:
        zp = dict(A=("dense", la), B=("dense", lb), zero_padded=True, dt="f32")
        al = dict(A=("dense", la), B=("dense", lb), dt="f32")
        _add("fast_f32", f"64_{ln}", f"fast<f32,64,64,64,{ln}>", 130, 70, 80, **zp, res=True)                        # N % 8: not lean
        _add("fast_f32", f"64_lean_{ln}", f"fast<f32,64,64,64,{ln},lean>", 132, 72, 84, **al, act="relu", res=True)
        _add("fast_f32", f"32_{ln}", f"fast<f32,32,32,128,{ln}>", 100, 72, 132, **al, alpha=0.5)
        _add("fast_f32", f"32_lean_{ln}", f"fast<f32,32,32,128,{ln},lean>", 100, 72, 260, **al, acc=True)
        _add("fast_f32", f"128_{ln}", f"fast<f32,128,128,32,{ln}>", 130, 130, 36, **zp, nb=(8, 8))
    _add("fast_f32", "32_m65", "fast<f32,32,32,128,KC,KC,lean>", 65, 8, 128, dt="f32")
    _add("fast_f32", "32_splitk", "fast<f32,32,32,128,KC,KC,lean>+splitk_reduce", 100, 72, 520, dt="f32", tile=32, splitk=2, acc=True, res=True)
    _add("fast_f32", "32_splitk3", "fast<f32,32,32,128,RC,RC,lean>+splitk_reduce", 96, 72, 650, dt="f32", tile=32, splitk=3, A=("dense", RC), B=("dense", RC),
         rowsum="acc")
    _add("fast_f32", "64_rowsum", "fast<f32,64,64,64,RC,RC,lean>", 132, 72, 264, dt="f32", A=("dense", RC), B=("dense", RC), rowsum="set", acc=True)
    _add("fast_f32", "64_splitk_mask", "fast<f32,64,64,64,KC,KC>+splitk_reduce+stage_pass", 130, 72, 200, dt="f32", splitk=2, emask=0, tile=64)
    _add("fast_f32", "64_drop", "fast<f32,64,64,64,KC,KC>", 130, 72, 80, dt="f32", drop_p=0.5, act="relu", res=True)
    _add("fast_f32", "64_conv1d", "fast<f32,64,64,64,KC,KC>", 66, 72, 36, dt="f32", A=("conv1d", KC), conv=(2, 33, 3, 12))
    _add("fast_f32", "64_conv2d", "fast<f32,64,64,64,KC,KC>", 130, 40, 108, dt="f32", A=("conv2d", KC), conv=(1, 2, 65, 12))
    _add("fast_f32", "64_sigmoid", "fast<f32,64,64,64,KC,KC>", 130, 72, 80, dt="f32", act="sigmoid", alpha=0.37, c_pre=True, regimes=("real",))
    _add("fast_f32", "32_swish_mask", "fast<f32,32,32,128,KC,KC>", 100, 72, 132, dt="f32", emask=1, drop_p=0.5, regimes=("real",))
    # ---- fast bf16: what the LDS-DMA family declines -- a conv operand with C % 8 == 0 and C < 64, tile_hint 32
    _add("fast_bf16", "conv1d_c24", "fast<bf16,64,64,128,KC,KC>", 66, 72, 72, A=("conv1d", KC), conv=(2, 33, 3, 24), res=True, act="relu")
    _add("fast_bf16", "conv1d_c24_t5", "fast<bf16,64,64,128,KC,KC>", 65, 64, 120, A=("conv1d", KC), conv=(13, 5, 5, 24))
    _add("fast_bf16", "conv1d_c24_wgrad", "fast<bf16,64,64,128,RC,RC>", 72, 72, 66, A=("dense", RC), B=("conv1d", RC), conv=(2, 33, 3, 24), cdt="f32", rowsum="set")
    _add("fast_bf16", "conv2d_c24", "fast<bf16,64,64,128,KC,KC>", 130, 40, 216, A=("conv2d", KC), conv=(1, 2, 65, 24))
    _add("fast_bf16", "conv1d_c24_128", "fast<bf16,128,128,64,KC,KC>", 130, 136, 72, A=("conv1d", KC), conv=(2, 65, 3, 24), tile=128)
    for ln, la, lb in _LAYOUTS:
        zp = dict(A=("dense", la), B=("dense", lb), zero_padded=True, tile=32)
        _add("fast_bf16", f"64_{ln}", f"fast<bf16,64,64,128,{ln}>", 100, 70, 136, **zp, alpha=0.5)
        _add("fast_bf16", f"128_{ln}", f"fast<bf16,128,128,64,{ln}>", 130, 130, 72, **zp, nb=(8, 8))
    _add("fast_bf16", "64_k1tile", "fast<bf16,64,64,128,KC,KC>", 65, 8, 128, tile=32)
    _add("fast_bf16", "64_splitk", "fast<bf16,64,64,128,KC,KC>+splitk_reduce", 100, 72, 648, tile=32, splitk=2, res=True, act="relu")
    # ---- LDS-DMA, 32 x 64 tiles (dense K-contiguous operands, M > 64, < 256 tiles of 64): 3 stages, the two-half k2 split from 12 K tiles
    #      on (lean epilogue, one problem), 5 stages from 16 K tiles per split on
    g = "glds_bm32"
    for K in (64, 72, 128, 192, 256, 320):                                                                               # 1 - 5 K tiles around the 3-stage depth
        _add(g, f"lean_k{K}", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 100, 72, K, act="relu", res=True)
    _add(g, "lean_m65_n8", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 65, 8, 136)
    _add(g, "lean_m95_n64", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 95, 64, 200)
    _add(g, "lean_m97_n65x", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 97, 136, 704, act="relu")                  # 11 K tiles: the last before k2
    _add(g, "lean_drop", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 100, 72, 136, drop_p=0.5, act="relu", res=True)
    _add(g, "lean_mask", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 100, 72, 136, emask=0, res=True)
    _add(g, "alpha", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 72, 136, alpha=0.5)
    _add(g, "c_f32", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 72, 64, cdt="f32", res=True)
    _add(g, "c_pre", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 72, 128, c_pre=True, act="relu")
    _add(g, "acc", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 72, 192, acc=True)
    _add(g, "n70", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 70, 256, res=True)
    _add(g, "res_unaligned", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 72, 136, res=True, misalign_res=True)
    _add(g, "tanh", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 72, 136, act="tanh", alpha=0.37, regimes=("real",))
    _add(g, "swish_mask", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 100, 72, 136, emask=1, drop_p=0.5, regimes=("real",))
    _add(g, "batched", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>", 65, 45, 96, nb=(3, 2), zero_padded=True)
    _add(g, "splitk3", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>+splitk_reduce", 100, 72, 264, splitk=3, res=True, act="relu")    # 5 K tiles over 3 splits
    _add(g, "splitk2_drop", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,3>+splitk_reduce+stage_pass", 100, 72, 200, splitk=2, drop_p=0.5)
    for K in (768, 776, 832, 1088):                                                                                      # 12, 13 (ragged), 13, 17 K tiles
        _add(g, f"k2_k{K}", "glds_k2<32,64,3>", 100, 72, K, act="relu", res=True, stages=3)
    _add(g, "k2_m65_n136", "glds_k2<32,64,3>", 65, 136, 840, drop_p=0.5)
    for K in (1024, 1088, 1096):                                                                                         # 16, 17, 18 (ragged) K tiles
        _add(g, f"deep_k{K}", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,5>", 100, 72, K, alpha=0.5, stages=5)
    _add(g, "deep_batched", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,5>", 65, 64, 1024, nb=(1, 2), stages=5)
    for K in (2048, 2112):                                                                                               # 32, 33 K tiles over two splits
        _add(g, f"deep_splitk_k{K}", "glds_dma<32,64,G_KC_DENSE,G_KC_DENSE,5>+splitk_reduce", 100, 72, K, splitk=2, stages=5, res=True)
    # ---- LDS-DMA, 64 x 64 tiles, all-DMA operand pairs (3-stage ring)
    g = "glds_dma64"
    _add(g, "lean_m40_k84", "glds_dma<64,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 40, 72, 84, zero_padded=True, act="relu", res=True)
    _add(g, "lean_289_tiles", "glds_dma<64,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 1030, 1032, 72)
    _add(g, "lean_k4tiles", "glds_dma<64,64,G_KC_DENSE,G_KC_DENSE,3,lean>", 63, 64, 260, zero_padded=True)
    _add(g, "m40_alpha", "glds_dma<64,64,G_KC_DENSE,G_KC_DENSE,3>", 40, 72, 84, zero_padded=True, alpha=2.0)
    _add(g, "attn_qk", "glds_dma<64,64,G_KC_DENSE,G_KC_DENSE,3>", 37, 45, 96, nb=(3, 2), alpha=0.5, bias=False)          # the attention shapes: T1 37, T2 45, dk 96
    _add(g, "m64_splitk", "glds_dma<64,64,G_KC_DENSE,G_KC_DENSE,3>+splitk_reduce", 64, 65, 328, splitk=2, zero_padded=True)
    for nm, cv in (("t5_k5_c64", (13, 5, 5, 64)), ("t33_k3_c72", (3, 33, 3, 72)), ("t96_k1_c64", (2, 96, 1, 64)), ("t96_k5_c72", (2, 96, 5, 72)),
                   ("t33_k5_c64", (2, 33, 5, 64))):
        _add(g, f"conv1d_{nm}", "glds_dma<64,64,G_KC_CONV1D,G_KC_DENSE,3>", cv[0] * cv[1], 72, cv[2] * cv[3], A=("conv1d", KC), conv=cv, act="relu", res=True)
    _add(g, "conv2d_c64", "glds_dma<64,64,G_KC_CONV2D,G_KC_DENSE,3>", 130, 72, 576, A=("conv2d", KC), conv=(1, 2, 65, 64), act="relu")
    _add(g, "conv2d_c72", "glds_dma<64,64,G_KC_CONV2D,G_KC_DENSE,3>", 132, 64, 648, A=("conv2d", KC), conv=(2, 2, 33, 72))
    _add(g, "conv2d_splitk", "glds_dma<64,64,G_KC_CONV2D,G_KC_DENSE,3>+splitk_reduce", 140, 72, 576, A=("conv2d", KC), conv=(2, 2, 35, 64), splitk=2)   # 9 K tiles: the second split starts inside tap row 1
    for pt, pf, tin, fin in ((0, 0, 9, 12), (0, 1, 9, 12), (1, 0, 9, 12), (1, 1, 9, 12), (0, 0, 10, 11), (1, 1, 10, 11)):
        Tc, Fc = (tin - pt + 1) // 2, (fin - pf + 1) // 2
        _add(g, f"tconv_{pt}{pf}_{tin}x{fin}", "glds_dma<64,64,G_KC_TCONV2D,G_KC_DENSE,3>", 2 * Tc * Fc, 64, (2 - pt) * (2 - pf) * 64, A=("tconv2d", KC),
             conv=(2, tin, fin, pt, pf, 64), bias=False, emask=0 if (pt + pf) % 2 == 0 else None)
    # ---- LDS-DMA family, register-staged kernels (gemm_glds_kernel): row sums, transpose-read operands, 128 x 128 tiles
    g = "glds_64"
    _add(g, "kc_kc_rowsum", "glds<64,64,G_KC_DENSE,G_KC_DENSE>", 100, 72, 136, rowsum="set")
    _add(g, "conv1d_rowsum", "glds<64,64,G_KC_CONV1D,G_KC_DENSE>", 99, 72, 192, A=("conv1d", KC), conv=(3, 33, 3, 64), rowsum="acc")
    _add(g, "conv2d_rowsum", "glds<64,64,G_KC_CONV2D,G_KC_DENSE>", 130, 72, 576, A=("conv2d", KC), conv=(1, 2, 65, 64), rowsum="set")
    _add(g, "wgrad", "glds<64,64,G_TR_DENSE,G_TR_DENSE>", 104, 72, 130, A=("dense", RC), B=("dense", RC), cdt="f32", acc=True, rowsum="acc")
    _add(g, "wgrad_ragged", "glds<64,64,G_TR_DENSE,G_TR_DENSE>", 65, 63, 200, A=("dense", RC), B=("dense", RC), zero_padded=True, cdt="f32")
    _add(g, "wgrad_splitk3", "glds<64,64,G_TR_DENSE,G_TR_DENSE>+splitk_reduce", 104, 72, 264, A=("dense", RC), B=("dense", RC), cdt="f32", splitk=3, rowsum="set")
    _add(g, "wgrad_splitk2", "glds<64,64,G_TR_DENSE,G_TR_DENSE>+splitk_reduce", 72, 136, 200, A=("dense", RC), B=("dense", RC), cdt="f32", splitk=2, acc=True)
    _add(g, "dgrad", "glds<64,64,G_KC_DENSE,G_TR_DENSE>", 100, 72, 136, B=("dense", RC), emask=0, drop_p=0.5)
    _add(g, "attn_pv", "glds<64,64,G_KC_DENSE,G_TR_DENSE>", 37, 96, 45, nb=(3, 2), B=("dense", RC), zero_padded=True, bias=False)
    _add(g, "tr_kc", "glds<64,64,G_TR_DENSE,G_KC_DENSE>", 104, 72, 136, A=("dense", RC), res=True)
    _add(g, "attn_dk", "glds<64,64,G_TR_DENSE,G_KC_DENSE>", 45, 96, 37, nb=(3, 2), A=("dense", RC), zero_padded=True, bias=False, alpha=0.5)
    _add(g, "conv1d_dgrad", "glds<64,64,G_KC_CONV1D,G_TR_DENSE>", 99, 72, 192, A=("conv1d", KC), B=("dense", RC), conv=(3, 33, 3, 64))
    _add(g, "conv1d_wgrad", "glds<64,64,G_TR_DENSE,G_TR_CONV1D>", 72, 192, 99, A=("dense", RC), B=("conv1d", RC), conv=(3, 33, 3, 64), cdt="f32", rowsum="set")
    _add(g, "conv1d_wgrad_t5", "glds<64,64,G_TR_DENSE,G_TR_CONV1D>", 64, 360, 65, A=("dense", RC), B=("conv1d", RC), conv=(13, 5, 5, 72), cdt="f32", acc=True)
    _add(g, "conv2d_wgrad", "glds<64,64,G_TR_DENSE,G_TR_CONV2D>", 72, 576, 130, A=("dense", RC), B=("conv2d", RC), conv=(1, 2, 65, 64), cdt="f32")
    g = "glds_128"
    _add(g, "kc_kc", "glds<128,128,G_KC_DENSE,G_KC_DENSE>", 130, 136, 136, tile=128, act="relu", res=True)
    _add(g, "kc_kc_tail", "glds<128,128,G_KC_DENSE,G_KC_DENSE>", 127, 129, 72, tile=128, zero_padded=True, nb=(2, 1))
    _add(g, "conv1d", "glds<128,128,G_KC_CONV1D,G_KC_DENSE>", 192, 72, 360, A=("conv1d", KC), conv=(2, 96, 5, 72), tile=128)
    _add(g, "conv2d", "glds<128,128,G_KC_CONV2D,G_KC_DENSE>", 130, 72, 648, A=("conv2d", KC), conv=(1, 2, 65, 72), tile=128)
    _add(g, "tconv", "glds<128,128,G_KC_TCONV2D,G_KC_DENSE>", 50, 64, 128, A=("tconv2d", KC), conv=(2, 10, 11, 0, 1, 64), tile=128, bias=False, emask=0)
    _add(g, "wgrad", "glds<128,128,G_TR_DENSE,G_TR_DENSE>", 136, 130, 200, A=("dense", RC), B=("dense", RC), tile=128, zero_padded=True, cdt="f32", rowsum="set")
    _add(g, "dgrad", "glds<128,128,G_KC_DENSE,G_TR_DENSE>", 130, 136, 72, B=("dense", RC), tile=128)
    _add(g, "tr_kc", "glds<128,128,G_TR_DENSE,G_KC_DENSE>", 136, 130, 72, A=("dense", RC), tile=128, splitk=1)
    _add(g, "conv1d_dgrad", "glds<128,128,G_KC_CONV1D,G_TR_DENSE>", 99, 136, 192, A=("conv1d", KC), B=("dense", RC), conv=(3, 33, 3, 64), tile=128)
    _add(g, "conv1d_wgrad", "glds<128,128,G_TR_DENSE,G_TR_CONV1D>", 136, 192, 99, A=("dense", RC), B=("conv1d", RC), conv=(3, 33, 3, 64), tile=128, cdt="f32")
    _add(g, "conv2d_wgrad", "glds<128,128,G_TR_DENSE,G_TR_CONV2D>", 136, 576, 130, A=("dense", RC), B=("conv2d", RC), conv=(1, 2, 65, 64), tile=128, cdt="f32",
         splitk=1)
    # ---- the 8-wave kernels: s2svc_gemm_set_8ph forces a geometry on small eligible problems (p8 = mode | geo << 4 | (1 + n96 mode) << 8)
    g = "p8_dense"
    for geo, k in ((1, "8ph_q<DENSE,2,4"), (2, "8ph_q<DENSE,4,2"), (3, "8ph_128<DENSE")):
        M, N = ((256, 264), (520, 136), (300, 64))[geo - 1]
        _add(g, f"lean_geo{geo}", f"{k},lean>", M, N, 192, p8=1 | geo << 4, act="relu", res=True)
        _add(g, f"lean_drop_geo{geo}", f"{k},lean>", 300, 136, 128, p8=1 | geo << 4, drop_p=0.5, emask=0)
        _add(g, f"skew_geo{geo}", f"{k},skew>", M, N, 128, p8=1 | geo << 4, alpha=0.5, nb=(2, 1))
        _add(g, f"skew_f32_geo{geo}", f"{k},skew>", 300, 136, 192, p8=1 | geo << 4, cdt="f32", acc=True)
        _add(g, f"noskew_geo{geo}", f"{k},noskew>", M, N, 192, p8=2 | geo << 4, act="relu", res=True)
    _add(g, "n96_2", "8ph_n96<2>", 300, 192, 128, p8=1 | (1 + 4) << 8, act="relu", res=True)
    _add(g, "n96_3", "8ph_n96<3>", 256, 288, 192, p8=1 | (1 + 5) << 8, drop_p=0.5)
    _add(g, "swish_fwd", "8ph_128<DENSE,swish>", 300, 136, 128, p8=1 | 3 << 4, act="swish", c_pre=True, drop_p=0.5, regimes=("real",))
    _add(g, "swish_bwd", "8ph_128<DENSE,swish>", 300, 136, 192, p8=1 | 3 << 4, emask=1, drop_p=0.5, bias=False, regimes=("real",))
    g = "p8_conv"
    for geo, k in ((1, "8ph_q<CONV2D,2,4"), (2, "8ph_q<CONV2D,4,2"), (3, "8ph_128<CONV2D")):
        _add(g, f"conv2d_skew_geo{geo}", f"{k},skew>", 260, (264, 136, 64)[geo - 1], 576, A=("conv2d", KC), conv=(2, 2, 65, 64), p8=1 | geo << 4, act="relu")
        _add(g, f"conv2d_noskew_geo{geo}", f"{k},noskew>", 396, 72, 576, A=("conv2d", KC), conv=(2, 3, 66, 64), p8=2 | geo << 4, nb=(1, 1))
    for geo, k in ((1, "8ph_q<CONV1D,2,4>"), (2, "8ph_q<CONV1D,4,2>"), (3, "8ph_128<CONV1D,lean>")):
        _add(g, f"conv1d_t96_geo{geo}", k, 288, (264, 136, 64)[geo - 1], 192, A=("conv1d", KC), conv=(3, 96, 3, 64), p8=1 | geo << 4, act="relu", res=True)
        _add(g, f"conv1d_t160_geo{geo}", k, 320, 72, 320, A=("conv1d", KC), conv=(2, 160, 5, 64), p8=1 | geo << 4)
    g = "p8_tconv"
    for geo, k in ((1, "8ph_q<TCONV2D,2,4"), (2, "8ph_q<TCONV2D,4,2"), (3, "8ph_128<TCONV2D")):
        for md, sk in ((1, "skew"), (2, "noskew")):
            pt, pf = ((0, 0), (0, 1), (1, 0))[(geo + md) % 3]
            tin, fin = (24, 23) if md == 1 else (23, 24)
            Tc, Fc = (tin - pt + 1) // 2, (fin - pf + 1) // 2
            _add(g, f"class{pt}{pf}_{sk}_geo{geo}", f"{k},{sk}>", 2 * Tc * Fc, 64, (2 - pt) * (2 - pf) * 64, A=("tconv2d", KC), conv=(2, tin, fin, pt, pf, 64),
                 p8=md | geo << 4, bias=False, emask=0 if md == 1 else None)
    _add(g, "class11_o128", "8ph_128<TCONV2D,skew>", 2 * 12 * 11, 64, 128, A=("tconv2d", KC), conv=(2, 24, 23, 1, 1, 128), p8=1 | 3 << 4, bias=False, emask=0)
    g = "p8_tr"                                                  # exact 256 x 128 tiles of row-contiguous operands, >= 128 tiles: cannot be forced smaller
    rc = dict(A=("dense", RC), B=("dense", RC), bias=False)
    _add(g, "tr_k64", "8ph_tr<skew>", 4096, 1024, 64, **rc, cdt="f32", acc=True)
    _add(g, "tr_k128_bf16", "8ph_tr<skew>", 4096, 1024, 128, **rc)
    _add(g, "tr_noskew", "8ph_tr<noskew>", 4096, 1024, 64, **rc, p8=2)
    _add(g, "tr_q_k64", "8ph_tr_q<skew>", 4096, 1024, 64, **rc, p8=1 | 1 << 4)
    _add(g, "tr_q_k128_f32", "8ph_tr_q<skew>", 4096, 1024, 128, **rc, p8=1 | 1 << 4, cdt="f32", acc=True)
    _add(g, "tr_q_noskew", "8ph_tr_q<noskew>", 4096, 1024, 64, **rc, p8=2 | 1 << 4, cdt="f32")


# ---- the grouped launchers take no route (each is a direct call): the recipes of one launch, in the order they are handed over
GROUPED = {}


def _grp(group, name, M, N, K, **kw):
    GROUPED.setdefault(group, []).append(case(f"{group}/{name}", "", M, N, K, **kw))


def _grouped_tables():
    rr = dict(A=("dense", RC), B=("dense", RC))
    # s2svc_gemm_grouped: 11 row-contiguous weight-gradient problems = two launches (10 per launch); ragged extents, every epilogue field
    g = "grouped"
    _grp(g, "130x72x40", 130, 72, 40, **rr, zero_padded=True, cdt="f32", acc=True)
    _grp(g, "136x8x64", 136, 8, 64, **rr, cdt="f32")
    _grp(g, "64x64x64", 64, 64, 64, **rr, res=True, act="relu")
    _grp(g, "72x136x200", 72, 136, 200, **rr, cdt="f32", rowsum="acc", acc=True)
    _grp(g, "8x8x8", 8, 8, 8, **rr, alpha=0.5)
    _grp(g, "104x72x130", 104, 72, 130, **rr, cdt="f32", rowsum="set")
    _grp(g, "65x63x33", 65, 63, 33, **rr, zero_padded=True, bias=False)
    _grp(g, "128x128x128", 128, 128, 128, **rr, c_pre=True)
    _grp(g, "129x65x72", 129, 65, 72, **rr, zero_padded=True, cdt="f32", acc=True, bias=False)
    _grp(g, "16x264x136", 16, 264, 136, **rr, cdt="f32", rowsum="acc")
    _grp(g, "264x16x66", 264, 16, 66, **rr, cdt="f32", acc=True, rowsum="set")
    # s2svc_gemm_grouped_batched: the batched products of an attention backward pass (T1 37, T2 45, dk 96), both A kinds
    _grp("grouped_batched_kc", "p_v", 37, 96, 45, nb=(3, 2), B=("dense", RC), zero_padded=True, bias=False)
    _grp("grouped_batched_kc", "ds_k", 37, 96, 45, nb=(3, 2), B=("dense", RC), zero_padded=True, bias=False, alpha=0.5)
    _grp("grouped_batched_kc", "square", 65, 64, 72, nb=(2, 1), B=("dense", RC), res=True)
    _grp("grouped_batched_rc", "dv", 45, 96, 37, nb=(3, 2), **rr, zero_padded=True, bias=False)
    _grp("grouped_batched_rc", "dk", 45, 96, 37, nb=(3, 2), **rr, zero_padded=True, bias=False, alpha=0.5)
    _grp("grouped_batched_rc", "tail", 136, 72, 130, nb=(1, 3), **rr, bias=False, cdt="f32")
    # s2svc_gemm_wgrad_grouped(_bg): fp32 C (+)= A^T B, M % 8 == N % 8 == 0, any K; with s2svc_gemm_set_w8(1, 2) a reduction of more than two K
    # tiles is cut into chunks that go through the workspace
    w = dict(**rr, cdt="f32", bias=False)
    for i, (M, N, K) in enumerate(((8, 8, 64), (136, 264, 130), (264, 136, 200), (8, 264, 200), (136, 8, 130), (264, 264, 64), (136, 136, 200))):
        _grp("wgrad", f"{M}x{N}x{K}", M, N, K, **w, acc=i % 2 == 1, rowsum=(None, "set", "acc")[i % 3])
    _grp("wgrad_conv2d", "c128", 136, 1152, 260, A=("dense", RC), B=("conv2d", RC), conv=(2, 2, 65, 128), cdt="f32", bias=False, acc=True)
    _grp("wgrad_conv2d", "c128_m8", 8, 1152, 260, A=("dense", RC), B=("conv2d", RC), conv=(2, 2, 65, 128), cdt="f32", bias=False, rowsum="set")
    _grp("wgrad_conv1d", "c128_k3", 5632, 384, 70, A=("dense", RC), B=("conv1d", RC), conv=(2, 35, 3, 128), cdt="f32", bias=False, acc=True)
    # the four parity classes of one transposed convolution as ONE s2svc_gemm_grouped launch (128 x 128 tiles)
    for pt, pf in ((0, 0), (0, 1), (1, 0), (1, 1)):
        Tc, Fc = (9 - pt + 1) // 2, (12 - pf + 1) // 2
        _grp("grouped_tconv", f"class{pt}{pf}", 2 * Tc * Fc, 64, (2 - pt) * (2 - pf) * 64, A=("tconv2d", KC), conv=(2, 9, 12, pt, pf, 64), bias=False)


_grouped_tables()

_tables()
CASES = [c for g in GROUPS.values() for c in g]
MAX_MADDS = 0.6e9            # per case, for the float64 truth on the CPU (chosen, not measured)

def routes_in_sources(csrc):
    """Every route name a launch site of csrc/gemm*.hip can hand to s2s_gemm_route / s2s_gemm_route_add: function-like macros that carry
    string literals are expanded at their invocations (`#P` stringifies), adjacent literals are joined, and each literal run inside a call of the
    setter is one name.  -> (set of kernel names, set of suffixes)."""
    import glob
    import os
    import re
    names, adds = set(), set()

    def call_args(text, start):
        depth, i = 0, start
        while True:
            ch = text[i]
            if ch == '"':
                i = text.index('"', i + 1)
            elif ch == "(":
                depth += 1
            elif ch == ")":
                depth -= 1
                if depth == 0:
                    return text[start + 1:i], i + 1
            i += 1

    def split_args(s):
        out, depth, cur, i = [], 0, "", 0
        while i < len(s):
            ch = s[i]
            if ch == '"':
                j = s.index('"', i + 1)
                cur += s[i:j + 1]
                i = j + 1
                continue
            if ch == "(":
                depth += 1
            if ch == ")":
                depth -= 1
            if ch == "," and depth == 0:
                out.append(cur.strip())
                cur = ""
            else:
                cur += ch
            i += 1
        out.append(cur.strip())
        return out

    for f in sorted(glob.glob(os.path.join(csrc, "gemm*.hip"))):
        text = open(f).read().replace("\\\n", " ")
        macros = {}
        for m in re.finditer(r"^[ \t]*#define[ \t]+(\w+)\(([^)]*)\)(.*)$", text, re.M):
            if '"' in m.group(3):
                macros[m.group(1)] = ([a.strip() for a in m.group(2).split(",")], m.group(3))
        text = re.sub(r"^[ \t]*#(define|undef).*$", "", text, flags=re.M)
        for _ in range(4):                                                # nested macros: a few rounds of textual expansion
            for name, (params, body) in macros.items():
                pos = 0
                while True:
                    m = re.search(r"\b%s\(" % name, text[pos:])
                    if not m:
                        break
                    s = pos + m.start()
                    args, end = call_args(text, s + len(name))
                    args = split_args(args)
                    exp = body
                    for prm, a in zip(params, args):
                        if prm == "...":
                            break
                        exp = re.sub(r"#\s*%s\b" % prm, '"%s"' % a.replace('"', ""), exp)
                        exp = re.sub(r"\b%s\b" % prm, a, exp)
                    text = text[:s] + exp + text[end:]
                    pos = s + len(exp)
        for setter, into in (("s2s_gemm_route", names), ("s2s_gemm_route_add", adds)):
            for m in re.finditer(r"\b%s\(" % setter, text):
                args, _ = call_args(text, m.end() - 1)
                if re.match(r"\s*const char\b", args):                    # the setter's own definition
                    continue
                for run in re.findall(r'(?:"[^"]*"\s*)+', args):
                    into.add("".join(re.findall(r'"([^"]*)"', run)))
    return names, adds
