"""Plain torch-CPU restatements of the attention operations that csrc/attn_fused.hip, attn_map.hip, relattn.hip and softmax.hip stand in
for, and the shape / seed tables and inputs that tests/gpu_attn_kernel_check.py and tests/test_attn_kernels_host.py share.  Test
infrastructure: it needs no GPU, imports nothing of seq2seq_vc_amd.ops, and the product never imports it.  The comparison rule is the one of
tests/step_kernels_ref.py (`compare`, `ulp_out`, `MARGIN`), applied per (utterance, head) slice.

Every restatement takes `dt`: torch.float64 gives `ref64` (the truth on exactly the values the kernel reads; bf16 inputs are upcast
exactly, and nothing in between is rounded), torch.float32 with `bf16=True` gives the `yard`: stock float32 torch, rounded to bf16 at the
points the kernels' header comments document and nowhere else:
  * the stored map;
  * the dropped copy: bf16(stored map * keep) in attn_fused.hip and relattn.hip (`drop_stored=True`), bf16(fp32 probability * keep) in
    attn_map.hip and softmax.hip (`drop_stored=False`); the context product consumes the dropped copy (the stored map without dropout);
  * dS before the dq / dk products (and the dropped copy before the dv product);
  * qu = q + u and qv = q + v of relattn.hip, which are stored and then read back as the operands of the score products;
  * the stored outputs.
Dropout enters as DATA: `keep` is the (B, H, T1, T2) tensor of 0 or 1 / (1 - p) that the kernels' mask function draws for the element index
in the padded (B, H, T1, ld) layout of the map.  A row with no admissible key gives map 0 and context 0 (as R.decode_attn states it).
`plant` names one deliberate error (the power check of the host test); None is the operation itself."""
import math

import torch

import step_kernels_ref as R
from step_kernels_ref import BF16, F32, F64, bf16_round

PLANTS = ("klen+1", "causal<", "no_dattn", "ds*0.97", "dv_last_row", "drop_T2", "shift+1", "uv_swapped")


def heads(x, H, dt):
    """(B, T, H * dk) -> (B, H, T, dk) in dt."""
    B, T, D = x.shape
    return x.to(dt).view(B, T, H, D // H).transpose(1, 2)


def unheads(x):
    B, H, T, dk = x.shape
    return x.transpose(1, 2).reshape(B, T, H * dk)


def key_mask(klen, T1, T2, causal, plant=None):
    """(B, 1, T1, T2) bool: key j of utterance b is admissible for query i (attention.py:63-93: j < klen[b]; causal: j <= i)."""
    kl = torch.as_tensor([max(0, min(int(n), T2)) for n in klen])
    if plant == "klen+1":
        kl = torch.clamp(kl + 1, max=T2)
    m = (torch.arange(T2)[None, :] < kl[:, None])[:, None, None, :].expand(len(klen), 1, T1, T2)
    if causal:
        i, j = torch.arange(T1)[:, None], torch.arange(T2)[None, :]
        m = m & ((j < i) if plant == "causal<" else (j <= i))[None, None]
    return m


def masked_softmax(s, m):
    """attention.py:63-93: masked_fill(min), softmax, masked_fill(0).  A row without an admissible key is 0."""
    p = torch.softmax(s.masked_fill(~m, torch.finfo(s.dtype).min), dim=-1)
    return p.masked_fill(~m, 0.0)


def _store(p, keep, bf16, drop_stored):
    """-> (stored map, dropped copy) of fp probabilities p."""
    ps = bf16_round(p) if bf16 else p
    if keep is None:
        return ps, ps
    pd = (ps if (bf16 and drop_stored) else p) * keep.to(p.dtype)
    return ps, (bf16_round(pd) if bf16 else pd)


def attn_fwd(q, k, v, klen, causal, scale, H, dt, keep=None, bf16=False, drop_stored=True, plant=None):
    """Plain attention forward, modules/transformer/attention.py:63-111.  q (B, T1, D), k / v (B, T2, D) (v may be None), klen (B) ints.
    -> map (B, H, T1, T2) with exact zeros at masked positions, its dropped copy, context (B, T1, D) or None."""
    T1, T2 = q.shape[1], k.shape[1]
    s = torch.matmul(heads(q, H, dt), heads(k, H, dt).transpose(-2, -1)) * torch.tensor(scale, dtype=dt)
    p = masked_softmax(s, key_mask(klen, T1, T2, causal, plant))
    ps, pd = _store(p, keep, bf16, drop_stored)
    ctx = None
    if v is not None:
        ctx = unheads(torch.matmul(pd, heads(v, H, dt)))
        ctx = bf16_round(ctx) if bf16 else ctx
    return ps, pd, ctx


def softmax_bwd_core(p, dp, scale, dt, dattn=None, keep=None, plant=None):
    """dS = P (dP keep + dattn - sum_j P (dP keep + dattn)) scale: the backward of dropout, masked softmax and the scaling, from the map."""
    t = dp if keep is None else dp * keep.to(dt)
    tsum = t
    if dattn is not None:
        t = t + dattn.to(dt)
        tsum = tsum if plant == "no_dattn" else t
    ds = p * (t - (p * tsum).sum(-1, keepdim=True)) * torch.tensor(scale, dtype=dt)
    return ds * 0.97 if plant == "ds*0.97" else ds


def unshift(ds, L=None):
    """The gradient of matrix_bd BEFORE the "new" rel_shift (attention.py:237-260): dbd[i, T - 1 - i + j] = dS[i, j], zero elsewhere."""
    B, H, T, _ = ds.shape
    L = 2 * T - 1 if L is None else L
    out = torch.zeros(B, H, T, L, dtype=ds.dtype)
    idx = (T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]).expand(B, H, T, T)
    return out.scatter(-1, idx, ds)


def attn_bwd(pmap, dctx, v, k, q, scale, H, dt, dattn=None, keep=None, bf16=False, rel=False, plant=None):
    """Plain attention backward from a GIVEN stored map pmap (B, H, T1, T2): dctx (B, T1, D), v / k (B, T2, D), q (B, T1, D) (k, q may
    be None: their product is left out).  -> dS (B, H, T1, T2), dq, dk, dv (B, T, D) [, dbd (B, H, T, 2T - 1) with rel]."""
    p = pmap.to(dt)
    do = heads(dctx, H, dt)
    ds = softmax_bwd_core(p, torch.matmul(do, heads(v, H, dt).transpose(-2, -1)), scale, dt, dattn, keep, plant)
    pd = p if keep is None else p * keep.to(dt)
    if bf16:
        ds, pd = bf16_round(ds), bf16_round(pd)
    if plant == "dv_last_row":
        pd = pd.clone()
        pd[:, :, -1] = 0
    dq = None if k is None else unheads(torch.matmul(ds, heads(k, H, dt)))
    dk = None if q is None else unheads(torch.matmul(ds.transpose(-2, -1), heads(q, H, dt)))
    dv = unheads(torch.matmul(pd.transpose(-2, -1), do))
    if bf16:
        dq, dk, dv = (None if t is None else bf16_round(t) for t in (dq, dk, dv))
    out = (ds, dq, dk, dv)
    return out + (unshift(ds),) if rel else out


def rel_shift_new(bd, plant=None):
    """attention.py:237-260 as an index: shifted[i, j] = bd[i, T - 1 - i + j] for bd (B, H, T, 2T - 1)."""
    B, H, T, L = bd.shape
    idx = T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]
    if plant == "shift+1":
        idx = torch.clamp(idx + 1, max=L - 1)
    return bd.gather(-1, idx.expand(B, H, T, T))


def rel_shift_legacy(bd):
    """attention.py:142-160 as an index, bd (B, H, T, T): element f = T + i T + j of the left-padded (T, T + 1) matrix; its column 0 is the pad."""
    B, H, T, _ = bd.shape
    f = T + torch.arange(T)[:, None] * T + torch.arange(T)[None, :]
    si, c = f // (T + 1), f % (T + 1)
    val = bd[:, :, si, torch.clamp(c - 1, min=0)]
    return torch.where((c >= 1)[None, None], val, torch.zeros((), dtype=bd.dtype))


def rel_attn_fwd(q, k, pos, u, v, klen, scale, H, dt, keep=None, bf16=False, plant=None):
    """Relative-position self-attention forward, attention.py:262-305 with the "new" shift: q, k (B, T, D), pos (2T - 1, D), u, v (D) fp32
    (pos_bias_u / pos_bias_v, head-major).  -> map, dropped copy (B, H, T, T), qu = q + u, qv = q + v (B, T, D)."""
    T = q.shape[1]
    if plant == "uv_swapped":
        u, v = v, u
    qu, qv = q.to(dt) + u.to(dt), q.to(dt) + v.to(dt)
    if bf16:
        qu, qv = bf16_round(qu), bf16_round(qv)
    ac = torch.matmul(heads(qu, H, dt), heads(k, H, dt).transpose(-2, -1))
    bd = torch.matmul(heads(qv, H, dt), heads(pos[None], H, dt).transpose(-2, -1))
    s = (ac + rel_shift_new(bd, plant)) * torch.tensor(scale, dtype=dt)
    ps, pd = _store(masked_softmax(s, key_mask(klen, T, T, False, plant)), keep, bf16, True)
    return ps, pd, qu, qv


def softmax_fwd(scores, scale, klen, causal, dt, bd=None, rel_mode=0, keep=None, out_bf16=False, plant=None):
    """The softmax kernel on GIVEN fp32 scores (B, H, T1, T2): (scores + shifted bd) * scale, mask, softmax, mask, dropout.  bd: the
    unshifted position term, (B, H, T, 2T - 1) for rel_mode 1, (B, H, T, T) for rel_mode 2.  -> map, dropped copy."""
    s = scores.to(dt)
    if bd is not None:
        s = s + (rel_shift_new(bd.to(dt), plant) if rel_mode == 1 else rel_shift_legacy(bd.to(dt)))
    p = masked_softmax(s * torch.tensor(scale, dtype=dt), key_mask(klen, s.shape[2], s.shape[3], causal, plant))
    return _store(p, keep, out_bf16, False)


def softmax_bwd(pmap, dp, scale, dt, dattn=None, keep=None, rel_mode=0, out_bf16=False, plant=None):
    """The softmax backward kernel on a given map and fp32 dP.  -> dscores, dbd (None for rel_mode 0; rel_mode 2: the legacy scatter)."""
    ds = softmax_bwd_core(pmap.to(dt), dp.to(dt), scale, dt, dattn, keep, plant)
    ds = bf16_round(ds) if out_bf16 else ds
    return ds, (scatter_bd(ds, rel_mode) if rel_mode else None)


def unshift_legacy(ds):
    """The gradient of matrix_bd before the LEGACY rel_shift (attention.py:142-160): dS[i, j] lands on the element rel_shift_legacy read for
    (i, j); the elements read from the pad column land nowhere.  (B, H, T, T) -> (B, H, T, T)."""
    B, H, T, _ = ds.shape
    f = T + torch.arange(T)[:, None] * T + torch.arange(T)[None, :]
    si, c = f // (T + 1), f % (T + 1)
    flat = torch.zeros(B, H, T * T + 1, dtype=ds.dtype)                       # slot T * T takes what came from the pad column
    tgt = torch.where(c >= 1, si * T + c - 1, torch.full_like(f, T * T)).reshape(-1)
    flat[:, :, tgt] = ds.reshape(B, H, T * T)
    return flat[:, :, :T * T].reshape(B, H, T, T)


def scatter_bd(ds, rel_mode, L=None):
    return unshift(ds, L) if rel_mode == 1 else unshift_legacy(ds)


# ---------------------------------------------------------------------------------------------------------------------------
# shapes, seeds and inputs of the GPU cases (the host test runs its power check on the very same tensors)
# ---------------------------------------------------------------------------------------------------------------------------
B_, H_ = 3, 2
SCORE_STD = 3.0              # of the scaled scores: a peaked softmax, P has O(0.1 - 1) entries, every term of the backward matters

# attn_fused: (T1, T2, dk, causal).  T1 != T2; a single row (T1 = 1) and a single key; waves without a valid row (T1 <= 48); ld > T2
# (T2 = 1, 15, 17, 33, 63); causal on the square ones; every dk.
FUSED_SHAPES = [(1, 33, 32, False), (15, 64, 64, False), (16, 16, 96, True), (17, 17, 128, True), (33, 63, 96, False),
                (63, 63, 32, True), (64, 64, 128, True), (64, 15, 64, False), (63, 1, 96, False), (64, 64, 96, False), (1, 1, 32, True)]

# attn_map: every T2 on both sides of the 2 / 4 / 8-wave variants and of the 8-column vectors, T1 around the 64-row block (and 130: three
# blocks), dk = 1 - 5 slices through the 3-stage pipeline (160: no second product); then the square ones, causal and with dbd.
_T2S = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)
_T1S, _DKS = (1, 63, 64, 65, 130), (32, 64, 96, 128, 160)
MAP_SHAPES = ([(_T1S[i % 5], t2, _DKS[(i + i // 5) % 5], False) for i, t2 in enumerate(_T2S)]
              + [(1, 1, 64, True), (63, 63, 96, True), (64, 64, 128, True), (65, 65, 64, True), (130, 130, 32, True), (130, 130, 96, True)])

REL_SHAPES = [(1, 32), (2, 96), (63, 192), (64, 32), (65, 96), (128, 192), (129, 32), (255, 96), (256, 192), (256, 32)]     # (T, dk)

# attn_softmax: (T1, T2, ld, causal, rel_mode).  ld > T2 everywhere; rel_mode 1 / 2 need T1 == T2 and come with ldb > Lp.
SOFTMAX_SHAPES = [(5, 1, 8, False, 0), (63, 63, 64, True, 0), (7, 64, 72, False, 0), (65, 65, 72, True, 0), (3, 129, 136, False, 0),
                  (2, 513, 520, False, 0), (63, 63, 64, False, 1), (65, 65, 72, False, 1), (129, 129, 136, False, 1), (64, 64, 72, False, 2),
                  (65, 65, 72, False, 2)]


def round8(n):
    return (n + 7) // 8 * 8


def klens(T2):
    """Per utterance: the full length, a length that cuts inside a 16-column tile (no multiple of 16), and 1."""
    cut = T2 - 5 if T2 > 5 else max(1, T2 - 1)
    if cut % 16 == 0:
        cut -= 1
    return [T2, cut, 1]


def edge_klens(T2):
    """Per utterance: no admissible key at all (map 0, context 0), a length beyond the keys (every kernel takes min(klen, T2)), the cut."""
    return [0, T2 + 3, klens(T2)[1]]


# The shapes of each table that run a second time with edge_klens, through every forward launcher and, by the all-zero (b 0) slices of the
# stored map this gives, through every backward one.
EDGE_KLEN_SHAPES = dict(fused=[(33, 63, 96, False), (17, 17, 128, True)],
                        map=[(63, 65, 96, False), (64, 127, 128, False), (65, 65, 64, True)],
                        rel=[(65, 96), (129, 32)],
                        softmax=[(63, 63, 64, True, 0), (3, 129, 136, False, 0), (65, 65, 72, False, 1), (65, 65, 72, False, 2)])


def with_edges(shapes, family):
    """[(shape, edge)]: every shape of the table with klens, then the family's EDGE_KLEN_SHAPES among them with edge_klens."""
    return [(s, False) for s in shapes] + [(s, True) for s in EDGE_KLEN_SHAPES[family] if s in shapes]


def keep_of(full, T2, plant=None):
    """The keep-scales of the map's elements out of the tensor drawn for the padded (B, H, T1, ld) layout."""
    B, H, T1, ld = full.shape
    if plant == "drop_T2":                                   # the element index taken with T2 in place of ld
        return full.reshape(-1)[:B * H * T1 * T2].view(B, H, T1, T2)
    return full[..., :T2]


def host_keep(B, H, T1, ld, p, seed):
    """A stand-in on the CPU for the kernels' mask function (the host test has no device): 0 or 1 / (1 - p), fp32, padded layout."""
    u = torch.rand(B, H, T1, ld, generator=R.gen(seed))
    return torch.where(u < p, torch.zeros(()), torch.tensor(1.0 / (1.0 - p), dtype=F32))


def _dattn(B, H, T1, T2, klen, causal, seed):
    """The gradient that reaches the map itself: unit scale, bf16, zero where the map is masked."""
    g = R.randn(B, H, T1, T2, seed=seed, dtype=BF16)
    return torch.where(key_mask(klen, T1, T2, causal), g, torch.zeros((), dtype=BF16))


def plain_inputs(T1, T2, dk, causal, seed, B=B_, H=H_, edge=False):
    """bf16 q (scaled so that the scaled scores have a standard deviation of about SCORE_STD), k, v, dctx, the map gradient, klen, scale."""
    D = H * dk
    klen = (edge_klens if edge else klens)(T2)[:B]
    return dict(q=R.randn(B, T1, D, seed=seed, scale=SCORE_STD, dtype=BF16), k=R.randn(B, T2, D, seed=seed + 1, dtype=BF16),
                v=R.randn(B, T2, D, seed=seed + 2, dtype=BF16), dctx=R.randn(B, T1, D, seed=seed + 3, dtype=BF16),
                dattn=_dattn(B, H, T1, T2, klen, causal, seed + 4), klen=klen, scale=R.f32(1.0 / math.sqrt(dk)), causal=causal, H=H)


def rel_inputs(T, dk, seed, B=B_, H=H_, edge=False):
    """q, k, pos (2T - 1, D) bf16, u / v fp32 of O(0.5): both score terms have a standard deviation of about SCORE_STD / sqrt(2)."""
    D = H * dk
    s = SCORE_STD / math.sqrt(2.0)
    return dict(q=R.randn(B, T, D, seed=seed, scale=s, dtype=BF16), k=R.randn(B, T, D, seed=seed + 1, dtype=BF16),
                pos=R.randn(2 * T - 1, D, seed=seed + 2, dtype=BF16), u=R.randn(D, seed=seed + 3, scale=0.5), v=R.randn(D, seed=seed + 4, scale=0.5),
                klen=(edge_klens if edge else klens)(T)[:B], scale=R.f32(1.0 / math.sqrt(dk)), H=H)


def softmax_inputs(T1, T2, causal, rel_mode, seed, B=B_, H=H_, edge=False):
    """fp32 scores (and position term) whose scaled sum has a standard deviation of about SCORE_STD, fp32 dP, the map gradient, klen, scale."""
    scale = R.f32(0.125)
    klen = (edge_klens if edge else klens)(T2)[:B]
    s = SCORE_STD / scale / (math.sqrt(2.0) if rel_mode else 1.0)
    Lp = {0: 0, 1: 2 * T1 - 1, 2: T1}[rel_mode]
    return dict(scores=R.randn(B, H, T1, T2, seed=seed, scale=s), bd=R.randn(B, H, T1, Lp, seed=seed + 1, scale=s) if rel_mode else None,
                dp=R.randn(B, H, T1, T2, seed=seed + 2), dattn=_dattn(B, H, T1, T2, klen, causal, seed + 3), klen=klen, scale=scale,
                causal=causal, Lp=Lp)


def fused_inputs(shape, edge=False):
    return plain_inputs(*shape, seed=1000 + 7 * FUSED_SHAPES.index(shape), edge=edge)


def map_inputs(shape, edge=False):
    return plain_inputs(*shape, seed=2000 + 7 * MAP_SHAPES.index(shape), edge=edge)


def rel_case_inputs(shape, edge=False):
    return rel_inputs(*shape, seed=3000 + 7 * REL_SHAPES.index(shape), edge=edge)


def softmax_case_inputs(shape, edge=False):
    T1, T2, ld, causal, rel_mode = shape
    return softmax_inputs(T1, T2, causal, rel_mode, seed=4000 + 7 * SOFTMAX_SHAPES.index(shape), edge=edge)


def stored_map(inp, dt_out=BF16):
    """What a backward case hands its kernel: the float64 map of the inputs, rounded to the map's type on the CPU."""
    return attn_fwd(inp["q"], inp["k"], None, inp["klen"], inp["causal"], inp["scale"], inp["H"], F64)[0].to(dt_out)


def slices(t, H):
    """The (utterance, head) slices of an output: (B, H, ...) as it is, (B, T, H * dk) by column block.  -> [((b, h), tensor)]."""
    if t.dim() == 4:
        return [((b, h), t[b, h]) for b in range(t.shape[0]) for h in range(t.shape[1])]
    dk = t.shape[2] // H
    return [((b, h), t[b, :, h * dk:(h + 1) * dk]) for b in range(t.shape[0]) for h in range(H)]
