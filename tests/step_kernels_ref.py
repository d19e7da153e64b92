"""Plain torch-CPU restatements of the decode-step, loss, length-regulator, Adam and glue operations that the hand-written kernels of
csrc/decode.hip, loss.hip, lenreg.hip, mas.hip (bin-loss backward), optim.hip and glue.hip stand in for, the comparison rule the GPU
checks apply, and the inputs the host test and the GPU cases share.  Test infrastructure: it needs no GPU, imports nothing of
seq2seq_vc_amd.ops, and the product never imports it.

Every restatement takes `dt`: torch.float64 gives `ref64` (the truth, evaluated on exactly the values the kernel reads; bf16 inputs
are upcast exactly), torch.float32 gives the `yard` (the same formula as stock torch computes it in float32).  With `bf16=True` the
float32 run also rounds where the kernel documents a rounding to bf16 (the packed LayerNorm output, the stored result).
tests/test_step_kernels_host.py pins each of them, in float64, to oracle/models.py and to stock torch.

The comparison rule (`compare`):  d = max |yard - ref64| over the tensor is what float32 (or bf16) arithmetic costs on this input;
a kernel passes when |got - ref64| <= MARGIN * d + ulp_out(|ref64|) at EVERY element, ulp_out being one unit in the last place of
the output type.  MARGIN = 4 is the margin the Griffin-Lim and time-stretcher yardsticks already give: it covers a 256-thread tree
summing in another order than torch's CPU loops.  Nothing here is fitted to what the kernels return.  A scalar output is a tensor of one
element: each call's loss, focus rate or sum is held to the d of that call alone."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 4.0
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(*shape, seed, scale=1.0, dtype=F32):
    """Seeded normal values, rounded to `dtype` (what the kernel will read) -- always returned on the CPU."""
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(dtype)


def bf16_round(t):
    return t.to(BF16).to(t.dtype)


def f32(v):
    """A Python float as the C ABI passes it: rounded to float32."""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------------------
def ulp_out(a, dtype):
    """One unit in the last place of `dtype` at magnitude |a| (float64 tensor): 2^(e - p) for 2^e <= |a| < 2^(e+1), p = 23 (fp32) or
    7 (bf16); below the smallest normal number (and at 0) the spacing of the denormals, 2^(-126 - p)."""
    p = {F32: 23, BF16: 7}[dtype]
    _, e = torch.frexp(a.abs().to(F64))                      # |a| = m * 2^e with m in [0.5, 1)  ->  floor(log2 |a|) = e - 1
    e = torch.where(a == 0, torch.full_like(e, -1000), e)   # frexp(0) answers e = 0
    return torch.exp2(torch.clamp(e.to(F64) - 1.0, min=-126.0) - p)


def compare(got, ref64, yard, out_dtype, margin=MARGIN):
    """-> (ok, ratio, d, message).  ratio = max |got - ref64| / d (0 when both are 0, inf when only d is).  Runs where ref64 lives."""
    ref64 = ref64.detach().to(F64)
    got, yard = got.detach().to(ref64.device).to(F64), yard.detach().to(ref64.device).to(F64)
    if got.shape != ref64.shape or yard.shape != ref64.shape:
        return False, float("inf"), 0.0, f"shapes {tuple(got.shape)} / {tuple(ref64.shape)} / {tuple(yard.shape)}"
    if got.numel() == 0:
        return True, 0.0, 0.0, "empty"
    d = float((yard - ref64).abs().max())
    err = (got - ref64).abs()
    bound = margin * d + ulp_out(ref64, out_dtype)
    bad = ~(err <= bound)                                    # a NaN in got fails
    worst = float(err.max())
    ratio = worst / d if d > 0 else (0.0 if worst == 0 else float("inf"))
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        need = float(((err - ulp_out(ref64, out_dtype)) / d).max()) if d > 0 else float("inf")
        return False, ratio, d, (f"{int(bad.sum())}/{bad.numel()} outside {margin:g} d + ulp (it would take {need:.3f} d): d {d:.3e}, max err {worst:.3e}, "
                                 f"first at {list(i)} got {float(got[i]):.9g} ref64 {float(ref64[i]):.9g}")
    return True, ratio, d, f"max|got - ref64| / d = {ratio:.3f} (d {d:.3e})"


def bits_equal(a, b):
    """Bit-for-bit equality of two tensors of one dtype and shape (so that -0.0 != 0.0 and a NaN equals itself)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {F32: torch.int32, BF16: torch.int16, F64: torch.int64}.get(a.dtype)
    return bool(torch.equal(a.view(view), b.view(view))) if view is not None else bool(torch.equal(a, b))


# ---------------------------------------------------------------------------------------------------------------------------
# decode step (csrc/decode.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def decode_posenc(x, xscale, alpha, pe, pos, dt, bf16=False):
    """modules/transformer/embedding.py:115-125 (ScaledPositionalEncoding.forward) for the one position `pos` of a decode step
    (modules/transformer/decoder.py:239-273):  y[b, :] = x[b, :] * xscale + alpha * pe[pos, :]."""
    a = 1.0 if alpha is None else alpha.to(dt)
    y = x.to(dt) * torch.tensor(xscale, dtype=dt) + a * pe[pos].to(dt)
    return bf16_round(y) if bf16 else y


def decode_attn(q, k, v, n, scale, dt, bf16=False):
    """modules/transformer/attention.py:63-111 (MultiHeadedAttention.forward_attention) for ONE query position against the first
    n[b] keys, as decoder_layer.py:85-132 uses it with a cache:  q (B, H, dk), k / v (B, Tk, H, dk), n (B) ints.
    -> ctx (B, H, dk), att (B, H, Tk) with exact zeros behind n[b].  A row without keys gives context 0 and attention 0."""
    B, H, dk = q.shape
    Tk = k.shape[1]
    ctx, att = torch.zeros(B, H, dk, dtype=dt), torch.zeros(B, H, Tk, dtype=dt)
    for b in range(B):
        nb = max(0, min(int(n[b]), Tk))
        if nb == 0:
            continue
        kb, vb = k[b, :nb].to(dt).transpose(0, 1), v[b, :nb].to(dt).transpose(0, 1)      # (H, nb, dk)
        s = torch.matmul(kb, q[b].to(dt).unsqueeze(-1)).squeeze(-1) * torch.tensor(scale, dtype=dt)
        p = torch.softmax(s, dim=-1)
        att[b, :, :nb] = p
        ctx[b] = torch.matmul(p.unsqueeze(1), vb).squeeze(1)
    return (bf16_round(ctx) if bf16 else ctx), att


def ln_linear(x, w, bias, norm, act, res, dt, bf16=False):
    """decoder_layer.py:85-132: LayerNorm in front of a projection of one decode position, then the projection:
    y = LayerNorm(x) (gamma, beta, eps = norm; None: y = x), out = act(y . w^T + bias) (+ res).  -> (out, y).
    bf16: the kernel packs y to bf16 for the matrix units and stores out in bf16; it accumulates in float32."""
    y = x.to(dt)
    if norm is not None:
        gamma, beta, eps = norm
        y = F.layer_norm(y, (y.shape[-1],), gamma.to(dt), beta.to(dt), eps)
        if bf16:
            y = bf16_round(y)
    out = F.linear(y, w.to(dt), None if bias is None else bias.to(dt))
    if act == "relu":
        out = torch.relu(out)
    if res is not None:
        out = out + res.to(dt)
    return (bf16_round(out) if bf16 else out), y


def ln_linear_supported_table():
    """(dtype, M, K, supported) on both sides of every boundary of s2svc_decode_ln_linear_supported: per = k-steps per wave = ceil(ceil(K /
    KSTEP) / 4), KSTEP = 32 (bf16) / 16 (fp32); per <= 6 for any M <= 64, per <= 12 up to M = 32; K a whole number of 16-byte vectors."""
    rows = []
    for dtype, ks in ((BF16, 32), (F32, 16)):
        vec = ks // 4
        rows += [(dtype, 33, 24 * ks, 1), (dtype, 33, 24 * ks + vec, 0), (dtype, 32, 24 * ks + vec, 1),        # per 6 -> 7 at M = 33
                 (dtype, 32, 48 * ks, 1), (dtype, 32, 48 * ks + vec, 0), (dtype, 1, 48 * ks + vec, 0),         # per 12 -> 13
                 (dtype, 33, 48 * ks, 0), (dtype, 64, 24 * ks, 1),
                 (dtype, 16, 80, 1), (dtype, 16, 80 + vec // 2, 0), (dtype, 16, vec, 1), (dtype, 16, vec - 1, 0),   # K % vec
                 (dtype, 64, 80, 1), (dtype, 65, 80, 0), (dtype, 0, 80, 0), (dtype, 16, 0, 0)]                  # M = 65, empty
    return rows


def stop_rule(probs_rows, threshold, minlen, maxlen):
    """models/vtn.py:344-389, the generation loop of one utterance reduced to its stop test (lines 378-381): probs_rows[idx - 1] holds the
    r stop probabilities of step idx = 1, 2, ...  -> the idx at which the loop breaks, 0 if it has not within the steps given."""
    idx = 0
    for probs in probs_rows:
        idx += 1
        if int(sum(p >= threshold for p in probs)) > 0 or idx >= maxlen:
            if idx < minlen:
                continue
            return idx
    return 0


def emit_rows(r):
    """The five utterances of the decode_emit cases over six positions, threshold 0.5: logits (5, 6, r), minlen, maxlen, the stop_at each
    row starts with, and what the rule makes of them.  Every logit is far from the threshold except the planted exact 0."""
    lg = torch.full((5, 6, r), -5.0)
    lg[0, 2, r - 1] = 0.0            # a probability exactly equal to the threshold fires (idx 3)
    lg[1, 1, 0] = 4.0                # a crossing at idx 2, blocked by minlen 4 ...
    lg[1, 4, r // 2] = 3.0           # ... the next one, at idx 5, stops
    lg[3, 2, 0] = 6.0                # crosses at idx 3, but the row stopped before (stop_at already 2)
    minlen = [0, 4, 0, 0, 0]
    maxlen = [100, 100, 4, 100, 100]  # row 2: forced at idx 4; row 4 never stops
    stop0 = [0, 0, 0, 2, 0]
    want = []
    for b in range(5):
        fired = stop_rule([[1.0 / (1.0 + math.exp(-float(x))) for x in lg[b, t]] for t in range(6)], 0.5, minlen[b], maxlen[b])
        want.append(stop0[b] if stop0[b] else fired)
    return lg, minlen, maxlen, stop0, want


# ---------------------------------------------------------------------------------------------------------------------------
# losses (csrc/loss.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def frame_mask(lens, T):
    return torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]


def seq_loss(after, before, logits, ys, labels, olens, pos_weight, dt, g_l1=None, g_bce=None, want_grads=False, bf16=False):
    """losses/seq2seq_loss.py:30-59: L1(after) + L1(before) and BCE-with-logits (pos_weight) over the frames t < olens[b], each a mean
    over the valid elements.  after / logits may be None (their term is left out).  -> (l1, bce, count[, d_after, d_before, d_logits]);
    the gradients are those of g_l1 * l1 + g_bce * bce, exactly 0 at masked frames and where a prediction equals its target."""
    B, Tm, D = before.shape
    m = frame_mask(olens, Tm)
    cnt = int(m.sum())
    md = m[:, :, None].to(dt)
    y = ys.to(dt)
    da = None if after is None else after.to(dt) - y
    db = before.to(dt) - y
    l1 = (db.abs() * md).sum() / (cnt * D)
    if da is not None:
        l1 = (da.abs() * md).sum() / (cnt * D) + l1
    bce = torch.zeros((), dtype=dt)
    if logits is not None:
        x, lab = logits.to(dt), labels.to(dt)
        lw = 1.0 + (pos_weight - 1.0) * lab
        term = (1.0 - lab) * x + lw * (torch.log1p(torch.exp(-x.abs())) + torch.clamp(-x, min=0.0))
        bce = (term * m.to(dt)).sum() / cnt
    if not want_grads:
        return l1, bce, cnt
    s1 = (1.0 if g_l1 is None else float(g_l1)) / (cnt * D)
    s2 = (1.0 if g_bce is None else float(g_bce)) / cnt
    d_after = None if da is None else torch.sign(da) * md * s1
    d_before = torch.sign(db) * md * s1
    d_logits = None
    if logits is not None:
        d_logits = ((1.0 - lab) - lw * (1.0 - torch.sigmoid(x))) * m.to(dt) * s2
    if bf16:
        d_after, d_before, d_logits = (None if t is None else bf16_round(t) for t in (d_after, d_before, d_logits))
    return l1, bce, cnt, d_after, d_before, d_logits


def seq_loss_stock(after, before, logits, ys, labels, olens, pos_weight, dt, g_l1=None, g_bce=None, want_grads=False, bf16=False):
    """The same loss as stock torch states it (F.l1_loss / F.binary_cross_entropy_with_logits on masked_select-ed tensors, gradients by
    autograd): the float32 yardstick of the GPU checks, and in float64 one of the two things `seq_loss` is pinned to."""
    B, Tm, D = before.shape
    m = frame_mask(olens, Tm)
    cnt = int(m.sum())
    leaves = [None if t is None else t.to(dt).clone().requires_grad_(want_grads) for t in (after, before, logits)]
    a, b, lg = leaves
    ys_ = ys.to(dt).masked_select(m[:, :, None])
    l1 = F.l1_loss(b.masked_select(m[:, :, None]), ys_)
    if a is not None:
        l1 = F.l1_loss(a.masked_select(m[:, :, None]), ys_) + l1
    bce = torch.zeros((), dtype=dt)
    if lg is not None:
        bce = F.binary_cross_entropy_with_logits(lg.masked_select(m), labels.to(dt).masked_select(m), pos_weight=torch.tensor(pos_weight, dtype=dt))
    if not want_grads:
        return l1.detach(), bce.detach(), cnt
    tot = l1 * (1.0 if g_l1 is None else float(g_l1)) + bce * (1.0 if g_bce is None else float(g_bce))
    tot.backward()
    grads = [None if t is None else t.grad for t in leaves]
    if bf16:
        grads = [None if t is None else bf16_round(t) for t in grads]
    return (l1.detach(), bce.detach(), cnt, *grads)


def guided_attn_weights(To, Ti, ilens, olens, sigma, dt):
    """losses/guided_attention_loss.py:142-165: w[b, to, ti] = 1 - exp(-(ti / il - to / ol)^2 / (2 sigma^2)) inside (ol, il), 0 outside."""
    B = len(ilens)
    w = torch.zeros(B, To, Ti, dtype=dt)
    for b in range(B):
        il, ol = min(int(ilens[b]), Ti), min(int(olens[b]), To)
        if il <= 0 or ol <= 0:
            continue
        gx, gy = torch.meshgrid(torch.arange(ol), torch.arange(il), indexing="ij")
        w[b, :ol, :il] = 1.0 - torch.exp(-((gy.to(dt) / il - gx.to(dt) / ol) ** 2) / (2 * torch.tensor(sigma, dtype=dt) ** 2))
    return w


def guided_attn_loss(att, ilens, olens, sigma, alpha, dt, gout=None, bf16=False):
    """losses/guided_attention_loss.py:142-165: alpha * mean over the valid (b, h, to, ti) of w * att.  -> (loss, count, datt): datt is the
    gradient of gout * loss, which does not depend on att: gout * alpha / count * w on valid elements, 0 elsewhere."""
    B, H, To, Ti = att.shape
    w = guided_attn_weights(To, Ti, ilens, olens, sigma, dt)
    cnt = H * sum(min(int(i), Ti) * min(int(o), To) for i, o in zip(ilens, olens))
    loss = torch.tensor(alpha, dtype=dt) * (w[:, None] * att.to(dt)).sum() / cnt
    datt = ((1.0 if gout is None else float(gout)) * torch.tensor(alpha, dtype=dt) / cnt * w)[:, None].expand(B, H, To, Ti).contiguous()
    return loss, cnt, (bf16_round(datt) if bf16 else datt)


# ---------------------------------------------------------------------------------------------------------------------------
# length regulator, durations from attention, bin-loss backward (csrc/lenreg.hip, csrc/mas.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def length_regulate_index(ds, Tout):
    """modules/length_regulator.py:46-97 as indices: frame i of utterance b is repeated max(ds[b, i], 0) times.  -> start (B, Tx) =
    exclusive prefix sums, idx (B, Tout) = source frame of every output frame (-1 behind the utterance's total), total (B)."""
    d = np.maximum(np.asarray(ds, np.int64), 0)
    B, Tx = d.shape
    incl = np.cumsum(d, axis=1)
    start = incl - d
    idx = np.full((B, Tout), -1, np.int32)
    for b in range(B):
        run = np.repeat(np.arange(Tx), d[b])[:Tout]
        idx[b, :len(run)] = run
    return start.astype(np.int32), idx, incl[:, -1].astype(np.int32)


def length_regulate_fwd(x, idx, pad_value):
    """y[b, t] = x[b, idx[b, t]] or pad_value where idx is -1: a torch gather (bit-exact copies)."""
    B, Tx, D = x.shape
    idx = torch.as_tensor(idx).long()
    y = torch.gather(x, 1, idx.clamp(min=0)[:, :, None].expand(B, idx.shape[1], D))
    return torch.where((idx >= 0)[:, :, None], y, torch.tensor(pad_value, dtype=x.dtype))


def length_regulate_bwd(dy, start, ds, Tx, dt, bf16=False):
    """The gradient of length_regulate_fwd: dx[b, i] = sum of dy[b, t] over the frame's run [start, start + d) cut at Tout."""
    B, Tout, D = dy.shape
    dx = torch.zeros(B, Tx, D, dtype=dt)
    g = dy.to(dt)
    for b in range(B):
        for i in range(Tx):
            s, d = int(start[b][i]), max(int(ds[b][i]), 0)
            e = min(s + d, Tout)
            if e > s:
                dx[b, i] = g[b, s:e].sum(0)
    return bf16_round(dx) if bf16 else dx


def length_regulate_bwd_stock(dy, idx, Tx, dt, bf16=False):
    """The same gradient as stock torch forms it: index_add_ of the output frames onto their source frames."""
    B, Tout, D = dy.shape
    dx = torch.zeros(B, Tx, D, dtype=dt)
    idx = torch.as_tensor(idx).long()
    for b in range(B):
        ok = idx[b] >= 0
        dx[b].index_add_(0, idx[b][ok], dy[b].to(dt)[ok])
    return bf16_round(dx) if bf16 else dx


def attn_durations(att, dt):
    """utils/duration_calculator.py:13-65 for a stack of heads att (NH, Tf, Tx): the head with the largest mean row maximum (the first, as
    torch.argmax), durations[j] = frames whose first arg-max is j, focus rate = that head's score.  -> (durations int64, scores (NH), head)."""
    a = att.to(dt)
    scores = a.max(dim=-1)[0].mean(dim=-1)
    head = int(scores.argmax())
    am = a[head].argmax(-1)
    dur = torch.stack([am.eq(i).sum() for i in range(a.shape[2])]).to(torch.int64)
    return dur, scores, head


def attn_durations_input(NH, Tf, Tx, seed, twin_heads=False):
    """fp32 attention-like maps whose heads differ in scale (so the diagonal scores of the best two are more than 1e-3 apart, which the host
    test asserts), with duplicated row maxima planted in every third row (the first arg-max decides); twin_heads: head 1 = head 0."""
    u = torch.rand(NH, Tf, Tx, generator=gen(seed)) * 0.5 + 0.1
    order = torch.randperm(NH, generator=gen(seed + 1))
    for h in range(NH):
        u[h] *= 1.0 + 0.15 * float(order[h])
    if Tx > 1:
        for h in range(NH):
            for t in range(0, Tf, 3):
                j = torch.randperm(Tx, generator=gen(seed + 7 * t + h))[:2]
                u[h, t, j[0]] = u[h, t, j[1]] = u[h, t].max() * 1.25
    if twin_heads and NH > 1:                               # the best head twice, at the front: the first of the two must win
        best = int(u.double().max(dim=-1)[0].mean(dim=-1).argmax())
        u[0] = u[best].clone()
        u[1] = u[0]
    return u.contiguous()


ATTN_DUR_SHAPES = [(NH, Tf, Tx) for NH in (1, 4) for Tf in (1, 255, 257, 600) for Tx in (1, 7, 300)]


def mas_binloss_bwd(path, feat_lens, gout, dlogp, dt):
    """modules/alignments.py:299-309: bin_loss = -(1 / B) sum_b mean_t log_p[b, t, path[b, t]]; its gradient, ADDED to dlogp:
    dlogp[b, t, path[b, t]] += -gout / (B * min(feat_lens[b], Tf)) for every path entry >= 0."""
    B, Tf = path.shape
    out = dlogp.to(dt).clone()
    g = torch.tensor(float(gout), dtype=dt)
    for b in range(B):
        fl = min(int(feat_lens[b]), Tf)
        for t in range(Tf):
            a = int(path[b, t])
            if a >= 0:
                out[b, t, a] = out[b, t, a] + (-g / (torch.tensor(float(B), dtype=dt) * torch.tensor(float(fl), dtype=dt)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# optimiser (csrc/optim.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def warmup_lr(base_lr, step, warmup_steps, dt):
    """schedulers/warmup_lr.py:54-61: lr of optimiser step `step` (1-based) = base * w^0.5 * min(step^-0.5, step * w^-1.5); w = 0: base."""
    base = torch.tensor(base_lr, dtype=dt)
    if warmup_steps <= 0:
        return base
    s, w = torch.tensor(float(step), dtype=dt), torch.tensor(float(warmup_steps), dtype=dt)
    return base * torch.sqrt(w) * torch.minimum(torch.rsqrt(s), s * torch.pow(w, -1.5))


def adam_step(p, g, m, v, step, base_lr, betas, eps, max_norm, warmup_steps, dt):
    """trainers/ar_vc.py:99-107: clip_grad_norm_(max_norm) (max_norm = 0: no clipping) -> torch.optim.Adam (no weight decay) at the WarmupLR
    rate of this step.  p, g, m, v: flat tensors; step: the 1-based count of THIS update.  Hyper-parameters are taken as given (the caller
    passes them as the C ABI does, rounded to float32).  -> (p, m, v, state) with state = [step, lr, grad norm, clip coefficient]."""
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    norm = torch.linalg.vector_norm(g)                       # what clip_grad_norm_ computes
    coef = torch.ones((), dtype=dt, device=p.device)
    if max_norm > 0:
        coef = torch.clamp(torch.tensor(max_norm, dtype=dt, device=p.device) / (norm + torch.tensor(f32(1e-6), dtype=dt, device=p.device)), max=1.0)
    lr = warmup_lr(base_lr, step, warmup_steps, dt).to(p.device)
    b1, b2 = (torch.tensor(b, dtype=dt, device=p.device) for b in betas)
    gi = g * coef
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - torch.pow(b1, step), 1.0 - torch.pow(b2, step)
    denom = torch.sqrt(v) / torch.sqrt(bc2) + torch.tensor(eps, dtype=dt, device=p.device)
    p = p - (lr / bc1) * (m / denom)
    state = torch.stack([torch.tensor(float(step), dtype=dt, device=p.device), lr, norm.to(dt), coef])
    return p, m, v, state


def shadow_probe_values():
    """fp32 values at which a float32 -> bf16 rounding goes wrong first: exact ties that round down and up to even (both signs), a tie next to
    a carry into the exponent, -0.0, a float32 denormal, the smallest normal, 3.39e38 (just below the tie between the largest bf16 and infinity), 3.40e38 (above it) and ordinary values."""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3FFF8000, 0x3F807FFF, 0x3F808001, 0x80000000, 0x00000000,
            0x00012345, 0x80012345, 0x00800000, 0x00408000, 0x7F7F0000]
    vals = torch.tensor(np.array(bits, np.uint32).view(np.float32).copy())
    return torch.cat([vals, torch.tensor([3.39e38, -3.39e38, 3.40e38, -3.40e38, 1.0, -2.5, 0.1, 1e-20], dtype=F32)])


# ---------------------------------------------------------------------------------------------------------------------------
# glue (csrc/glue.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def weighted_sum(xs, ws, dt):
    """trainers/aas_vc.py:100-139, the loss composition: sum_i w_i * sum(x_i)."""
    tot = torch.zeros((), dtype=dt)
    for x, w in zip(xs, ws):
        tot = tot + torch.tensor(w, dtype=dt) * x.to(dt).sum()
    return tot


def scalars_axpy(xs, ws, acc, beta, dt):
    """trainers/aas_vc.py:100-139, the running sums of the logged losses: acc[i] = beta * acc[i] + w_i * sum(x_i); beta = 0 does not read acc."""
    out = acc.to(dt).clone()
    for i, (x, w) in enumerate(zip(xs, ws)):
        out[i] = (torch.tensor(beta, dtype=dt) * out[i] if beta != 0 else 0.0) + torch.tensor(w, dtype=dt) * x.to(dt).sum()
    return out


def decoder_input(ys, r):
    """models/vtn.py:228-243: the teacher-forcing input cat(zeros, ys[:, r-1::r][:, :-1]) over the T // r steps."""
    B, T, D = ys.shape
    Tin = T // r
    sub = ys[:, r - 1::r][:, :Tin]
    return torch.cat([ys.new_zeros(B, 1, D), sub[:, :-1]], dim=1)


def append_eos(xs, lens, eos, pad):
    """models/transformer_tts.py:139-142: F.pad(xs, [0, 1], value = pad), then eos written behind each sequence."""
    out = F.pad(xs, [0, 1], "constant", pad)
    for i, l in enumerate(lens):
        out[i, int(l)] = eos
    return out


def stop_labels(labels, lens, T):
    """models/vtn.py:262-275 (the stop labels of a reduced target): torch.scatter(labels, 1, (olens - 1).unsqueeze(1), 1.0) on labels[:, :T]; a row of
    length 0 has no last frame and is left as it is (torch.scatter would refuse the index -1)."""
    out = labels[:, :T].clone()
    rows = [b for b, l in enumerate(lens) if int(l) >= 1]
    if rows:
        sel = torch.tensor(rows)
        idx = (torch.as_tensor(lens)[sel].long() - 1).unsqueeze(1)
        out[sel] = torch.scatter(out[sel], 1, idx, 1.0)
    return out
