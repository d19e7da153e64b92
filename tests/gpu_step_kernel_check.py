"""Kernel-level parity for the launchers no other kernel-level check calls: the decode step (csrc/decode.hip), the sequence and
guided-attention losses (csrc/loss.hip), the length regulator and the durations from attention (csrc/lenreg.hip), the bin-loss backward
(csrc/mas.hip), the fused Adam step (csrc/optim.hip) and the glue of a training step (csrc/glue.hip, add_n).  Runs on the MI355X:
  * `python tests/gpu_step_kernel_check.py [--only a,b]` prints a PASS/FAIL table for all cases and never stops early;
  * tests/test_gpu_step_kernels.py imports CASES and turns each into a `@pytest.mark.gpu` test.

Floats are compared by the rule of tests/step_kernels_ref.py: ref64 = the float64 restatement on exactly the values the kernel reads,
yard = the same formula by stock torch in float32 on the CPU (rounded to bf16 where the kernel documents it), d = max |yard - ref64|,
pass when |got - ref64| <= 4 d + ulp_out(|ref64|) at every element; each PASS line prints max |got - ref64| / d.  Copies, integers and
decisions (cache appends, regulated frames, indices, durations, the chosen head, stop positions, tokens, labels, the bf16 shadow) are
compared bit for bit.  Every output buffer starts as a finite sentinel and whatever the kernel should not write is compared bit for
bit with it.  References run on the CPU, except for the one Adam case of 2^26 + 7 parameters, whose float64 reference is torch on the
card.  The only calls expected to fail are ones a launcher's host-side argument check refuses before any launch."""
import ctypes
import math
import os
import sys
import traceback

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_kernels_ref as R  # noqa: E402
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402
from seq2seq_vc_amd.ops import kernels_aas as KA  # noqa: E402
from seq2seq_vc_amd.ops import kernels_decode as KD  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = -776.0                 # finite, not zero, exact in bf16
ISENT = -7777
CASES = []
# Checks whose kernel is correct and yet takes more than 4 d: 1.5 x the measured margin, with the cause (profiles/AB_LOG.md has the runs).
MEASURED_MARGINS = {}


def case(fn):
    CASES.append(fn)
    return fn


def both_dtypes(fn):
    def run():
        return fn(F32) + fn(BF16)
    run.__name__ = fn.__name__
    run.__doc__ = fn.__doc__
    return run


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def sent(shape, dtype):
    return torch.full(shape, ISENT if dtype in (torch.int32, torch.int64) else SENT, dtype=dtype, device=DEV)


def same_bits(a, b):
    """Bit-for-bit equality, wherever the tensors live."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {F32: torch.int32, BF16: torch.int16, F64: torch.int64}.get(a.dtype)
    a, b = a.contiguous(), b.to(a.device).contiguous()
    return bool(torch.equal(a.view(view), b.view(view))) if view is not None else bool(torch.equal(a, b))


def name_of(dtype):
    return "fp32" if dtype == F32 else "bf16"


class Tally:
    """The float comparisons and exact conditions of one PASS/FAIL line."""

    def __init__(self, key=None):
        self.fail, self.n, self.ratio, self.where, self.d, self.need = [], 0, 0.0, "-", 0.0, 0.0
        self.margin = MEASURED_MARGINS.get(key, R.MARGIN)

    def close(self, where, got, ref64, yard, out_dtype):
        ok, ratio, d, msg = R.compare(got, ref64, yard, out_dtype, self.margin)
        self.n += 1
        if d > 0:                                             # the margin this comparison takes once the ulp of the output is spent
            r64 = ref64.detach().to(F64)
            err = (got.detach().to(r64.device).to(F64) - r64).abs() - R.ulp_out(r64, out_dtype)
            self.need = max(self.need, float(err.max()) / d)
        if not ok:
            self.fail.append(f"{where}: {msg}")
        if math.isfinite(ratio) and ratio >= self.ratio:
            self.ratio, self.where, self.d = ratio, where, d
        return ok

    def exact(self, where, cond, what):
        if not cond:
            self.fail.append(f"{where}: {what}")
        return cond

    def line(self, name, extra=""):
        if self.fail:
            more = f" (+{len(self.fail) - 3} more)" if len(self.fail) > 3 else ""
            return False, f"{name}: " + "; ".join(self.fail[:3]) + more
        tail = (f"{self.n} comparisons, max|got - ref64| / d = {self.ratio:.3f} at {self.where} (d {self.d:.2e}), margin used {self.need:.2f} of {self.margin:g}"
                if self.n else "exact")
        return True, f"{name}: {tail}{extra}"


def refused(res, name, fn, expect, untouched=()):
    """fn() must raise the launcher's own message, and every (tensor, copy) pair of `untouched` must still agree bit for bit."""
    try:
        fn()
        ok, msg = False, "the call was accepted"
    except RuntimeError as e:
        ok, msg = expect in str(e), str(e)
    torch.cuda.synchronize()
    clean = all(same_bits(t, c) for t, c in untouched)
    res.append((ok and clean, f"{name}: refused with '{expect}'" + ("" if clean else ", BUT an output changed") if ok else f"{name}: wanted '{expect}', got: {msg}"))


# ---------------------------------------------------------------------------------------------------------------------------
# decode step: positional encoding, attention over the cache, emit / advance
# ---------------------------------------------------------------------------------------------------------------------------
@case
@both_dtypes
def decode_posenc_kernel(dtype):
    """B * D = 240 (no multiple of 256), the first and the last row of the table, alpha given and absent."""
    t = Tally()
    B, D, rows = 3, 80, 12
    xscale = R.f32(math.sqrt(D))
    x, pe = R.randn(B, D, seed=11, dtype=dtype), R.randn(rows, D, seed=12)
    for pos in (0, rows - 1):
        for alpha in (torch.tensor([0.7]), None):
            buf = sent((B * D + 16,), dtype)
            y = buf[:B * D].view(B, D)
            KD.decode_posenc(x.to(DEV), xscale, None if alpha is None else alpha.to(DEV), pe.to(DEV), i32([pos]), y)
            where = f"pos {pos}, alpha {'given' if alpha is not None else 'None'}"
            t.close(where, y, R.decode_posenc(x, xscale, alpha, pe, pos, F64), R.decode_posenc(x, xscale, alpha, pe, pos, F32, dtype == BF16), dtype)
            t.exact(where, bool((buf[B * D:] == SENT).all()), "wrote behind the B * D outputs")
    return [t.line(f"decode_posenc[{name_of(dtype)}] B 3, D 80")]


DKS = (3, 8, 20, 64, 96, 256)
TKS = (1, 63, 64, 65, 257, 700)


def _attn_call(q, q_off, ldq, kc, k_off, vc, v_off, ldt, cbs, new, kn_off, vn_off, ldn, pos, klen, Tk, scale, B, H, dk, rows):
    """One launch into sentinel-filled outputs: ctx (B, D + 4) and att (B, H, rows, Tk + 3).  -> ctx, att (on the device)."""
    D = H * dk
    ctx, att = sent((B, D + 4), q.dtype), sent((B, H, rows, Tk + 3), F32)
    KD.decode_attn(q, q_off, ldq, kc, k_off, vc, v_off, ldt, cbs, new, kn_off, vn_off, ldn, pos, klen, Tk, scale, ctx, B, H, dk,
                   att=att, att_strides=(att.stride(0), att.stride(1), att.stride(2)))
    return ctx, att


def _attn_verdict(tc, ta, where, ctx, att, p, qh, kh, vh, n, scale, dtype):
    """ctx / att of one launch against the restatement; everything outside (the ctx pad columns, the other attention rows, the columns behind
    Tk) against the sentinel; exact zeros behind n."""
    B, H, dk = qh.shape
    Tk, D = kh.shape[1], H * dk
    r64c, r64a = R.decode_attn(qh, kh, vh, n, scale, F64)
    y32c, y32a = R.decode_attn(qh, kh, vh, n, scale, F32, dtype == BF16)
    tc.close(where, ctx[:, :D].reshape(B, H, dk), r64c, y32c, dtype)
    row = att[:, :, p, :Tk]
    ta.close(where, row, r64a, y32a, F32)
    tc.exact(where, bool((ctx[:, D:] == SENT).all()), "ctx columns behind H * dk were written")
    for b in range(B):
        nb = max(0, min(int(n[b]), Tk))
        ta.exact(where, bool((row[b, :, nb:] == 0).all()), f"row {b}: attention behind its {nb} keys is not exactly 0")
    rest = att.clone()
    rest[:, :, p, :Tk] = SENT
    ta.exact(where, bool((rest == SENT).all()), "attention rows other than pos, or columns behind Tk, were written")
    ta.exact(where, bool(torch.isfinite(ctx[:, :D]).all() and torch.isfinite(row).all()), "non-finite output")


def _decode_attn_self(dtype):
    """Self-attention as decode.py lays it out: q | knew | vnew inside one packed (B, 3D) projection, caches (B, Lcap, D)."""
    res, B = [], 3
    for dk in DKS:
        tc, ta, tx = Tally(), Tally(), Tally()
        for i, Tk in enumerate(TKS):
            H = (1, 4)[i % 2]
            D, scale = H * dk, R.f32(1.0 / math.sqrt(dk))
            kc0, vc0 = R.randn(B, Tk, D, seed=100 + dk + i, dtype=dtype), R.randn(B, Tk, D, seed=200 + dk + i, dtype=dtype)
            kc, vc = kc0.to(DEV), vc0.to(DEV)
            mk, mv = kc0.clone(), vc0.clone()                       # the CPU mirror of the caches
            for pos in sorted({p for p in (0, 63, 64, Tk - 1) if p < Tk}):
                where = f"H {H}, Tk {Tk}, pos {pos}"
                qkv = R.randn(B, 3 * D, seed=300 + 7 * pos + dk + i, dtype=dtype)
                qd = qkv.to(DEV)
                before_k, before_v = kc.clone(), vc.clone()
                ctx, att = _attn_call(qd, 0, 3 * D, kc, 0, vc, 0, D, Tk * D, qd, D, 2 * D, 3 * D, i32([pos]), None, Tk, scale, B, H, dk, pos + 1)
                mk[:, pos], mv[:, pos] = qkv[:, D:2 * D], qkv[:, 2 * D:]
                tx.exact(where, same_bits(kc[:, pos], mk[:, pos]) and same_bits(vc[:, pos], mv[:, pos]), "the appended key / value row differs from knew / vnew")
                before_k[:, pos], before_v[:, pos] = kc[:, pos], vc[:, pos]
                tx.exact(where, same_bits(kc, before_k) and same_bits(vc, before_v), "a cache row other than pos changed")
                _attn_verdict(tc, ta, where, ctx.cpu(), att.cpu(), pos, qkv[:, :D].view(B, H, dk), mk.view(B, Tk, H, dk), mv.view(B, Tk, H, dk),
                              [pos + 1] * B, scale, dtype)
        res += [tc.line(f"decode_attn self[{name_of(dtype)}] dk {dk}: context"), ta.line(f"decode_attn self[{name_of(dtype)}] dk {dk}: attention row"),
                tx.line(f"decode_attn self[{name_of(dtype)}] dk {dk}: cache append, other rows untouched")]
    # the cache views one element off a 16-byte boundary: the element-wise instantiation at dk = 64; and row b of the B = 3 call == the B = 1 call
    tc, ta, tx = Tally(), Tally(), Tally()
    H, dk, Tk, pos = 4, 64, 65, 64
    D, scale = H * dk, R.f32(1.0 / math.sqrt(dk))
    kc0, vc0 = R.randn(B, Tk, D, seed=401, dtype=dtype), R.randn(B, Tk, D, seed=402, dtype=dtype)
    qkv = R.randn(B, 3 * D, seed=403, dtype=dtype)

    def off_by_one(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        flat[1:] = t.reshape(-1).to(DEV)
        return flat[1:].view(t.shape)
    kc, vc, qd = off_by_one(kc0), off_by_one(vc0), qkv.to(DEV)
    ctx, att = _attn_call(qd, 0, 3 * D, kc, 0, vc, 0, D, Tk * D, qd, D, 2 * D, 3 * D, i32([pos]), None, Tk, scale, B, H, dk, Tk)
    mk, mv = kc0.clone(), vc0.clone()
    mk[:, pos], mv[:, pos] = qkv[:, D:2 * D], qkv[:, 2 * D:]
    tx.exact("offset view", same_bits(kc, mk) and same_bits(vc, mv), "cache after the append differs")
    _attn_verdict(tc, ta, "caches offset by one element", ctx.cpu(), att.cpu(), pos, qkv[:, :D].view(B, H, dk), mk.view(B, Tk, H, dk), mv.view(B, Tk, H, dk),
                  [pos + 1] * B, scale, dtype)
    for b in range(B):
        k1, v1, q1 = kc0[b:b + 1].to(DEV), vc0[b:b + 1].to(DEV), qkv[b:b + 1].to(DEV)
        c1, a1 = _attn_call(q1, 0, 3 * D, k1, 0, v1, 0, D, Tk * D, q1, D, 2 * D, 3 * D, i32([pos]), None, Tk, scale, 1, H, dk, Tk)
        k3, v3 = kc0.to(DEV), vc0.to(DEV)
        c3, a3 = _attn_call(qd, 0, 3 * D, k3, 0, v3, 0, D, Tk * D, qd, D, 2 * D, 3 * D, i32([pos]), None, Tk, scale, B, H, dk, Tk)
        tx.exact(f"row {b}", same_bits(c3[b:b + 1], c1) and same_bits(a3[b:b + 1], a1) and same_bits(k3[b:b + 1], k1), "B = 3 row differs from the B = 1 call")
    res += [tc.line(f"decode_attn self[{name_of(dtype)}] dk 64, caches offset by one element: context"),
            ta.line(f"decode_attn self[{name_of(dtype)}] dk 64, caches offset by one element: attention row"),
            tx.line(f"decode_attn self[{name_of(dtype)}] offset append; rows of a B = 3 call equal the B = 1 calls")]
    return res


@case
def decode_attn_self_fp32():
    return _decode_attn_self(F32)


@case
def decode_attn_self_bf16():
    return _decode_attn_self(BF16)


def _decode_attn_cross(dtype):
    """Source attention as decode.py lays it out: K and V interleaved in one (B, Tcap, 2D) buffer, V at offset D; per-row klen."""
    res, B, pos, rows = [], 3, 2, 4
    for dk in DKS:
        tc, ta = Tally(), Tally()
        for i, Tk in enumerate(TKS):
            H = (4, 1)[i % 2]
            D, scale = H * dk, R.f32(1.0 / math.sqrt(dk))
            kv = R.randn(B, Tk, 2 * D, seed=500 + dk + i, dtype=dtype)
            q = R.randn(B, D, seed=600 + dk + i, dtype=dtype)
            kvd, qd = kv.to(DEV), q.to(DEV)
            kh, vh = kv[:, :, :D].reshape(B, Tk, H, dk), kv[:, :, D:].reshape(B, Tk, H, dk)
            for klen in (None, [1, 64, 65], [Tk, Tk + 5, 0]):
                where = f"H {H}, Tk {Tk}, klen {klen}"
                ctx, att = _attn_call(qd, 0, D, kvd, 0, kvd, D, 2 * D, Tk * 2 * D, None, 0, 0, 0, i32([pos]), None if klen is None else i32(klen), Tk,
                                      scale, B, H, dk, rows)
                n = [Tk] * B if klen is None else klen
                ctx, att = ctx.cpu(), att.cpu()
                _attn_verdict(tc, ta, where, ctx, att, pos, q.view(B, H, dk), kh, vh, n, scale, dtype)
                for b in range(B):
                    if int(n[b]) == 0:        # today's behaviour for a row without keys: context 0, attention row 0, nothing non-finite
                        tc.exact(where, bool((ctx[b, :D] == 0).all()), f"row {b} has no key but its context is not 0")
                        ta.exact(where, bool((att[b, :, pos, :Tk] == 0).all()), f"row {b} has no key but its attention row is not 0")
            tc.exact(f"Tk {Tk}", same_bits(kvd, kv), "the source K | V buffer changed")
        res += [tc.line(f"decode_attn cross[{name_of(dtype)}] dk {dk}: context"), ta.line(f"decode_attn cross[{name_of(dtype)}] dk {dk}: attention row")]
    # scaled scores of about +-80; the K | V buffer one element off a 16-byte boundary; row b of the B = 3 call == the B = 1 call
    tc, ta, tx = Tally(), Tally(), Tally()
    H, dk, Tk = 4, 64, 257
    D, scale = H * dk, R.f32(1.0 / math.sqrt(dk))
    kv, q = R.randn(B, Tk, 2 * D, seed=701, dtype=dtype), R.randn(B, D, seed=702, dtype=dtype)
    kh, vh = kv[:, :, :D].reshape(B, Tk, H, dk), kv[:, :, D:].reshape(B, Tk, H, dk)
    s = torch.einsum("bthd,bhd->bht", kh.double(), q.view(B, H, dk).double()) * scale
    qbig = (q.double().view(B, H, dk) * (80.0 / s.abs().amax(-1, keepdim=True))).view(B, D).to(dtype)
    sbig = float((torch.einsum("bthd,bhd->bht", kh.double(), qbig.view(B, H, dk).double()) * scale).abs().max())
    ctx, att = _attn_call(qbig.to(DEV), 0, D, kv.to(DEV), 0, kv.to(DEV), D, 2 * D, Tk * 2 * D, None, 0, 0, 0, i32([pos]), None, Tk, scale, B, H, dk, rows)
    _attn_verdict(tc, ta, f"scaled scores up to +-{sbig:.1f}", ctx.cpu(), att.cpu(), pos, qbig.view(B, H, dk), kh, vh, [Tk] * B, scale, dtype)
    flat = torch.empty(kv.numel() + 1, dtype=dtype, device=DEV)
    flat[1:] = kv.reshape(-1).to(DEV)
    kvo = flat[1:].view(B, Tk, 2 * D)
    klen = [65, Tk, 1]
    ctx, att = _attn_call(q.to(DEV), 0, D, kvo, 0, kvo, D, 2 * D, Tk * 2 * D, None, 0, 0, 0, i32([pos]), i32(klen), Tk, scale, B, H, dk, rows)
    _attn_verdict(tc, ta, "K | V offset by one element", ctx.cpu(), att.cpu(), pos, q.view(B, H, dk), kh, vh, klen, scale, dtype)
    c3, a3 = _attn_call(q.to(DEV), 0, D, kv.to(DEV), 0, kv.to(DEV), D, 2 * D, Tk * 2 * D, None, 0, 0, 0, i32([pos]), i32(klen), Tk, scale, B, H, dk, rows)
    for b in range(B):
        kv1 = kv[b:b + 1].to(DEV)
        c1, a1 = _attn_call(q[b:b + 1].to(DEV), 0, D, kv1, 0, kv1, D, 2 * D, Tk * 2 * D, None, 0, 0, 0, i32([pos]), i32(klen[b:b + 1]), Tk, scale, 1, H, dk, rows)
        tx.exact(f"row {b}", same_bits(c3[b:b + 1], c1) and same_bits(a3[b:b + 1], a1), "B = 3 row differs from the B = 1 call")
    res += [tc.line(f"decode_attn cross[{name_of(dtype)}] dk 64, scores +-80 and offset view: context"),
            ta.line(f"decode_attn cross[{name_of(dtype)}] dk 64, scores +-80 and offset view: attention row"),
            tx.line(f"decode_attn cross[{name_of(dtype)}] rows of a B = 3 call equal the B = 1 calls")]
    return res


@case
def decode_attn_cross_fp32():
    return _decode_attn_cross(F32)


@case
def decode_attn_cross_bf16():
    return _decode_attn_cross(BF16)


@case
@both_dtypes
def decode_emit_then_advance(dtype):
    """Six positions of decode_emit + decode_advance against the plain-Python stop rule (vtn.py:378-381), and against decode_emit_advance on
    the same inputs, bit for bit."""
    res = []
    for r in (1, 4):
        for odim in (20, 81):
            t, tp = Tally(), Tally()
            B, L, stride = 5, 6, 0x10001
            lg, minlen, maxlen, stop0, want = R.emit_rows(r)
            feats = R.randn(L, B, r * odim, seed=800 + r + odim, dtype=dtype)
            packed = torch.cat([feats, lg.transpose(0, 1).to(dtype)], dim=2).to(DEV)             # (L, B, r * odim + r)

            def state():
                return dict(outs=sent((B, (L + 1) * r * odim), F32), probs=sent((B, (L + 1) * r), F32), prev=sent((B, odim), dtype),
                            stop_at=i32(stop0), pos=i32([0]), seed=torch.tensor([12345], dtype=torch.int64, device=DEV))
            a, f = state(), state()
            ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
            mn, mx = i32(minlen), i32(maxlen)
            for p in range(L):
                KD.decode_emit(packed[p, :, :r * odim].contiguous(), packed[p, :, r * odim:].contiguous(), r, odim, 0.5, mn, mx, a["pos"], a["outs"],
                               a["probs"], a["prev"], a["stop_at"])
                KD.decode_advance(a["pos"], a["seed"].data_ptr(), stride)
                KD.decode_emit_advance(packed[p], r, odim, 0.5, mn, mx, f["pos"], f["outs"], f["probs"], f["prev"], f["stop_at"], f["seed"].data_ptr(),
                                       stride, ticket)
            where = f"r {r}, odim {odim}"
            outs = a["outs"].cpu()
            t.exact(where, same_bits(outs[:, :L * r * odim].reshape(B, L, r * odim), feats.float().transpose(0, 1).contiguous()), "frames differ from feat")
            t.exact(where, bool((outs[:, L * r * odim:] == SENT).all()) and bool((a["probs"][:, L * r:] == SENT).all()), "wrote behind position 5")
            t.exact(where, same_bits(a["prev"].cpu(), feats[L - 1, :, (r - 1) * odim:]), "prev is not the last of the r frames")
            t.exact(where, a["stop_at"].tolist() == want, f"stop_at {a['stop_at'].tolist()}, the rule gives {want}")
            t.exact(where, int(a["pos"]) == L and int(a["seed"]) == 12345 + L * stride, "pos / seed after six advances")
            for k in ("outs", "probs", "prev", "stop_at", "pos", "seed"):
                t.exact(where, same_bits(a[k], f[k]), f"decode_emit + decode_advance and decode_emit_advance differ in {k}")
            x = lg.to(dtype)
            tp.close(where, a["probs"][:, :L * r].cpu().reshape(B, L, r), torch.sigmoid(x.double()), torch.sigmoid(x.float()), F32)
            res += [t.line(f"decode_emit / advance[{name_of(dtype)}] {where}: frames, prev, stop rule {want}, equals decode_emit_advance"),
                    tp.line(f"decode_emit[{name_of(dtype)}] {where}: stop probabilities")]
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm -> Linear of a decode step
# ---------------------------------------------------------------------------------------------------------------------------
LN_KS = {BF16: (8, 80, 384, 392, 768, 1536), F32: (4, 80, 192, 196, 384, 768)}
LN_MS = (1, 16, 17, 32, 33, 48, 49, 64)
LN_NS = (1, 16, 17, 324, 1152)


def _ln_linear_into(out, x, w, bias, norm=None, act=None, res=None, y_out=None, drop_p=0.0, seed=(None, 0)):
    """KD.ln_linear writing into a caller's `out` view (row stride = ldc), so that the columns behind N can be watched."""
    M, Kd = x.shape
    N = w.shape[0]
    d = _lib.GemmDesc()
    d.A, d.B = K.operand(x, x.stride(0)), K.operand(w, w.stride(0))
    d.C, d.ldc, d.c_dtype = out.data_ptr(), out.stride(0), K.dt(out)
    d.bias, d.res, d.ldr = K.ptr(bias), K.ptr(res), (res.stride(0) if res is not None else N)
    d.M, d.N, d.K, d.nb0, d.nb1 = M, N, Kd, 1, 1
    d.act, d.alpha, d.dtype, d.splitk = K.ACT[act], 1.0, K.dt(x), 1
    if drop_p > 0.0:
        d.drop_p, d.seed_base, d.seed_off = drop_p, seed[0], seed[1]
    g, b, eps = (None, None, 0.0) if norm is None else norm
    _lib.check(_lib.lib().s2svc_decode_ln_linear(ctypes.byref(d), K.ptr(g), K.ptr(b), float(eps), K.ptr(y_out), y_out.stride(0) if y_out is not None else 0,
                                                 K.stream()), "decode_ln_linear")


def _ln_linear(dtype):
    res = []
    vec = 4 if dtype == F32 else 8
    for Kd in LN_KS[dtype]:
        t, ty = Tally(), Tally()
        w = R.randn(max(LN_NS), Kd, seed=900 + Kd, scale=1.0 / math.sqrt(Kd), dtype=dtype)
        bias, gamma, beta = R.randn(max(LN_NS), seed=901 + Kd), 1.0 + 0.2 * R.randn(Kd, seed=902 + Kd), 0.3 * R.randn(Kd, seed=903 + Kd)
        for iM, M in enumerate(LN_MS):
            if Kd == LN_KS[dtype][-1] and M > 32:
                continue                                      # 12 k-steps per wave: up to M = 32
            x = R.randn(M, Kd, seed=910 + Kd + M, dtype=dtype)
            x[0] = 0.5                                        # a constant row: variance 0, where only eps keeps rstd finite
            if M > 1:
                x[1] = (x[1].float() * 1e-2).to(dtype)        # a row whose variance is of the order of the larger eps
            rs = R.randn(M, max(LN_NS), seed=920 + Kd + M, dtype=dtype)
            xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
            for iN, N in enumerate(LN_NS):
                opt = (iM + iN) % 5
                eps = R.f32(1e-12 if iN % 2 == 0 else 1e-5)
                norm = None if opt == 1 else (gamma, beta, eps)
                act = "relu" if opt in (2, 4) else None
                r_ = rs[:, :N].contiguous() if opt in (3, 4) else None
                wd, bsd = w[:N].contiguous().to(DEV), bias[:N].contiguous().to(DEV)
                where = f"M {M}, N {N}, {('LN', 'plain linear', 'LN relu', 'LN res', 'LN relu res y_out')[opt]}, eps {eps:g}"
                ybuf = sent((M, Kd + vec), dtype) if opt == 4 else None
                kw = dict(norm=None if norm is None else (gd, bd, eps), act=act, res=None if r_ is None else r_.to(DEV),
                          y_out=None if ybuf is None else ybuf[:, :Kd])
                if opt == 0 and N in (17, 324):               # a padded C: the columns behind N stay as they were
                    obuf = sent((M, N + 7), dtype)
                    _ln_linear_into(obuf[:, :N], xd, wd, bsd, **kw)
                    out = obuf[:, :N]
                    t.exact(where, bool((obuf[:, N:] == SENT).all()), "columns behind N of a padded C were written")
                else:
                    out = KD.ln_linear(xd, wd, bsd, **kw)
                r64, y64 = R.ln_linear(x, w[:N], bias[:N], norm, act, r_, F64)
                y32, yy32 = R.ln_linear(x, w[:N], bias[:N], norm, act, r_, F32, dtype == BF16)
                t.close(where, out, r64, y32, dtype)
                if ybuf is not None:
                    ty.close(where, ybuf[:, :Kd], y64, yy32, dtype)
                    ty.exact(where, bool((ybuf[:, Kd:] == SENT).all()), "the pad columns of y_out were written")
        res += [t.line(f"ln_linear[{name_of(dtype)}] K {Kd}: output"), ty.line(f"ln_linear[{name_of(dtype)}] K {Kd}: y_out = LayerNorm(x), padded ldy")]
    return res


@case
def ln_linear_fp32():
    return _ln_linear(F32)


@case
def ln_linear_bf16():
    return _ln_linear(BF16)


@case
@both_dtypes
def ln_linear_dropout(dtype):
    """The dropout stage at p = 0.5: reproducible for a seed, the mask K.gemm draws for that seed, kept values doubled, half of them kept."""
    res = []
    K.manual_seed(4321)
    for (M, N, Kd) in ((64, 1152, 384 if dtype == BF16 else 192), (17, 324, 80)):
        x, w, bias = R.randn(M, Kd, seed=1000 + M, dtype=dtype), R.randn(N, Kd, seed=1001 + M, scale=0.1, dtype=dtype), R.randn(N, seed=1002 + M)
        gamma, beta = 1.0 + 0.2 * R.randn(Kd, seed=1003), 0.3 * R.randn(Kd, seed=1004)
        xd, wd, bd, norm = x.to(DEV), w.to(DEV), bias.to(DEV), (gamma.to(DEV), beta.to(DEV), 1e-12)
        sd = K.new_seed(xd.device)
        plain = KD.ln_linear(xd, wd, bd, norm=norm)
        o1 = KD.ln_linear(xd, wd, bd, norm=norm, drop_p=0.5, seed=sd)
        o2 = KD.ln_linear(xd, wd, bd, norm=norm, drop_p=0.5, seed=sd)
        og = torch.empty(M, N, dtype=dtype, device=DEV)
        K.gemm(K.operand(xd, Kd), K.operand(wd, Kd), M, N, Kd, og, in_dtype=dtype, bias=bd, drop_p=0.5, seed=sd)
        t = Tally()
        where = f"{M} x {N} x {Kd}"
        t.exact(where, same_bits(o1, o2), "two calls with one seed differ")
        t.exact(where, bool(torch.equal(o1 == 0, og == 0)), "the zero pattern differs from K.gemm's for the same seed and drop_p")
        kept = o1 != 0
        t.exact(where, same_bits(torch.where(kept, o1, torch.zeros_like(o1)), torch.where(kept, plain * 2, torch.zeros_like(o1))), "kept values are not the undropped result x 2")
        frac = float(kept.float().mean())
        if M * N == 64 * 1152:                                 # 5 standard deviations of a fair coin over 73728 draws: 5 * 0.5 / sqrt(73728) = 0.0092
            t.exact(where, abs(frac - 0.5) <= 0.0092, f"kept fraction {frac:.4f} is not within 0.0092 of 0.5")
        res.append(t.line(f"ln_linear dropout[{name_of(dtype)}] {where}: reproducible, K.gemm's mask, kept = 2 x undropped, kept fraction {frac:.4f}"))
    return res


@case
def ln_linear_supported_agrees_with_the_launcher():
    """Where ln_linear_supported answers 1 the launcher runs; where it answers 0 the launcher returns its error and writes nothing."""
    t, res = Tally(), []
    for dtype, M, Kd, want in R.ln_linear_supported_table():
        where = f"{name_of(dtype)} M {M} K {Kd}"
        got = KD.ln_linear_supported(dtype, M, Kd)
        t.exact(where, got == bool(want), f"supported() says {got}, the table {bool(want)}")
        if M == 0 or Kd == 0:
            continue
        N = 17
        x, w, bias = R.randn(M, Kd, seed=1100, dtype=dtype).to(DEV), R.randn(N, Kd, seed=1101, dtype=dtype).to(DEV), R.randn(N, seed=1102).to(DEV)
        norm = (torch.ones(Kd, device=DEV), torch.zeros(Kd, device=DEV), 1e-12)
        out, ybuf = sent((M, N), dtype), sent((M, Kd + 8), dtype)
        try:
            _ln_linear_into(out, x, w, bias, norm=norm, y_out=ybuf[:, :Kd] if (Kd + 8) % (4 if dtype == F32 else 8) == 0 else None)
            torch.cuda.synchronize()
            ran, msg = True, ""
        except RuntimeError as e:
            ran, msg = False, str(e)
        t.exact(where, ran == got, f"supported() says {got} but the launcher {'ran' if ran else 'refused: ' + msg}")
        if not ran:
            t.exact(where, "decode_ln_linear" in msg and bool((out == SENT).all()) and bool((ybuf == SENT).all()), f"refusal wrote an output or has no message: {msg}")
        else:
            t.exact(where, bool((out != SENT).all()), "an accepted call left outputs unwritten")
    res.append(t.line("ln_linear_supported == the launcher over the boundary table (per 6 -> 7 at M 33, 12 -> 13, K % vec, M 65)"))
    # a misaligned operand is refused too
    x = torch.empty(16 * 80 + 1, dtype=F32, device=DEV)[1:].view(16, 80)
    out = sent((16, 17), F32)
    refused(res, "ln_linear, x one element off a 16-byte boundary",
            lambda: _ln_linear_into(out, x, torch.zeros(17, 80, device=DEV), torch.zeros(17, device=DEV)), "decode_ln_linear: 16-byte aligned operands",
            [(out, sent((16, 17), F32))])
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------
def _seq_loss_inputs(B, Tm, D, olens, dtype, seed):
    ys = R.randn(B, Tm, D, seed=seed)
    before = (ys + 0.5 * R.randn(B, Tm, D, seed=seed + 1)).to(dtype)
    after = (ys + 0.3 * R.randn(B, Tm, D, seed=seed + 2)).to(dtype)
    ys[0, min(3, Tm - 1)] = after[0, min(3, Tm - 1)].float()                   # predictions exactly equal to the target: gradient 0, as torch.sign
    ys[B - 1, 0, 0] = before[B - 1, 0, 0].float()
    logits = (3.0 * R.randn(B, Tm, seed=seed + 3))
    labels = (torch.rand(B, Tm, generator=R.gen(seed + 4)) < 0.2).float()
    for j, v in enumerate((30.0, -30.0, 90.0, -90.0, 90.0, -90.0)):          # inside row 0 (full length), both labels at the extremes
        if j < Tm:
            logits[0, j], labels[0, j] = v, float(j % 2 if j < 4 else (j + 1) % 2)
    return after, before, logits.to(dtype), ys, labels


def _seq_loss(dtype):
    res = []
    t_out, t_g, t_x = Tally(f"seq_loss_fwd[{name_of(dtype)}]"), Tally(), Tally()
    ncalls = 0
    shapes = [(5, 37, 1, [37, 1, 0, 20, 36]), (5, 37, 80, [37, 1, 0, 20, 36]), (5, 700, 80, [700, 1, 0, 350, 699])]     # the last: > 1024 * 256 elements
    for (B, Tm, D, olens) in shapes:
        after, before, logits, ys, labels = _seq_loss_inputs(B, Tm, D, olens, dtype, seed=1200 + D + Tm)
        big = Tm > 100
        variants = [(10.0, True, True, True)] if big else [(pw, a, l, g) for pw in (1.0, 10.0) for (a, l) in ((True, True), (False, True), (True, False))
                                                            for g in (True, False)]
        m = R.frame_mask(olens, Tm)
        for (pw, has_a, has_l, has_g) in variants:
            a_, l_ = (after if has_a else None), (logits if has_l else None)
            g1, g2 = (torch.tensor([0.7]), torch.tensor([1.3])) if has_g else (None, None)
            where = f"B {B} Tm {Tm} D {D} pos_weight {pw:g}" + ("" if has_a else " after=None") + ("" if has_l else " logits=None") + (" g given" if has_g else "")
            dv = lambda x: None if x is None else x.to(DEV)          # noqa: E731
            out = K.seq_loss_fwd(dv(a_), dv(before), dv(l_), dv(ys), dv(labels), i32(olens), pw)
            da, db, dl = K.seq_loss_bwd(dv(a_), dv(before), dv(l_), dv(ys), dv(labels), i32(olens), pw, out, dv(g1), dv(g2))
            kw = dict(g_l1=None if g1 is None else float(g1), g_bce=None if g2 is None else float(g2), want_grads=True)
            r64 = R.seq_loss(a_, before, l_, ys, labels, olens, pw, F64, **kw)
            y32 = R.seq_loss_stock(a_, before, l_, ys, labels, olens, pw, F32, bf16=dtype == BF16, **kw)
            o = out.cpu()
            t_x.exact(where, float(o[2]) == float(r64[2]), f"count {float(o[2])}, {r64[2]} valid frames")
            ncalls += 1
            t_out.close(f"{where} l1", o[0:1], r64[0].reshape(1), y32[0].reshape(1), F32)       # a scalar is a tensor of one element: its own d
            t_out.close(f"{where} bce", o[1:2], r64[1].reshape(1), y32[1].reshape(1), F32)
            for nm, got, a64, a32 in (("d_after", da, r64[3], y32[3]), ("d_before", db, r64[4], y32[4]), ("d_logits", dl, r64[5], y32[5])):
                if a64 is None:
                    t_x.exact(where, got is None, f"{nm} returned without its input")
                    continue
                got = got.cpu()
                t_g.close(f"{where} {nm}", got, a64, a32, dtype)
                mask = m if got.dim() == 2 else m[:, :, None].expand_as(got)
                t_x.exact(where, bool((got[~mask] == 0).all()), f"{nm} of a masked frame is not exactly 0")
            t_x.exact(where, bool((db.cpu()[B - 1, 0, 0] == 0)) and (da is None or bool((da.cpu()[0, min(3, Tm - 1)] == 0).all())), "gradient where prediction == target is not 0")
    res += [t_out.line(f"seq_loss_fwd[{name_of(dtype)}] l1 and bce of {ncalls} calls, each against its own d (D 1 / 80, olens with 0, 1, full; 280000 elements)"),
            t_g.line(f"seq_loss_bwd[{name_of(dtype)}] d_after / d_before / d_logits"),
            t_x.line(f"seq_loss[{name_of(dtype)}] count exact, masked frames and prediction == target give exactly 0")]
    return res


@case
def seq_loss_fp32():
    return _seq_loss(F32)


@case
def seq_loss_bf16():
    return _seq_loss(BF16)


@case
@both_dtypes
def guided_attn_loss(dtype):
    res = []
    t_l, t_g, t_x = Tally(f"guided_attn_loss_fwd[{name_of(dtype)}]"), Tally(), Tally()
    B, H = 3, 2
    for (To, Ti, ilens, olens) in ((1, 1, [1, 1, 0], [1, 1, 1]), (37, 29, [29, 1, 0], [37, 1, 12]), (37, 29, [29, 13, 29], [37, 20, 0]),
                                   (37, 29, [35, 29, 7], [37, 50, 9]),                           # lengths above Ti / To count as Ti / To
                                   (300, 160, [160, 1, 77], [300, 1, 0])):                       # the last: 288000 elements > 1024 * 256
        att = torch.rand(B, H, To, Ti, generator=R.gen(1300 + To)).to(dtype)
        for sigma in ((0.4, 0.2) if To < 100 else (0.4,)):
            for gout in (None, torch.tensor([0.6])):
                where = f"To {To} Ti {Ti} ilens {ilens} olens {olens} sigma {sigma}" + (" gout given" if gout is not None else "")
                sg, al = R.f32(sigma), 5.0
                out = K.guided_attn_loss_fwd(att.to(DEV), i32(ilens), i32(olens), sg, al)
                got_d = K.guided_attn_loss_bwd((B, H, To, Ti), dtype, torch.device(DEV), i32(ilens), i32(olens), sg, al, out, None if gout is None else gout.to(DEV))
                g = None if gout is None else float(gout)
                l64, cnt, d64 = R.guided_attn_loss(att, ilens, olens, sg, al, F64, g)
                l32, _, d32 = R.guided_attn_loss(att, ilens, olens, sg, al, F32, g, dtype == BF16)
                o = out.cpu()
                t_x.exact(where, float(o[1]) == float(cnt), f"count {float(o[1])}, {cnt} valid elements")
                t_l.close(where, o[0:1], l64.reshape(1), l32.reshape(1), F32)
                t_g.close(where, got_d, d64, d32, dtype)
    res += [t_l.line(f"guided_attn_loss_fwd[{name_of(dtype)}] each loss against its own d (alpha 5, sigma 0.4 / 0.2, zero-length rows, lengths above To / Ti, 288000 elements)"),
            t_g.line(f"guided_attn_loss_bwd[{name_of(dtype)}] datt"), t_x.line(f"guided_attn_loss[{name_of(dtype)}] count exact")]
    return res


@case
def loss_backward_launchers_refuse_empty_problems():
    """Each loss launcher refuses an empty problem exactly where its forward does, before any launch; s2svc_mas_binloss_bwd returns cleanly for
    an empty batch, as s2svc_mas does."""
    res = []
    L = _lib.lib()
    z32 = lambda *s: torch.zeros(*s, device=DEV)          # noqa: E731
    for (B, Tm, D) in ((0, 5, 4), (2, 0, 4), (2, 5, 0)):
        e = torch.empty(B, Tm, D, device=DEV)
        refused(res, f"seq_loss_fwd B {B} Tm {Tm} D {D}", lambda: K.seq_loss_fwd(e, e, None, e, None, i32([1] * B), 1.0), "seq_loss_fwd: bad args")
        refused(res, f"seq_loss_bwd B {B} Tm {Tm} D {D}", lambda: K.seq_loss_bwd(e, e, None, e, None, i32([1] * B), 1.0, z32(3), None, None), "seq_loss_bwd: bad args")
        # the same through the C ABI with real, sentinel-filled outputs: nothing is written
        buf, keep = sent((64,), F32), sent((64,), F32)
        src = z32(64)
        rc = L.s2svc_seq_loss_bwd(0, B, Tm, D, src.data_ptr(), src.data_ptr(), None, src.data_ptr(), None, i32([1, 1]).data_ptr(), 1.0, z32(3).data_ptr(), None, None,
                                  buf.data_ptr(), buf.data_ptr(), None, K.stream())
        torch.cuda.synchronize()
        res.append((rc == -1 and same_bits(buf, keep), f"s2svc_seq_loss_bwd B {B} Tm {Tm} D {D} with real buffers: rc {rc}, outputs untouched"))
    for shape in ((0, 2, 5, 4), (2, 0, 5, 4), (2, 2, 0, 4), (2, 2, 5, 0)):
        B = shape[0]
        e = torch.empty(shape, device=DEV)
        refused(res, f"guided_attn_loss_fwd {shape}", lambda: K.guided_attn_loss_fwd(e, i32([1] * B), i32([1] * B), 0.4, 1.0), "guided_attn_loss_fwd: bad args")
        refused(res, f"guided_attn_loss_bwd {shape}", lambda: K.guided_attn_loss_bwd(shape, F32, torch.device(DEV), i32([1] * B), i32([1] * B), 0.4, 1.0, z32(2), None),
                "guided_attn_loss_bwd: bad args")
        buf, keep = sent((64,), F32), sent((64,), F32)
        rc = L.s2svc_guided_attn_loss_bwd(0, *shape, i32([1, 1]).data_ptr(), i32([1, 1]).data_ptr(), 0.4, 1.0, z32(2).data_ptr(), None, buf.data_ptr(), K.stream())
        torch.cuda.synchronize()
        res.append((rc == -1 and same_bits(buf, keep), f"s2svc_guided_attn_loss_bwd {shape} with a real buffer: rc {rc}, output untouched"))
    # the refusals that do not hang on an empty tensor's null pointer: real, sentinel-filled buffers through the C ABI
    att, il2, st2 = z32(2 * 2 * 5 * 4), i32([1, 1]), z32(3)
    part, out2, keep2 = sent((1024,), F32), sent((2,), F32), sent((2,), F32)
    for shape in ((0, 2, 5, 4), (2, 0, 5, 4), (2, 2, 0, 4), (2, 2, 5, 0)):
        rc = L.s2svc_guided_attn_loss_fwd(0, *shape, att.data_ptr(), il2.data_ptr(), il2.data_ptr(), 0.4, 1.0, part.data_ptr(), out2.data_ptr(), K.stream())
        torch.cuda.synchronize()
        msg = L.s2svc_last_error().decode()
        res.append((rc == -1 and "guided_attn_loss_fwd: bad args" in msg and same_bits(out2, keep2) and bool((part == SENT).all()),
                    f"s2svc_guided_attn_loss_fwd {shape} with real buffers: rc {rc} '{msg}', outputs untouched"))
    for sigma in (0.0, -0.4):
        rc = L.s2svc_guided_attn_loss_fwd(0, 2, 2, 5, 4, att.data_ptr(), il2.data_ptr(), il2.data_ptr(), sigma, 1.0, part.data_ptr(), out2.data_ptr(), K.stream())
        m1 = L.s2svc_last_error().decode()
        rcb = L.s2svc_guided_attn_loss_bwd(0, 2, 2, 5, 4, il2.data_ptr(), il2.data_ptr(), sigma, 1.0, st2.data_ptr(), None, part.data_ptr(), K.stream())
        m2 = L.s2svc_last_error().decode()
        torch.cuda.synchronize()
        res.append((rc == -1 and rcb == -1 and "guided_attn_loss_fwd: sigma must be positive" in m1 and "guided_attn_loss_bwd: sigma must be positive" in m2
                    and same_bits(out2, keep2) and bool((part == SENT).all()), f"guided_attn_loss fwd / bwd sigma {sigma}: rc {rc} / {rcb}, '{m1}' / '{m2}', outputs untouched"))
    src, ol2, buf = z32(2 * 5 * 4), i32([5, 3]), sent((64,), F32)
    for what, after, logits, labels, d_after, d_logits in (("d_after without after", None, None, None, buf, None), ("d_logits without logits", None, None, src, None, buf),
                                                            ("d_logits without labels", None, src, None, None, buf)):
        p_ = lambda x: None if x is None else x.data_ptr()      # noqa: E731
        rc = L.s2svc_seq_loss_bwd(0, 2, 5, 4, p_(after), src.data_ptr(), p_(logits), src.data_ptr(), p_(labels), ol2.data_ptr(), 1.0, st2.data_ptr(), None, None,
                                  p_(d_after), part.data_ptr(), p_(d_logits), K.stream())
        torch.cuda.synchronize()
        msg = L.s2svc_last_error().decode()
        res.append((rc == -1 and "seq_loss_bwd: a gradient without its input" in msg and bool((buf == SENT).all()) and bool((part == SENT).all()),
                    f"s2svc_seq_loss_bwd, {what}: rc {rc} '{msg}', outputs untouched"))
    dl, keep = sent((2, 3, 4), F32), sent((2, 3, 4), F32)
    pth, g1 = i32([0] * 6), z32(1)
    for what, a in (("path", (None, il2.data_ptr(), g1.data_ptr(), dl.data_ptr())), ("feat_lens", (pth.data_ptr(), None, g1.data_ptr(), dl.data_ptr())),
                    ("gout", (pth.data_ptr(), il2.data_ptr(), None, dl.data_ptr()))):
        rc = L.s2svc_mas_binloss_bwd(2, 3, 4, *a, K.stream())
        torch.cuda.synchronize()
        msg = L.s2svc_last_error().decode()
        res.append((rc == -1 and "mas_binloss_bwd: bad args" in msg and same_bits(dl, keep), f"s2svc_mas_binloss_bwd without {what}: rc {rc} '{msg}', dlogp untouched"))
    refused(res, "mas_binloss_bwd Tf 0", lambda: K.mas_binloss_bwd(torch.empty(2, 0, dtype=torch.int32, device=DEV), i32([1, 1]), z32(1), torch.empty(2, 0, 4, device=DEV)),
            "mas_binloss_bwd: bad shape")
    rc = L.s2svc_mas_binloss_bwd(2, 0, 4, i32([0] * 6).data_ptr(), i32([1, 1]).data_ptr(), z32(1).data_ptr(), dl.data_ptr(), K.stream())
    rc0 = L.s2svc_mas_binloss_bwd(0, 3, 4, i32([0] * 6).data_ptr(), i32([1, 1]).data_ptr(), z32(1).data_ptr(), dl.data_ptr(), K.stream())
    torch.cuda.synchronize()
    res.append((rc == -1 and rc0 == 0 and same_bits(dl, keep), f"s2svc_mas_binloss_bwd: Tf 0 refused (rc {rc}), B 0 returns cleanly (rc {rc0}), dlogp untouched"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# length regulator, bin-loss backward, durations from attention
# ---------------------------------------------------------------------------------------------------------------------------
def _durations(B, Tx, seed):
    ds = torch.randint(0, 5, (B, Tx), generator=R.gen(seed), dtype=torch.int32)
    ds[0, Tx // 2] = 40                                       # one frame repeated 40 times
    ds[1, Tx - 1] = -3                                        # a negative duration counts as 0
    ds[B - 1, 0] = 0
    return ds


@case
def length_regulate_index_kernel():
    """The 256-wide scan and its carry across chunks: start, idx and total exact at Tx 1 / 255 / 256 / 257 / 600 and at every kind of Tout."""
    t = Tally()
    B = 3
    for Tx in (1, 255, 256, 257, 600):
        ds = _durations(B, Tx, 1400 + Tx)
        tot = int(ds.clamp(min=0).sum(1).max())
        for Tout in sorted({tot, max(tot - 17, 1), tot + 9, 0}):
            start, idx, total = KA.length_regulate_index(ds.to(DEV), Tout)
            s_, i_, t_ = R.length_regulate_index(ds.numpy(), Tout)
            where = f"Tx {Tx}, Tout {Tout} (largest total {tot})"
            t.exact(where, np.array_equal(start.cpu().numpy(), s_), "start differs")
            t.exact(where, np.array_equal(idx.cpu().numpy(), i_), "idx differs")
            t.exact(where, np.array_equal(total.cpu().numpy(), t_), "total differs")
    return [t.line("length_regulate_index: start / idx / total, Tx 1 .. 600, Tout = total, below, above, 0")]


@case
@both_dtypes
def length_regulate_fwd_bwd(dtype):
    """fwd bit-equal to a torch gather (D 6 is scalar in both types, 4 in bf16; one input one element off a 16-byte boundary; pad -3.5);
    bwd against float64 segment sums, the truncated run included."""
    tf, tb = Tally(), Tally()
    B = 3
    for (Tx, D, off) in ((257, 4, False), (257, 6, False), (257, 8, False), (257, 80, False), (257, 8, True), (1, 8, False), (600, 8, False)):
        ds = _durations(B, Tx, 1500 + Tx + D)
        tot = int(ds.clamp(min=0).sum(1).max())
        x = R.randn(B, Tx, D, seed=1501 + Tx + D, dtype=dtype)
        if off:
            flat = torch.empty(x.numel() + 1, dtype=dtype, device=DEV)
            flat[1:] = x.reshape(-1).to(DEV)
            xd = flat[1:].view(B, Tx, D)
        else:
            xd = x.to(DEV)
        for Tout in sorted({tot, max(tot - 17, 1), tot + 9}):
            where = f"Tx {Tx} D {D} Tout {Tout}" + (" offset view" if off else "")
            start, idx, _ = KA.length_regulate_index(ds.to(DEV), Tout)
            y = KA.length_regulate_fwd(xd, idx, Tout, pad_value=-3.5)
            s_, i_, _ = R.length_regulate_index(ds.numpy(), Tout)
            tf.exact(where, same_bits(y.cpu(), R.length_regulate_fwd(x, i_, -3.5)), "fwd differs from the torch gather")
            dy = R.randn(B, Tout, D, seed=1502 + Tout, dtype=dtype)
            dx = KA.length_regulate_bwd(dy.to(DEV), start, ds.to(DEV), Tx)
            tb.close(where, dx, R.length_regulate_bwd(dy, s_, ds.numpy(), Tx, F64), R.length_regulate_bwd_stock(dy, i_, Tx, F32, dtype == BF16), dtype)
        start0, idx0, _ = KA.length_regulate_index(ds.to(DEV), 0)                  # an empty output: fwd returns it, bwd gives exact zeros
        y0 = KA.length_regulate_fwd(xd, idx0, 0)
        dx0 = KA.length_regulate_bwd(torch.empty(B, 0, D, dtype=dtype, device=DEV), start0, ds.to(DEV), Tx)
        tf.exact(f"Tx {Tx} D {D} Tout 0", tuple(y0.shape) == (B, 0, D), "Tout = 0 is not a clean empty result")
        tb.exact(f"Tx {Tx} D {D} Tout 0", tuple(dx0.shape) == (B, Tx, D) and bool((dx0 == 0).all()), "the gradient of an empty output is not exactly 0")
    return [tf.line(f"length_regulate_fwd[{name_of(dtype)}] bit-equal to a torch gather, pad -3.5"), tb.line(f"length_regulate_bwd[{name_of(dtype)}] segment sums")]


@case
def mas_binloss_bwd_kernel():
    """Accumulates into a non-zero dlogp; -1 entries of the path are skipped; a feat_lens row above Tf is clamped."""
    t = Tally()
    for (B, Tf, Tx) in ((3, 50, 16), (2, 1, 1), (4, 300, 70)):
        flens = [Tf, max(1, Tf // 2), Tf + 9, max(1, Tf - 1)][:B]
        path = torch.randint(0, Tx, (B, Tf), generator=R.gen(1600 + Tf), dtype=torch.int32)
        for b in range(B):
            path[b, min(flens[b], Tf):] = -1
        dl0 = R.randn(B, Tf, Tx, seed=1601 + Tf)
        dl = dl0.clone().to(DEV)
        K.mas_binloss_bwd(path.to(DEV), i32(flens), torch.tensor([0.8], device=DEV), dl)
        t.close(f"B {B} Tf {Tf} Tx {Tx} feat_lens {flens}", dl, R.mas_binloss_bwd(path, flens, R.f32(0.8), dl0, F64), R.mas_binloss_bwd(path, flens, R.f32(0.8), dl0, F32), F32)
    return [t.line("mas_binloss_bwd: dlogp += -g / (B * min(feat_len, Tf)) on the path")]


@case
def attn_durations_kernel():
    """Durations, head and focus rate over NH 1 / 4, Tf 1 .. 600, Tx 1 .. 300, with duplicated row maxima; two identical heads: the first wins."""
    t, tf = Tally(), Tally("attn_durations focus rate")
    inputs = [(s, R.attn_durations_input(*s, seed=1700 + i)) for i, s in enumerate(R.ATTN_DUR_SHAPES)]
    inputs.append(((4, 257, 7, "twin heads"), R.attn_durations_input(4, 257, 7, seed=1790, twin_heads=True)))
    for s, att in inputs:
        dur, focus, head = KA.attn_durations(att.to(DEV))
        d64, sc64, h64 = R.attn_durations(att, F64)
        _, sc32, _ = R.attn_durations(att, F32)
        where = f"NH {s[0]} Tf {s[1]} Tx {s[2]}" + (" twin heads" if len(s) > 3 else "")
        t.exact(where, int(head) == h64, f"head {int(head)}, wanted {h64}")
        t.exact(where, bool(torch.equal(dur.cpu(), d64)), "durations differ")
        t.exact(where, int(dur.sum()) == s[1], f"durations sum to {int(dur.sum())}, not Tf")
        tf.close(where, focus.reshape(1), sc64[h64].reshape(1), sc32[h64].reshape(1), F32)
    return [t.line(f"attn_durations: durations and head exact on {len(inputs)} inputs, durations sum to Tf"), tf.line("attn_durations: focus rate, each input against its own d")]


# ---------------------------------------------------------------------------------------------------------------------------
# fused Adam
# ---------------------------------------------------------------------------------------------------------------------------
BETAS, EPS = (R.f32(0.9), R.f32(0.999)), R.f32(1e-8)


def _adam_inputs(n, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    p = torch.randn(n, generator=g, device=device)
    m = 0.1 * torch.randn(n, generator=g, device=device)
    v = 0.01 * torch.rand(n, generator=g, device=device) + 1e-4
    return p, m, v, g


def _adam_run(n, combos, on_card=False):
    """Three consecutive steps per combo from non-zero moments and state[0] = 0; every step is judged from the values the kernel itself read
    (its own previous output).  -> [(ok, msg)]"""
    tp, ts, tx = Tally(), Tally("adam_step state"), Tally()
    rdev = DEV if on_card else "cpu"
    for ci, (mode, warm, lr, with_shadow) in enumerate(combos):
        p, m, v, gen_ = _adam_inputs(n, 1800 + n % 1000 + ci, rdev)
        pd, md, vd = p.to(DEV).clone(), m.to(DEV).clone(), v.to(DEV).clone()
        state, partial = torch.zeros(4, device=DEV), torch.empty(1024, dtype=F64, device=DEV)
        shadow = sent((n,), BF16) if with_shadow else None
        max_norm = None
        for step in (1, 2, 3):
            g = torch.randn(n, generator=gen_, device=rdev)
            if max_norm is None:
                gn = float(torch.linalg.vector_norm(g.double()))
                max_norm = R.f32({"none": 0.0, "above": 4.0 * gn + 1.0, "below": 0.3 * gn}[mode])
            p0, m0, v0 = pd.to(rdev).clone(), md.to(rdev).clone(), vd.to(rdev).clone()                 # what this step reads
            K.adam_step(pd, g.to(DEV), md, vd, shadow, state, partial, R.f32(lr), betas=BETAS, eps=EPS, max_norm=max_norm, warmup_steps=float(warm))
            where = f"n {n}, max_norm {mode}, warmup {warm}, lr {lr:g}, step {step}" + (", shadow" if with_shadow else "")
            r64 = R.adam_step(p0, g, m0, v0, step, R.f32(lr), BETAS, EPS, max_norm, warm, F64)
            y32 = R.adam_step(p0, g, m0, v0, step, R.f32(lr), BETAS, EPS, max_norm, warm, F32)
            for nm, got, a, b in (("p", pd, r64[0], y32[0]), ("m", md, r64[1], y32[1]), ("v", vd, r64[2], y32[2])):
                tp.close(f"{where} {nm}", got.to(rdev), a, b, F32)
            st = state.cpu().clone()
            tx.exact(where, float(st[0]) == float(step), f"step counter {float(st[0])}")
            if mode == "above":
                tx.exact(where, float(st[3]) == 1.0, f"clip coefficient {float(st[3])} with max_norm above the norm")
            for j, k in ((1, "lr"), (2, "grad norm"), (3, "clip coefficient")):                         # each scalar of the state alone
                ts.close(f"{where} {k}", st[j:j + 1], r64[3][j:j + 1].cpu(), y32[3][j:j + 1].cpu(), F32)
            if shadow is not None:
                tx.exact(where, same_bits(shadow, pd.to(BF16)), "the bf16 shadow is not p.to(bfloat16)")
    return [tp.line(f"adam_step n {n}: p / m / v over {len(combos)} settings x 3 steps"), ts.line(f"adam_step n {n}: lr / grad norm / clip coefficient"),
            tx.line(f"adam_step n {n}: step count exact, coefficient exactly 1 above the norm, shadow == p.to(bfloat16)")]


ADAM_COMBOS = [(mode, warm, (1e-3, 0.05, 0.5)[(i + j) % 3], (i + j) % 2 == 0) for i, mode in enumerate(("none", "above", "below")) for j, warm in enumerate((0, 2, 4000))]


@case
def adam_step_small():
    """The scalar tail (n % 4 != 0) and n below one vector."""
    res = []
    for n in (1, 3, 4, 5, 1021):
        res += _adam_run(n, ADAM_COMBOS)
    return res


@case
def adam_step_block_cap():
    """n = 1024 * 256 + 7: past the 1024-block cap of the grad-norm reduction, with a scalar tail."""
    return _adam_run(1024 * 256 + 7, ADAM_COMBOS)


@case
def adam_step_non_temporal():
    """n = 2^26 + 7 (n * 4 > 256 MB): the non-temporal path.  The only reference that runs on the card."""
    return _adam_run((1 << 26) + 7, [("below", 4000, 0.05, True)], on_card=True)


@case
def adam_step_shadow_rounding():
    """g = m = v = 0 passes p through unchanged, so the shadow is the rounding of chosen values: ties in both directions, -0.0, a denormal,
    3.39e38 -- in the vector body and in the scalar tail."""
    res = []
    probe = R.shadow_probe_values()
    for p0 in (probe, torch.cat([probe, probe[[0, 7, 14]]]), torch.cat([probe[5:], probe[:5], probe[[14]]])):
        n = p0.numel()
        pd, z = p0.to(DEV).clone(), torch.zeros(n, device=DEV)
        md, vd, shadow = z.clone(), z.clone(), sent((n,), BF16)
        state = torch.zeros(4, device=DEV)
        K.adam_step(pd, z, md, vd, shadow, state, torch.empty(1024, dtype=F64, device=DEV), 1e-3, betas=BETAS, eps=EPS, max_norm=1.0, warmup_steps=4000.0)
        ok_p = same_bits(pd, p0) and same_bits(md, z) and same_bits(vd, z)
        want = p0.to(BF16)
        bad = (shadow.cpu().view(torch.int16) != want.view(torch.int16)).nonzero().flatten().tolist()
        res.append((ok_p and not bad, f"adam_step shadow rounding, n {n} (tail {n % 4}): p passed through {'unchanged' if ok_p else 'CHANGED'}, shadow == p.to(bfloat16) bit for bit"
                    + (f" EXCEPT at {bad[:5]}: p {[float(p0[i]) for i in bad[:5]]}" if bad else "")))
    return res


@case
def adam_step_rejection_leaves_state_alone():
    """A buffer one element off a 16-byte boundary is refused before anything is launched: state, p, m and v keep their bits."""
    res = []
    n = 1024
    for which in ("params", "grads", "exp_avg", "exp_avg_sq"):
        bufs = {k: R.randn(n + 1, seed=1900 + i).to(DEV) for i, k in enumerate(("params", "grads", "exp_avg", "exp_avg_sq"))}
        view = {k: (b[1:] if k == which else b[:n]) for k, b in bufs.items()}
        keep = {k: b.clone() for k, b in bufs.items()}
        state = torch.tensor([5.0, 0.1, 2.0, 0.5], device=DEV)
        refused(res, f"adam_step with {which} one element off",
                lambda: K.adam_step(view["params"], view["grads"], view["exp_avg"], view["exp_avg_sq"], None, state, torch.empty(1024, dtype=F64, device=DEV), 1e-3),
                "adam_step: 16-byte aligned buffers", [(state, torch.tensor([5.0, 0.1, 2.0, 0.5]))] + [(bufs[k], keep[k]) for k in bufs])
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# glue
# ---------------------------------------------------------------------------------------------------------------------------
@case
def scalar_glue_kernels():
    """weighted_sum, scalars_axpy, weighted_sum_bwd: k 1 / 8, term sizes 0 / 1 / 65 / 1000, beta = 0 over a NaN accumulator, k = 9 refused."""
    res = []
    tw, ta, tb = Tally("weighted_sum"), Tally(), Tally()
    sizes = (1, 65, 1000, 1, 65, 1000, 65, 1)
    for k in (1, 8):
        xs = [R.randn(sizes[i], seed=2000 + i + k) for i in range(k)]
        ws = [R.f32(0.3 * (i + 1) * (-1) ** i) for i in range(k)]
        xd = [x.to(DEV) for x in xs]
        for empty in (None, 0, k - 1):                           # a term of size 0: its pointer stays valid, its count is 0 (C ABI)
            t = K._terms(list(zip(xd, ws)))
            xs_ = list(xs)
            if empty is not None:
                t.n[empty] = 0
                xs_[empty] = xs[empty][:0]
            out, acc = sent((3,), F32), torch.full((k + 2,), float("nan"), device=DEV)
            acc[k:] = SENT
            _lib.check(_lib.lib().s2svc_weighted_sum(ctypes.byref(t), out.data_ptr(), K.stream()), "weighted_sum")
            _lib.check(_lib.lib().s2svc_scalars_axpy(ctypes.byref(t), 0.0, acc.data_ptr(), K.stream()), "scalars_axpy")
            where = f"k {k}" + ("" if empty is None else f", term {empty} of size 0")
            tw.exact(where, bool((out[1:] == SENT).all()), "weighted_sum wrote behind its scalar")
            tw.close(where, out[0:1], R.weighted_sum(xs_, ws, F64).reshape(1), R.weighted_sum(xs_, ws, F32).reshape(1), F32)
            nan = torch.full((k,), float("nan"))
            ta.close(f"{where}, beta 0 over NaN", acc[:k], R.scalars_axpy(xs_, ws, nan, 0.0, F64), R.scalars_axpy(xs_, ws, nan, 0.0, F32), F32)
            ta.exact(where, bool((acc[k:] == SENT).all()), "scalars_axpy wrote behind its k accumulators")
        # through the wrappers, and a running sum (beta != 0)
        out = K.weighted_sum(list(zip(xd, ws)))
        tw.close(f"k {k}, through the wrapper", out.reshape(1), R.weighted_sum(xs, ws, F64).reshape(1), R.weighted_sum(xs, ws, F32).reshape(1), F32)
        acc0 = R.randn(k, seed=2100 + k)
        acc = K.scalars_axpy(list(zip(xd, ws)), acc0.to(DEV), beta=0.75)
        ta.close(f"k {k}, beta 0.75", acc, R.scalars_axpy(xs, ws, acc0, 0.75, F64), R.scalars_axpy(xs, ws, acc0, 0.75, F32), F32)
        g = torch.tensor([R.f32(1.7)])
        shapes = [((sizes[i],) if i % 2 else (1, sizes[i]), ws[i]) for i in range(k)]
        outs = K.weighted_sum_bwd(g.to(DEV), shapes, torch.device(DEV))
        for i, o in enumerate(outs):
            tb.exact(f"k {k} term {i}", tuple(o.shape) == tuple(shapes[i][0]), "shape")
            tb.close(f"k {k} term {i}", o, torch.full(shapes[i][0], ws[i], dtype=F64) * g.double(), torch.full(shapes[i][0], ws[i], dtype=F32) * g, F32)
    # weighted_sum_bwd with a term of size 0 (C ABI: a valid pointer, count 0): that term's buffer is left alone, the others are written
    for k in (1, 8):
        bufs = [sent((sizes[i],), F32) for i in range(k)]
        ws = [R.f32(0.3 * (i + 1) * (-1) ** i) for i in range(k)]
        g = torch.tensor([R.f32(1.7)])
        for empty in (0, k - 1):
            for b in bufs:
                b.fill_(SENT)
            t = K._terms(list(zip(bufs, ws)))
            t.n[empty] = 0
            _lib.check(_lib.lib().s2svc_weighted_sum_bwd(ctypes.byref(t), g.to(DEV).data_ptr(), K.stream()), "weighted_sum_bwd")
            for i, b in enumerate(bufs):
                if i == empty:
                    tb.exact(f"k {k}, term {i} of size 0", bool((b == SENT).all()), "a term of size 0 was written")
                else:
                    tb.close(f"k {k} term {i}, term {empty} of size 0", b, torch.full((sizes[i],), ws[i], dtype=F64) * g.double(), torch.full((sizes[i],), ws[i], dtype=F32) * g, F32)
    res += [tw.line("weighted_sum, each sum against its own d"), ta.line("scalars_axpy (beta 0 over NaN is clean)"), tb.line("weighted_sum_bwd")]
    # refusals: nine terms (the wrapper counts them itself; the launcher refuses a hand-made k = 9), a term without a pointer
    x = [torch.ones(4, device=DEV)] * 9
    try:
        K.weighted_sum([(t, 1.0) for t in x])
        res.append((False, "weighted_sum wrapper accepted nine terms"))
    except ValueError as e:
        res.append(("1 to 8 terms" in str(e), f"weighted_sum wrapper refuses nine terms: {e}"))
    out, acc = sent((2,), F32), sent((10,), F32)
    t9 = K._terms([(t, 1.0) for t in x[:8]])
    t9.k = 9
    for nm, call, buf in (("weighted_sum", lambda: _lib.lib().s2svc_weighted_sum(ctypes.byref(t9), out.data_ptr(), K.stream()), out),
                          ("scalars_axpy", lambda: _lib.lib().s2svc_scalars_axpy(ctypes.byref(t9), 1.0, acc.data_ptr(), K.stream()), acc),
                          ("weighted_sum_bwd", lambda: _lib.lib().s2svc_weighted_sum_bwd(ctypes.byref(t9), out.data_ptr(), K.stream()), out)):
        refused(res, f"{nm} with k = 9", lambda: _lib.check(call(), nm), f"{nm}: 1..8 terms, every pointer set", [(buf, torch.full_like(buf, SENT))])
    refused(res, "weighted_sum with an empty tensor (no pointer)", lambda: K.weighted_sum([(torch.ones(4, device=DEV), 1.0), (torch.empty(0, device=DEV), 1.0)], out=out[0]),
            "weighted_sum: 1..8 terms, every pointer set", [(out, torch.full_like(out, SENT))])
    return res


@case
@both_dtypes
def copy_glue_kernels(dtype):
    """pad_cols, decoder_input, dense_rows, add_n against their torch formulations, bit for bit."""
    t, ts = Tally(), Tally()
    for (rows, N, ldo) in ((1, 1, 1), (37, 5, 8), (300, 81, 88)):
        x = R.randn(rows, N, seed=2200 + rows, dtype=dtype)
        t.exact(f"pad_cols {rows} x {N} -> {ldo}", same_bits(K.pad_cols(x.to(DEV), ldo).cpu(), F.pad(x, (0, ldo - N))), "differs from F.pad")
    for (B, T, D, r) in ((3, 10, 7, 1), (3, 10, 7, 3), (2, 11, 80, 3), (1, 3, 5, 3), (2, 1, 4, 1)):
        big = R.randn(B, T + 5, D, seed=2300 + T + r)
        ys = big[:, :T]                                           # a view with a larger batch stride
        got = K.decoder_input(big.to(DEV)[:, :T], r, dtype)
        t.exact(f"decoder_input B {B} T {T} D {D} r {r}", same_bits(got.cpu(), R.decoder_input(ys, r).to(dtype)), "differs from cat(zeros, ys[:, r-1::r][:, :-1])")
    for (B, T, D) in ((2, 9, 8), (3, 1, 80)):
        wide = R.randn(B, T, 3 * D, seed=2400 + T, dtype=dtype)
        for blk in range(3):
            v = wide.to(DEV)[:, :, blk * D:(blk + 1) * D]
            t.exact(f"dense_rows block {blk} of (B {B}, T {T}, 3 x {D})", same_bits(K.dense_rows(v).cpu(), wide[:, :, blk * D:(blk + 1) * D].contiguous()), "differs from .contiguous()")
    for n in (1, 65, 1000, 1003):
        for k in (2, 3, 4):
            xs = [R.randn(n, seed=2500 + n + i, dtype=dtype) for i in range(k)]
            out = K.add_n([x.to(DEV) for x in xs])
            y32 = xs[0].float()
            for x in xs[1:]:
                y32 = y32 + x.float()
            ts.close(f"add_n n {n} k {k}", out, sum(x.double() for x in xs), R.bf16_round(y32) if dtype == BF16 else y32, dtype)
    return [t.line(f"pad_cols / decoder_input / dense_rows[{name_of(dtype)}] bit-equal to F.pad, cat(zeros, ys[:, r-1::r][:, :-1]), .contiguous()"),
            ts.line(f"add_n[{name_of(dtype)}]")]


@case
def token_and_label_glue_kernels():
    """append_eos and stop_labels against F.pad + eos write and torch.scatter, bit for bit; lengths 1, T, and a row of length 0 for stop_labels."""
    t = Tally()
    for (B, T) in ((4, 9), (2, 1), (3, 300)):
        wide = torch.randint(3, 50, (B, T + 4), generator=R.gen(2600 + T), dtype=torch.int64)
        lens = [T, 1, max(1, T // 2), T][:B]
        got = K.append_eos(wide.to(DEV)[:, :T], i32(lens), 1, 0)
        t.exact(f"append_eos B {B} T {T} lens {lens}", bool(torch.equal(got.cpu(), R.append_eos(wide[:, :T], lens, 1, 0))), "differs from F.pad + eos write")
        lab = (torch.rand(B, T + 4, generator=R.gen(2601 + T)) < 0.3).float()
        lens0 = [T, 1, 0, max(1, T // 2)][:B]
        got = K.stop_labels(lab.to(DEV), i32(lens0), T)
        want = R.stop_labels(lab, lens0, T)
        t.exact(f"stop_labels B {B} T {T} lens {lens0}", same_bits(got.cpu(), want), "differs from torch.scatter")
        if 0 in lens0:
            b = lens0.index(0)
            t.exact(f"stop_labels lens 0, T {T}", same_bits(got.cpu()[b], lab[b, :T].contiguous()), "a row of length 0 was changed")
    return [t.line("append_eos / stop_labels bit-equal to F.pad + eos, torch.scatter; a stop_labels row of length 0 is copied unchanged")]


@case
def fill_zero_and_seed_advance():
    """K.zero_ over ragged byte ranges (a head before the first 16-byte boundary, a tail behind the last, fewer than 16 bytes, several
    workgroups) leaves exact zeros inside and the sentinel outside; K.advance_seed adds 0x10001 to the device-resident seed."""
    res, t = [], Tally()
    for dtype in (F32, BF16, torch.int32):
        for off in (0, 1, 3):
            for n in (1, 2, 5, 64, 1000, 4096 * 256 * 4 + 13):
                buf = sent((off + n + 7,), dtype)
                K.zero_(buf[off:off + n])
                where = f"{dtype} offset {off} n {n}"
                t.exact(where, bool((buf[off:off + n] == 0).all()) and (dtype == torch.int32 or not bool(torch.signbit(buf[off:off + n]).any())), "not all +0 inside")
                sv = ISENT if dtype == torch.int32 else SENT
                t.exact(where, bool((buf[:off] == sv).all()) and bool((buf[off + n:] == sv).all()), "wrote outside the range")
    z = K.zeros((3, 5), F32, torch.device(DEV))
    t.exact("K.zeros", tuple(z.shape) == (3, 5) and bool((z == 0).all()), "K.zeros is not zero")
    res.append(t.line("fill_zero: exact zeros inside ragged byte ranges, sentinel outside"))
    K.manual_seed(777)
    dev = torch.device(DEV, torch.cuda.current_device())
    seed = K.SEED.tensor(dev)
    s0 = int(seed.item())
    K.advance_seed(dev)
    K.advance_seed(dev)
    torch.cuda.synchronize()
    res.append((s0 == 777 and int(seed.item()) == 777 + 2 * 0x10001, f"seed_advance: {s0} -> {int(seed.item())} after two advances of 0x10001"))
    return res


@case
def decode_attn_refusals():
    """dk above 256 and a key capacity whose score buffer exceeds the 60 KB LDS limit are refused by the launcher's argument check."""
    res = []
    for (dk, Tk, expect) in ((264, 8, "decode_attn: bad arguments"), (8, 16000, "decode_attn: key capacity too large for the LDS score buffer")):
        B, H = 1, 1
        D = H * dk
        q, kv = torch.zeros(B, D, device=DEV), torch.zeros(B, Tk, 2 * D, device=DEV)
        ctx, att = sent((B, D), F32), sent((B, H, 1, Tk), F32)
        refused(res, f"decode_attn dk {dk}, Tk {Tk}",
                lambda: KD.decode_attn(q, 0, D, kv, 0, kv, D, 2 * D, Tk * 2 * D, None, 0, 0, 0, i32([0]), None, Tk, 1.0, ctx, B, H, dk, att=att,
                                       att_strides=(att.stride(0), att.stride(1), att.stride(2))),
                expect, [(ctx, torch.full_like(ctx, SENT)), (att, torch.full_like(att, SENT))])
    return res


def main():
    torch.manual_seed(0)
    nfail = 0
    only = None
    if "--only" in sys.argv:
        only = set(sys.argv[sys.argv.index("--only") + 1].split(","))
    for fn in CASES:
        if only is not None and fn.__name__ not in only:
            continue
        try:
            results = fn()
        except Exception:
            results = [(False, f"{fn.__name__}: EXCEPTION\n{traceback.format_exc()}")]
        for ok, msg in results:
            print(("PASS " if ok else "FAIL ") + msg, flush=True)
            nfail += 0 if ok else 1
        torch.cuda.synchronize()
    print(f"== {nfail} failures")
    return nfail


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
