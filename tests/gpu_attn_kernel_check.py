"""Kernel-level, element-wise parity of the attention launchers: the fused short-sequence attention (csrc/attn_fused.hip), the one-launch
attention map and its backward (csrc/attn_map.hip), the relative-position forward (csrc/relattn.hip) and the softmax kernels
(csrc/softmax.hip).  Runs on the MI355X:
  * `python tests/gpu_attn_kernel_check.py [--only a,b]` prints a PASS/FAIL table for all cases and never stops early;
  * tests/test_gpu_attn_kernels.py imports CASES and turns each into a `@pytest.mark.gpu` test.

Floats are compared by the rule of tests/step_kernels_ref.py, applied per (utterance, head) slice of every output: ref64 = the float64
restatement of tests/attn_kernels_ref.py on exactly the values the kernel reads, yard = the same formula in float32 on the CPU, rounded to
bf16 where the kernel's header comment documents it, d = max |yard - ref64| over the slice, pass when |got - ref64| <= 4 d + ulp at every
element of the slice.  Backward kernels are handed bf16(ref64 map) from the CPU, never a forward kernel's output.  Dropout enters ref64 and
the yard as data: the keep-scales K.act_dropout_fwd draws on a ones tensor of the map's padded layout with the same seed.  Exact
conditions: masked positions and pad columns are zero bit for bit, every output sits in a sentinel-filled buffer (a column block of a
packed buffer with one more row than the output has; a tail behind the contiguous maps) whose remainder comes back unchanged.  Some
shapes of every family (A.EDGE_KLEN_SHAPES) run a second time with klen = (0, T2 + 3, the cut): every kernel takes min(klen, T2), the
utterance without a key has map, dropped map, context, dS, dq, dk, dv and dbd all zero, and the same exact conditions hold.  The only
calls expected to fail are ones a launcher's host-side argument check refuses before any launch."""
import os
import sys
import traceback
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_kernels_ref as A  # noqa: E402
import gpu_step_kernel_check as S  # noqa: E402  (Tally, sent, same_bits, refused: the idiom of the step-kernel check)
import step_kernels_ref as R  # noqa: E402
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402
from seq2seq_vc_amd.ops import kernels_attn as KAT  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = S.SENT
CASES = []
# Checks whose kernel is correct and yet takes more than 4 d: 1.5 x the measured margin, with the cause (profiles/AB_LOG.md has the runs).
MEASURED_MARGINS = {
    # the row sum of P (dP keep + dattn): 64 strided per-lane partial sums and a shuffle tree add in another order than torch's CPU loop, and
    # t - rowsum cancels; d is 3 - 4 ulp of the fp32 output here.  Measured need 4.42 (T 3 x 129, dattn, p 0).  The entry covers both fp32
    # outputs of the kernel: dbd holds the very values of dscores
    "attn_softmax_bwd[fp32]": 6.63,
}
sent, same_bits, refused = S.sent, S.same_bits, S.refused


def case(fn):
    CASES.append(fn)
    return fn


class Tally(S.Tally):
    def __init__(self, key=None):
        super().__init__()
        self.margin = MEASURED_MARGINS.get(key, R.MARGIN)

    def slices(self, where, got, ref64, yard, H, out_dtype):
        """The rule per (utterance, head) slice, each held to the d of its own slice."""
        got = got.detach().cpu()
        for ((b, h), g), (_, r), (_, y) in zip(A.slices(got, H), A.slices(ref64, H), A.slices(yard, H)):
            self.close(f"{where} [b {b}, h {h}]", g, r, y, out_dtype)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


_SEED_BASE = []


def case_seed(*key):
    """(base pointer, offset) as the launchers take a dropout seed, a function of `key` alone: the keep-scales of a line, and with them the
    margin it uses, do not depend on which cases ran before it in the process."""
    if not _SEED_BASE:
        _SEED_BASE.append(torch.full((1,), 0x5EED, dtype=torch.int64, device=DEV))
    return _SEED_BASE[0].data_ptr(), (zlib.crc32(repr(key).encode()) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def view_in(x):
    """A (B, T, D) input as the models pass it: a column block of a packed buffer (row stride 2 D + 8, one row more per utterance)."""
    B, T, D = x.shape
    buf = sent((B, T + 1, 2 * D + 8), x.dtype)
    v = buf[:, :T, D:2 * D]
    v.copy_(x)
    return v


class OutView:
    """A (B, T, D) output as a column block of a sentinel-filled packed buffer."""

    def __init__(self, B, T, D, dtype=BF16):
        self.buf = sent((B, T + 1, 2 * D + 8), dtype)
        self.v = self.buf[:, :T, D:2 * D]
        self.T, self.D = T, D

    def rest_untouched(self):
        c = self.buf.clone()
        c[:, :self.T, self.D:2 * self.D] = SENT
        return bool((c == SENT).all())


class OutFlat:
    """A contiguous output (the maps' (B, H, T1, ld) layout) with a sentinel tail behind it."""

    def __init__(self, shape, dtype=BF16, tail=64):
        n = 1
        for s in shape:
            n *= s
        self.buf = sent((n + tail,), dtype)
        self.v = self.buf[:n].view(*shape)
        self.n = n

    def rest_untouched(self):
        return bool((self.buf[self.n:] == SENT).all())


def padded(x, ld, dtype=None, fill=0.0):
    """(B, H, T1, T2) CPU tensor -> device tensor in the padded (B, H, T1, ld) layout."""
    B, H, T1, T2 = x.shape
    out = torch.full((B, H, T1, ld), fill, dtype=dtype or x.dtype)
    out[..., :T2] = x.to(out.dtype)
    return out.to(DEV)


def zero_bits(x, where_zero):
    """Every element of x (fp32 / bf16, any device) selected by the CPU bool mask is +0.0 bit for bit."""
    x = x.detach().cpu().contiguous()
    return bool((x.view(torch.int32 if x.dtype == F32 else torch.int16)[where_zero] == 0).all())


def must_be_zero(mask, ld):
    """(B, 1 or H, T1, T2) admissibility -> (B, H, T1, ld) bool: masked positions and the pad columns [T2, ld)."""
    B, _, T1, T2 = mask.shape
    z = torch.ones(B, A.H_, T1, ld, dtype=torch.bool)
    z[..., :T2] = ~mask.expand(B, A.H_, T1, T2)
    return z


def dropped_zero(zmask, keep):
    z = zmask.clone()
    z[..., :keep.shape[-1]] |= keep == 0
    return z


def klen_tag(edge, klen):
    return f", klen {klen}" if edge else ""


def no_key_zero(t, where, klen, outs):
    """Every output slice of an utterance without an admissible key (klen <= 0) is zero: outs = [(name, (B, ...) tensor)]."""
    for b in [b for b, n in enumerate(klen) if n <= 0]:
        for name, o in outs:
            t.exact(where, bool((o[b] == 0).all()), f"{name} of utterance {b}, which has no admissible key, is not 0")


class Keep:
    """The keep-scales of one seed, and the keep rate over everything drawn so far (an exact condition of its own)."""

    def __init__(self):
        self.kept, self.total, self.bad_value = 0, 0, False

    def draw(self, shape, p, seed):
        full = K.act_dropout_fwd(torch.ones(shape, dtype=F32, device=DEV), None, p, seed).cpu()
        inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
        self.bad_value = self.bad_value or not bool(((full == 0) | (full == inv)).all())
        self.kept, self.total = self.kept + int((full != 0).sum()), self.total + full.numel()
        return full

    def verdict(self, t, p):
        t.exact("keep-scales", not self.bad_value, "a keep-scale is neither 0 nor 1 / (1 - p)")
        # (0.02 is 4 standard deviations of the rate of 10000 draws at p = 0.3: every family draws far more)
        t.exact("keep rate", self.total >= 10000, f"only {self.total} keep-scales drawn: too few to hold the rate to 0.02")
        t.exact("keep rate", abs(self.kept / max(1, self.total) - (1 - p)) <= 0.02, f"keep rate {self.kept / max(1, self.total):.4f} not within 0.02 of {1 - p}")


def ccall(name, rc):
    _lib.check(rc, name)


# ---------------------------------------------------------------------------------------------------------------------------
# attn_fused: forward + backward
# ---------------------------------------------------------------------------------------------------------------------------
def fused_fwd_launch(q, k, v, klen, causal, H, scale, p, seed, attn, ld, out):
    B, T1, D = q.shape
    ccall("attn_fused_fwd", _lib.lib().s2svc_attn_fused_fwd(B, H, T1, k.shape[1], D // H, K.ptr(q), q.stride(1), q.stride(0), K.ptr(k), k.stride(1),
                                                            k.stride(0), K.ptr(v), v.stride(1), v.stride(0), K.ptr(klen), 1 if causal else 0, scale, p,
                                                            seed[0], seed[1], K.ptr(attn), ld, K.ptr(out), out.stride(1), out.stride(0), K.stream()))


def _fused(dk):
    P_DROP = 0.3
    res, keeps = [], Keep()
    B, H = A.B_, A.H_
    for shape, edge in A.with_edges([s for s in A.FUSED_SHAPES if s[2] == dk], "fused"):
        T1, T2, _, causal = shape
        tf, tb = Tally("attn_fused_fwd"), Tally("attn_fused_bwd")
        inp = A.fused_inputs(shape, edge)
        D, ld, scale, klen = H * dk, A.round8(T2), inp["scale"], inp["klen"]
        q, k, v, dctx = (view_in(inp[n]) for n in ("q", "k", "v", "dctx"))
        assert KAT.supported(q, k, v, H), shape
        mask = A.key_mask(klen, T1, T2, causal)
        zmask = must_be_zero(mask, ld)
        pm = A.stored_map(inp)
        pm_d = padded(pm, ld)
        for p in (0.0, P_DROP):
            seed = case_seed("fused", shape, edge, p)
            keep = A.keep_of(keeps.draw((B, H, T1, ld), p, seed), T2) if p else None
            where = f"p {p}"
            fa = (inp["q"], inp["k"], inp["v"], klen, causal, scale, H)
            r64, y32 = A.attn_fwd(*fa, F64, keep=keep), A.attn_fwd(*fa, F32, keep=keep, bf16=True, drop_stored=True)
            attn, out = OutFlat((B, H, T1, ld)), OutView(B, T1, D)
            fused_fwd_launch(q, k, v, i32(klen), causal, H, scale, p, seed, attn.v, ld, out.v)
            tf.slices(where + " map", attn.v[..., :T2], r64[0], y32[0], H, BF16)
            tf.slices(where + " context", out.v, r64[2], y32[2], H, BF16)
            tf.exact(where, zero_bits(attn.v, zmask), "a masked position or pad column of the map is not +0")
            tf.exact(where, attn.rest_untouched() and out.rest_untouched(), "wrote outside the map / outside the context's column block and rows")
            no_key_zero(tf, where, klen, [("the map", attn.v), ("the context", out.v)])
            for use_dattn in (False, True):
                where = f"p {p}, dattn {use_dattn}"
                dattn = inp["dattn"] if use_dattn else None
                ba = (pm, inp["dctx"], inp["v"], inp["k"], inp["q"], scale, H)
                r64b, y32b = A.attn_bwd(*ba, F64, dattn=dattn, keep=keep), A.attn_bwd(*ba, F32, dattn=dattn, keep=keep, bf16=True)
                dq, dkk, dv = OutView(B, T1, D), OutView(B, T2, D), OutView(B, T2, D)
                KAT.fused_bwd(q, k, v, dctx, pm_d, padded(dattn, ld) if use_dattn else None, H, scale, p, seed, dq.v, dkk.v, dv.v)
                for nm, o, i in (("dq", dq, 1), ("dk", dkk, 2), ("dv", dv, 3)):
                    tb.slices(f"{where} {nm}", o.v, r64b[i], y32b[i], H, BF16)
                    tb.exact(f"{where} {nm}", o.rest_untouched(), "wrote outside its column block or behind its last row")
                no_key_zero(tb, where, klen, [("dq", dq.v), ("dk", dkk.v), ("dv", dv.v)])
        tag = f"T {T1} x {T2}, dk {dk}{', causal' if causal else ''}{klen_tag(edge, klen)}"
        res += [tf.line(f"attn_fused_fwd {tag}"), tb.line(f"attn_fused_bwd {tag}")]
    t = Tally()
    keeps.verdict(t, P_DROP)
    res.append(t.line(f"attn_fused dk {dk}: keep-scales of p {P_DROP}", f" ({keeps.kept} of {keeps.total} kept)"))
    return res


@case
def attn_fused_dk32():
    return _fused(32)


@case
def attn_fused_dk64():
    return _fused(64)


@case
def attn_fused_dk96():
    return _fused(96)


@case
def attn_fused_dk128():
    return _fused(128)


# ---------------------------------------------------------------------------------------------------------------------------
# attn_map: forward (+ context) and backward (+ dq, + dbd)
# ---------------------------------------------------------------------------------------------------------------------------
def map_fwd_launch(q, k, klen, causal, H, scale, p, seed, attn, pdrop, ld, v, ctx):
    B, T1, D = q.shape
    ccall("attn_map_fwd", _lib.lib().s2svc_attn_map_fwd(B, H, T1, k.shape[1], D // H, K.ptr(q), q.stride(1), q.stride(0), K.ptr(k), k.stride(1), k.stride(0),
                                                        K.ptr(klen), 1 if causal else 0, scale, p, seed[0], seed[1], K.ptr(attn), K.ptr(pdrop), ld,
                                                        K.ptr(v), v.stride(1) if v is not None else 0, v.stride(0) if v is not None else 0,
                                                        K.ptr(ctx), ctx.stride(1) if ctx is not None else 0, ctx.stride(0) if ctx is not None else 0,
                                                        K.stream()))


def map_bwd_launch(dctx, v, attn, dattn, H, scale, p, seed, ds, ld, dbd, ldb, k, dq):
    B, T1, D = dctx.shape
    ccall("attn_map_bwd", _lib.lib().s2svc_attn_map_bwd(B, H, T1, v.shape[1], D // H, K.ptr(dctx), dctx.stride(1), dctx.stride(0), K.ptr(v), v.stride(1),
                                                        v.stride(0), K.ptr(attn), K.ptr(dattn), scale, p, seed[0], seed[1], K.ptr(ds), ld, K.ptr(dbd), ldb,
                                                        K.ptr(k), k.stride(1) if k is not None else 0, k.stride(0) if k is not None else 0,
                                                        K.ptr(dq), dq.stride(1) if dq is not None else 0, dq.stride(0) if dq is not None else 0, K.stream()))


def _map(dk):
    P_DROP = 0.1
    res, keeps = [], Keep()
    B, H = A.B_, A.H_
    for shape, edge in A.with_edges([s for s in A.MAP_SHAPES if s[2] == dk], "map"):
        T1, T2, _, causal = shape
        tf, tb = Tally("attn_map_fwd"), Tally("attn_map_bwd")
        inp = A.map_inputs(shape, edge)
        D, ld, scale, klen = H * dk, A.round8(T2), inp["scale"], inp["klen"]
        q, k, v, dctx = (view_in(inp[n]) for n in ("q", "k", "v", "dctx"))
        assert KAT.map_supported(q, k, H), shape
        product = KAT.map_product_ok(v, H)
        assert product == (dk in (64, 96, 128)), shape
        mask = A.key_mask(klen, T1, T2, causal)
        zmask = must_be_zero(mask, ld)
        pm = A.stored_map(inp)
        pm_d = padded(pm, ld)
        square = T1 == T2
        ldb = A.round8(2 * T1 - 1) + 8 if square else 0
        if square:                                                       # the elements of dbd that no dS lands on, or a masked one does
            hit = A.unshift(mask.expand(B, H, T1, T2).to(F32), L=ldb) > 0
        for p in (0.0, P_DROP):
            seed = case_seed("map", shape, edge, p)
            keep = A.keep_of(keeps.draw((B, H, T1, ld), p, seed), T2) if p else None
            for with_ctx in ((False, True) if product else (False,)):
                where = f"p {p}, context {with_ctx}"
                fa = (inp["q"], inp["k"], inp["v"] if with_ctx else None, klen, causal, scale, H)
                r64, y32 = A.attn_fwd(*fa, F64, keep=keep), A.attn_fwd(*fa, F32, keep=keep, bf16=True, drop_stored=False)
                attn, pdrop, ctx = OutFlat((B, H, T1, ld)), OutFlat((B, H, T1, ld)), OutView(B, T1, D)
                map_fwd_launch(q, k, i32(klen), causal, H, scale, p, seed, attn.v, pdrop.v if p else None, ld, v if with_ctx else None,
                               ctx.v if with_ctx else None)
                tf.slices(where + " map", attn.v[..., :T2], r64[0], y32[0], H, BF16)
                tf.exact(where, zero_bits(attn.v, zmask), "a masked position or pad column of the map is not +0")
                if p:
                    tf.slices(where + " dropped map", pdrop.v[..., :T2], r64[1], y32[1], H, BF16)
                    tf.exact(where, zero_bits(pdrop.v, dropped_zero(zmask, keep)), "a masked, dropped or pad element of the dropped map is not +0")
                else:
                    tf.exact(where, same_bits(pdrop.buf, torch.full_like(pdrop.buf, SENT)), "the dropped map was written without dropout")
                if with_ctx:
                    tf.slices(where + " context", ctx.v, r64[2], y32[2], H, BF16)
                else:
                    tf.exact(where, same_bits(ctx.buf, torch.full_like(ctx.buf, SENT)), "the context was written without v")
                tf.exact(where, attn.rest_untouched() and pdrop.rest_untouched() and ctx.rest_untouched(), "wrote outside an output")
                no_key_zero(tf, where, klen, [("the map", attn.v)] + ([("the dropped map", pdrop.v)] if p else []) + ([("the context", ctx.v)] if with_ctx else []))
            for use_dattn in (False, True):
                for with_dq in ((False, True) if product else (False,)):
                    where = f"p {p}, dattn {use_dattn}, dq {with_dq}"
                    dattn = inp["dattn"] if use_dattn else None
                    ba = (pm, inp["dctx"], inp["v"], inp["k"] if with_dq else None, None, scale, H)
                    r64b = A.attn_bwd(*ba, F64, dattn=dattn, keep=keep)
                    y32b = A.attn_bwd(*ba, F32, dattn=dattn, keep=keep, bf16=True)
                    ds, dq = OutFlat((B, H, T1, ld)), OutView(B, T1, D)
                    dbd = OutFlat((B, H, T1, ldb)) if square else None
                    map_bwd_launch(dctx, v, pm_d, padded(dattn, ld) if use_dattn else None, H, scale, p, seed, ds.v, ld, dbd.v if square else None, ldb,
                                   k if with_dq else None, dq.v if with_dq else None)
                    tb.slices(where + " dS", ds.v[..., :T2], r64b[0], y32b[0], H, BF16)
                    tb.exact(where, zero_bits(ds.v, zmask), "a masked position or pad column of dS is not +0")
                    if with_dq:
                        tb.slices(where + " dq", dq.v, r64b[1], y32b[1], H, BF16)
                    else:
                        tb.exact(where, same_bits(dq.buf, torch.full_like(dq.buf, SENT)), "dq was written without k")
                    if square:
                        tb.slices(where + " dbd", dbd.v, A.unshift(r64b[0], L=ldb), A.unshift(y32b[0], L=ldb), H, BF16)
                        tb.exact(where, zero_bits(dbd.v, ~hit), "an element of dbd that no admissible dS lands on is not +0")
                        tb.exact(where, dbd.rest_untouched(), "wrote behind dbd")
                    tb.exact(where, ds.rest_untouched() and dq.rest_untouched(), "wrote outside an output")
                    no_key_zero(tb, where, klen, [("dS", ds.v)] + ([("dq", dq.v)] if with_dq else []) + ([("dbd", dbd.v)] if square else []))
        tag = f"T {T1} x {T2}, dk {dk}{', causal, dbd' if causal else ''}{klen_tag(edge, klen)}"
        res += [tf.line(f"attn_map_fwd {tag}"), tb.line(f"attn_map_bwd {tag}")]
    t = Tally()
    keeps.verdict(t, P_DROP)
    res.append(t.line(f"attn_map dk {dk}: keep-scales of p {P_DROP}", f" ({keeps.kept} of {keeps.total} kept)"))
    return res


@case
def attn_map_dk32():
    return _map(32)


@case
def attn_map_dk64():
    return _map(64)


@case
def attn_map_dk96():
    return _map(96)


@case
def attn_map_dk128():
    return _map(128)


@case
def attn_map_dk160():
    return _map(160)


# ---------------------------------------------------------------------------------------------------------------------------
# relattn_fwd
# ---------------------------------------------------------------------------------------------------------------------------
def rel_fwd_launch(q, k, pos, u, v, klen, H, scale, p, seed, attn, pdrop, ld, qu, qv):
    B, T, D = q.shape
    ccall("relattn_fwd", _lib.lib().s2svc_relattn_fwd(B, H, T, D // H, K.ptr(q), q.stride(1), q.stride(0), K.ptr(k), k.stride(1), k.stride(0), K.ptr(pos),
                                                      pos.stride(0), pos.shape[0], K.ptr(u), K.ptr(v), K.ptr(klen), scale, p, seed[0], seed[1],
                                                      K.ptr(attn), K.ptr(pdrop), ld, K.ptr(qu), K.ptr(qv), K.stream()))


def _rel(dk):
    P_DROP = 0.1
    res, keeps = [], Keep()
    B, H = A.B_, A.H_
    for shape, edge in A.with_edges([s for s in A.REL_SHAPES if s[1] == dk], "rel"):
        T = shape[0]
        t = Tally("relattn_fwd")
        inp = A.rel_case_inputs(shape, edge)
        D, ld, scale, klen = H * dk, A.round8(T), inp["scale"], inp["klen"]
        q, k = view_in(inp["q"]), view_in(inp["k"])
        pos = view_in(inp["pos"][None])[0]                                # (2T - 1, D), rows 2 D + 8 apart
        u, v = inp["u"].to(DEV), inp["v"].to(DEV)
        assert _lib.lib().s2svc_relattn_supported(K.dt(BF16), T, dk, 1) == 1 and KAT.view_ok(q) and KAT.view_ok(k), shape
        zmask = must_be_zero(A.key_mask(klen, T, T, False), ld)
        for p in (0.0, P_DROP):
            seed = case_seed("rel", shape, edge, p)
            keep = A.keep_of(keeps.draw((B, H, T, ld), p, seed), T) if p else None
            where = f"p {p}"
            fa = (inp["q"], inp["k"], inp["pos"], inp["u"], inp["v"], klen, scale, H)
            r64, y32 = A.rel_attn_fwd(*fa, F64, keep=keep), A.rel_attn_fwd(*fa, F32, keep=keep, bf16=True)
            attn, pdrop, qu, qv = OutFlat((B, H, T, ld)), OutFlat((B, H, T, ld)), OutFlat((B, T, D)), OutFlat((B, T, D))
            rel_fwd_launch(q, k, pos, u, v, i32(klen), H, scale, p, seed, attn.v, pdrop.v if p else None, ld, qu.v, qv.v)
            t.slices(where + " map", attn.v[..., :T], r64[0], y32[0], H, BF16)
            t.exact(where, zero_bits(attn.v, zmask), "a masked position or pad column of the map is not +0")
            if p:
                t.slices(where + " dropped map", pdrop.v[..., :T], r64[1], y32[1], H, BF16)
                t.exact(where, zero_bits(pdrop.v, dropped_zero(zmask, keep)), "a masked, dropped or pad element of the dropped map is not +0")
            else:
                t.exact(where, same_bits(pdrop.buf, torch.full_like(pdrop.buf, SENT)), "the dropped map was written without dropout")
            t.slices(where + " qu", qu.v, r64[2], y32[2], H, BF16)
            t.slices(where + " qv", qv.v, r64[3], y32[3], H, BF16)
            t.exact(where, all(o.rest_untouched() for o in (attn, pdrop, qu, qv)), "wrote behind an output")
            no_key_zero(t, where, klen, [("the map", attn.v)] + ([("the dropped map", pdrop.v)] if p else []))
        res.append(t.line(f"relattn_fwd T {T}, dk {dk}{klen_tag(edge, klen)}"))
    t = Tally()
    keeps.verdict(t, P_DROP)
    res.append(t.line(f"relattn dk {dk}: keep-scales of p {P_DROP}", f" ({keeps.kept} of {keeps.total} kept)"))
    return res


@case
def relattn_dk32():
    return _rel(32)


@case
def relattn_dk96():
    return _rel(96)


@case
def relattn_dk192():
    return _rel(192)


# ---------------------------------------------------------------------------------------------------------------------------
# attn_softmax_fwd / bwd on given fp32 scores
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_fwd_launch(out_dtype, B, H, T1, T2, ld, scores, bd, Lp, ldb, rel_mode, scale, klen, causal, p, seed, attn, pdrop):
    ccall("attn_softmax_fwd", _lib.lib().s2svc_attn_softmax_fwd(K.dt(out_dtype), B, H, T1, T2, ld, K.ptr(scores), K.ptr(bd), Lp, ldb, rel_mode, scale, K.ptr(klen),
                                                                1 if causal else 0, p, seed[0], seed[1], K.ptr(attn), K.ptr(pdrop), K.stream()))


def softmax_bwd_launch(dtype, B, H, T1, T2, ld, attn, dp, dattn, scale, p, seed, dscores, dbd, Lp, ldb, rel_mode):
    ccall("attn_softmax_bwd", _lib.lib().s2svc_attn_softmax_bwd(K.dt(dtype), B, H, T1, T2, ld, K.ptr(attn), K.ptr(dp), K.ptr(dattn), scale, p, seed[0], seed[1],
                                                                K.ptr(dscores), K.ptr(dbd), Lp, ldb, rel_mode, K.stream()))


def _softmax(dtype):
    P_DROP = 0.3
    res, keeps = [], Keep()
    B, H = A.B_, A.H_
    nm = S.name_of(dtype)
    for shape, edge in A.with_edges(A.SOFTMAX_SHAPES, "softmax"):
        T1, T2, ld, causal, rel_mode = shape
        tf, tb = Tally(f"attn_softmax_fwd[{nm}]"), Tally(f"attn_softmax_bwd[{nm}]")
        inp = A.softmax_case_inputs(shape, edge)
        scale, klen, Lp = inp["scale"], inp["klen"], inp["Lp"]
        ldb = Lp + 5 if rel_mode else 0
        mask = A.key_mask(klen, T1, T2, causal)
        zmask = must_be_zero(mask, ld)
        scores, dp = padded(inp["scores"], ld, fill=SENT), padded(inp["dp"], ld, fill=SENT)
        bd = None
        if rel_mode:
            bd = torch.full((B, H, T1, ldb), SENT, dtype=F32)
            bd[..., :Lp] = inp["bd"]
            bd = bd.to(DEV)
        sa = (inp["scores"], scale, klen, causal)
        pm = A.softmax_fwd(*sa, F64, bd=inp["bd"], rel_mode=rel_mode)[0].to(dtype)
        pm_d = padded(pm, ld)
        for p in (0.0, P_DROP):
            seed = case_seed("softmax", nm, shape, edge, p)
            keep = A.keep_of(keeps.draw((B, H, T1, ld), p, seed), T2) if p else None
            where = f"p {p}"
            r64 = A.softmax_fwd(*sa, F64, bd=inp["bd"], rel_mode=rel_mode, keep=keep)
            y32 = A.softmax_fwd(*sa, F32, bd=inp["bd"], rel_mode=rel_mode, keep=keep, out_bf16=dtype == BF16)
            attn, pdrop = OutFlat((B, H, T1, ld), dtype), OutFlat((B, H, T1, ld), dtype)
            softmax_fwd_launch(dtype, B, H, T1, T2, ld, scores, bd, Lp, ldb, rel_mode, scale, i32(klen), causal, p, seed, attn.v, pdrop.v if p else None)
            tf.slices(where + " map", attn.v[..., :T2], r64[0], y32[0], H, dtype)
            tf.exact(where, zero_bits(attn.v, zmask), "a masked position or pad column of the map is not +0")
            if p:
                tf.slices(where + " dropped map", pdrop.v[..., :T2], r64[1], y32[1], H, dtype)
                tf.exact(where, zero_bits(pdrop.v, dropped_zero(zmask, keep)), "a masked, dropped or pad element of the dropped map is not +0")
            tf.exact(where, attn.rest_untouched() and pdrop.rest_untouched(), "wrote behind an output")
            no_key_zero(tf, where, klen, [("the map", attn.v)] + ([("the dropped map", pdrop.v)] if p else []))
            for use_dattn in (False, True):
                where = f"p {p}, dattn {use_dattn}"
                dattn = inp["dattn"].to(dtype) if use_dattn else None
                r64b = A.softmax_bwd(pm, inp["dp"], scale, F64, dattn=dattn, keep=keep, rel_mode=rel_mode)
                y32b = A.softmax_bwd(pm, inp["dp"], scale, F32, dattn=dattn, keep=keep, rel_mode=rel_mode, out_bf16=dtype == BF16)
                ds = OutFlat((B, H, T1, ld), dtype)
                dbd = OutFlat((B, H, T1, ldb), dtype) if rel_mode else None
                softmax_bwd_launch(dtype, B, H, T1, T2, ld, pm_d, dp, padded(dattn, ld) if use_dattn else None, scale, p, seed, ds.v,
                                   dbd.v if rel_mode else None, Lp, ldb, rel_mode)
                tb.slices(where + " dscores", ds.v[..., :T2], r64b[0], y32b[0], H, dtype)
                tb.exact(where, zero_bits(ds.v, zmask), "a masked position or pad column of dscores is not +0")
                tb.exact(where, ds.rest_untouched(), "wrote behind dscores")
                if rel_mode:
                    tb.slices(where + " dbd", dbd.v[..., :Lp], r64b[1], y32b[1], H, dtype)
                    hit = torch.zeros(B, H, T1, ldb, dtype=torch.bool)
                    hit[..., :Lp] = A.scatter_bd(mask.expand(B, H, T1, T2).to(F32), rel_mode) > 0
                    tb.exact(where, zero_bits(dbd.v, ~hit), "an element of dbd that no admissible dscore lands on is not +0")
                    tb.exact(where, dbd.rest_untouched(), "wrote behind dbd")
                no_key_zero(tb, where, klen, [("dscores", ds.v)] + ([("dbd", dbd.v)] if rel_mode else []))
        tag = f"[{nm}] T {T1} x {T2}, ld {ld}{', causal' if causal else ''}{', rel_mode %d, ldb %d' % (rel_mode, ldb) if rel_mode else ''}{klen_tag(edge, klen)}"
        res += [tf.line(f"attn_softmax_fwd{tag}"), tb.line(f"attn_softmax_bwd{tag}")]
    t = Tally()
    keeps.verdict(t, P_DROP)
    res.append(t.line(f"attn_softmax[{nm}]: keep-scales of p {P_DROP}", f" ({keeps.kept} of {keeps.total} kept)"))
    return res


@case
def attn_softmax_fp32():
    return _softmax(F32)


@case
def attn_softmax_bf16():
    return _softmax(BF16)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: the launchers' host-side argument checks
# ---------------------------------------------------------------------------------------------------------------------------
@case
def attn_launcher_refusals():
    """A shape outside *_supported, a misaligned pointer or stride, and ld < T2 are refused by each launcher before any launch; attn_fused_fwd
    also refuses ld > 64 (its kernel writes the columns below 64 only)."""
    res = []
    B, H, dk = 1, 2, 32
    D = H * dk
    seed = case_seed("refusals")

    def ops(T1, T2):
        x = {n: view_in(torch.zeros(B, T, D, dtype=BF16)) for n, T in (("q", T1), ("k", T2), ("v", T2), ("dctx", T1))}
        ld = A.round8(T2)
        x.update(ld=ld, attn=OutFlat((B, H, T1, ld)), pdrop=OutFlat((B, H, T1, ld)), out=OutView(B, T1, D), dq=OutView(B, T1, D), dk=OutView(B, T2, D),
                 dv=OutView(B, T2, D), T1=T1, T2=T2)
        return x

    def clean(x):
        return [(o.buf, torch.full_like(o.buf, SENT)) for o in x.values() if isinstance(o, (OutFlat, OutView))]

    def odd_ptr(t):                                              # the same strides, the base 8 bytes further: not 16-byte aligned
        return t.as_strided(t.shape, t.stride(), t.storage_offset() - 4)

    def odd_stride(t):                                           # a row stride that is no multiple of 8 elements
        return t.as_strided(t.shape, (t.stride(0), t.stride(1) - 4, 1), t.storage_offset())

    def fused_f(x, q=None, ld=None):
        fused_fwd_launch(q if q is not None else x["q"], x["k"], x["v"], None, False, H, 1.0, 0.0, seed, x["attn"].v, ld or x["ld"], x["out"].v)

    def fused_b(x, q=None, ld=None):
        B_, H_, T1, lda = x["attn"].v.shape
        a = x["attn"].v if ld is None else x["attn"].v.reshape(-1)[:B_ * H_ * T1 * ld].view(B_, H_, T1, ld)
        KAT.fused_bwd(q if q is not None else x["q"], x["k"], x["v"], x["dctx"], a, None, H, 1.0, 0.0, seed, x["dq"].v, x["dk"].v, x["dv"].v)

    def map_f(x, q=None, ld=None):
        map_fwd_launch(q if q is not None else x["q"], x["k"], None, False, H, 1.0, 0.0, seed, x["attn"].v, None, ld or x["ld"], None, None)

    def map_b(x, q=None, ld=None):
        map_bwd_launch(q if q is not None else x["dctx"], x["v"], x["pdrop"].v, None, H, 1.0, 0.0, seed, x["attn"].v, ld or x["ld"], None, 0, None, None)

    def rel_f(x, q=None, ld=None):
        T = x["T1"]
        pos = view_in(torch.zeros(1, 2 * T - 1, D, dtype=BF16))[0]
        u = torch.zeros(D, device=DEV)
        rel_fwd_launch(q if q is not None else x["q"], x["k"], pos, u, u, None, H, 1.0, 0.0, seed, x["attn"].v, None, ld or x["ld"], x["dq"].v, x["dv"].v)

    x = ops(65, 16)
    refused(res, "attn_fused_fwd T1 65", lambda: fused_f(x), "attn_fused_fwd: unsupported shape", clean(x))
    refused(res, "attn_fused_bwd T1 65", lambda: fused_b(x), "attn_fused_bwd: unsupported shape", clean(x))
    x = ops(16, 513)
    refused(res, "attn_map_fwd T2 513", lambda: map_f(x), "attn_map_fwd: bf16, T2 <= 512", clean(x))
    refused(res, "attn_map_bwd T2 513", lambda: map_b(x), "attn_map_bwd: bf16, T2 <= 512", clean(x))
    x = ops(257, 257)
    refused(res, "relattn_fwd T 257", lambda: rel_f(x), "relattn_fwd: bf16, T <= 256", clean(x))
    x = ops(24, 24)
    for name, fn, ptr_msg, stride_msg, ld_msg in (
            ("attn_fused_fwd", fused_f, "attn_fused_fwd: 16-byte aligned q/k/v", "attn_fused_fwd: strides must be multiples of 8 elements", "attn_fused_fwd: the map's row pitch ld must be in [T2, 64]"),
            ("attn_fused_bwd", fused_b, "attn_fused_bwd: 16-byte aligned q/k/v/dout", "attn_fused_bwd: strides must be multiples of 8 elements", "attn_fused_bwd: the map's row pitch ld must be >= T2"),
            ("attn_map_fwd", map_f, "attn_map_fwd: 16-byte aligned operands", "attn_map_fwd: 16-byte aligned operands", "attn_map_fwd: bad args"),
            ("attn_map_bwd", map_b, "attn_map_bwd: 16-byte aligned operands", "attn_map_bwd: 16-byte aligned operands", "attn_map_bwd: bad args"),
            ("relattn_fwd", rel_f, "relattn_fwd: 16-byte aligned operands", "relattn_fwd: 16-byte aligned operands", "relattn_fwd: bad args")):
        src = x["dctx"] if name == "attn_map_bwd" else x["q"]
        refused(res, f"{name} misaligned pointer", lambda: fn(x, q=odd_ptr(src)), ptr_msg, clean(x))
        refused(res, f"{name} row stride 8 n + 4", lambda: fn(x, q=odd_stride(src)), stride_msg, clean(x))
        refused(res, f"{name} ld 16 < T2 24", lambda: fn(x, ld=16), ld_msg, clean(x))
    x = ops(64, 64)
    big = OutFlat((B, H, 64, 72))
    refused(res, "attn_fused_fwd ld 72 > 64",
            lambda: fused_fwd_launch(x["q"], x["k"], x["v"], None, False, H, 1.0, 0.0, seed, big.v, 72, x["out"].v),
            "attn_fused_fwd: the map's row pitch ld must be in [T2, 64]", clean(x) + [(big.buf, torch.full_like(big.buf, SENT))])
    # the softmax kernels: ld < T2 (forward and backward), a position term whose row stride is below its length
    T = 24
    sc = torch.zeros(B * H * T * 48, device=DEV)                 # (large enough for every ld / ldb named below)
    for dtype in (F32, BF16):
        o, o2 = OutFlat((B, H, T, 16), dtype), OutFlat((B, H, T, 16), dtype)
        m = torch.zeros(B * H * T * 24, dtype=dtype, device=DEV)
        un = [(o.buf, torch.full_like(o.buf, SENT)), (o2.buf, torch.full_like(o2.buf, SENT))]
        refused(res, f"attn_softmax_fwd[{S.name_of(dtype)}] ld 16 < T2 24",
                lambda: softmax_fwd_launch(dtype, B, H, T, T, 16, sc, None, 0, 0, 0, 1.0, None, False, 0.0, seed, o.v, None), "attn_softmax_fwd: bad shape", un)
        refused(res, f"attn_softmax_bwd[{S.name_of(dtype)}] ld 16 < T2 24",
                lambda: softmax_bwd_launch(dtype, B, H, T, T, 16, m, sc, None, 1.0, 0.0, seed, o.v, None, 0, 0, 0), "attn_softmax_bwd: bad shape", un)
        refused(res, f"attn_softmax_fwd[{S.name_of(dtype)}] ldb 40 < Lp 47",
                lambda: softmax_fwd_launch(dtype, B, H, T, T, 24, sc, sc, 47, 40, 1, 1.0, None, False, 0.0, seed, o.v, None),
                "attn_softmax_fwd: bd row stride smaller than its length", un)
        refused(res, f"attn_softmax_bwd[{S.name_of(dtype)}] ldb 40 < Lp 47",
                lambda: softmax_bwd_launch(dtype, B, H, T, T, 24, m, sc, None, 1.0, 0.0, seed, o.v, o2.v, 47, 40, 1), "attn_softmax_bwd: bad shape", un)
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
