"""Kernel-level pins of the per-channel column sums (csrc/colsum.h as csrc/norm.hip, csrc/batchnorm.hip and csrc/convmod.hip use it)
on the MI355X, in the three regimes of tests/colsum_ref.py: exact (integer inputs: the float64 truth bit for bit), order pin (N(0, 1)
inputs: the float32 restatement of the documented order bit for bit) and rule (step_kernels_ref.compare, unchanged).
  * `python tests/gpu_colsum_check.py [--only a,b] [--dump FILE]` prints a PASS/FAIL table for all cases and never stops early;
    --dump saves every tensor a kernel returned (torch.save) for a byte comparison of two builds of the library;
  * tests/test_gpu_colsum.py imports CASES and turns each into a `@pytest.mark.gpu` test.
Every output lies in a sentinel-padded buffer whose tail must come back untouched.  References run on the CPU."""
import os
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import colsum_ref as CS  # noqa: E402
import step_kernels_ref as R  # noqa: E402
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402
from seq2seq_vc_amd.ops import kernels_aas as KA  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = -776.0                 # finite, not zero, exact in bf16
PAD = 16
EPS, MOM = 1e-5, 0.1
CASES = []
DUMP = {}                     # name -> tensor the kernel returned (CPU), for --dump
# Rule-regime checks at which the library takes more than 4 d before this module existed: 1.5 x the ratio measured there, with the
# cause (profiles/AB_LOG.md has the runs).  Keys are the `where` of the comparison.
MEASURED_MARGINS = {}


def case(fn):
    CASES.append(fn)
    return fn


def name_of(dtype):
    return "fp32" if dtype == F32 else "bf16"


def dev(t):
    return None if t is None else t.to(DEV)


def i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


class Out:
    """A float32 output of n values in a sentinel-padded buffer; prev: its previous contents (accumulated outputs)."""

    def __init__(self, n, prev=None):
        self.buf = torch.full((n + PAD,), SENT, dtype=F32, device=DEV)
        self.v = self.buf[:n]
        if prev is not None:
            self.v.copy_(prev)

    def tail_ok(self):
        return bool((self.buf[self.v.numel():] == SENT).all())


class Tally:
    def __init__(self):
        self.fail, self.n, self.ratio, self.where = [], 0, 0.0, "-"

    def bits(self, where, got, want):
        DUMP[where] = got.detach().cpu().clone()
        self.n += 1
        if not R.bits_equal(got.detach().cpu(), want.to(got.dtype)):
            bad = int((got.detach().cpu() != want.to(got.dtype)).sum())
            self.fail.append(f"{where}: {bad}/{got.numel()} values differ from the restatement")

    def close(self, where, got, ref64, yard, out_dtype=F32):
        DUMP[where] = got.detach().cpu().clone()
        ok, ratio, d, msg = R.compare(got, ref64, yard, out_dtype, MEASURED_MARGINS.get(where, R.MARGIN))
        self.n += 1
        print(f"    ratio {where}: {ratio:.3f} (d {d:.3e})", flush=True)
        if not ok:
            self.fail.append(f"{where}: {msg}")
        if ratio >= self.ratio and ratio != float("inf"):
            self.ratio, self.where = ratio, where

    def true(self, where, cond, what):
        self.n += 1
        if not cond:
            self.fail.append(f"{where}: {what}")

    def line(self, name):
        if self.fail:
            more = f" (+{len(self.fail) - 3} more)" if len(self.fail) > 3 else ""
            return False, f"{name}: " + "; ".join(self.fail[:3]) + more
        return True, f"{name}: {self.n} checks" + (f", max|got - ref64| / d = {self.ratio:.3f} at {self.where}" if self.ratio else "")


def run_colreduce(mode, inp, rows, D, scale, osum, odot, accumulate, vlens=None, Tn=0):
    K.colreduce(mode, dev(inp["dy"]), dev(inp["x"]), dev(inp["mean"]), dev(inp["rstd"]), scale=scale, rows=rows, D=D, out_sum=osum.v,
                out_dot=None if odot is None else odot.v, accumulate=accumulate, vlens=i32(vlens), Tn=Tn)


def colreduce_exact_one(t, tag, mode, rows, D, dtype, accumulate, vlens=None, Tn=0, scale=1.0):
    inp = CS.colreduce_inputs(mode, rows, D, dtype, exact=True)
    t0, t1 = CS.colreduce_terms(mode, inp, F64)
    keep = CS.present(rows, Tn, vlens)
    prev = [CS.ints(D, seed=11 + mode), CS.ints(D, seed=12 + mode)] if accumulate else [None, None]
    osum = Out(D, prev[0])
    odot = Out(D, prev[1]) if mode in CS.HAS_DOT else None
    run_colreduce(mode, inp, rows, D, scale, osum, odot, accumulate, vlens, Tn)
    sc = R.f32(1.0 / CS.n_present(rows, Tn, vlens)) if scale < 0 else scale
    t.bits(f"{tag} sum", osum.v, CS.finish(CS.colsum(t0, keep).to(F32), sc, prev[0]))
    if odot is not None:
        t.bits(f"{tag} dot", odot.v, CS.finish(CS.colsum(t1, keep).to(F32), sc, prev[1]))
    t.true(tag, osum.tail_ok() and (odot is None or odot.tail_ok()), "wrote past D")


@case
def colreduce_exact():
    """s2svc_colreduce, modes 0-6, fp32 and bf16, accumulate on and off: the float64 truth bit for bit on integer inputs."""
    res = []
    for dtype in (F32, BF16):
        t = Tally()
        for (rows, D) in CS.COLREDUCE_SHAPES:
            for mode in CS.COLREDUCE_MODES:
                for acc in (False, True):
                    colreduce_exact_one(t, f"colreduce exact {name_of(dtype)} {rows}x{D} mode {mode} acc {int(acc)}", mode, rows, D, dtype, acc)
        res.append(t.line(f"colreduce exact {name_of(dtype)}"))
    t = Tally()
    for (rows, D) in CS.COLREDUCE_VEC_SHAPES:
        for mode in CS.COLREDUCE_MODES:
            for acc in (False, True):
                colreduce_exact_one(t, f"colreduce exact 16-byte {rows}x{D} mode {mode} acc {int(acc)}", mode, rows, D, BF16, acc)
    res.append(t.line("colreduce exact 16-byte bf16"))
    return res


@case
def colreduce_masked_exact():
    """Absent rows (vlens = (21, 0, 7) of Tn = 21): skipped by stage 1; scale < 0 = 1 / 28 present rows.  The mean over the present
    rows is taken without `accumulate` (prev + sum * scale may be one fused multiply-add: not the two roundings of the restatement);
    the accumulating runs use scale 1."""
    res = []
    B, Tn, vlens = CS.MASKED["B"], CS.MASKED["Tn"], CS.MASKED["vlens"]
    for dtype in (F32, BF16):
        t = Tally()
        for mode in CS.MASKED_MODES:
            for D in (8, 72):
                colreduce_exact_one(t, f"colreduce masked {name_of(dtype)} D {D} mode {mode} mean", mode, B * Tn, D, dtype, False, vlens, Tn, scale=-1.0)
                colreduce_exact_one(t, f"colreduce masked {name_of(dtype)} D {D} mode {mode} acc", mode, B * Tn, D, dtype, True, vlens, Tn)
        res.append(t.line(f"colreduce masked exact {name_of(dtype)}"))
    return res


def mode7_partials(chunks, D, exact, seed):
    mk = CS.ints if exact else R.randn
    return mk(chunks, 2, D, seed=seed)


@case
def colreduce_grouped_exact():
    """s2svc_colreduce_grouped through K.recording / GradBatch.flush: 25 items (more than one launch holds), two items on one
    output (successive launches), mode-7 items over hand-made partials."""
    t = Tally()
    queue, want, keepalive = K.GradBatch(), [], []
    specs = [(mode, rows, D, dtype) for dtype in (F32, BF16) for (rows, D) in CS.COLREDUCE_SHAPES[1:5] for mode in (0, 1, 2)]
    specs.append((4, 300, 776, BF16))                                     # the 16-byte stage 1 inside the grouped kernel
    assert len(specs) == 25 and len(specs) > CS.CR_MAX
    with K.recording(queue):
        for i, (mode, rows, D, dtype) in enumerate(specs):
            inp = CS.colreduce_inputs(mode, rows, D, dtype, exact=True, seed=i)
            t0, t1 = CS.colreduce_terms(mode, inp, F64)
            prev = [CS.ints(D, seed=50 + i), CS.ints(D, seed=90 + i)]
            osum, odot = Out(D, prev[0]), (Out(D, prev[1]) if mode in CS.HAS_DOT else None)
            run_colreduce(mode, inp, rows, D, 1.0, osum, odot, True)
            tag = f"grouped item {i} ({name_of(dtype)} {rows}x{D} mode {mode})"
            want.append((tag + " sum", osum, CS.finish(CS.colsum(t0).to(F32), 1.0, prev[0])))
            if odot is not None:
                want.append((tag + " dot", odot, CS.finish(CS.colsum(t1).to(F32), 1.0, prev[1])))
        # two reductions into ONE output: they must land in successive launches and both be added
        shared, total = Out(40, CS.ints(40, seed=5)), CS.ints(40, seed=5).to(F64)
        for j in range(2):
            inp = CS.colreduce_inputs(0, 63, 40, F32, exact=True, seed=200 + j)
            run_colreduce(0, inp, 63, 40, 1.0, shared, None, True)
            total = total + CS.colsum(inp["dy"].to(F64))
        want.append(("grouped two items on one output", shared, total.to(F32)))
        for chunks in CS.MODE7_CHUNKS:
            ws = mode7_partials(chunks, 72, True, 300 + chunks)
            prev = [CS.ints(72, seed=310 + chunks), CS.ints(72, seed=320 + chunks)]
            osum, odot, wsd = Out(72, prev[0]), Out(72, prev[1]), ws.to(DEV)
            keepalive.append(wsd)
            K.colreduce_partials(wsd, chunks, 72, osum.v, odot.v)
            want.append((f"grouped mode 7 chunks {chunks} sum", osum, prev[0] + ws[:, 0].to(F64).sum(0).to(F32)))
            want.append((f"grouped mode 7 chunks {chunks} dot", odot, prev[1] + ws[:, 1].to(F64).sum(0).to(F32)))
    t.true("grouped", len(queue.colreduces) == 25 + 2 + len(CS.MODE7_CHUNKS), f"{len(queue.colreduces)} items queued")
    queue.flush()
    for tag, out, w in want:
        t.bits(tag, out.v, w)
        t.true(tag, out.tail_ok(), "wrote past D")
    return [t.line("colreduce grouped exact")]


def bn_buffers(C, seed, exact):
    rm = CS.ints(C, seed=seed) if exact else R.randn(C, seed=seed)
    rv = CS.ints(C, seed=seed + 1).abs() if exact else R.randn(C, seed=seed + 1).abs() + 0.5
    return rm, rv


def run_bn_stats(x, rows, C, vec, vlens, Tn, rm0, rv0):
    rm, rv, nb = Out(C, rm0), Out(C, rv0), torch.full((), 5, dtype=torch.int64, device=DEV)
    if vec:
        mean, rstd = K.bn_stats_vec(dev(x), rows, C, EPS, MOM, rm.v, rv.v, nb, vlens=i32(vlens), Tn=Tn)
    else:
        mean, rstd = K.bn_stats(dev(x), rows, C, EPS, MOM, rm.v, rv.v, nb, vlens=i32(vlens), Tn=Tn)
    return mean, rstd, rm, rv, int(nb)


def bn_stats_one(t, tag, rows, C, dtype, vec, vlens=None, Tn=0, exact=True):
    x = CS.ints(rows, C, seed=rows + C, dtype=dtype) if exact else R.randn(rows, C, seed=rows + C, dtype=dtype)
    rm0, rv0 = bn_buffers(C, rows + C + 1, exact)
    keep = CS.present(rows, Tn, vlens)
    mean, rstd, rm, rv, nb = run_bn_stats(x, rows, C, vec, vlens, Tn, rm0, rv0)
    n = CS.n_present(rows, Tn, vlens)
    if exact:              # mean = float32(sum) * float32(1 / n) bit for bit; n = 1 takes the other branch of the unbiased variance
        t.bits(f"{tag} mean", mean, CS.finish(CS.colsum(x.to(F64), keep).to(F32), R.f32(1.0 / n)))
    t.true(tag, nb == 6, f"num_batches advanced {nb - 5} times")
    t.true(tag, rm.tail_ok() and rv.tail_ok(), "running statistics written past C")
    ref, yard = CS.bn_stats64(x, EPS, MOM, rm0, rv0, keep), CS.bn_stats_yard(x, EPS, MOM, rm0, rv0, keep)
    for nm, got, r64, y in zip(("mean", "rstd", "running mean", "running var"), (mean, rstd, rm.v, rv.v), ref, yard):
        if not (exact and nm == "mean"):
            t.close(f"{tag} {nm}", got, r64, y)


@case
def bn_stats_exact():
    """s2svc_bn_stats (fp32 / bf16, with and without vlens) and s2svc_bn_stats_vec on integer inputs: mean bit-equal to
    float32(sum) * float32(1 / n), num_batches advanced once; rstd and the running statistics under the rule (E[x^2] - m^2 may or may
    not be contracted to a fused multiply-add: no bits demanded there)."""
    res = []
    t = Tally()
    for dtype in (F32, BF16):
        for (rows, C) in CS.BN_SCALAR_SHAPES:
            bn_stats_one(t, f"bn_stats exact {name_of(dtype)} {rows}x{C}", rows, C, dtype, False)
        m = CS.MASKED
        bn_stats_one(t, f"bn_stats exact {name_of(dtype)} masked", m["B"] * m["Tn"], 72, dtype, False, m["vlens"], m["Tn"])
    res.append(t.line("bn_stats exact"))
    t = Tally()
    for C in CS.BN_VEC_C:
        for rows in CS.BN_VEC_ROWS:
            bn_stats_one(t, f"bn_stats_vec exact {rows}x{C}", rows, C, BF16, True)
    m = CS.MASKED
    bn_stats_one(t, "bn_stats_vec exact masked", m["B"] * m["Tn"], 72, BF16, True, m["vlens"], m["Tn"])
    res.append(t.line("bn_stats_vec exact"))
    return res


@case
def bn_finalize_rule():
    """s2svc_bn_finalize on given mean / var (biased variance and E[x^2]), n = 1 and n > 1, with and without vlens."""
    t = Tally()
    for (C, n, ex2, vlens, Tn) in ((8, 1, False, None, 0), (72, 300, False, None, 0), (72, 300, True, None, 0), (300, 63, True, (21, 0, 7), 21)):
        mean = R.randn(C, seed=C + n)
        var = (mean * mean + R.randn(C, seed=C + n + 1).abs()) if ex2 else R.randn(C, seed=C + n + 1).abs()
        rm0, rv0 = bn_buffers(C, C + n + 2, False)
        rm, rv, nb = Out(C, rm0), Out(C, rv0), torch.full((), 5, dtype=torch.int64, device=DEV)
        rstd = K.bn_finalize(dev(mean), dev(var), n, EPS, MOM, rm.v, rv.v, nb, var_is_ex2=ex2, vlens=i32(vlens), Tn=Tn)
        np_ = CS.n_present(n, Tn, vlens)
        tag = f"bn_finalize C {C} n {np_} ex2 {int(ex2)}"
        ref, yard = (CS.bn_finalize(mean, var, np_, EPS, MOM, rm0, rv0, d, ex2) for d in (F64, F32))
        for nm, got, r64, y in zip(("rstd", "running mean", "running var"), (rstd, rm.v, rv.v), ref, yard):
            t.close(f"{tag} {nm}", got, r64, y)
        t.true(tag, int(nb) == 6 and rm.tail_ok() and rv.tail_ok(), "num_batches not advanced once, or written past C")
    return [t.line("bn_finalize rule")]


def run_convmod_fwd(y2, w, b, ks, vlens, rm0, rv0):
    C = w.shape[0]
    rm, rv, nb = Out(C, rm0), Out(C, rv0), torch.full((), 5, dtype=torch.int64, device=DEV)
    z, mean, rstd = KA.convmod_fwd(dev(y2), dev(w), dev(b), ks, EPS, MOM, rm.v, rv.v, nb, vlens=i32(vlens))
    return z, mean, rstd, rm, rv, int(nb)


@case
def convmod_fwd_stats_exact():
    """s2svc_convmod_fwd's statistics with z = a exactly (one-hot centre tap, bias 0, gate 30): z bit for bit, mean bit-equal to
    float32(sum) * float32(1 / n); rstd and the running statistics under the rule."""
    t = Tally()
    for (B, T, C, ks, vlens) in CS.CONVMOD_SHAPES:
        y2, w, b, a = CS.convmod_exact_inputs(B, T, C, ks, seed=B * T + C)
        rm0, rv0 = bn_buffers(C, B * T + C + 1, True)
        z, mean, rstd, rm, rv, nb = run_convmod_fwd(y2, w, b, ks, vlens, rm0, rv0)
        tag = f"convmod_fwd exact B{B} T{T} C{C} k{ks}" + (" masked" if vlens else "")
        keep = CS.present(B * T, T, vlens)
        n = CS.n_present(B * T, T, vlens)
        zf = z.reshape(B * T, C).cpu()
        t.bits(f"{tag} z", zf[keep], a.reshape(B * T, C)[keep])
        t.bits(f"{tag} mean", mean, CS.finish(CS.colsum(a.reshape(B * T, C).to(F64), keep).to(F32), R.f32(1.0 / n)))
        t.true(tag, nb == 6 and rm.tail_ok() and rv.tail_ok(), "num_batches not advanced once, or written past C")
        x = a.reshape(B * T, C)
        ref, yard = CS.bn_stats64(x, EPS, MOM, rm0, rv0, keep), CS.bn_stats_yard(x, EPS, MOM, rm0, rv0, keep)
        for nm, got, r64, y in list(zip(("mean", "rstd", "running mean", "running var"), (mean, rstd, rm.v, rv.v), ref, yard))[1:]:
            t.close(f"{tag} {nm}", got, r64, y)
    return [t.line("convmod_fwd statistics exact")]


def run_bn_act_bwd(dz, x, mean, rstd, gamma, acc, prev):
    C = x.shape[-1]
    dg, db = (Out(C, prev[0]), Out(C, prev[1])) if acc else (None, None)
    dx, sdy, sdyx = K.bn_act_bwd_vec(dev(dz), None, dev(x), dev(mean), dev(rstd), dev(gamma), act=None, p=0.0,
                                     dgamma_acc=dg.v if acc else None, dbeta_acc=db.v if acc else None)
    return dx, sdy, sdyx, dg, db


@case
def bn_act_bwd_vec_exact():
    """s2svc_bn_act_bwd_vec with act none, p = 0, mean 0, rstd 1: sdy = sum dz and sdyx = sum dz * x exactly, with and without the
    gradient slots dgamma_acc / dbeta_acc."""
    t = Tally()
    for C in CS.BN_VEC_C:
        for rows in CS.BN_VEC_ROWS:
            dz, x = CS.ints(rows, C, seed=rows + C + 3, dtype=BF16), CS.ints(rows, C, seed=rows + C + 4, dtype=BF16)
            s0, s1 = CS.colsum(dz.to(F64)).to(F32), CS.colsum(dz.to(F64) * x.to(F64)).to(F32)
            for acc in (False, True):
                prev = [CS.ints(C, seed=C + 1), CS.ints(C, seed=C + 2)]
                _, sdy, sdyx, dg, db = run_bn_act_bwd(dz, x, torch.zeros(C), torch.ones(C), torch.ones(C), acc, prev)
                tag = f"bn_act_bwd_vec exact {rows}x{C} acc {int(acc)}"
                t.bits(f"{tag} sdy", sdy, s0)
                t.bits(f"{tag} sdyx", sdyx, s1)
                if acc:
                    t.bits(f"{tag} dbeta_acc", db.v, prev[1] + s0)
                    t.bits(f"{tag} dgamma_acc", dg.v, prev[0] + s1)
                    t.true(tag, dg.tail_ok() and db.tail_ok(), "wrote past C")
    return [t.line("bn_act_bwd_vec exact")]


@case
def order_pin():
    """The fixed order of additions, executable: colreduce mode 0 (scalar fp32, scalar bf16, 16-byte), the mode-7 stage 2 and sdy of
    s2svc_bn_act_bwd_vec (act none, p = 0) on N(0, 1) inputs equal the float32 restatement of the documented order bit for bit."""
    t = Tally()
    for dtype, shapes in ((F32, CS.COLREDUCE_SHAPES), (BF16, CS.COLREDUCE_SHAPES), (BF16, CS.COLREDUCE_VEC_SHAPES)):
        for (rows, D) in shapes:
            inp = CS.colreduce_inputs(0, rows, D, dtype, exact=False)
            osum = Out(D)
            run_colreduce(0, inp, rows, D, 1.0, osum, None, False)
            chunks, rpc = CS.colreduce_chunks(rows)
            t.bits(f"order colreduce mode 0 {name_of(dtype)} {rows}x{D}", osum.v, CS.ordered_colsum(inp["dy"], chunks, rpc))
    for chunks in CS.MODE7_CHUNKS:
        ws = mode7_partials(chunks, 72, False, 400 + chunks)
        osum, odot = Out(72, torch.zeros(72)), Out(72, torch.zeros(72))
        K.colreduce_partials(ws.to(DEV), chunks, 72, osum.v, odot.v)
        t.bits(f"order mode 7 chunks {chunks} sum", osum.v, CS.stage2_ordered(ws[:, 0]))
        t.bits(f"order mode 7 chunks {chunks} dot", odot.v, CS.stage2_ordered(ws[:, 1]))
    for (rows, C) in ((1, 8), (63, 64), (65, 72), (4100, 72), (300, 520)):
        dz, x = R.randn(rows, C, seed=rows + C + 5, dtype=BF16), R.randn(rows, C, seed=rows + C + 6, dtype=BF16)
        _, sdy, _, _, _ = run_bn_act_bwd(dz, x, torch.zeros(C), torch.ones(C), torch.ones(C), False, None)
        chunks, rpc = CS.bn_vec_chunks(rows)
        t.bits(f"order bn_act_bwd_vec sdy {rows}x{C}", sdy, CS.ordered_colsum(dz, chunks, rpc, step=32))
    return [t.line("order pin")]


@case
def colreduce_rule():
    """s2svc_colreduce, modes 0-6, on N(0, 1) inputs, rows <= 300: every output under step_kernels_ref.compare."""
    res = []
    for dtype in (F32, BF16):
        t = Tally()
        for (rows, D) in CS.RULE_SHAPES:
            for mode in CS.COLREDUCE_MODES:
                inp = CS.colreduce_inputs(mode, rows, D, dtype, exact=False)
                scale = R.f32(1.0 / rows)
                osum, odot = Out(D), (Out(D) if mode in CS.HAS_DOT else None)
                run_colreduce(mode, inp, rows, D, scale, osum, odot, False)
                r64, y32 = CS.colreduce_terms(mode, inp, F64), CS.colreduce_terms(mode, inp, F32)
                tag = f"colreduce rule {name_of(dtype)} {rows}x{D} mode {mode}"
                t.close(f"{tag} sum", osum.v, CS.finish(CS.colsum(r64[0]), scale, dt=F64), CS.finish(CS.colsum(y32[0]), scale))
                if odot is not None:
                    t.close(f"{tag} dot", odot.v, CS.finish(CS.colsum(r64[1]), scale, dt=F64), CS.finish(CS.colsum(y32[1]), scale))
        res.append(t.line(f"colreduce rule {name_of(dtype)}"))
    return res


@case
def bn_stats_rule():
    """s2svc_bn_stats / s2svc_bn_stats_vec on N(0, 1) inputs: mean, rstd and the running statistics under the rule."""
    t = Tally()
    m = CS.MASKED
    for dtype in (F32, BF16):
        for (rows, C) in ((65, 72), (257, 136)):
            bn_stats_one(t, f"bn_stats rule {name_of(dtype)} {rows}x{C}", rows, C, dtype, False, exact=False)
        bn_stats_one(t, f"bn_stats rule {name_of(dtype)} masked", m["B"] * m["Tn"], 72, dtype, False, m["vlens"], m["Tn"], exact=False)
    for (rows, C) in ((63, 8), (65, 72), (300, 520)):
        bn_stats_one(t, f"bn_stats_vec rule {rows}x{C}", rows, C, BF16, True, exact=False)
    bn_stats_one(t, "bn_stats_vec rule masked", m["B"] * m["Tn"], 72, BF16, True, m["vlens"], m["Tn"], exact=False)
    return [t.line("bn_stats rule")]


@case
def convmod_bwd_stats_rule():
    """The statistics of s2svc_convmod_bwd (sdy = sum dpre, sdyx = sum dpre * xhat, dpre = da * swish'(BN(z))) on N(0, 1) inputs under
    the rule, and the gradient slots they are added to."""
    t = Tally()
    for (B, T, C, ks, vlens) in CS.CONVMOD_SHAPES:
        s = B * T + C
        da, z, y2 = (R.randn(*sh, seed=s + i, dtype=BF16) for i, sh in enumerate(((B, T, C), (B, T, C), (B, T, 2 * C))))
        w = R.randn(C, 1, ks, seed=s + 3, scale=0.3)
        mean, rstd = R.randn(C, seed=s + 4, scale=0.3), R.randn(C, seed=s + 5, scale=0.2).abs() + 0.8
        gamma, beta = 1.0 + R.randn(C, seed=s + 6, scale=0.2), R.randn(C, seed=s + 7, scale=0.2)
        prev = [R.randn(C, seed=s + 8), R.randn(C, seed=s + 9)]
        dg, db = Out(C, prev[0]), Out(C, prev[1])
        _, sdy, sdyx, _ = KA.convmod_bwd(dev(da), dev(z), dev(y2), dev(w), dev(mean), dev(rstd), dev(gamma), dev(beta), ks,
                                         dgamma_acc=dg.v, dbeta_acc=db.v, vlens=i32(vlens))
        keep = CS.present(B * T, T, vlens)
        r64, y32 = (CS.convmod_bwd_stats(da.reshape(B * T, C), z.reshape(B * T, C), mean, rstd, gamma, beta, d, keep) for d in (F64, F32))
        tag = f"convmod_bwd rule B{B} T{T} C{C} k{ks}" + (" masked" if vlens else "")
        t.close(f"{tag} sdy", sdy, r64[0], y32[0])
        t.close(f"{tag} sdyx", sdyx, r64[1], y32[1])
        t.close(f"{tag} dbeta_acc", db.v, prev[1].to(F64) + r64[0], prev[1] + y32[0])
        t.close(f"{tag} dgamma_acc", dg.v, prev[0].to(F64) + r64[1], prev[0] + y32[1])
        t.true(tag, dg.tail_ok() and db.tail_ok(), "wrote past C")
    return [t.line("convmod_bwd statistics rule")]


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
    if "--dump" in sys.argv:
        torch.save(DUMP, sys.argv[sys.argv.index("--dump") + 1])
        print(f"== dumped {len(DUMP)} tensors")
    return nfail


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
