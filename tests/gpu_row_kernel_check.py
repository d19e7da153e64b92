"""Kernel-level pins of the row-wise and element-wise kernels between the GEMMs on the MI355X (csrc/norm.hip: LayerNorm with residual,
dropout and hscale, every route; csrc/sdp.hip: ln_act_fwd / ln_act_bwd / dw_ln_act_fwd; csrc/elementwise.hip: activation + dropout,
positional encoding, GLU, adds, casts; csrc/batchnorm.hip: the element-wise BatchNorm kernels), in the regimes of
tests/row_kernels_ref.py: exact (the float64 truth bit for bit), rule (step_kernels_ref.compare, unchanged) and route equality.
  * `python tests/gpu_row_kernel_check.py [--only a,b] [--dump FILE]` prints a PASS/FAIL table for all cases and never stops early;
    --dump saves every tensor a kernel returned (torch.save) for a byte comparison of two builds of the library;
  * tests/test_gpu_row_kernels.py imports CASES and turns each into a `@pytest.mark.gpu` test.
Every output lies in a sentinel-padded buffer whose surroundings must come back untouched; the slack of strided inputs holds NaN.  Dropout
is data: the keep-scales are what the standalone dropout kernel draws on ones with the same seed.  References run on the CPU."""
import math
import os
import sys
import traceback
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import row_kernels_ref as RK  # noqa: E402
import step_kernels_ref as R  # noqa: E402
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = -776.0                 # finite, not zero, exact in bf16
PAD = 16
P_DROP = 0.5                  # keep-scale 2: exact in every type
CASES = []
DUMP = {}                     # name -> tensor the kernel returned (CPU), for --dump
# Rule-regime checks at which the library takes more than 4 d before this module existed: 1.5 x the ratio measured there, with the
# cause (profiles/AB_LOG.md has the runs).  Keys are the `where` of the comparison, values (margin, cause).
MEASURED_MARGINS = {
    # Seven values of which three are kept: d is torch's error at three elements (0.3 ulp).  erff on the card is good to 2 - 3 ulp, and
    # 1 + erf cancels for x < 0: 3.3 ulp of y, 3.6 ulp of dx.  Measured need 6.869 (y) and 7.537 (dx).
    "act_dropout fp32 n 7 gelu p 0.5 y": (10.31, "erff 3 ulp against a three-element d"),
    "act_dropout fp32 n 7 gelu p 0.5 dx": (11.31, "erff 3 ulp against a three-element d"),
}
_SEED_BASE = []


def case(fn):
    CASES.append(fn)
    return fn


def name_of(dtype):
    return "fp32" if dtype == F32 else "bf16"


def ccall(name, rc):
    _lib.check(rc, name)


def case_seed(*key):
    """(base pointer, offset) as the launchers take a dropout seed, a function of `key` alone."""
    if not _SEED_BASE:
        _SEED_BASE.append(torch.full((1,), 0x5EED, dtype=torch.int64, device=DEV))
    return _SEED_BASE[0].data_ptr(), (zlib.crc32(repr(key).encode()) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


class Buf:
    """A tensor of `shape` inside a flat sentinel-filled buffer, `off` elements behind its (512-byte aligned) start -- off = 1 takes a
    pointer off the 16-byte routes -- and PAD elements in front of its end.  src: its contents (an input), else the sentinel (an output)."""

    def __init__(self, shape, dtype, off=0, src=None, fill=SENT):
        self.n = int(math.prod(shape))
        self.off = off
        self.buf = torch.full((off + self.n + PAD,), fill, dtype=dtype, device=DEV)
        self.v = self.buf[off:off + self.n].view(shape)
        if src is not None:
            self.v.copy_(src.to(dtype))

    def rest_ok(self):
        b = self.buf.cpu()
        return bool((b[:self.off] == SENT).all()) and bool((b[self.off + self.n:] == SENT).all())


def dev(t, off=0):
    """An input on the card (None stays None)."""
    return None if t is None else Buf(tuple(t.shape), t.dtype, off, src=t).v


def strided(t, ld):
    """A (rows, D) input as a column block of a (rows, ld) buffer whose slack holds NaN."""
    rows, D = t.shape
    buf = torch.full((rows, ld), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :D] = t.to(DEV)
    return buf[:, :D]


_HELD = []


def H(t, off=0):
    """The device pointer of an input handed straight to a launcher.  The tensor is HELD until the next Tally starts: a temporary would be
    freed as soon as its pointer is taken, and the next input's allocation could land on it before the kernel has been launched."""
    if t is None:
        return None
    d = t if t.is_cuda else dev(t, off)
    _HELD.append(d)
    return d.data_ptr()


class Keep:
    """The keep-scales of one p, and the keep rate over everything drawn so far (an exact condition of its own)."""

    def __init__(self, p):
        self.p, self.kept, self.total, self.bad_value = p, 0, 0, False

    def draw(self, shape, seed):
        n = int(math.prod(shape))
        full = K.act_dropout_fwd(torch.ones(n, dtype=F32, device=DEV), None, self.p, seed).cpu().view(shape)
        inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(self.p, dtype=F32))
        self.bad_value = self.bad_value or not bool(((full == 0) | (full == inv)).all())
        self.kept, self.total = self.kept + int((full != 0).sum()), self.total + n
        return full

    def verdict(self, t):
        t.true("keep-scales", not self.bad_value, "a keep-scale is neither 0 nor 1 / (1 - p)")
        t.true("keep rate", self.total >= 10000, f"only {self.total} keep-scales drawn: too few to hold the rate to 0.02")
        rate = self.kept / max(1, self.total)
        t.true("keep rate", abs(rate - (1 - self.p)) <= 0.02, f"keep rate {rate:.4f} not within 0.02 of {1 - self.p}")


def draw(keeps, shape, p, seed):
    return keeps[p].draw(shape, seed) if p else None


class Tally:
    def __init__(self):
        self.fail, self.n, self.ratio, self.where = [], 0, 0.0, "-"
        del _HELD[:]

    def bits(self, where, got, want):
        got = got.detach().cpu()
        DUMP[where] = got.clone()
        self.n += 1
        want = want.to(F32).to(got.dtype) if want.dtype == F64 else want.to(got.dtype)
        if not R.bits_equal(got, want):
            bad = (got.contiguous().view(torch.int16 if got.dtype == BF16 else torch.int32) != want.contiguous().view(torch.int16 if got.dtype == BF16 else torch.int32))
            i = tuple(torch.nonzero(bad)[0].tolist())
            self.fail.append(f"{where}: {int(bad.sum())}/{got.numel()} values differ from the restatement, first at {list(i)} got {float(got[i])!r} want {float(want[i])!r}")

    def close(self, where, got, ref64, yard, out_dtype):
        DUMP[where] = got.detach().cpu().clone()
        margin = MEASURED_MARGINS.get(where, (R.MARGIN,))[0]
        ok, ratio, d, msg = R.compare(got, ref64, yard, out_dtype, margin)
        self.n += 1
        if ratio > 1.0 or not ok:
            print(f"    ratio {where}: {ratio:.3f} (d {d:.3e})", flush=True)
        if not ok:
            self.fail.append(f"{where}: {msg}")
        if ratio >= self.ratio and ratio != float("inf"):
            self.ratio, self.where = ratio, where

    def true(self, where, cond, what):
        self.n += 1
        if not cond:
            self.fail.append(f"{where}: {what}")

    def zero_bits(self, where, got, mask, what):
        """got[mask] is +0 bit for bit (mask broadcasts over the trailing dimensions)."""
        g = got.detach().cpu().contiguous()
        bitsv = g.view(torch.int16 if g.dtype == BF16 else torch.int32)
        m = mask.reshape(tuple(mask.shape) + (1,) * (g.dim() - mask.dim())).expand(g.shape)
        bad = int((bitsv[m] != 0).sum())
        self.true(where, bad == 0, f"{bad}/{int(m.sum())} {what} are not +0")

    def line(self, name):
        if self.fail:
            more = f" (+{len(self.fail) - 3} more)" if len(self.fail) > 3 else ""
            return False, f"{name}: " + "; ".join(self.fail[:3]) + more
        return True, f"{name}: {self.n} checks" + (f", max|got - ref64| / d = {self.ratio:.3f} at {self.where}" if self.ratio else "")


class JointStats:
    """The per-row statistics (fp32 mean, rstd) of several launches of one shape family, compared as ONE tensor: the d of a one-row launch
    alone is the error of a single float32 sum of torch's, which can be a small fraction of an ulp by luck."""

    def __init__(self):
        self.parts = {}

    def add(self, name, got, ref64, yard):
        self.parts.setdefault(name, []).append((got.detach().cpu().reshape(-1), ref64.reshape(-1), yard.reshape(-1)))

    def close(self, t, tag):
        for name, parts in self.parts.items():
            t.close(f"{tag} {name}", *(torch.cat([p[i] for p in parts]) for i in range(3)), F32)


def new_keeps():
    return {P_DROP: Keep(P_DROP), 0.2: Keep(0.2)}


def keeps_verdict(t, keeps):
    for k in keeps.values():
        if k.total:
            k.verdict(t)


def refused(fn, text):
    """True if the launcher refuses with the documented error."""
    try:
        fn()
    except RuntimeError as e:
        return text in str(e)
    return False


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------------------------------------------------------
LN_COMBOS = ((False, 0.0, 1.0), (True, 0.0, 1.0), (True, 0.0, 0.5), (True, P_DROP, 1.0), (True, P_DROP, 0.5))     # res, p, hscale


def ln_fwd_launch(dtype, rows, D, x, res, p, hscale, seed, gamma, beta, y, s_out, mean, rstd):
    ccall("layernorm_fwd", _lib.lib().s2svc_layernorm_fwd(K.dt(dtype), rows, D, K.ptr(x), K.ptr(res), p, hscale, seed[0], seed[1], K.ptr(gamma), K.ptr(beta),
                                                           RK.LN_EPS, K.ptr(y), K.ptr(s_out), K.ptr(mean), K.ptr(rstd), K.stream()))


def ln_fwd_one(t, keeps, tag, dtype, rows, D, with_res, p, hscale, regime, mis=None, stats=None):
    seed = case_seed("ln_fwd", tag)
    keep = draw(keeps, (rows, D), p if with_res else 0.0, seed)
    if regime == "exact":
        inp = RK.ln_fwd_exact_inputs(rows, D, dtype, with_res, keep, hscale, seed=D + rows)
    else:
        inp = RK.ln_rule_inputs(rows, D, dtype, with_res, seed=D + rows, offset=(regime == "offset"))
    off = {n: int(mis == n) for n in RK.LN_MISALIGN_FWD}
    x, res = dev(inp["x"], off["x"]), dev(inp["res"], off["res"])
    gamma, beta = dev(inp["gamma"], off["gamma"]), dev(inp["beta"], off["beta"])
    y, s = Buf((rows, D), dtype, off["y"]), (Buf((rows, D), dtype, off["s_out"]) if with_res else None)
    mean, rstd = Buf((rows,), F32), Buf((rows,), F32)
    ln_fwd_launch(dtype, rows, D, x, res, p, hscale, seed, gamma, beta, y.v, None if s is None else s.v, mean.v, rstd.v)
    args = (inp["x"], inp["res"], keep, hscale, inp["gamma"], inp["beta"], RK.LN_EPS)
    if regime == "exact":
        want = RK.exact_premise(lambda d: RK.ln_fwd(*args, d, store=dtype), f" ({tag})")
        t.bits(f"{tag} y", y.v, want[0])
        if with_res:
            t.bits(f"{tag} s", s.v, want[1])
        t.bits(f"{tag} mean", mean.v, want[2])
        t.bits(f"{tag} rstd", rstd.v, want[3])
    else:
        ref, yard = RK.ln_fwd(*args, F64, store=dtype), RK.ln_fwd(*args, F32, store=dtype)
        # the last row is constant unless dropout breaks it up: y = beta there, and its rstd (1e6) is held to a d of its own
        const = rows > 1 and not (with_res and p)
        body = slice(0, rows - 1) if const else slice(0, rows)
        t.close(f"{tag} y", y.v[body], ref[0][body], yard[0][body], dtype)
        if with_res:
            t.close(f"{tag} s", s.v, ref[1], yard[1], dtype)
        if stats is None:
            t.close(f"{tag} mean", mean.v, ref[2], yard[2], F32)
            t.close(f"{tag} rstd", rstd.v[body], ref[3][body], yard[3][body], F32)
        else:       # held jointly with the other row counts of this combination (JointStats)
            stats.add("mean", mean.v, ref[2], yard[2])
            stats.add("rstd", rstd.v[body], ref[3][body], yard[3][body])
        if const:
            t.bits(f"{tag} y of the constant row", y.v[-1], inp["beta"].to(dtype))
            t.close(f"{tag} rstd of the constant row", rstd.v[-1:], ref[3][-1:], yard[3][-1:], F32)
    t.true(tag, y.rest_ok() and (s is None or s.rest_ok()) and mean.rest_ok() and rstd.rest_ok(), "wrote outside an output")


def ln_fwd_family(dtype, regime):
    res, keeps = [], new_keeps()
    for (dt_, D, al) in RK.LN_CASES:
        if dt_ != dtype or not al or (regime == "exact" and D % 2):
            continue
        t = Tally()
        for (with_res, p, hscale) in LN_COMBOS:
            stats = None if regime == "exact" else JointStats()
            for rows in RK.ROWS:
                ln_fwd_one(t, keeps, f"ln_fwd {regime} {name_of(dtype)} {rows}x{D} res {int(with_res)} p {p} hscale {hscale}", dtype, rows, D, with_res, p, hscale, regime, stats=stats)
            if stats is not None:
                stats.close(t, f"ln_fwd {regime} {name_of(dtype)} rows {RK.ROWS} D {D} res {int(with_res)} p {p} hscale {hscale}")
        res.append(t.line(f"layernorm_fwd {regime} {name_of(dtype)} D {D} ({RK.ln_fwd_route(dtype, D)})"))
    t = Tally()
    keeps_verdict(t, keeps)
    res.append(t.line(f"layernorm_fwd {regime} {name_of(dtype)} keep-scales"))
    return res


@case
def layernorm_fwd_exact_fp32():
    """Balanced +-1 rows, integer gamma / beta: y, s, mean = 0 and rstd = 1 bit for bit on every fp32 route (D = 1 is rule-only: no even D)."""
    return ln_fwd_family(F32, "exact")


@case
def layernorm_fwd_exact_bf16():
    return ln_fwd_family(BF16, "exact")


@case
def layernorm_fwd_rule_fp32():
    """N(0, 1) rows and rows offset by up to +-30 at scale 0.1, one constant row per case."""
    return ln_fwd_family(F32, "rule") + ln_fwd_family(F32, "offset")


@case
def layernorm_fwd_rule_bf16():
    return ln_fwd_family(BF16, "rule") + ln_fwd_family(BF16, "offset")


@case
def layernorm_misaligned():
    """bf16, D = 384 with ONE pointer off the 16-byte grid at a time (bf16 tensors by 2 bytes; the fp32 gamma / beta by one element, the
    smallest offset a float pointer can have): the scalar kernels must take over, forward and backward, exact and rule."""
    t, keeps = Tally(), new_keeps()
    for mis in RK.LN_MISALIGN_FWD:
        for regime in ("exact", "rule"):
            ln_fwd_one(t, keeps, f"ln_fwd {regime} bf16 5x384 {mis} misaligned", BF16, 5, 384, True, P_DROP, 0.5, regime, mis=mis)
    for mis in RK.LN_MISALIGN_BWD:
        ln_bwd_one(t, keeps, f"ln_bwd rule bf16 5x384 {mis} misaligned", BF16, 5, 384, P_DROP, 0.5, True, "rule", mis=mis)
    keeps_verdict(t, keeps)
    return [t.line("layernorm misaligned pointers (ln_fwd_reg_kernel<bf16_t, 8>, ln_bwd_kernel<bf16_t>)")]


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------
def ln_bwd_launch(dtype, rows, D, dy, s, mean, rstd, gamma, extra, p, hscale, seed, ds, dh):
    ccall("layernorm_bwd", _lib.lib().s2svc_layernorm_bwd(K.dt(dtype), rows, D, K.ptr(dy), K.ptr(s), K.ptr(mean), K.ptr(rstd), K.ptr(gamma), K.ptr(extra), p, hscale,
                                                           seed[0], seed[1], K.ptr(ds), K.ptr(dh), K.stream()))


def ln_bwd_one(t, keeps, tag, dtype, rows, D, p, hscale, use_extra, regime, mis=None):
    seed = case_seed("ln_bwd", tag)
    keep = draw(keeps, (rows, D), p, seed)
    inp = RK.ln_bwd_inputs(rows, D, dtype, seed=D + rows, exact=(regime == "exact"), offset=(regime == "offset"))
    extra = inp["ds_extra"] if use_extra else None
    off = {n: int(mis == n) for n in RK.LN_MISALIGN_BWD}
    dy, s, ex, gamma = dev(inp["dy"], off["dy"]), dev(inp["s"], off["s"]), dev(extra, off["ds_extra"]), dev(inp["gamma"], off["gamma"])
    mean, rstd = dev(inp["mean"]), dev(inp["rstd"])
    ds, dh = Buf((rows, D), dtype, off["ds"]), Buf((rows, D), dtype, off["dh"])
    ln_bwd_launch(dtype, rows, D, dy, s, mean, rstd, gamma, ex, p, hscale, seed, ds.v, dh.v)
    args = (inp["dy"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], extra, keep, hscale)
    ref, yard = RK.ln_bwd(*args, F64, store=dtype), RK.ln_bwd(*args, F32, store=dtype)
    if regime == "exact":
        raw = RK.ln_bwd(*args, F32)
        t.true(tag, all(bool((u.to(F64) == v).all()) for u, v in zip(raw[:2], ref[:2])), "exact premise broken")
        t.bits(f"{tag} ds", ds.v, ref[0])
        t.bits(f"{tag} dh", dh.v, ref[1])
    else:
        t.close(f"{tag} ds", ds.v, ref[0], yard[0], dtype)
        t.close(f"{tag} dh", dh.v, ref[1], yard[1], dtype)
    if keep is not None:
        t.zero_bits(tag, dh.v, keep == 0, "dropped elements of dh")
    t.true(tag, ds.rest_ok() and dh.rest_ok(), "wrote outside an output")
    return ds, dh


def ln_bwd_family(dtype):
    res, keeps = [], new_keeps()
    for (dt_, D, al) in RK.LN_CASES:
        if dt_ != dtype or not al:
            continue
        t = Tally()
        regimes = ("rule", "offset") + (("exact",) if D & (D - 1) == 0 else ())        # exact: D a power of two (the row means are exact)
        for regime in regimes:
            for rows in RK.ROWS:
                for (p, hscale, use_extra) in ((0.0, 1.0, False), (P_DROP, 0.5, True), (P_DROP, 1.0, False)):
                    ln_bwd_one(t, keeps, f"ln_bwd {regime} {name_of(dtype)} {rows}x{D} p {p} hscale {hscale} extra {int(use_extra)}", dtype, rows, D, p, hscale, use_extra, regime)
        res.append(t.line(f"layernorm_bwd {name_of(dtype)} D {D} ({RK.ln_bwd_route(dtype, D)}; " + ("exact + rule" if "exact" in regimes else "rule only") + ")"))
    t = Tally()
    keeps_verdict(t, keeps)
    res.append(t.line(f"layernorm_bwd {name_of(dtype)} keep-scales"))
    return res


@case
def layernorm_bwd_fp32():
    """ds and dh on every route: integer / power-of-two inputs bit for bit where D is a power of two, N(0, 1) and offset rows under the rule."""
    return ln_bwd_family(F32)


@case
def layernorm_bwd_bf16():
    return ln_bwd_family(BF16)


@case
def layernorm_bwd_pg():
    """ln_bwd_vec_pg_kernel<1 / 2 / 4>: ds and dh under the rule and bit-equal to ln_bwd_vec_kernel's (same arithmetic, same order), the
    summed partials (colreduce_partials) against the float64 column sums of dy and dy * xhat; shapes the eligibility test must decline."""
    res, keeps = [], new_keeps()
    L = _lib.lib()
    for (rows, D) in RK.LN_PG_SHAPES:
        t = Tally()
        for (p, use_extra) in ((0.0, False), (0.2, True), (0.2, False), (0.0, True)):
            tag = f"ln_bwd_pg {rows}x{D} p {p} extra {int(use_extra)}"
            seed = case_seed("ln_bwd_pg", tag)
            keep = draw(keeps, (rows, D), p, seed)
            inp = RK.ln_bwd_inputs(rows, D, BF16, seed=D + rows, exact=False)
            extra = inp["ds_extra"] if use_extra else None
            dy, s, ex, gamma, mean, rstd = (dev(v) for v in (inp["dy"], inp["s"], extra, inp["gamma"], inp["mean"], inp["rstd"]))
            ds, dh = Buf((rows, D), BF16), Buf((rows, D), BF16)
            chunks = L.s2svc_layernorm_bwd_pg_chunks(K.dt(BF16), rows, D, K.ptr(dy), K.ptr(s), K.ptr(gamma), K.ptr(ex), K.ptr(ds.v), K.ptr(dh.v))
            t.true(tag, chunks == RK.pg_eligible(BF16, rows, D) and chunks > 0, f"eligibility: {chunks} chunks, the restated test says {RK.pg_eligible(BF16, rows, D)}")
            if chunks <= 0:
                continue
            ws = Buf((chunks, 2, D), F32)
            ccall("layernorm_bwd_pg", L.s2svc_layernorm_bwd_pg(K.dt(BF16), rows, D, K.ptr(dy), K.ptr(s), K.ptr(mean), K.ptr(rstd), K.ptr(gamma), K.ptr(ex), p, 0.5,
                                                               seed[0], seed[1], K.ptr(ds.v), K.ptr(dh.v), K.ptr(ws.v), K.stream()))
            args = (inp["dy"], inp["s"], inp["mean"], inp["rstd"], inp["gamma"], extra, keep, 0.5)
            ref, yard = RK.ln_bwd(*args, F64, store=BF16), RK.ln_bwd(*args, F32, store=BF16)
            t.close(f"{tag} ds", ds.v, ref[0], yard[0], BF16)
            t.close(f"{tag} dh", dh.v, ref[1], yard[1], BF16)
            if keep is not None:
                t.zero_bits(tag, dh.v, keep == 0, "dropped elements of dh")
            osum, odot = Buf((D,), F32, src=torch.zeros(D)), Buf((D,), F32, src=torch.zeros(D))
            K.colreduce_partials(ws.v.reshape(-1), chunks, D, osum.v, odot.v)
            t.close(f"{tag} sum dy", osum.v, ref[2], yard[2], F32)
            t.close(f"{tag} sum dy xhat", odot.v, ref[3], yard[3], F32)
            t.true(tag, ds.rest_ok() and dh.rest_ok() and ws.rest_ok() and osum.rest_ok() and odot.rest_ok(), "wrote outside an output")
            # route equality: the plain 16-byte backward kernel on the same tensors
            ds2, dh2 = Buf((rows, D), BF16), Buf((rows, D), BF16)
            ln_bwd_launch(BF16, rows, D, dy, s, mean, rstd, gamma, ex, p, 0.5, seed, ds2.v, dh2.v)
            t.bits(f"{tag} ds = ln_bwd_vec's", ds.v, ds2.v.cpu())
            t.bits(f"{tag} dh = ln_bwd_vec's", dh.v, dh2.v.cpu())
        res.append(t.line(f"layernorm_bwd_pg {rows}x{D} ({RK.ln_bwd_pg_route(D)})"))
    t = Tally()
    for (rows, D) in RK.LN_PG_DECLINED:
        z = torch.zeros(rows * D + 8, dtype=BF16, device=DEV)
        g = torch.zeros(D + 8, dtype=F32, device=DEV)
        chunks = L.s2svc_layernorm_bwd_pg_chunks(K.dt(BF16), rows, D, K.ptr(z), K.ptr(z), K.ptr(g), None, K.ptr(z), K.ptr(z))
        t.true(f"ln_bwd_pg {rows}x{D}", chunks == 0, f"eligible ({chunks} chunks): the source's test declines it")
    z, g = torch.zeros(2931 * 512 + 8, dtype=BF16, device=DEV), torch.zeros(520, dtype=F32, device=DEV)
    t.true("ln_bwd_pg fp32", L.s2svc_layernorm_bwd_pg_chunks(K.dt(F32), 2931, 512, K.ptr(z), K.ptr(z), K.ptr(g), None, K.ptr(z), K.ptr(z)) == 0, "fp32 is eligible")
    t.true("ln_bwd_pg misaligned", L.s2svc_layernorm_bwd_pg_chunks(K.dt(BF16), 2931, 512, K.ptr(z[1:]), K.ptr(z), K.ptr(g), None, K.ptr(z), K.ptr(z)) == 0,
           "a misaligned dy is eligible")
    keeps_verdict(t, keeps)
    res.append(t.line("layernorm_bwd_pg declined shapes, keep-scales"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the ln_act family
# ---------------------------------------------------------------------------------------------------------------------------
def ln_act_one(t, keeps, dtype, D, a, p, rows, with_lens, stats=None):
    m = RK.LN_ACT_LENS
    T, lens = (m["T"], m["lens"]) if with_lens else (0, None)
    tag = f"ln_act {name_of(dtype)} {rows}x{D} {a} p {p} lens {int(with_lens)}"
    seed = case_seed("ln_act", tag)
    keep = draw(keeps, (rows, D), p, seed)
    x, res = R.randn(rows, D, seed=D + rows, dtype=dtype), (R.randn(rows, D, seed=D + rows + 1, dtype=dtype) if with_lens else None)
    gamma, beta = 1.0 + R.randn(D, seed=D + 2, scale=0.2), R.randn(D, seed=D + 3, scale=0.2)
    dy = R.randn(rows, D, seed=D + rows + 4, dtype=dtype)
    xd, rd, gd, bd, dyd, ld = dev(x), dev(res), dev(gamma), dev(beta), dev(dy), i32(lens)
    y, mean, rstd = Buf((rows, D), dtype), Buf((rows,), F32), Buf((rows,), F32)
    L = _lib.lib()
    ccall("ln_act_fwd", L.s2svc_ln_act_fwd(K.dt(dtype), rows, D, T, K.ptr(xd), K.ptr(gd), K.ptr(bd), 1e-5, K.ACT[a], K.ptr(rd), K.ptr(ld), p, seed[0], seed[1],
                                           K.ptr(y.v), K.ptr(mean.v), K.ptr(rstd.v), K.stream()))
    ref, yard = (RK.ln_act_fwd(x, gamma, beta, 1e-5, a, res, lens, T, keep, d, store=dtype) for d in (F64, F32))
    for nm, got, r64, y32, od in zip(("y", "mean", "rstd"), (y.v, mean.v, rstd.v), ref, yard, (dtype, F32, F32)):
        if stats is not None and nm != "y":
            stats.add(nm, got, r64, y32)
        else:
            t.close(f"{tag} {nm}", got, r64, y32, od)
    invalid = ~RK.row_valid(rows, T, lens)
    if with_lens:
        t.zero_bits(tag, y.v, invalid, "values of masked rows of y")
    elif keep is not None:
        t.zero_bits(tag, y.v, keep == 0, "dropped elements of y")
    # backward: mean / rstd are inputs (the float64 statistics rounded to float32)
    mi, ri = ref[1].to(F32), ref[2].to(F32)
    du, dx, dres = Buf((rows, D), dtype), Buf((rows, D), dtype), Buf((rows, D), dtype)
    ccall("ln_act_bwd", L.s2svc_ln_act_bwd(K.dt(dtype), rows, D, T, K.ptr(dyd), K.ptr(xd), H(mi), H(ri), K.ptr(gd), K.ptr(bd), K.ACT[a], K.ptr(ld), p,
                                           seed[0], seed[1], K.ptr(du.v), K.ptr(dx.v), K.ptr(dres.v), K.stream()))
    refb, yardb = (RK.ln_act_bwd(dy, x, mi, ri, gamma, beta, a, lens, T, keep, d, store=dtype) for d in (F64, F32))
    for nm, got, r64, y32 in zip(("du", "dx", "dres"), (du.v, dx.v, dres.v), refb, yardb):
        t.close(f"{tag} {nm}", got, r64, y32, dtype)
        if with_lens:
            t.zero_bits(f"{tag} {nm}", got, invalid, "values of masked rows")
    if keep is not None:
        t.zero_bits(tag, du.v, keep == 0, "dropped elements of du")
    t.true(tag, all(b.rest_ok() for b in (y, mean, rstd, du, dx, dres)), "wrote outside an output")


def ln_act_family(dtype):
    res, keeps = [], new_keeps()
    for D in RK.LN_ACT_D:
        t = Tally()
        for a in RK.LN_ACT_ACTS:
            stats = JointStats()                                       # the one-row launch's statistics, held jointly with the five-row launch's
            for p in (0.0, P_DROP):
                ln_act_one(t, keeps, dtype, D, a, p, 9, True)          # residual, a full, a partial and an empty utterance
                ln_act_one(t, keeps, dtype, D, a, p, 5, False, stats=(stats if p == 0.0 else None))
            ln_act_one(t, keeps, dtype, D, a, 0.0, 1, False, stats=stats)
            stats.close(t, f"ln_act {name_of(dtype)} rows (5, 1) D {D} {a} p 0.0 lens 0")
        routes = sorted({RK.ln_act_route("ln_act_fwd_kernel", dtype, D, a) for a in RK.LN_ACT_ACTS})
        res.append(t.line(f"ln_act fwd + bwd {name_of(dtype)} D {D} ({'; '.join(routes)})"))
    t = Tally()
    z = torch.zeros(1025 * 4 + 8, dtype=dtype, device=DEV)
    g, st = torch.zeros(1032, dtype=F32, device=DEV), torch.zeros(8, dtype=F32, device=DEV)
    L = _lib.lib()
    t.true("ln_act_fwd D 1025", refused(lambda: ccall("ln_act_fwd", L.s2svc_ln_act_fwd(K.dt(dtype), 4, 1025, 0, K.ptr(z), K.ptr(g), K.ptr(g), 1e-5, K.ACT["gelu"], None, None, 0.0,
                                                                                          None, 0, K.ptr(z), K.ptr(st), K.ptr(st), K.stream())), "D <= 1024"), "not refused with the documented error")
    t.true("ln_act_bwd D 1025", refused(lambda: ccall("ln_act_bwd", L.s2svc_ln_act_bwd(K.dt(dtype), 4, 1025, 0, K.ptr(z), K.ptr(z), K.ptr(st), K.ptr(st), K.ptr(g), K.ptr(g), K.ACT["gelu"],
                                                                                          None, 0.0, None, 0, K.ptr(z), K.ptr(z), None, K.stream())), "D <= 1024"), "not refused with the documented error")
    keeps_verdict(t, keeps)
    res.append(t.line(f"ln_act {name_of(dtype)} D 1025 refused, keep-scales"))
    return res


@case
def ln_act_fp32():
    """s2svc_ln_act_fwd / s2svc_ln_act_bwd, every NV / ACT instantiation, p = 0 and 0.5 (what AAS-VC trains the duration predictor with)."""
    return ln_act_family(F32)


@case
def ln_act_bf16():
    return ln_act_family(BF16)


@case
def dw_ln_act():
    """s2svc_dw_ln_act_fwd: u, y, mean and rstd with taps that fall outside on both sides; D = 520 and an even kernel size refused."""
    res = []
    L = _lib.lib()
    B = 2
    for D in RK.DW_D:
        t = Tally()
        for (ks, dil) in RK.DW_KS_DIL:
            for T in RK.DW_T:
                for a in RK.LN_ACT_ACTS:
                    tag = f"dw_ln_act D {D} k {ks} dil {dil} T {T} {a}"
                    x, w, b = R.randn(B, T, D, seed=D + T), R.randn(D, ks, seed=D + ks, scale=0.5), R.randn(D, seed=D + 1, scale=0.2)
                    gamma, beta = 1.0 + R.randn(D, seed=D + 2, scale=0.2), R.randn(D, seed=D + 3, scale=0.2)
                    u, y, mean, rstd = Buf((B, T, D), F32), Buf((B, T, D), F32), Buf((B * T,), F32), Buf((B * T,), F32)
                    ccall("dw_ln_act_fwd", L.s2svc_dw_ln_act_fwd(B, T, D, ks, dil, H(x), H(w), H(b), H(gamma), H(beta), 1e-5, K.ACT[a],
                                                                 K.ptr(u.v), K.ptr(y.v), K.ptr(mean.v), K.ptr(rstd.v), K.stream()))
                    ref, yard = (RK.dw_ln_act_fwd(x, w, b, ks, dil, gamma, beta, 1e-5, a, d) for d in (F64, F32))
                    for nm, got, r64, y32 in zip(("u", "y", "mean", "rstd"), (u.v, y.v, mean.v, rstd.v), ref, yard):
                        t.close(f"{tag} {nm}", got, r64, y32, F32)
                    t.true(tag, all(o.rest_ok() for o in (u, y, mean, rstd)), "wrote outside an output")
        res.append(t.line(f"dw_ln_act_fwd D {D} ({'; '.join(sorted({RK.dw_ln_act_route(D, a) for a in RK.LN_ACT_ACTS}))})"))
    t = Tally()
    z, st = torch.zeros(2 * 5 * 520, dtype=F32, device=DEV), torch.zeros(16, dtype=F32, device=DEV)
    for (D, ks, what) in ((520, 3, "D = 520"), (256, 4, "an even kernel size")):
        t.true(f"dw_ln_act {what}", refused(lambda: ccall("dw_ln_act_fwd", L.s2svc_dw_ln_act_fwd(2, 5, D, ks, 1, K.ptr(z), K.ptr(z), K.ptr(z), K.ptr(z), K.ptr(z), 1e-5, K.ACT["gelu"],
                                                                                                    K.ptr(z), K.ptr(z), K.ptr(st), K.ptr(st), K.stream())), "D <= 512, odd kernel size"),
               "not refused with the documented error")
    res.append(t.line("dw_ln_act_fwd refusals"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# activation + dropout
# ---------------------------------------------------------------------------------------------------------------------------
def act_fwd_launch(dtype, n, x, a, p, seed, y):
    ccall("act_dropout_fwd", _lib.lib().s2svc_act_dropout_fwd(K.dt(dtype), n, K.ptr(x), K.ACT[a], p, seed[0], seed[1], K.ptr(y), K.stream()))


def act_bwd_launch(dtype, n, dz, saved, a, p, seed, dx):
    ccall("act_dropout_bwd", _lib.lib().s2svc_act_dropout_bwd(K.dt(dtype), n, K.ptr(dz), K.ptr(saved), K.ACT[a], p, seed[0], seed[1], K.ptr(dx), K.stream()))


def act_one(t, keeps, dtype, n, a, p, off=0, x=None, tag_extra=""):
    tag = f"act_dropout {name_of(dtype)} n {n} {a} p {p}{tag_extra}"
    seed = case_seed("act", dtype, n, a, p)
    keep = draw(keeps, (n,), p, seed)
    x = R.randn(n, seed=n + 1, scale=2.0, dtype=dtype) if x is None else x
    dz = R.randn(n, seed=n + 2, dtype=dtype)
    y = Buf((n,), dtype, off)
    act_fwd_launch(dtype, n, dev(x, off), a, p, seed, y.v)
    ref, yard = (RK.act_dropout_fwd(x, a, keep, d, store=dtype) for d in (F64, F32))
    t.close(f"{tag} y", y.v, ref, yard, dtype)
    saved = y.v.cpu() if a in RK.SAVED_IS_OUTPUT else x          # what the kernel itself stored
    dx = Buf((n,), dtype, off)
    act_bwd_launch(dtype, n, dev(dz, off), dev(saved, off), a, p, seed, dx.v)
    refb, yardb = (RK.act_dropout_bwd(dz, saved, a, keep, d, store=dtype) for d in (F64, F32))
    t.close(f"{tag} dx", dx.v, refb, yardb, dtype)
    if keep is not None:
        t.zero_bits(tag, y.v, keep == 0, "dropped elements of y")
        t.zero_bits(tag, dx.v, keep == 0, "dropped elements of dx")
    t.true(tag, y.rest_ok() and dx.rest_ok(), "wrote outside an output")
    return y, dx


@case
def act_dropout():
    """s2svc_act_dropout_fwd / _bwd: every activation, p = 0 and 0.5, fp32, bf16 scalar (n % 8 != 0 or misaligned) and bf16 16-byte;
    n = 2048 * 256 + 11 makes a thread of the capped grid take a second element; the two bf16 routes give the same bits."""
    res, keeps = [], new_keeps()
    for dtype in (F32, BF16):
        t = Tally()
        for n in RK.EW_N + (4096,):
            for a in RK.ACTS:
                for p in (0.0, P_DROP):
                    y, dx = act_one(t, keeps, dtype, n, a, p)
                    if dtype == BF16 and n % 8 == 0:             # route equality: the same data behind a pointer one element off
                        y1, dx1 = act_one(t, keeps, dtype, n, a, p, off=1, tag_extra=" scalar route")
                        t.bits(f"act_dropout bf16 n {n} {a} p {p} y: 16-byte route = scalar route", y.v, y1.v.cpu())
                        t.bits(f"act_dropout bf16 n {n} {a} p {p} dx: 16-byte route = scalar route", dx.v, dx1.v.cpu())
        act_one(t, keeps, dtype, RK.EW_BIG, "swish", P_DROP)
        if dtype == BF16:
            act_one(t, keeps, dtype, RK.EW_BIG + 5, "tanh", P_DROP)          # n % 8 == 0: the 16-byte route at the same size
        keeps_verdict(t, keeps)
        res.append(t.line(f"act_dropout fwd + bwd {name_of(dtype)}"))
    return res


@case
def act_tails():
    """|x| up to 1e4 in a tensor of their own: under the rule, finite, of the right sign, and for |x| >= 88 what DESIGN.md promises (swish:
    a signed zero or x; sigmoid: 0 or 1).  The backward kernels on the same values (as pre-activations, or as the outputs act() gives)."""
    res = []
    for dtype in (F32, BF16):
        t = Tally()
        for n_pad in (1, 6):                                     # 19 values: scalar route; 24: the 16-byte route (bf16)
            x = RK.tails(dtype, n_pad)
            n = x.numel()
            for a in RK.ACTS:
                tag = f"tails {name_of(dtype)} n {n} {a}"
                y = Buf((n,), dtype)
                act_fwd_launch(dtype, n, dev(x), a, 0.0, (None, 0), y.v)
                ref, yard = (RK.act_dropout_fwd(x, a, None, d, store=dtype) for d in (F64, F32))
                t.close(f"{tag} y", y.v, ref, yard, dtype)
                got, xf = y.v.cpu().to(F64), x.to(F64)
                t.true(tag, bool(torch.isfinite(got).all()), "a NaN or inf in y")
                t.true(tag, bool((got * ref >= 0).all()), "y has the wrong sign")
                far = xf.abs() >= RK.GUARANTEE_FROM
                if a == "swish":
                    t.true(tag, bool(((got[far] == 0) | (got[far] == xf[far])).all()), "swish of |x| >= 88 is neither a zero nor x")
                    t.true(tag, bool((got[far & (xf < 0)] == 0).all()) and bool((got[far & (xf > 0)] == xf[far & (xf > 0)]).all()), "swish of |x| >= 88: zero and x swapped")
                if a == "sigmoid":
                    t.true(tag, bool((got[far & (xf < 0)] == 0).all()) and bool((got[far & (xf > 0)] == 1).all()), "sigmoid of |x| >= 88 is not 0 / 1")
                saved = y.v.cpu() if a in RK.SAVED_IS_OUTPUT else x
                dz = torch.ones(n, dtype=dtype)
                dx = Buf((n,), dtype)
                act_bwd_launch(dtype, n, dev(dz), dev(saved), a, 0.0, (None, 0), dx.v)
                refb, yardb = (RK.act_dropout_bwd(dz, saved, a, None, d, store=dtype) for d in (F64, F32))
                t.close(f"{tag} dx", dx.v, refb, yardb, dtype)
                gdx = dx.v.cpu().to(F64)
                t.true(tag, bool(torch.isfinite(gdx).all()), "a NaN or inf in dx")
                # |x| >= 88 (dz = 1): 1 for None; 1 / 0 right / left for relu, swish and gelu; 0 for tanh and sigmoid (saturated outputs)
                up = torch.ones_like(xf) if a is None else torch.zeros_like(xf) if a in ("tanh", "sigmoid") else (xf > 0).to(F64)
                t.true(tag, bool((gdx[far] == up[far]).all()), "dx of |x| >= 88 is not the saturated derivative (0 or 1)")
                t.true(tag, y.rest_ok() and dx.rest_ok(), "wrote outside an output")
        res.append(t.line(f"activation tails {name_of(dtype)}"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# positional encoding, GLU
# ---------------------------------------------------------------------------------------------------------------------------
@case
def posenc():
    """s2svc_posenc_fwd / _bwd: alpha given or not, xscale sqrt(D), pe given or None, p = 0 and 0.5; dalpha a tensor of one element, at the
    second shape summed over more block partials than one pass of sum_partials' wave takes."""
    res, keeps = [], new_keeps()
    L = _lib.lib()
    for dtype in (F32, BF16):
        t = Tally()
        for (B, T, D) in RK.POSENC_SHAPES:
            n = B * T * D
            x, dy = R.randn(B, T, D, seed=n, dtype=dtype), R.randn(B, T, D, seed=n + 1, dtype=dtype)
            pe, alpha = R.randn(T + 2, D, seed=n + 2), torch.tensor([0.7], dtype=F32)
            for (use_alpha, use_pe, xscale, p) in ((True, True, 1.0, P_DROP), (False, True, R.f32(math.sqrt(D)), 0.0), (False, False, R.f32(math.sqrt(D)), P_DROP), (True, True, 1.0, 0.0)):
                tag = f"posenc {name_of(dtype)} {B}x{T}x{D} alpha {int(use_alpha)} pe {int(use_pe)} xscale {xscale:.3f} p {p}"
                seed = case_seed("posenc", tag)
                keep = draw(keeps, (B, T, D), p, seed)
                a_, pe_ = (alpha if use_alpha else None), (pe if use_pe else None)
                y = Buf((B, T, D), dtype)
                ccall("posenc_fwd", L.s2svc_posenc_fwd(K.dt(dtype), B, T, D, H(x), xscale, H(a_), H(pe_), p, seed[0], seed[1], K.ptr(y.v), K.stream()))
                ref, yard = (RK.posenc_fwd(x, xscale, a_, pe_, keep, d, store=dtype) for d in (F64, F32))
                t.close(f"{tag} y", y.v, ref, yard, dtype)
                dx, dalpha, part = Buf((B, T, D), dtype), (Buf((1,), F32) if use_pe else None), Buf((2048,), F32)
                ccall("posenc_bwd", L.s2svc_posenc_bwd(K.dt(dtype), B, T, D, H(dy), xscale, H(pe_), p, seed[0], seed[1], K.ptr(dx.v),
                                                       None if dalpha is None else K.ptr(dalpha.v), K.ptr(part.v), K.stream()))
                refb, yardb = (RK.posenc_bwd(dy, xscale, pe_, keep, d, store=dtype) for d in (F64, F32))
                t.close(f"{tag} dx", dx.v, refb[0], yardb[0], dtype)
                if use_pe:
                    t.close(f"{tag} dalpha", dalpha.v, refb[1], yardb[1], F32)
                if keep is not None:
                    t.zero_bits(tag, y.v, keep == 0, "dropped elements of y")
                    t.zero_bits(tag, dx.v, keep == 0, "dropped elements of dx")
                t.true(tag, y.rest_ok() and dx.rest_ok() and part.rest_ok() and (dalpha is None or dalpha.rest_ok()), "wrote outside an output")
        keeps_verdict(t, keeps)
        res.append(t.line(f"posenc fwd + bwd {name_of(dtype)}"))
    return res


@case
def glu():
    """s2svc_glu_fwd / _bwd on (rows, 2 C) rows, C odd and even, and at a size where the grid-stride loop loops."""
    res = []
    L = _lib.lib()
    for dtype in (F32, BF16):
        t = Tally()
        for (rows, C) in ((1, 1), (7, 1), (5, 8), (9, 455), (1027, 513)):
            x, dy = R.randn(rows, 2 * C, seed=rows + C, scale=2.0, dtype=dtype), R.randn(rows, C, seed=rows + C + 1, dtype=dtype)
            tag = f"glu {name_of(dtype)} {rows}x{C}"
            y, dx = Buf((rows, C), dtype), Buf((rows, 2 * C), dtype)
            ccall("glu_fwd", L.s2svc_glu_fwd(K.dt(dtype), rows, C, H(x), K.ptr(y.v), K.stream()))
            ccall("glu_bwd", L.s2svc_glu_bwd(K.dt(dtype), rows, C, H(x), H(dy), K.ptr(dx.v), K.stream()))
            ref, yard = (RK.glu_fwd(x, d, store=dtype) for d in (F64, F32))
            t.close(f"{tag} y", y.v, ref, yard, dtype)
            refb, yardb = (RK.glu_bwd(x, dy, d, store=dtype) for d in (F64, F32))
            t.close(f"{tag} dx", dx.v, refb, yardb, dtype)
            t.true(tag, y.rest_ok() and dx.rest_ok(), "wrote outside an output")
        res.append(t.line(f"glu fwd + bwd {name_of(dtype)}"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm, element-wise part (the statistics are inputs)
# ---------------------------------------------------------------------------------------------------------------------------
def bn_params(C, seed):
    return (R.randn(C, seed=seed, scale=0.3), R.randn(C, seed=seed + 1, scale=0.2).abs() + 0.8, 1.0 + R.randn(C, seed=seed + 2, scale=0.2), R.randn(C, seed=seed + 3, scale=0.2))


def bn_apply_one(t, keeps, tag, dtype, rows, C, a, p, vec, vlens=None, Tn=0):
    seed = case_seed("bn_apply", tag)
    keep = draw(keeps, (rows, C), p, seed)
    x = R.randn(rows, C, seed=rows + C, dtype=dtype)
    mean, rstd, gamma, beta = bn_params(C, rows + C + 1)
    y, pre = Buf((rows, C), dtype), Buf((rows, C), dtype)
    L = _lib.lib()
    ptrs = [H(v) for v in (x, mean, rstd, gamma, beta)]
    vl = i32(vlens)
    if vec:
        ccall("bn_act_apply_vec", L.s2svc_bn_act_apply_vec(rows, C, *ptrs, K.ACT[a], p, seed[0], seed[1], K.ptr(y.v), K.ptr(pre.v), Tn, K.ptr(vl), K.stream()))
    else:
        ccall("bn_apply", L.s2svc_bn_apply(K.dt(dtype), rows, C, *ptrs, K.ACT[a], p, seed[0], seed[1], K.ptr(y.v), K.ptr(pre.v), Tn, K.ptr(vl), K.stream()))
    ref, yard = (RK.bn_apply(x, mean, rstd, gamma, beta, a, keep, vlens, Tn, d, store=dtype) for d in (F64, F32))
    t.close(f"{tag} y", y.v, ref[0], yard[0], dtype)
    t.close(f"{tag} pre", pre.v, ref[1], yard[1], dtype)
    if vlens is not None:
        absent = ~RK.present(rows, Tn, vlens)
        t.zero_bits(tag, y.v, absent, "values of absent rows of y")
        t.zero_bits(tag, pre.v, absent, "values of absent rows of pre")
    if keep is not None:
        t.zero_bits(tag, y.v, keep == 0, "dropped elements of y")
    t.true(tag, y.rest_ok() and pre.rest_ok(), "wrote outside an output")


@case
def batchnorm_apply():
    """s2svc_bn_apply (y and pre, fp32 / bf16) and s2svc_bn_act_apply_vec: every activation, p = 0 and 0.5, vlens = (21, 0, 7) of 21."""
    res, keeps = [], new_keeps()
    m = RK.MASKED
    for dtype in (F32, BF16):
        t = Tally()
        for (rows, C) in RK.BN_SCALAR_SHAPES:
            for a in RK.ACTS:
                for p in (0.0, P_DROP):
                    bn_apply_one(t, keeps, f"bn_apply {name_of(dtype)} {rows}x{C} {a} p {p}", dtype, rows, C, a, p, False)
        for a in (None, "tanh", "swish"):
            bn_apply_one(t, keeps, f"bn_apply {name_of(dtype)} masked C 72 {a}", dtype, m["B"] * m["Tn"], 72, a, P_DROP, False, m["vlens"], m["Tn"])
        keeps_verdict(t, keeps)
        res.append(t.line(f"bn_apply {name_of(dtype)}"))
    t = Tally()
    for C in RK.BN_VEC_C:
        for rows in RK.BN_VEC_ROWS + (257,):
            for a in RK.ACTS:
                for p in (0.0, P_DROP):
                    bn_apply_one(t, keeps, f"bn_act_apply_vec {rows}x{C} {a} p {p}", BF16, rows, C, a, p, True)
    for a in (None, "tanh", "swish"):
        bn_apply_one(t, keeps, f"bn_act_apply_vec masked C 72 {a}", BF16, m["B"] * m["Tn"], 72, a, P_DROP, True, m["vlens"], m["Tn"])
    keeps_verdict(t, keeps)
    res.append(t.line("bn_act_apply_vec"))
    return res


@case
def batchnorm_bwd():
    """s2svc_bn_bwd in training and eval mode (exact on integer / power-of-two inputs with N a power of two, rule on N(0, 1), masked) and dx
    of s2svc_bn_act_bwd_vec (every activation, p = 0 and 0.5, masked)."""
    res, keeps = [], new_keeps()
    L = _lib.lib()
    m = RK.MASKED

    def launch(dtype, rows, C, inp, training, dx, vlens=None, Tn=0):
        ptrs = [H(inp[k]) for k in ("g", "x", "mean", "rstd", "gamma", "sdy", "sdyx")]
        ccall("bn_bwd", L.s2svc_bn_bwd(K.dt(dtype), rows, C, *ptrs, 1 if training else 0, K.ptr(dx.v), Tn, H(i32(vlens)), K.stream()))

    for dtype in (F32, BF16):
        t = Tally()
        for (rows, C) in ((1, 8), (64, 72), (256, 136)):                   # exact: N a power of two
            inp = RK.bn_bwd_exact_inputs(rows, C, dtype, seed=rows + C)
            for training in (True, False):
                tag = f"bn_bwd exact {name_of(dtype)} {rows}x{C} training {int(training)}"
                a = (inp["g"], inp["x"], inp["mean"], inp["rstd"], inp["gamma"], inp["sdy"], inp["sdyx"], training, None, 0)
                want, raw = RK.bn_bwd(*a, F64), RK.bn_bwd(*a, F32)
                t.true(tag, bool((raw.to(F64) == want).all()), "exact premise broken")
                dx = Buf((rows, C), dtype)
                launch(dtype, rows, C, inp, training, dx)
                t.bits(f"{tag} dx", dx.v, want)
                t.true(tag, dx.rest_ok(), "wrote outside dx")
        for (rows, C, vlens, Tn) in [(r, c, None, 0) for r, c in RK.BN_SCALAR_SHAPES] + [(m["B"] * m["Tn"], 72, m["vlens"], m["Tn"])]:
            g, x = R.randn(rows, C, seed=rows + C + 7, dtype=dtype), R.randn(rows, C, seed=rows + C + 8, dtype=dtype)
            mean, rstd, gamma, _ = bn_params(C, rows + C + 9)
            ok = RK.present(rows, Tn, vlens)
            xh = (x.to(F64) - mean.to(F64)) * rstd.to(F64)
            inp = dict(g=g, x=x, mean=mean, rstd=rstd, gamma=gamma, sdy=g.to(F64)[ok].sum(0).to(F32), sdyx=(g.to(F64) * xh)[ok].sum(0).to(F32))
            for training in (True, False):
                tag = f"bn_bwd rule {name_of(dtype)} {rows}x{C} training {int(training)}" + (" masked" if vlens else "")
                a = (g, x, mean, rstd, gamma, inp["sdy"], inp["sdyx"], training, vlens, Tn)
                dx = Buf((rows, C), dtype)
                launch(dtype, rows, C, inp, training, dx, vlens, Tn)
                t.close(f"{tag} dx", dx.v, RK.bn_bwd(*a, F64, store=dtype), RK.bn_bwd(*a, F32, store=dtype), dtype)
                if vlens is not None:
                    t.zero_bits(tag, dx.v, ~ok, "values of absent rows of dx")
                t.true(tag, dx.rest_ok(), "wrote outside dx")
        res.append(t.line(f"bn_bwd {name_of(dtype)}"))
    t = Tally()
    shapes = [(rows, C, None, 0) for C in RK.BN_VEC_C for rows in RK.BN_VEC_ROWS] + [(m["B"] * m["Tn"], 72, m["vlens"], m["Tn"])]
    for (rows, C, vlens, Tn) in shapes:
        for a in RK.ACTS:
            for p in (0.0, P_DROP):
                tag = f"bn_act_bwd_vec {rows}x{C} {a} p {p}" + (" masked" if vlens else "")
                seed = case_seed("bn_act_bwd", tag)
                keep = draw(keeps, (rows, C), p, seed)
                dz, x = R.randn(rows, C, seed=rows + C + 11, dtype=BF16), R.randn(rows, C, seed=rows + C + 12, dtype=BF16)
                mean, rstd, gamma, beta = bn_params(C, rows + C + 13)
                ok = RK.present(rows, Tn, vlens)
                yf, pre = RK.bn_apply(x, mean, rstd, gamma, beta, a, keep, vlens, Tn, F32, store=BF16)
                saved = (yf if a in RK.SAVED_IS_OUTPUT else pre).to(BF16)
                dx, sdy, sdyx = Buf((rows, C), BF16), Buf((C,), F32), Buf((C,), F32)
                ws = Buf((((rows + 63) // 64) * 2 * C,), F32)
                ccall("bn_act_bwd_vec", L.s2svc_bn_act_bwd_vec(rows, C, H(dz), H(saved), H(x), H(mean), H(rstd), H(gamma),
                                                               K.ACT[a], p, seed[0], seed[1], K.ptr(dx.v), K.ptr(sdy.v), K.ptr(sdyx.v), None, None, K.ptr(ws.v), Tn, H(i32(vlens)),
                                                               K.stream()))
                ref, yard = [], []
                for d, out in ((F64, ref), (F32, yard)):
                    gg = RK.act_dropout_bwd(dz, saved, a, keep, d)
                    xh = (x.to(d) - mean.to(d)) * rstd.to(d)
                    out.append(RK.bn_bwd(gg, x, mean, rstd, gamma, gg[ok].sum(0), (gg * xh)[ok].sum(0), True, vlens, Tn, d, store=BF16))
                t.close(f"{tag} dx", dx.v, ref[0], yard[0], BF16)       # (one row: sdy = g, dx = -gamma rstd xhat^2 g)
                if vlens is not None:
                    t.zero_bits(tag, dx.v, ~ok, "values of absent rows of dx")
                t.true(tag, dx.rest_ok() and sdy.rest_ok() and sdyx.rest_ok() and ws.rest_ok(), "wrote outside an output")
    keeps_verdict(t, keeps)
    res.append(t.line("bn_act_bwd_vec dx"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# pure adds and copies: the float32 restatement of the documented order, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@case
def small_launchers():
    """s2svc_add_n (k = 2, 3, 4; scalar and 16-byte route, and both give the same bits), s2svc_axpby, s2svc_add_head_bias, s2svc_add_head_bias_ld,
    s2svc_add_rows (lda, ldb, ldo > D, NaN in the slack) and s2svc_cast in both directions."""
    res = []
    L = _lib.lib()
    for dtype in (F32, BF16):
        t = Tally()
        for n in RK.EW_N + (4096, RK.EW_BIG):
            xs = [R.randn(n, seed=n + i, dtype=dtype) for i in range(4)]
            for k in (2, 3, 4):
                outs = []
                for off in ((0, 1) if (dtype == BF16 and n % 8 == 0) else (0,)):
                    out = Buf((n,), dtype, off)
                    p = [H(v, off) for v in xs[:k]] + [None] * (4 - k)
                    ccall("add_n", L.s2svc_add_n(K.dt(dtype), n, k, p[0], p[1], p[2], p[3], K.ptr(out.v), K.stream()))
                    t.bits(f"add_n {name_of(dtype)} n {n} k {k} off {off}", out.v, RK.add_n(xs[:k], dtype))
                    t.true(f"add_n n {n} k {k}", out.rest_ok(), "wrote outside the output")
                    outs.append(out)
                if len(outs) == 2:
                    t.bits(f"add_n bf16 n {n} k {k}: 16-byte route = scalar route", outs[0].v, outs[1].v.cpu())
            for (a, b, use_y) in ((0.5, -2.0, True), (-4.0, 0.0, False)):
                out = Buf((n,), dtype)
                ccall("axpby", L.s2svc_axpby(K.dt(dtype), n, a, H(xs[0]), b, H(xs[1]) if use_y else None, K.ptr(out.v), K.stream()))
                t.bits(f"axpby {name_of(dtype)} n {n} a {a} b {b}", out.v, RK.axpby(a, xs[0], b, xs[1] if use_y else None, dtype))
                t.true(f"axpby n {n}", out.rest_ok(), "wrote outside the output")
            other = BF16 if dtype == F32 else F32
            out = Buf((n,), other)
            ccall("cast", L.s2svc_cast(K.dt(dtype), K.dt(other), n, H(xs[2]), K.ptr(out.v), K.stream()))
            t.bits(f"cast {name_of(dtype)} -> {name_of(other)} n {n}", out.v, xs[2].to(other))
            t.true(f"cast n {n}", out.rest_ok(), "wrote outside the output")
        for (rows, D, ld) in ((1, 1, 3), (7, 50, 58), (65, 72, 72), (2051, 257, 300)):
            q, b2 = R.randn(rows, D, seed=rows + D, dtype=dtype), R.randn(rows, D, seed=rows + D + 1, dtype=dtype)
            u, v = R.randn(D, seed=D + 2), R.randn(D, seed=D + 3)
            want = RK.add_head_bias(q, u, v, dtype)
            for ldq in (None, ld):
                qu, qv = Buf((rows, D), dtype), Buf((rows, D), dtype)
                if ldq is None:
                    ccall("add_head_bias", L.s2svc_add_head_bias(K.dt(dtype), rows, D, H(q), H(u), H(v), K.ptr(qu.v), K.ptr(qv.v), K.stream()))
                else:
                    ccall("add_head_bias_ld", L.s2svc_add_head_bias_ld(K.dt(dtype), rows, D, H(strided(q, ldq)), ldq, H(u), H(v), K.ptr(qu.v), K.ptr(qv.v), K.stream()))
                tag = f"add_head_bias{'_ld' if ldq else ''} {name_of(dtype)} {rows}x{D}"
                t.bits(f"{tag} qu", qu.v, want[0])
                t.bits(f"{tag} qv", qv.v, want[1])
                t.true(tag, qu.rest_ok() and qv.rest_ok(), "wrote outside an output")
            out = torch.full((rows, ld + 2), SENT, dtype=dtype, device=DEV)
            ccall("add_rows", L.s2svc_add_rows(K.dt(dtype), rows, D, H(strided(q, ld)), ld, H(strided(b2, ld + 1)), ld + 1, K.ptr(out), ld + 2, K.stream()))
            t.bits(f"add_rows {name_of(dtype)} {rows}x{D}", out[:, :D], RK.add_n([q, b2], dtype))
            t.true(f"add_rows {rows}x{D}", bool((out[:, D:] == SENT).all()), "wrote into the slack of the output rows")
        res.append(t.line(f"add_n, axpby, cast, add_head_bias(_ld), add_rows {name_of(dtype)}"))
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
    if "--dump" in sys.argv:
        torch.save(DUMP, sys.argv[sys.argv.index("--dump") + 1])
        print(f"== dumped {len(DUMP)} tensors")
    return nfail


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
