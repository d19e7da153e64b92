"""Kernel-level, element-wise parity of the fused attention backward that carries the out-projection's data gradient in its prologue
(csrc/attn_fused.hip: attn_proj_bwd_kernel, launcher s2svc_attn_proj_bwd).  Runs on the MI355X:
  * `python tests/gpu_attn_proj_kernel_check.py [--only a,b]` prints a PASS/FAIL table for all cases and never stops early;
  * tests/test_gpu_attn_proj_kernels.py imports CASES and turns each into a `@pytest.mark.gpu` test.

Rule 1, the rule of tests/gpu_attn_kernel_check.py: per (utterance, head) slice of dq / dk / dv, ref64 = the float64 restatement of
tests/attn_proj_ref.py on exactly the values the kernel reads (dY, W_o, q, k, v, bf16(ref64 map) from the CPU, the keep-scales the
kernels' mask function gives for the seed), yard = the same in float32 on the CPU with the roundings the kernel documents, pass when
|got - ref64| <= 4 d + ulp with d = max |yard - ref64| over the slice.
Rule 2, a condition: dq / dk / dv are bit for bit what the separate launches give on the same inputs and seed -- K.gemm on the route
the out-projection's data gradient takes (dY as A operand, W_o^T as K-contiguous B operand), then KAT.fused_bwd on its output.  One
route is exempt, by its code and not by its results: with B T1 <= 64 rows the GEMM runs gemm_skinny_kernel, whose four wavefronts sum a
quarter of K each and add the quarters through LDS -- for D > 64 (more than one 32-step per quarter) that is another order of the fp32
additions than the one accumulator over ascending 32-steps of the tile kernels and of the prologue here, so Rule 1 alone holds such a
case and its line says how many outputs agreed all the same (the models do not take the fold there: ops/functional.py).
Exact conditions: every output is a column block of a sentinel-filled packed buffer with one more row per utterance and 8 more columns
than the gradients fill (self-attention: the packed (B, T, 3D) gradient written in place; source attention: dk | dv as block 1 of a
(B, T2, 3 * 2D) gradient, the kv block read from the same place of its tensor), whose remainder comes back unchanged.  The only calls
expected to fail are ones the launcher's host-side argument check refuses before any launch."""
import os
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_kernels_ref as A  # noqa: E402
import attn_proj_ref as P  # noqa: E402
import gpu_attn_kernel_check as G  # noqa: E402  (Keep, OutView, padded, case_seed, refused: the idiom of the attention check)
import step_kernels_ref as R  # noqa: E402
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402
from seq2seq_vc_amd.ops import kernels_attn as KAT  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = G.SENT
CASES = []
# Checks whose kernel is correct and yet takes more than 4 d: 1.5 x the measured margin, with the cause (profiles/AB_LOG.md has the runs).
MEASURED_MARGINS = {}


def case(fn):
    CASES.append(fn)
    return fn


class Tally(G.Tally):
    def __init__(self, key=None):
        super().__init__()
        self.margin = MEASURED_MARGINS.get(key, R.MARGIN)


def proj_bwd_launch(H, q, k, v, dy, ldy, ybs, wot, ldw, attn, dattn, ld, scale, p, seed, dq, dkk, dv, T1=None, dk=None):
    """The launcher itself, every argument as given (the refusal checks pass ones the wrapper would not)."""
    B, T, D = q.shape
    G.ccall("attn_proj_bwd", _lib.lib().s2svc_attn_proj_bwd(
        B, H, T if T1 is None else T1, k.shape[1], D // H if dk is None else dk, K.ptr(q), q.stride(1), q.stride(0), K.ptr(k), k.stride(1),
        k.stride(0), K.ptr(v), v.stride(1), v.stride(0), dy if isinstance(dy, int) else K.ptr(dy), ldy, ybs, wot if isinstance(wot, int) else K.ptr(wot),
        ldw, K.ptr(attn), K.ptr(dattn), ld, scale, p, seed[0], seed[1], K.ptr(dq), dq.stride(1), dq.stride(0), K.ptr(dkk), dkk.stride(1),
        dkk.stride(0), K.ptr(dv), dv.stride(1), dv.stride(0), K.stream()))


class Layout:
    """The operands and gradient buffers of one case as the models lay them out (see the module comment)."""

    def __init__(self, kind, inp, T1, T2, D):
        B = P.B_
        self.kind, self.D, self.T1, self.T2 = kind, D, T1, T2
        if kind == "self":
            buf = G.sent((B, T1 + 1, 3 * D + 8), BF16)
            for i, n in enumerate(("q", "k", "v")):
                buf[:, :T1, i * D:(i + 1) * D].copy_(inp[n])
            self.q, self.k, self.v = (buf[:, :T1, i * D:(i + 1) * D] for i in range(3))
        else:
            self.q = inp["q"].to(DEV)
            buf = G.sent((B, T2 + 1, 3 * 2 * D), BF16)
            buf[:, :T2, 2 * D:3 * D].copy_(inp["k"])
            buf[:, :T2, 3 * D:4 * D].copy_(inp["v"])
            self.k, self.v = buf[:, :T2, 2 * D:3 * D], buf[:, :T2, 3 * D:4 * D]
        self.src = buf

    def grads(self):
        """-> (dq, dk, dv views, check): check() is True when nothing but the three blocks was written."""
        B, D, T1, T2 = P.B_, self.D, self.T1, self.T2
        if self.kind == "self":
            g = G.sent((B, T1 + 1, 3 * D + 8), BF16)
            outs = tuple(g[:, :T1, i * D:(i + 1) * D] for i in range(3))

            def check():
                c = g.clone()
                c[:, :T1, :3 * D] = SENT
                return bool((c == SENT).all())
            return outs + (check,)
        gq, g = G.sent((B, T1 + 1, D + 8), BF16), G.sent((B, T2 + 1, 3 * 2 * D), BF16)

        def check():
            c, cq = g.clone(), gq.clone()
            c[:, :T2, 2 * D:4 * D] = SENT
            cq[:, :T1, :D] = SENT
            return bool((c == SENT).all()) and bool((cq == SENT).all())
        return gq[:, :T1, :D], g[:, :T2, 2 * D:3 * D], g[:, :T2, 3 * D:4 * D], check


def separate_launches(lay, dy, wot, pm_d, dattn_d, H, scale, p, seed):
    """dq, dk, dv of today's two launches: the out-projection's data-gradient GEMM as _Linear.backward issues it, then the fused backward."""
    B, T1, D = dy.shape
    dctx = torch.empty((B * T1, D), dtype=BF16, device=DEV)
    K.gemm(K.operand(dy.view(B * T1, D), D), K.operand(wot, D), B * T1, D, D, dctx, in_dtype=BF16)
    last_route = _lib.lib().s2svc_gemm_last_route              # (a name query, no kernel)
    route = last_route().decode()
    dq, dkk, dv, _ = lay.grads()
    KAT.fused_bwd(lay.q, lay.k, lay.v, dctx.view(B, T1, D), pm_d, dattn_d, H, scale, p, seed, dq, dkk, dv)
    return dq, dkk, dv, route


def _case(c):
    D, H, dk, kind, T1, T2, causal = c
    B = P.B_
    inp = P.inputs(c)
    scale, ld = inp["scale"], A.round8(T2)
    lay = Layout(kind, inp, T1, T2, D)
    dy = inp["dy"].to(DEV)
    wot = inp["w_o"].t().contiguous().to(DEV)                # the optimiser's transposed shadow: W_o^T (D_in, D_out)
    assert KAT.proj_bwd_ok(lay.q, lay.k, lay.v, dy, wot, H), c
    pm = A.stored_map(inp)
    pm_d = G.padded(pm, ld)
    t, keeps, skinny = Tally("attn_proj_bwd"), G.Keep(), [0, 0]
    for p in (0.0, P.P_DROP):
        seed = G.case_seed("proj_bwd", c, p)
        keep = A.keep_of(keeps.draw((B, H, T1, ld), p, seed), T2) if p else None
        for use_dattn in (False, True):
            where = f"p {p}, dattn {use_dattn}"
            dattn = inp["dattn"] if use_dattn else None
            dattn_d = G.padded(dattn, ld) if use_dattn else None
            a = (pm, inp["dy"], inp["w_o"], inp["v"], inp["k"], inp["q"], scale, H)
            r64, y32 = P.proj_bwd(*a, F64, dattn=dattn, keep=keep), P.proj_bwd(*a, F32, dattn=dattn, keep=keep, bf16=True)
            dq, dkk, dv, untouched = lay.grads()
            KAT.proj_bwd(lay.q, lay.k, lay.v, dy, wot, pm_d, dattn_d, H, scale, p, seed, dq, dkk, dv)
            sep = separate_launches(lay, dy, wot, pm_d, dattn_d, H, scale, p, seed)
            for nm, o, i, s in (("dq", dq, 1, sep[0]), ("dk", dkk, 2, sep[1]), ("dv", dv, 3, sep[2])):
                got = o.detach().cpu()
                for ((b, h), g_), (_, r_), (_, y_) in zip(A.slices(got, H), A.slices(r64[i], H), A.slices(y32[i], H)):
                    t.close(f"{where} {nm} [b {b}, h {h}]", g_, r_, y_, BF16)
                same = G.same_bits(o, s)
                if sep[3].startswith("skinny") and D > 64:
                    skinny[0], skinny[1] = skinny[0] + int(same), skinny[1] + 1
                else:
                    t.exact(f"{where} {nm}", same, f"differs from the separate launches (data-gradient GEMM on {sep[3]}, then attn_fused_bwd)")
            t.exact(where, untouched(), "wrote outside the gradient blocks or behind their last row")
    tag = f"D {D}, H {H}, dk {dk}, {kind} T {T1} x {T2}{', causal' if causal else ''}"
    extra = f" (keep-scales: {keeps.kept} of {keeps.total} kept)" if keeps.total else ""
    if skinny[1]:
        extra += f"; the separate GEMM ran the skinny kernel (K in four quarters): {skinny[0]} of {skinny[1]} outputs agree bit for bit, not required"
    return [t.line(f"attn_proj_bwd {tag}", extra)]


def _named(i, c):
    def run():
        return _case(c)
    D, H, dk, kind, T1, T2, causal = c
    run.__name__ = f"attn_proj_bwd_D{D}_dk{dk}_{kind}_{T1}x{T2}{'_causal' if causal else ''}"
    return run


for _i, _c in enumerate(P.CASES):
    case(_named(_i, _c))


def _block_run(kind, mode, inp, D, H, T1, T2, causal, p):
    """Outputs and gradients of one attention block on the wiring `mode`: "nodes" = Fn.linear -> Fn.attention_packed_* -> Fn.linear (the
    separate autograd nodes), "block" = the one-node block, "block_off" = the one-node block with the switch S2SVC_NO_ATTN_PROJ=bwd."""
    from seq2seq_vc_amd.ops import functional as Fn
    from seq2seq_vc_amd.ops import functional_attn as FAttn
    n_in = 3 * D if kind == "self" else D
    x = inp["dy"].to(DEV).clone().requires_grad_(True)                                   # (B, T1, D) bf16 of unit scale
    w_in = R.randn(n_in, D, seed=901, scale=D ** -0.5).to(DEV).requires_grad_(True)
    b_in = R.randn(n_in, seed=902, scale=0.1).to(DEV).requires_grad_(True)
    w_o = inp["w_o"].to(F32).to(DEV).requires_grad_(True)
    b_o = R.randn(D, seed=903, scale=0.1).to(DEV).requires_grad_(True)
    w_o._s2s_bf16_t = w_o.detach().t().contiguous().to(BF16)                             # what FlatAdam keeps beside the weight
    mem = torch.cat([inp["k"], inp["v"]], dim=-1).to(DEV).requires_grad_(True) if kind == "source" else None
    klen = G.i32(inp["klen"])
    K.reset_op_counter()                                                                 # the same dropout seed on every wiring
    off = KAT._PROJ_OFF
    KAT._PROJ_OFF = {"bwd"} if mode == "block_off" else set()
    try:
        if mode == "nodes":
            h, xp = Fn.linear(x, w_in, b_in, passthrough=True)
            cv, attn = (FAttn.attention_packed_qkv(h, klen, causal, H, p) if kind == "self" else FAttn.attention_packed_kv(h, mem, klen, causal, H, p))
            y = Fn.linear(cv, w_o, b_o)
        else:
            assert FAttn.attn_block_ok(x, T2, mem, H, w_o) == (mode == "block")
            y, attn, xp = (FAttn.attention_block_qkv(x, w_in, b_in, w_o, b_o, klen, causal, H, p, True) if kind == "self" else
                           FAttn.attention_block_kv(x, w_in, b_in, mem, w_o, b_o, klen, causal, H, p, True))
        gy, gx = R.randn(*y.shape, seed=904, dtype=BF16).to(DEV), R.randn(*x.shape, seed=905, dtype=BF16).to(DEV)
        ((y.float() * gy.float()).sum() + (attn.float() * inp["dattn"].to(DEV).float()).sum() + (xp.float() * gx.float()).sum()).backward()
    finally:
        KAT._PROJ_OFF = off
    outs = dict(y=y.detach(), attn=attn.detach().contiguous(), dx=x.grad, dw_in=w_in.grad, db_in=b_in.grad, dw_o=w_o.grad, db_o=b_o.grad)
    if mem is not None:
        outs["dkv"] = mem.grad
    return outs


@case
def attn_block_wiring():
    """The one-node attention blocks of ops/functional.py (projection + fused core + out-projection; their backward hands dY to
    attn_proj_bwd) give, bit for bit, the outputs and every gradient of the separate autograd nodes -- with the fold, and with the switch
    S2SVC_NO_ATTN_PROJ=bwd that sends the block's backward through the separate data-gradient GEMM; p = 0.3, the map gradient and the
    pass-through residual gradient present."""
    res = []
    for c in (P.CASES[2], P.CASES[4]):
        D, H, dk, kind, T1, T2, causal = c
        inp = P.inputs(c)
        ref = _block_run(kind, "nodes", inp, D, H, T1, T2, causal, P.P_DROP)
        for mode in ("block", "block_off"):
            got = _block_run(kind, mode, inp, D, H, T1, T2, causal, P.P_DROP)
            bad = [n for n in ref if got[n] is None or not G.same_bits(got[n], ref[n])]
            res.append((not bad, f"attention block ({kind} T {T1} x {T2}, D {D}) as {mode}: {len(ref)} outputs and gradients equal the separate nodes'"
                        + (f" EXCEPT {bad}" if bad else "")))
    return res


@case
def attn_proj_bwd_refusals():
    """A shape outside s2svc_attn_proj_supported (T1 65, D 640 > 512), a misaligned pointer or stride of dY / W_o^T and ld < T2 are refused
    by the launcher before any launch: its own message, every output untouched."""
    res = []
    c = P.CASES[4]
    D, H, dk, kind, T1, T2, causal = c
    inp = P.inputs(c)
    lay = Layout(kind, inp, T1, T2, D)
    ld, scale = A.round8(T2), inp["scale"]
    dy, wot = inp["dy"].to(DEV), inp["w_o"].t().contiguous().to(DEV)
    pm_d = G.padded(A.stored_map(inp), ld)
    dq, dkk, dv, untouched = lay.grads()
    seed = G.case_seed("proj_bwd refusals")
    lib = _lib.lib()
    for args, want in (((0, T1, T2, dk, D, 0), 1), ((0, T1, T2, 128, 512, 0), 1), ((0, T1, T2, dk, D, 3), 0), ((0, T1, T2, 128, 640, 0), 0), ((0, 65, T2, dk, D, 0), 0), ((0, T1, T2, dk, D + 32, 0), 0),
                       ((0, T1, T2, 48, 96, 0), 0)):
        got = lib.s2svc_attn_proj_supported(K._DT[BF16], *args[1:])
        res.append((bool(got) == bool(want), f"attn_proj_supported{args[1:]}: {got}, expected {want}"))
    res.append((not lib.s2svc_attn_proj_supported(K._DT[F32], T1, T2, dk, D, 0), "attn_proj_supported: fp32 is not supported"))

    def call(**kw):
        a = dict(H=H, q=lay.q, k=lay.k, v=lay.v, dy=dy, ldy=D, ybs=T1 * D, wot=wot, ldw=D, attn=pm_d, dattn=None, ld=ld, scale=scale, p=0.0,
                 seed=seed, dq=dq, dkk=dkk, dv=dv)
        a.update(kw)
        return lambda: proj_bwd_launch(**a)

    clean = [(o, o.clone()) for o in (dq, dkk, dv)]
    big = torch.zeros((5 * 128) ** 2, dtype=BF16, device=DEV)           # room for every row the refused shapes would name
    G.refused(res, "attn_proj_bwd T1 65", call(T1=65), "attn_proj_bwd: unsupported shape", clean)
    qb = torch.zeros((P.B_, T1, 640), dtype=BF16, device=DEV)
    kb = torch.zeros((P.B_, T2, 640), dtype=BF16, device=DEV)
    G.refused(res, "attn_proj_bwd D 640 > 512", call(H=5, dk=128, q=qb, k=kb, v=kb, dy=big, ldy=640, ybs=T1 * 640, wot=big, ldw=640),
              "attn_proj_bwd: unsupported shape", clean)
    G.refused(res, "attn_proj_bwd dY off by 2 bytes", call(dy=K.ptr(dy) + 2), "attn_proj_bwd: 16-byte aligned q/k/v/dY/W_o^T", clean)
    G.refused(res, "attn_proj_bwd W_o^T off by 8 bytes", call(wot=K.ptr(wot) + 8), "attn_proj_bwd: 16-byte aligned q/k/v/dY/W_o^T", clean)
    G.refused(res, "attn_proj_bwd ldy D + 4", call(ldy=D + 4), "attn_proj_bwd: strides must be multiples of 8 elements", clean)
    G.refused(res, "attn_proj_bwd ldw D + 4", call(ldw=D + 4), "attn_proj_bwd: strides must be multiples of 8 elements", clean)
    G.refused(res, "attn_proj_bwd ybs + 4", call(ybs=T1 * D + 4), "attn_proj_bwd: strides must be multiples of 8 elements", clean)
    G.refused(res, "attn_proj_bwd ldy < D", call(ldy=D - 8), "attn_proj_bwd: rows of dY and W_o^T hold D elements", clean)
    G.refused(res, "attn_proj_bwd ld < T2", call(ld=T2 - 7), "attn_proj_bwd: the map's row pitch ld must be >= T2", clean)
    res.append((untouched(), "attn_proj_bwd refusals: the gradient buffers hold their sentinels"))
    return res


def main():
    only = None
    if "--only" in sys.argv:
        only = set(sys.argv[sys.argv.index("--only") + 1].split(","))
    bad = 0
    for fn in CASES:
        if only and fn.__name__ not in only:
            continue
        try:
            results = fn()
        except Exception:
            results = [(False, f"{fn.__name__}: raised\n{traceback.format_exc()}")]
        for ok, msg in results:
            bad += 0 if ok else 1
            print(("PASS  " if ok else "FAIL  ") + msg, flush=True)
    print(f"{bad} failing lines")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
