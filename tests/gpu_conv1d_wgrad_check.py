"""Kernel-level, element-wise parity of the grouped Conv1d weight-gradient launch (csrc/conv1d_wgrad.hip: conv1d_wgrad_kernel, launchers
s2svc_conv1d_wgrad_grouped / s2svc_conv1d_wgrad_supported).  Runs on the MI355X:
  * `python tests/gpu_conv1d_wgrad_check.py [--only a,b]` prints a PASS/FAIL table for all cases and never stops early;
  * tests/test_gpu_conv1d_wgrad.py imports CASES and turns each into a `@pytest.mark.gpu` test.

Rule 1, the rule of tests/step_kernels_ref.py: compare -- ref64 = the float64 restatement of tests/conv1d_wgrad_ref.py on exactly the
values the kernel reads, yard = the same in float32 on the CPU, pass when |got - ref64| <= 4 d + ulp with d = max |yard - ref64|.
Rule 2, conditions on integer inputs whose every partial sum is exact in float32 (conv1d_wgrad_ref.exact_ok): the result equals float64
bit for bit, and equals bit for bit what the launches it replaces leave in the slot (K.gemm on the implicit-im2col operand with the
split-K plan of ops/functional.py, then K.permute_inner adding into the slot).
Rule 3, a condition on NORMAL inputs wherever T % 64 == 0 (the kernel's 64-frame steps are then the K tiles of those launches and it sums
them in the runs their split-K plan cuts): bit for bit the slot those launches leave, provided they ran the tile kernel whose order the
kernel mirrors (s2svc_gemm_last_route is asked; a case written for it FAILS when they take another route).
Exact conditions of every launch: dy and x are views into NaN-filled buffers with slack in front of row 0 and behind the last row (a
row read outside the tensor, or a tap that is not zeroed, turns the result into NaN); the rows at the utterance edges carry ~100 x the rest;
dw is a block of a sentinel-filled buffer, pre-filled with known values, whose surroundings come back unchanged.  The only calls expected
to fail are ones the launcher's host-side argument check refuses before any launch."""
import ctypes
import os
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv1d_wgrad_ref as C  # noqa: E402
import gpu_step_kernel_check as S  # noqa: E402  (Tally, sent, same_bits, refused: the idiom of the step-kernel check)
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import functional as Fn  # noqa: E402
from seq2seq_vc_amd.ops import schedule as Sched  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = S.SENT
SLACK = 3                     # rows of NaN in front of and behind an operand
GUARD = 16                    # sentinel floats around a dw block
CASES = []


def case(fn):
    CASES.append(fn)
    return fn


def nan_view(t):
    """A (B, T, C) bf16 operand as a contiguous view into a NaN-filled buffer, SLACK rows of NaN on either side (16-byte aligned: C % 8 == 0)."""
    B, T, Cc = t.shape
    buf = torch.full(((B * T + 2 * SLACK) * Cc,), float("nan"), dtype=t.dtype, device=DEV)
    v = buf[SLACK * Cc:(SLACK + B * T) * Cc].view(B, T, Cc)
    v.copy_(t)
    return v


class Slot:
    """dw as a block of a sentinel-filled buffer, pre-filled with `pre`."""

    def __init__(self, pre):
        self.n = pre.numel()
        self.buf = S.sent((self.n + 2 * GUARD,), F32)
        self.v = self.buf[GUARD:GUARD + self.n].view(pre.shape)
        self.v.copy_(pre)

    def rest_untouched(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())


TILE_ROUTE = "glds<64,64,G_TR_DENSE,G_TR_CONV1D>"
last_route = _lib.lib().s2svc_gemm_last_route            # (a name query, no kernel)


def old_launches(dy, x, slot, ks):
    """What _Conv1d.backward launches without the grouped kernel: GEMM (split-K as planned) -> fp32 (Cout, ks Cin), then the permutation
    that adds into the slot.  Clean contiguous operands: this is the reference side of Rule 2."""
    B, T, Cout = dy.shape
    Cin, pad = x.shape[2], (ks - 1) // 2
    dy, x = dy.clone(), x.clone()
    dwp = torch.empty((Cout, ks * Cin), dtype=F32, device=DEV)
    tile, sk = K.plan_gemm(Cout, ks * Cin, B * T)
    K.gemm(K.operand(dy, Cout, layout=K.RC), K.operand(x, Cin, layout=K.RC, mode=K.CONV1D, C=Cin, T=T, pad=pad), Cout, ks * Cin, B * T, dwp,
           in_dtype=BF16, splitk=sk, tile=tile, wgrad=True)
    route = last_route().decode()
    K.permute_inner(dwp, Cout, ks, Cin, out=slot, accumulate=True)
    return route, sk


def _shape_case(c):
    def run():
        B, T, Cin, Cout, ks = c
        res = []
        for regime in ("normal", "exact"):
            t = S.Tally()
            dy, x, pre = C.inputs(c, regime)
            slot = Slot(pre.to(DEV))
            K.conv1d_wgrad_grouped([(nan_view(dy.to(DEV)), nan_view(x.to(DEV)), slot.v)], 0)
            torch.cuda.synchronize()
            ref64, yard = C.wgrad(dy, x, ks, F64, pre), C.wgrad(dy, x, ks, F32, pre)
            t.close("dw", slot.v, ref64, yard, F32)
            t.exact("dw", slot.rest_untouched(), "the sentinels around the slot changed")
            extra = ""
            if regime == "exact":
                t.exact("dw", S.same_bits(slot.v.cpu(), ref64.to(F32)), "differs from float64 on exact integer inputs")
            old = Slot(pre.to(DEV))
            route, sk = old_launches(dy.to(DEV), x.to(DEV), old.v, ks)
            torch.cuda.synchronize()
            if regime == "exact":
                t.exact("dw", S.same_bits(slot.v, old.v), "differs from K.gemm + K.permute_inner on exact integer inputs")
            elif T % 64 == 0 and route.startswith(TILE_ROUTE):
                t.exact("dw", S.same_bits(slot.v, old.v), f"T % 64 == 0 and differs from K.gemm ({route}, split-K {sk}) + K.permute_inner")
                extra = f"; bit-equal to {route}, split-K {sk}"
            if T % 64 == 0 and regime == "normal":             # every case written for Rule 3 must reach it
                t.exact("dw", route.startswith(TILE_ROUTE), f"the old launches ran {route}: Rule 3 was not checked")
            if c in C.SPLIT_CASES and regime == "normal":
                t.exact("dw", sk > 1, f"the old launches ran with split-K {sk}: the case no longer probes the runs")
            res.append(t.line(f"conv1d_wgrad ({C.name_of(c)}), {regime} inputs", extra))
        return res
    run.__name__ = "conv1d_wgrad_" + "_".join(str(v) for v in c)
    run.__doc__ = f"One item, {C.name_of(c)}: Rule 1 on normal inputs, Rule 2 on exact integer inputs; NaN slack, heavy edge rows, sentinels."
    return run


for _c in C.CASES + C.SPLIT_CASES:
    case(_shape_case(_c))


@case
def conv1d_wgrad_grouped_caps():
    """The five shapes as five items of ONE launch: caps 1, 3, 64 and 0 (one workgroup per unit) give the same bits, which are the bits of
    five launches of one item; two further items that add into ONE slot do not race (exact integer inputs: the slot ends at pre + both sums,
    bit for bit what float64 gives)."""
    res = []
    data = [C.inputs(c, "normal") for c in C.CASES]
    ops = [(nan_view(dy.to(DEV)), nan_view(x.to(DEV))) for dy, x, _ in data]
    singles = []
    for (dy, x), (_, _, pre) in zip(ops, data):
        s = Slot(pre.to(DEV))
        K.conv1d_wgrad_grouped([(dy, x, s.v)], 0)
        singles.append(s)
    for cap in (1, 3, 64, 0):
        slots = [Slot(pre.to(DEV)) for _, _, pre in data]
        K.conv1d_wgrad_grouped([(dy, x, s.v) for (dy, x), s in zip(ops, slots)], cap)
        torch.cuda.synchronize()
        bad = [C.name_of(c) for c, s, one in zip(C.CASES, slots, singles) if not (S.same_bits(s.v, one.v) and s.rest_untouched())]
        res.append((not bad, f"five items in one launch, cap {cap}: every slot equals its single-item launch bit for bit"
                    + (f" EXCEPT {bad}" if bad else "")))
    c = C.CASES[0]
    (dy1, x1, pre), (dy2, x2, _) = C.inputs(c, "exact"), C.inputs(c, "exact", salt=1)
    for cap in (0, 64):
        s = Slot(pre.to(DEV))
        K.conv1d_wgrad_grouped([(nan_view(dy1.to(DEV)), nan_view(x1.to(DEV)), s.v), (nan_view(dy2.to(DEV)), nan_view(x2.to(DEV)), s.v)], cap)
        torch.cuda.synchronize()
        want = (C.wgrad(dy1, x1, c[4], F64, pre) + C.wgrad(dy2, x2, c[4], F64)).to(F32)
        res.append((S.same_bits(s.v.cpu(), want) and s.rest_untouched(), f"two items on one slot, cap {cap}: pre + both sums, bit for bit float64's"))
    # the launcher itself keeps overlapping slots apart (the wrapper above already did): the same pair through the C entry point
    s = Slot(pre.to(DEV))
    keep = [nan_view(t.to(DEV)) for t in (dy1, x1, dy2, x2)]
    arr = (_lib.Conv1dWgradItem * 2)(K._c1w_item(keep[0], keep[1], s.v), K._c1w_item(keep[2], keep[3], s.v))
    _lib.check(_lib.lib().s2svc_conv1d_wgrad_grouped(ctypes.addressof(arr), 2, 64, K.stream()), "s2svc_conv1d_wgrad_grouped")
    torch.cuda.synchronize()
    res.append((S.same_bits(s.v.cpu(), want) and s.rest_untouched(), "two items on one slot in one call of the launcher: successive launches, same bits"))
    return res


@case
def conv1d_wgrad_refusals():
    """fp32 operands, Cin % 16 != 0, ks 3, a misaligned dy / x and a layer with a bias: s2svc_conv1d_wgrad_supported (the wrapper, for the
    bias) answers 0, and the launcher refuses before any launch -- its own message, the slot untouched, also when the refused item is the
    last of three."""
    res = []
    lib = _lib.lib()
    for args, want in (((256, 256, 5, 1), 1), ((80, 256, 5, 1), 1), ((16, 16, 5, 1), 1), ((256, 256, 5, 0), 0), ((256, 24, 5, 1), 0),
                       ((40, 256, 5, 1), 0), ((256, 256, 3, 1), 0), ((256, 256, 4, 1), 0), ((0, 16, 5, 1), 0)):
        got = lib.s2svc_conv1d_wgrad_supported(*args)
        res.append((got == want, f"conv1d_wgrad_supported{args}: {got}, expected {want}"))
    res.append((K.conv1d_wgrad_supported(32, 32, 5, BF16) and not K.conv1d_wgrad_supported(32, 32, 5, BF16, bias=torch.zeros(32)),
                "conv1d_wgrad_supported: a layer with a bias is not supported"))
    res.append((not K.conv1d_wgrad_supported(32, 32, 5, F32), "conv1d_wgrad_supported: fp32 is not supported"))
    c = C.CASES[2]
    dy, x, pre = C.inputs(c, "normal")
    good = (nan_view(dy.to(DEV)), nan_view(x.to(DEV)))
    slot, other, third = Slot(pre.to(DEV)), Slot(pre.to(DEV)), Slot(pre.to(DEV))
    clean = [(s.buf, s.buf.clone()) for s in (slot, other, third)]

    def off_by_one(t):          # the same values, 2 bytes further on: contiguous, not 16-byte aligned
        buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    unsupported = "conv1d_wgrad_grouped: unsupported item"
    S.refused(res, "conv1d_wgrad fp32 operands", lambda: K.conv1d_wgrad_grouped([(dy.float().to(DEV), x.float().to(DEV), slot.v)], 0), unsupported, clean)
    x24 = torch.zeros(c[0], c[1], 24, dtype=BF16, device=DEV)
    s24 = torch.zeros(c[3], 24, 5, dtype=F32, device=DEV)
    S.refused(res, "conv1d_wgrad Cin 24", lambda: K.conv1d_wgrad_grouped([(good[0], x24, s24)], 0), unsupported, clean + [(s24, s24.clone())])
    s3 = torch.zeros(c[3], c[2], 3, dtype=F32, device=DEV)
    S.refused(res, "conv1d_wgrad ks 3", lambda: K.conv1d_wgrad_grouped([(good[0], good[1], s3)], 0), unsupported, clean + [(s3, s3.clone())])
    aligned = "conv1d_wgrad_grouped: dy and x must be 16-byte aligned"
    S.refused(res, "conv1d_wgrad dy off by 2 bytes", lambda: K.conv1d_wgrad_grouped([(off_by_one(good[0]), good[1], slot.v)], 0), aligned, clean)
    S.refused(res, "conv1d_wgrad x off by 2 bytes", lambda: K.conv1d_wgrad_grouped([(good[0], off_by_one(good[1]), slot.v)], 0), aligned, clean)
    S.refused(res, "conv1d_wgrad: a refused item behind two good ones",
              lambda: K.conv1d_wgrad_grouped([(good[0], good[1], slot.v), (good[0], good[1], other.v), (off_by_one(good[0]), good[1], third.v)], 0), aligned, clean)
    return res


def _postnet_run(off, x0, dy0):
    """Forward and backward of a small Postnet whose parameters a FlatAdam manages, the parameter gradients in ONE forked batch."""
    from seq2seq_vc_amd.modules import Postnet
    from seq2seq_vc_amd.optim import FlatAdam
    torch.manual_seed(3)
    net = Postnet(0, 16, n_layers=5, n_chans=32, n_filts=5, dropout_rate=0.5).to(DEV).train()
    opt = FlatAdam(net, lr=1e-3, grad_norm=1.0, warmup_steps=0, bf16_shadow=True)
    opt.zero_grad()
    K.manual_seed(11)
    rec, orig = [], Fn.conv1d

    def spy(xs, weight, bias=None, act=None, vlens=None):
        y = orig(xs, weight, bias, act=act, vlens=vlens)
        y.retain_grad()
        rec.append((xs.detach(), y, weight))
        return y

    calls, launch = [], K.conv1d_wgrad_grouped

    def counted(items, cap=0):
        calls.append((len(items), cap))
        return launch(items, cap)

    prev = os.environ.get("S2SVC_NO_CONV1D_WGRAD")
    os.environ["S2SVC_NO_CONV1D_WGRAD"] = "1" if off else "0"          # the switch itself, as INTEGRATION.md names it (read per call)
    Fn.enable_side_streams(4)
    Fn.conv1d, K.conv1d_wgrad_grouped = spy, counted
    try:
        x = x0.clone().requires_grad_(True)
        y = net(x)
        y.backward(dy0)
        Sched._side_flush()                 # the batch is forked HERE, capped (the one side_join flushes runs uncapped behind the chain)
        Fn.side_join()
        torch.cuda.synchronize()
    finally:
        Fn.conv1d, K.conv1d_wgrad_grouped = orig, launch
        Fn.enable_side_streams(0)
        if prev is None:
            del os.environ["S2SVC_NO_CONV1D_WGRAD"]
        else:
            os.environ["S2SVC_NO_CONV1D_WGRAD"] = prev
    outs = {"y": y.detach(), "dx": x.grad}
    for name, p in net.named_parameters():
        outs["grad " + name] = p._s2s_grad.detach().clone()
    for name, b in net.named_buffers():
        outs["buffer " + name] = b.detach().clone()
    layers = [(xs.cpu(), yy.grad.detach().cpu(), w._s2s_grad.detach().clone()) for xs, yy, w in rec]
    return outs, layers, calls


@case
def postnet_wiring():
    """A small Postnet (chans 32, odim 16, T 37, B 2, bf16) forward and backward inside a forked gradient batch, with the grouped launch
    and with the environment switch S2SVC_NO_CONV1D_WGRAD=1: the five conv weight gradients take ONE call of the grouped wrapper / none; every output, buffer and gradient
    other than the conv weights' is bit-equal between the two; the conv weight gradients of both hold Rule 1 against the float64
    restatement on the layer's own dy and x."""
    res = []
    g = torch.Generator().manual_seed(29)
    x0 = torch.randn(2, 37, 16, generator=g).to(BF16).to(DEV)
    dy0 = torch.randn(2, 37, 16, generator=g).to(BF16).to(DEV)
    new, new_layers, n_new = _postnet_run(False, x0, dy0)
    old, old_layers, n_old = _postnet_run(True, x0, dy0)
    res.append((n_new == [(5, 64)] and n_old == [], f"K.conv1d_wgrad_grouped calls as (items, cap): {n_new} with the grouped launch (expected one call, 5 items, cap 64), "
                f"{n_old} with S2SVC_NO_CONV1D_WGRAD=1 (expected none)"))
    conv = {n for n in new if n.startswith("grad ") and n.endswith(".0.weight")}
    res.append((len(conv) == 5 and len(new_layers) == 5, f"{len(conv)} conv weights, {len(new_layers)} conv layers seen"))
    bad = [n for n in new if n not in conv and not S.same_bits(new[n], old[n])]
    res.append((not bad, f"{len(new) - len(conv)} outputs, buffers and other gradients equal bit for bit with and without the switch" + (f" EXCEPT {bad}" if bad else "")))
    for tag, layers in (("grouped launch", new_layers), ("switch", old_layers)):
        t = S.Tally()
        for i, (xs, dy, got) in enumerate(layers):
            ref64, yard = C.wgrad(dy, xs, 5, F64), C.wgrad(dy, xs, 5, F32)
            t.close(f"layer {i}", got, ref64, yard, F32)
            t.exact(f"layer {i}", bool(ref64.abs().max() > 0), "the gradient is zero: nothing was checked")
        res.append(t.line(f"Postnet conv weight gradients, {tag}"))
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
