"""The one-launch refresh of the derived weight copies (s2svc_derived_refresh: csrc/elementwise.hip; ops.kernels.derived_refresh,
tconv2d_weights_cached; optim.FlatAdam.refresh_derived) on the MI355X, bit for bit:
  * `python tests/gpu_derived_refresh_check.py [--only a,b]` prints a PASS/FAIL table for all cases and never stops early;
  * tests/test_gpu_derived_refresh.py imports CASES and turns each into a `@pytest.mark.gpu` test.

The launch is a copy plus at most one fp32 -> bf16 rounding, so every comparison is torch.equal against what the single launchers
(K.gather3, K.tconv2d_weights) return for the same source.  Every output buffer lies between two guard runs of a finite sentinel that
must survive the launch.  The shapes are the smallest that reach every path of the kernel (slab, tile with either row order,
class-matrix tile, element-wise loop) and every tile edge: rows and columns that are no multiple of the tile, more than one tile in
each direction, a negative stride, an offset, n2 < 32."""
import os
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from seq2seq_vc_amd.ops import functional as Fn  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = -776.0                 # finite, not zero, exact in bf16
GUARD = 64
CASES = []
ELEMENT, TILE, SLAB, TCONV = 0, 1, 2, 3

# (what, n, strides, off, elements the source needs): gather3 jobs as the models register them, at the smallest shapes
SHAPES = [
    ("Conv2d taps (64, 32)", (64, 9, 32), (288, 1, 9), 0, 64 * 32 * 9),
    ("Conv2d taps (40, 24)", (40, 9, 24), (216, 1, 9), 0, 40 * 24 * 9),
    ("Conv1d forward (80, 5, 48)", (80, 5, 48), (240, 1, 5), 0, 80 * 48 * 5),
    ("Conv1d flipped (48, 5, 80)", (48, 5, 80), (5, -1, 240), 4, 80 * 48 * 5),
    ("permuted Linear (24, 19, 40)", (24, 19, 40), (760, 1, 19), 0, 24 * 760),
    ("permuted Linear, data gradient, n2 = 24 < 32", (19, 40, 24), (1, 19, 760), 0, 24 * 760),
    ("permuted Linear, data gradient, rows with i0 fastest", (19, 24, 40), (1, 19, 456), 0, 40 * 456),
    ("slab of 64 columns, off = 7, a partial second chunk", (3, 40, 70), (2800, 1, 40), 7, 3 * 2800 + 7),
    ("slab, one partial chunk of 512 columns", (5, 3, 300), (900, 1, 3), 0, 5 * 900),
    ("slab, chunks of 1024 columns, the second partial", (2, 3, 1100), (3300, 1, 3), 0, 2 * 3300),
    ("tile, 7 x 4 tiles with ragged edges", (130, 3, 200), (3, 1, 390), 0, 200 * 390),
    ("contiguous copy (element-wise loop)", (7, 3, 5), (15, 5, 1), 0, 105),
]
PATHS = [SLAB, SLAB, SLAB, TILE, SLAB, ELEMENT, TILE, SLAB, SLAB, SLAB, TILE, ELEMENT]


def case(fn):
    CASES.append(fn)
    return fn


def guarded(numel, dtype):
    """(buffer of `numel` elements, the whole allocation): the buffer lies between two GUARD-element runs of SENT."""
    whole = torch.full((numel + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + numel], whole


def guards_intact(whole):
    return bool((whole[:GUARD] == SENT).all()) and bool((whole[-GUARD:] == SENT).all())


def gather_jobs(specs, seed):
    """[(source, key, buffer)] as ops.kernels.PermRegistry holds them, and the guarded allocations."""
    g = torch.Generator().manual_seed(seed)
    jobs, wholes = [], []
    for (what, n, st, off, size), dtype in specs:
        src = torch.randn(size, generator=g).to(DEV)
        buf, whole = guarded(n[0] * n[1] * n[2], dtype)
        jobs.append((src, (n, st, off, dtype), buf.view(n)))
        wholes.append(whole)
    return jobs, wholes


def check_gathers(res, jobs, wholes, specs):
    for (src, key, buf), whole, ((what, *_), dtype) in zip(jobs, wholes, specs):
        ok = torch.equal(buf, K.gather3(src, *key)) and guards_intact(whole)
        res.append((ok, f"{what}, {str(dtype)[6:]}: equal to K.gather3, guards intact"))


def class_matrices(w):
    return torch.cat([v.reshape(-1) for v in K.tconv2d_weights(w.detach())])


@case
def grouped_refresh_against_gather3():
    """27 jobs in ONE call (the grouped launch it replaces takes 24): every shape of SHAPES to fp32 and to bf16, the first three once
    more from other sources; job by job torch.equal with K.gather3."""
    specs = [(s, dt) for s in SHAPES for dt in (F32, BF16)] + [(s, BF16) for s in SHAPES[:3]]
    jobs, wholes = gather_jobs(specs, 11)
    res = [(len(jobs) == 27, "27 jobs")]
    plan = K.derived_refresh_plan(jobs)
    want = [p for p in PATHS for _ in (0, 1)] + PATHS[:3]
    res.append(([p for p, _ in plan] == want, f"paths {[p for p, _ in plan]} (0 element-wise, 1 tile, 2 slab)"))
    K.derived_refresh(jobs)
    torch.cuda.synchronize()
    check_gathers(res, jobs, wholes, specs)
    return res


@case
def more_jobs_than_one_launch_takes():
    """50 small jobs: the launcher splits them 48 + 2."""
    specs = [(SHAPES[i % 3 + 1], BF16 if i % 2 else F32) for i in range(50)]
    jobs, wholes = gather_jobs(specs, 12)
    K.derived_refresh(jobs)
    torch.cuda.synchronize()
    res = []
    check_gathers(res, jobs, wholes, specs)
    return [(all(ok for ok, _ in res), f"50 jobs equal to K.gather3: {sum(ok for ok, _ in res)}")]


@case
def class_weights_from_the_refresh():
    """The class matrices of the transposed convolution from the refresh launch == K.tconv2d_weights: (O, C) = (64, 32), (32, 64)
    and (40, 24) (ragged tiles in both directions), alone and in one call with gather jobs."""
    g = torch.Generator().manual_seed(13)
    res = []
    ws = [torch.randn(O, C, 3, 3, generator=g).to(DEV) for O, C in ((64, 32), (32, 64), (40, 24))]
    for together in (False, True):
        bufs = [guarded(w.numel(), BF16) for w in ws]
        tconvs = [(w, b) for w, (b, _) in zip(ws, bufs)]
        specs = [(s, BF16) for s in SHAPES[:4]] if together else []
        jobs, wholes = gather_jobs(specs, 14)
        plan = K.derived_refresh_plan(jobs, tconvs)
        res.append(([p for p, _ in plan[len(jobs):]] == [TCONV] * 3, f"class-matrix jobs take the class-matrix tile path: {plan[len(jobs):]}"))
        if together:
            K.derived_refresh(jobs, tconvs)
        else:
            for t in tconvs:
                K.derived_refresh([], [t])
        torch.cuda.synchronize()
        for w, (b, whole) in zip(ws, bufs):
            ok = torch.equal(b, class_matrices(w)) and guards_intact(whole)
            res.append((ok, f"(O, C) = {tuple(w.shape[:2])}, {'with gather jobs' if together else 'alone'}: equal to K.tconv2d_weights, guards intact"))
        check_gathers(res, jobs, wholes, specs)
    try:
        K.derived_refresh([], [(ws[0], torch.empty(7, dtype=BF16, device=DEV))])
        res.append((False, "a class-matrix buffer of the wrong size was accepted"))
    except ValueError:
        res.append((True, "a class-matrix buffer of the wrong size is refused before any launch"))
    return res


@case
def class_weights_stay_fresh_in_training():
    """Tiny VTN in bf16 (golden vtn_tiny_train, set up as gpu_model_check.derived_weight_copies_are_fresh_after_every_update does): the
    class buffer of the front-end's Conv2d weight == K.tconv2d_weights(weight) after two eager steps, after a captured opt.step() and
    two replays, after load_state_dict + refresh_shadow, and -- computed again on use -- after an in-place change of the weight and
    for a copy registered after the capture.  The tiny front-end has 32 channels, below the 64 from which the backward pass runs
    the class GEMMs, so the test registers the copy itself, by the call the backward pass makes at full size."""
    import gpu_model_check as mc
    from seq2seq_vc_amd import losses as L
    from seq2seq_vc_amd import models as M
    from seq2seq_vc_amd.optim import FlatAdam
    cfg, z = mc.load("vtn_tiny_train")
    res = []
    try:
        Fn.set_compute_dtype(BF16)
        K.manual_seed(7)
        model = M.VTN(**mc.model_cfg(cfg))
        model.load_state_dict(mc.sd_of(z))
        model.to(DEV).train()
        for m in model.modules():
            if hasattr(m, "dropout_rate"):
                m.dropout_rate = 0.0
        opt = FlatAdam(model, lr=1e-3, grad_norm=1.0, warmup_steps=10, bf16_shadow=True)
        crit = L.Seq2SeqLoss(10.0)
        t = lambda k: torch.from_numpy(z[k])
        xs, ys, labels = t("in.xs").to(DEV), t("in.ys").to(DEV), t("in.labels").to(DEV)
        params = dict(model.named_parameters())
        w, w_first = params["encoder.embed.conv.2.weight"], params["encoder.embed.conv.0.weight"]
        reg = opt._perm_jobs
        views = K.tconv2d_weights_cached(w)
        buf = reg.tconv[0][1] if reg.tconv else None
        res.append((len(reg.tconv) == 1 and reg.tconv[0][0] is w and views[0].data_ptr() == buf.data_ptr() and
                    [tuple(v.shape) for v in views] == [(32, 4 * 32), (32, 2 * 32), (32, 2 * 32), (32, 32)], "first use registers the class buffer"))

        def fresh(point, use=False):
            torch.cuda.synchronize()
            got = K.tconv2d_weights_cached(w) if use else views
            same = all(a is b for a, b in zip(got, views))
            res.append((same and torch.equal(buf, class_matrices(w)), f"{point}: the class buffer equals K.tconv2d_weights(weight)"))

        for step in range(2):
            opt.zero_grad()
            o = model(xs, t("in.ilens"), ys, labels, t("in.olens"))
            l1, bce = crit(o[0], o[1], o[2], o[3], o[4], o[5])
            (l1 + bce).backward()
            Fn.side_join()
            before = w.detach().clone()
            opt.step()
            fresh(f"eager step {step + 1}")
            res.append((not torch.equal(before, w.detach()), f"eager step {step + 1} changed the weight"))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
        res.append((reg.tconv_covered == 1 and reg.covered == len(reg), "the captured refresh covers every copy registered so far"))
        for replay in range(2):
            before = w.detach().clone()
            g.replay()
            fresh(f"captured step, replay {replay + 1}")
            res.append((not torch.equal(before, w.detach()), f"replay {replay + 1} changed the weight"))
        late = K.tconv2d_weights_cached(w_first)                 # registered after the capture: computed again on use
        g.replay()
        torch.cuda.synchronize()
        got = K.tconv2d_weights_cached(w_first)
        res.append((len(reg.tconv) == 2 and got[0] is late[0] and torch.equal(reg.tconv[1][1], class_matrices(w_first)),
                    "a class buffer registered after the capture is computed again on use"))
        fresh("replay after a late registration")
        model.load_state_dict(mc.sd_of(z))
        opt.refresh_shadow()
        fresh("load_state_dict + refresh_shadow")
        res.append((torch.equal(reg.tconv[1][1], class_matrices(w_first)), "refresh_shadow from Python rewrites the late copy as well"))
        with torch.no_grad():
            w.mul_(1.5)
        torch.cuda.synchronize()
        res.append((not torch.equal(buf, class_matrices(w)), "an in-place change of the weight leaves the buffer stale until it is used"))
        fresh("in-place change, then use", use=True)
    finally:
        Fn.set_compute_dtype(torch.float32)
    return res


@case
def conv2d_backward_with_a_managed_weight():
    """dx of conv2d_s2_relu's backward pass (bf16, O = 64: the four class GEMMs) with a weight that a FlatAdam manages == dx with an
    unmanaged clone of it, bit for bit: on first use (the copy is computed in the backward pass) and after an optimiser step (the
    copy comes from the refresh launch and the backward pass launches nothing for it)."""
    from seq2seq_vc_amd.optim import FlatAdam
    torch.manual_seed(5)
    net = torch.nn.Conv2d(32, 64, 3, 2).to(DEV)
    opt = FlatAdam(net, lr=1e-2, grad_norm=1.0, warmup_steps=0, bf16_shadow=True)
    g = torch.Generator().manual_seed(15)
    x0 = torch.randn(2, 13, 11, 32, generator=g).to(DEV).to(BF16)
    dy = torch.randn(2, 6, 5, 64, generator=g).to(DEV).to(BF16)

    def dx_of(weight, bias):
        x = x0.clone().requires_grad_(True)
        y = Fn.conv2d_s2_relu(x, weight, bias)
        y.backward(dy)
        Fn.side_join()
        torch.cuda.synchronize()
        return x.grad

    res = []
    for point in ("first use", "after an optimiser step"):
        managed = dx_of(net.weight, net.bias)
        clone_w, clone_b = net.weight.detach().clone().requires_grad_(True), net.bias.detach().clone().requires_grad_(True)
        plain = dx_of(clone_w, clone_b)
        n_reg = len(opt._perm_jobs.tconv)
        res.append((n_reg == 1 and managed is not None and bool(managed.float().abs().sum() > 0) and torch.equal(managed, plain),
                    f"{point}: dx with the managed weight equals dx with an unmanaged clone ({n_reg} class buffer registered)"))
        res.append((torch.equal(opt._perm_jobs.tconv[0][1], class_matrices(net.weight)), f"{point}: the class buffer is fresh"))
        before = net.weight.detach().clone()
        opt.step()
        res.append((not torch.equal(before, net.weight.detach()), f"{point}: the step behind it changed the weight"))
    return res


def main():
    only = None
    if "--only" in sys.argv:
        only = set(sys.argv[sys.argv.index("--only") + 1].split(","))
    failed = 0
    for fn in CASES:
        if only and fn.__name__ not in only:
            continue
        try:
            results = fn()
        except Exception:  # noqa: BLE001
            results = [(False, "raised:\n" + traceback.format_exc())]
        for ok, msg in results:
            failed += not ok
            print(f"{'PASS' if ok else 'FAIL'}  {fn.__name__}: {msg}", flush=True)
    print(f"{failed} failed")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
