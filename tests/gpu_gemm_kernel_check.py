"""Kernel-level parity of the GEMM families (csrc/gemm.hip, gemm_fast.hip, gemm_glds.hip, gemm_8ph.hip, gemm_skinny.hip) against the float64
restatement of tests/gemm_kernels_ref.py.  Runs on the MI355X:
  * `python tests/gpu_gemm_kernel_check.py [--only a,b]` prints a PASS/FAIL table for all cases (it stops only at a HIP error); with
    `--plant NAME` the truth carries that planted error of G.PLANTS wherever it applies, and those lines are expected to FAIL;
  * tests/test_gpu_gemm_kernels.py imports CASES (one function per family of G.GROUPS) and turns each into a `@pytest.mark.gpu` test.

Every case is (descriptor recipe, expected route): it FAILS when the library's s2svc_gemm_last_route names another kernel than the case was written
for, so a change of the dispatch policy has to move the shape or add one.  Each recipe runs in the regimes it lists:
  * exact -- small integers; an fp32 C (and c_pre, a_rowsum) must equal the float64 truth bit for bit, a bf16 C its bf16 rounding;
  * real  -- N(0, 1) x N(0, 1) / sqrt(K); |got - ref64| <= 4 d + ulp_out(|ref64|) at every element, d = max |yard - ref64|, yard = the
    restatement in float32 without output rounding.
Operand buffers carry NaN in their slack (ld > K, guard rows), outputs sit in sentinel-filled buffers (ldc > N, guard rows, a tail behind
the split-K workspaces) that must come back unchanged outside the M x N block.  Dropout is data: the keep-scales come from the standalone
dropout kernel (K.act_dropout_fwd on ones) with the seed the descriptor carries.  Nothing here is expected to fail a launch."""
import ctypes
import os
import sys
import traceback
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_kernels_ref as G  # noqa: E402
import gpu_step_kernel_check as S  # noqa: E402  (Tally)
import step_kernels_ref as R  # noqa: E402
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import kernels as K  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = G.SENT
WS_TAIL = 64
assert SENT == S.SENT


def route_of_last_call():
    last_route = _lib.lib().s2svc_gemm_last_route            # (a name query, no kernel: the coverage ledger lists it as such)
    return last_route().decode()


_SEED_BASE = []


def case_seed(*key):
    """(base pointer, offset) of a dropout seed that is a function of `key` alone."""
    if not _SEED_BASE:
        _SEED_BASE.append(torch.full((1,), 0x5EED, dtype=torch.int64, device=DEV))
    return _SEED_BASE[0].data_ptr(), (zlib.crc32(repr(key).encode()) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def draw_keep(M, N, p, seed):
    """The keep-scales of the (M, N) output: what the standalone dropout kernel makes of ones, element index m N + n."""
    full = K.act_dropout_fwd(torch.ones(M, N, dtype=F32, device=DEV), None, p, seed).cpu()
    inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    return full, bool(((full == 0) | (full == inv)).all())


def dev_operand(o, keep_alive):
    t = o.buf.to(DEV)
    keep_alive.append(t)
    d = _lib.Operand()
    d.ptr = t.data_ptr() + o.off * t.element_size()
    d.ld, d.layout, d.mode, d.C, d.T, d.pad = o.ld, o.layout, o.mode, o.C, o.T, o.pad
    d.T1, d.F1, d.T2, d.F2, d.bs0, d.bs1, d.zero_padded = o.T1, o.F1, o.T2, o.F2, o.bs0, o.bs1, o.zero_padded
    return d


def dev_out(x):
    t = x.buf.to(DEV)
    return t, t.data_ptr() + x.off * t.element_size()


def descriptor(p, seed):
    """-> (GemmDesc, dict of the device tensors behind its pointers)."""
    alive = []
    dev = {}
    d = _lib.GemmDesc()
    d.A, d.B = dev_operand(p.A, alive), dev_operand(p.B, alive)
    dev["C"], d.C = dev_out(p.Cbuf)
    d.ldc, d.cbs0, d.cbs1 = p.Cbuf.ld, p.Cbuf.bs0, p.Cbuf.bs1
    d.c_dtype, d.dtype = K.dt(p.c_dtype), K.dt(p.dtype)
    if p.bias is not None:
        dev["bias"] = p.bias.to(DEV)
        d.bias = dev["bias"].data_ptr()
    if p.res is not None:
        dev["res"], d.res = dev_out(p.res)
        d.ldr, d.rbs0, d.rbs1 = p.res.ld, p.res.bs0, p.res.bs1
    d.M, d.N, d.K, d.nb0, d.nb1 = p.M, p.N, p.K, p.nb0, p.nb1
    d.act, d.alpha = K.ACT[p.act], p.alpha
    d.accumulate, d.splitk, d.tile_hint = (1 if p.accumulate else 0), p.splitk, p.tile
    if p.splitk > 1:
        dev["ws"] = torch.full((p.ws_floats + WS_TAIL,), SENT, dtype=F32, device=DEV)
        d.ws = dev["ws"].data_ptr()
    if p.a_rowsum is not None:
        dev["a_rowsum"], d.a_rowsum = dev_out(p.a_rowsum)
        d.a_rowsum_accumulate = 1 if p.a_rowsum_accumulate else 0
        if p.splitk > 1:
            dev["a_rowsum_ws"] = torch.full((p.splitk * p.M + WS_TAIL,), SENT, dtype=F32, device=DEV)
            d.a_rowsum_ws = dev["a_rowsum_ws"].data_ptr()
    if p.emask is not None:
        dev["emask"], d.emask = dev_out(p.emask)
        d.ldm, d.emask_mode = p.emask.ld, p.emask_mode
    if p.drop_p > 0:
        d.drop_p, d.seed_base, d.seed_off = p.drop_p, seed[0], seed[1]
    if p.c_map is not None:
        d.c_map = 1
        d.cm_T1, d.cm_F1, d.cm_Tc, d.cm_Fc, d.cm_pt, d.cm_pf = p.c_map
    if p.c_pre is not None:
        dev["c_pre"], d.c_pre = dev_out(p.c_pre)
    dev["_alive"] = alive
    return d, dev


def launch(c, p, seed):
    """Run the descriptor of problem p (under the 8-wave mode the case asks for) -> (device tensors, route name)."""
    d, dev = descriptor(p, seed)
    L = _lib.lib()
    prev = L.s2svc_gemm_set_8ph(c.p8) if c.p8 is not None else None
    try:
        _lib.check(L.s2svc_gemm(ctypes.byref(d), K.stream()), "s2svc_gemm")
        route = route_of_last_call()
    finally:
        if prev is not None:
            L.s2svc_gemm_set_8ph(prev)
    torch.cuda.synchronize()
    return dev, route


def verdict(t, c, p, regime, dev, keep):
    """The comparisons and exact conditions of one (case, regime) into Tally t."""
    plant = PLANT if PLANT in G.plants_of(c) else None       # (the yard carries it too: d stays what float32 costs)
    r64 = G.gemm_ref(p, F64, keep, plant=plant)
    yard = G.gemm_ref(p, F32, keep, plant=plant) if regime == "real" else None
    outs = [("C", p.Cbuf, r64.C, yard.C if yard else None, r64.rows, p.c_dtype)]
    if p.c_pre is not None:
        outs.append(("c_pre", p.c_pre, r64.c_pre, yard.c_pre if yard else None, None, p.c_dtype))
    if p.a_rowsum is not None:
        outs.append(("a_rowsum", p.a_rowsum, r64.rowsum.view(1, 1, p.M, 1), yard.rowsum.view(1, 1, p.M, 1) if yard else None, None, F32))
    for name, x, ref, yd, rows, odt in outs:
        back = dev[name].cpu()
        got = G.view2(G.NS(buf=back, off=x.off, ld=x.ld, bs0=x.bs0, bs1=x.bs1), x.nb0, x.nb1, x.rows if rows is None else rows, x.N)
        if regime == "exact":
            want = ref.to(odt)
            same = R.bits_equal(got, want)
            if not same:
                bad = torch.nonzero(~((got == want) & (torch.signbit(got) == torch.signbit(want))))
                i = tuple(bad[0].tolist())
                t.exact(name, False, f"{len(bad)}/{got.numel()} elements differ from the float64 truth, first at {list(i)}: got {float(got[i])!r} want {float(want[i])!r}")
        else:
            t.close(name, got, ref, yd, odt)
        t.exact(name, G.outside_untouched(x, back, rows), f"wrote outside the {x.rows} x {x.N} block of {name} (ld {x.ld}, guard rows)")
    for name, n in (("ws", p.ws_floats), ("a_rowsum_ws", p.splitk * p.M)):
        if name in dev:
            tail = dev[name][n:].cpu()
            t.exact(name, R.bits_equal(tail, torch.full_like(tail, SENT)), f"wrote behind the {n} floats of {name}")


def run_case(c):
    """-> [(ok, line)] of one case: one line per regime."""
    res = []
    for regime in c.regimes:
        t = S.Tally()
        p = G.problem(c, regime)
        seed = case_seed(c.name, regime)
        keep = None
        if p.drop_p > 0:
            keep, clean = draw_keep(p.M, p.N, p.drop_p, seed)
            t.exact("keep-scales", clean, "a keep-scale is neither 0 nor 1 / (1 - p)")
        dev, route = launch(c, p, seed)
        t.exact("route", route == c.route, f"ran {route!r}, the case was written for {c.route!r}")
        verdict(t, c, p, regime, dev, keep)
        res.append(t.line(f"{c.name} [{regime}] {p.M} x {p.N} x {p.K}{' x %d x %d' % (p.nb0, p.nb1) if p.nb0 * p.nb1 > 1 else ''} -> {route}"))
    return res


_FAULTED = []                # a HIP error of an earlier case: nothing more is started on the card in this process


def _family(group):
    def run():
        out = []
        for c in G.GROUPS[group]:
            if _FAULTED:
                out.append((False, f"{c.name}: not run, {_FAULTED[0]} hit a HIP error before it"))
                continue
            try:
                out += run_case(c)
            except Exception as e:
                out.append((False, f"{c.name}: EXCEPTION\n{traceback.format_exc()}"))
                if "HIP" in str(e) or "hip" in str(e) or "memory access" in str(e):
                    _FAULTED.append(c.name)
        return out
    run.__name__ = group
    return run


CASES = [_family(g) for g in G.GROUPS]
PLANT = None                 # `--plant NAME` (manual spot check): the float64 truth carries that planted error wherever it applies -- expect FAIL


def case(fn):
    CASES.append(fn)
    return fn


# ---------------------------------------------------------------------------------------------------------------------------
# the grouped launchers: no route (each is a direct call); the same two regimes, poison and sentinels
# ---------------------------------------------------------------------------------------------------------------------------
def _run_group(group, call, regimes=("exact", "real"), check_ok=None):
    """call(array of descriptors, n, list of problems) launches; -> lines, one per (problem, regime), and the device tensors of the last regime."""
    res, devs = [], None
    L = _lib.lib()
    for regime in regimes:
        probs = [G.problem(c, regime) for c in G.GROUPED[group]]
        built = [descriptor(p, case_seed(group, regime)) for p in probs]
        arr = (_lib.GemmDesc * len(built))(*[d for d, _ in built])
        t0 = S.Tally()
        if check_ok is not None:
            for i, c in enumerate(G.GROUPED[group]):
                t0.exact(c.name, check_ok(ctypes.addressof(arr) + i * ctypes.sizeof(_lib.GemmDesc)) == 1, "the launcher's own eligibility test refuses the descriptor")
        call(arr, len(built), probs, t0)
        torch.cuda.synchronize()
        res.append(t0.line(f"{group} [{regime}] launch of {len(built)} problems"))
        for c, p, (_, dev) in zip(G.GROUPED[group], probs, built):
            t = S.Tally()
            verdict(t, c, p, regime, dev, None)
            res.append(t.line(f"{c.name} [{regime}] {p.M} x {p.N} x {p.K}{' x %d x %d' % (p.nb0, p.nb1) if p.nb0 * p.nb1 > 1 else ''}"))
        devs = [dev for _, dev in built]
    return res, devs


def _grouped(tile):
    L = _lib.lib()

    def call(arr, n, probs, t):
        _lib.check(L.s2svc_gemm_grouped(ctypes.addressof(arr), n, tile, K.stream()), "s2svc_gemm_grouped")
    return _run_group("grouped", call, check_ok=lambda a: L.s2svc_gemm_grouped_ok(a))[0]


@case
def gemm_grouped_tile64():
    """11 problems = two launches of gemm_grouped_kernel<64, 64>."""
    return _grouped(64)


@case
def gemm_grouped_tile128():
    return _grouped(128)


@case
def gemm_grouped_tconv_classes():
    """The four parity classes of a transposed convolution in one launch (gemm_grouped_kernel<128, 128, G_KC_TCONV2D, G_KC_DENSE>)."""
    L = _lib.lib()

    def call(arr, n, probs, t):
        _lib.check(L.s2svc_gemm_grouped(ctypes.addressof(arr), n, 128, K.stream()), "s2svc_gemm_grouped")
    return _run_group("grouped_tconv", call)[0]


@case
def gemm_grouped_batched():
    L = _lib.lib()
    out = []
    for group in ("grouped_batched_kc", "grouped_batched_rc"):
        def call(arr, n, probs, t):
            rc = L.s2svc_gemm_grouped_batched(ctypes.addressof(arr), n, K.stream())
            t.exact(group, rc == 0, f"s2svc_gemm_grouped_batched returned {rc}: the group was not launched")
        out += _run_group(group, call)[0]
    return out


def _wgrad(group):
    """s2svc_gemm_wgrad_grouped with chunks of two K tiles (s2svc_gemm_set_w8(1, 2)), then s2svc_gemm_wgrad_grouped_bg on grids capped at 1 and
    3 workgroups: the same bits as the uncapped launch."""
    L = _lib.lib()
    prev = L.s2svc_gemm_set_w8(1, 2)
    out = []
    try:
        runs = {}
        for cap in (0, 1, 3):
            def call(arr, n, probs, t, cap=cap):
                nws = int(L.s2svc_gemm_wgrad_ws_floats(ctypes.addressof(arr), n))
                want = 0                                                   # the workspace the header documents: nchunks M N (+ nchunks M, rounded up to 4)
                for p in probs:
                    kt = (p.K + 63) // 64
                    conv2 = p.B.mode == G.CONV2D_S2
                    nc = 1 if (conv2 and kt <= 75) or ((p.M + 255) // 256) * ((p.N + 127) // 128) >= 64 else (kt + 1) // 2
                    if nc > 1:
                        want += nc * p.M * p.N + ((nc * p.M + 3) // 4 * 4 if p.a_rowsum is not None else 0)
                t.exact("ws_floats", nws == want, f"s2svc_gemm_wgrad_ws_floats says {nws}, the chunking rule gives {want}")
                ws = torch.full((nws + WS_TAIL,), SENT, dtype=F32, device=DEV)
                runs.setdefault("ws", []).append((ws, nws))
                if cap == 0:
                    _lib.check(L.s2svc_gemm_wgrad_grouped(ctypes.addressof(arr), n, ws.data_ptr(), K.stream()), "s2svc_gemm_wgrad_grouped")
                else:
                    _lib.check(L.s2svc_gemm_wgrad_grouped_bg(ctypes.addressof(arr), n, ws.data_ptr(), K.stream(), cap), "s2svc_gemm_wgrad_grouped_bg")
            lines, devs = _run_group(group, call, regimes=("exact", "real") if cap == 0 else ("real",), check_ok=lambda a: L.s2svc_gemm_wgrad_ok(a))
            out += [(ok, (f"[wgs_cap {cap}] " if cap else "") + msg) for ok, msg in lines]
            runs[cap] = devs
        t = S.Tally()
        for cap in (1, 3):
            for c, d0, d1 in zip(G.GROUPED[group], runs[0], runs[cap]):
                for name in ("C", "a_rowsum"):
                    if name in d0:
                        t.exact(c.name, S.same_bits(d0[name], d1[name]), f"{name} of the launch capped at {cap} workgroups differs from the uncapped launch")
        for ws, nws in runs["ws"]:
            t.exact("ws", S.same_bits(ws[nws:], torch.full_like(ws[nws:], SENT)), f"wrote behind the {nws} floats of the workspace")
        out.append(t.line(f"{group}: capped launches (1, 3 workgroups) bit-equal to the uncapped one, workspace tails intact"))
    finally:
        L.s2svc_gemm_set_w8(prev & 255, prev >> 8)
    return out


@case
def gemm_wgrad_grouped_dense():
    return _wgrad("wgrad")


@case
def gemm_wgrad_grouped_conv2d():
    return _wgrad("wgrad_conv2d")


@case
def gemm_wgrad_grouped_conv1d():
    return _wgrad("wgrad_conv1d")


@case
def tconv2d_weights_layout():
    """s2svc_tconv2d_weights: class (pt, pf) = [C][ntaps O], element [c][tap O + o] = w[o, c, pt + 2 ta, pf + 2 fb], tap = ta (2 - pf) + fb, at offsets
    0, 4 C O, 6 C O, 8 C O; bf16(w) bit for bit, nothing behind 9 C O.  (O, C) multiples of 32 take the tiled kernel, the others the plain one."""
    res = []
    for O, C in ((64, 64), (32, 96), (24, 40), (8, 8)):
        t = S.Tally()
        w = R.randn(O, C, 3, 3, seed=O * 100 + C)
        out = torch.full((9 * C * O + WS_TAIL,), SENT, dtype=BF16, device=DEV)
        _lib.check(_lib.lib().s2svc_tconv2d_weights(O, C, w.to(DEV).data_ptr(), out.data_ptr(), K.stream()), "s2svc_tconv2d_weights")
        torch.cuda.synchronize()
        got, off = out.cpu(), 0
        for pt in (0, 1):
            for pf in (0, 1):
                ntap = (2 - pt) * (2 - pf)
                want = torch.stack([w[:, :, pt + 2 * (tap // (2 - pf)), pf + 2 * (tap % (2 - pf))] for tap in range(ntap)], 0).permute(2, 0, 1).reshape(-1).to(BF16)
                t.exact(f"class ({pt}, {pf})", R.bits_equal(got[off:off + want.numel()], want), "differs from bf16(w) in the documented layout")
                off += want.numel()
        t.exact("tail", off == 9 * C * O and R.bits_equal(got[off:], torch.full_like(got[off:], SENT)), "wrote behind 9 C O elements")
        res.append(t.line(f"tconv2d_weights O {O}, C {C}"))
    return res


def main():
    torch.manual_seed(0)
    nfail = 0
    only = None
    global PLANT
    if "--plant" in sys.argv:
        PLANT = sys.argv[sys.argv.index("--plant") + 1]
        assert PLANT in G.PLANTS, PLANT
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
        if _FAULTED:
            break
        torch.cuda.synchronize()
    print(f"== {nfail} failures")
    return nfail


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
