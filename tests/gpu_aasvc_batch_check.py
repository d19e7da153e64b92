"""AASVC.inference_batch on the MI355X.  Each case returns [(ok, message)]; tests/test_gpu_aasvc_batch.py turns them into pytest tests.

Kernel level.  The fused inference core of the convolution module (csrc/convmod_infer.hip) against the float64 restatement of
tests/aasvc_batch_ref.py (pinned to stock torch by tests/test_aasvc_batch_host.py) on the inputs as the kernel sees them.  Yardstick:
the existing separate launches (glu -> depthwise conv -> BatchNorm-eval + Swish) on each row CROPPED to its length, against the same
restatement; the fused kernel must lie within 2 x the yardstick's maximum error of the case + one ulp of the output dtype at the output's
magnitude (the fusion only removes roundings to storage and reorders a ks-term sum).  The output is pre-filled with NaN and y2 holds NaN
beyond every row's length: valid outputs must be finite, frames beyond exactly 0.  durations_finalize and the per-row resampling are
compared exactly (tolerance 0).

Model level, fp32.  The fixtures hold B = 4 utterances run one at a time through the reference; every row of the batched call must meet
the bound the single call has against its fixture (tests/gpu_model_check.py: _aas_inference: max 4e-4, mean 1e-4), durations and lengths
exactly, zeros beyond; the same in reverse row order, with NaN in all padding (bit-identical to the zero-padded call), one row at a time
(B = 1) and with the fused core switched off.  bf16: structural invariants only (see the case)."""
import os

import numpy as np
import torch

import aasvc_batch_ref as AR
from seq2seq_vc_amd import models as M
from seq2seq_vc_amd.ops import functional as Fn
from seq2seq_vc_amd.ops import functional_aas as FA
from seq2seq_vc_amd.ops import kernels as K
from seq2seq_vc_amd.ops import kernels_aas as KA

DEV = "cuda:0"
NAN = float("nan")
ATOL, L1_TOL = 4e-4, 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _ulp(ref, dtype):
    """One unit in the last place of `dtype` at the magnitude of every element of ref (float64)."""
    mant = 23 if dtype == torch.float32 else 7
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - mant)


def _convmod_case(shape, vlens, dtype, seed):
    B, Tn, C, ks = shape
    p = AR.convmod_problem(shape, seed)
    dv = lambda t: t.to(DEV)
    y2 = p["y2"].to(dtype)                                   # the values the kernels see
    ref = AR.convmod_infer_ref(y2.double(), p["w"], p["bias"], p["mean"], p["var"], p["gamma"], p["beta"], p["eps"], vlens)
    w, bias, mean, var, gamma, beta = (dv(p[k]) for k in ("w", "bias", "mean", "var", "gamma", "beta"))
    y2d = dv(y2).clone()
    lens = list(vlens) if vlens is not None else [Tn] * B
    for b in range(B):
        y2d[b, lens[b]:] = NAN
    vl = None if vlens is None else torch.tensor(vlens, dtype=torch.int32, device=DEV)
    out = torch.full((B, Tn, C), NAN, dtype=dtype, device=DEV)
    got = KA.convmod_infer(y2d, w, bias, mean, var, gamma, beta, p["eps"], vlens=vl, out=out)
    assert got is out
    got = got.double().cpu()
    # the yardstick: the separate launches, row by row on the cropped row
    nb = torch.zeros((), dtype=torch.int64, device=DEV)
    yard = 0.0
    with torch.no_grad():
        for b in range(B):
            x = dv(y2)[b:b + 1, :lens[b]].contiguous()
            x = Fn.batch_norm_act(FA.dwconv1d(Fn.glu(x), w, bias), gamma, beta, mean, var, nb, False, "swish", 0.0, p["eps"], 0.1)
            yard = max(yard, float((x[0].double().cpu() - ref[b, :lens[b]]).abs().max()))
    valid = torch.zeros(B, Tn, dtype=torch.bool)
    for b in range(B):
        valid[b, :lens[b]] = True
    finite = bool(torch.isfinite(got[valid]).all())
    zeros = bool((got[~valid] == 0).all())
    err = (got - ref).abs()[valid]
    bound = 2.0 * yard + _ulp(ref, dtype)[valid]
    worst = float((err / bound).max()) if finite else float("inf")
    ok = finite and zeros and worst <= 1.0
    tag = f"convmod_infer {str(dtype)[6:]} {shape} vlens {vlens}"
    return ok, (f"{tag}: max err {float(err.max()) if finite else NAN:.3e}, yardstick (separate launches) {yard:.3e}, err / bound {worst:.3f}, "
                f"fused / yardstick {float(err.max()) / yard if finite and yard else NAN:.3f}; valid finite {finite}, beyond vlens exactly 0 {zeros}")


def convmod_infer_fp32():
    """s2svc_convmod_infer, fp32: every shape of AR.CONVMOD_CASES."""
    return [_convmod_case(s, v, torch.float32, 11 + i) for i, (s, v) in enumerate(AR.CONVMOD_CASES)]


def convmod_infer_bf16():
    """s2svc_convmod_infer, bf16."""
    return [_convmod_case(s, v, torch.bfloat16, 11 + i) for i, (s, v) in enumerate(AR.CONVMOD_CASES)]


def convmod_infer_supported_table():
    res = [(KA.convmod_infer_supported(C, ks), f"convmod_infer_supported({C}, {ks})") for C in (32, 128, 384, 1536) for ks in (7, 15, 31)]
    res += [(not KA.convmod_infer_supported(C, ks), f"not convmod_infer_supported({C}, {ks})") for C, ks in ((30, 7), (32, 8), (32, 33))]
    return res


def durations_finalize_exact():
    """s2svc_durations_finalize, fp32 and int64, B = 5 at Tx = 13 (one pass of the wave) and Tx = 70 (two): a row of zeros (ones on its valid
    entries only), values 11 and 10 (the clamp), text_lens 1 and Tx, padding pre-filled with 7 (must come out 0), totals = row sums."""
    res = []
    for Tx in (13, 70):
        g = np.random.default_rng(Tx)
        lens = [Tx, 1, Tx - 4, 5, Tx // 2]
        d = g.integers(0, 5, size=(5, Tx)).astype(np.int64)
        d[0, 3], d[0, 4], d[0, Tx - 1] = 11, 10, 12          # the clamp (the last valid entry of a full row too)
        d[2, :] = 0                                           # an all-zero row: ones on its Tx - 4 valid entries
        d[1, 0] = 0                                           # ... and an all-zero row of one entry
        for b, L in enumerate(lens):
            d[b, L:] = 7
        for dtype in (np.float32, np.int64):
            dd = d.astype(dtype)
            want = AR.durations_finalize_ref(dd, lens)
            got = KA.durations_finalize(torch.from_numpy(dd).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), AR.MAX_DP_OUTPUT)
            same = [np.array_equal(gt.cpu().numpy(), w) and gt.cpu().numpy().dtype == w.dtype for gt, w in zip(got, want)]
            sums = np.array_equal(got[2].cpu().numpy(), got[1].cpu().numpy().sum(1).astype(np.int32))
            res.append((all(same) and sums, f"durations_finalize {np.dtype(dtype).name} Tx {Tx} lens {lens}: d_outs / ds / total equal {same}, "
                                            f"total = row sums {sums}, totals {got[2].tolist()}"))
    return res


def interp_nearest_rows_exact():
    """s2svc_interp_nearest_rows against F.interpolate on every row's own frames (a copy: exact), NaN beyond the input lengths."""
    res = []
    for dtype in (torch.float32, torch.bfloat16):
        for (Tin, Tout, C), lin, lout in (((40, 41, 32), [40, 8, 1, 5], [41, 9, 2, 6]), ((7, 70, 24), [7, 3], [70, 65])):
            g = torch.Generator().manual_seed(Tin)
            x = torch.randn(len(lin), Tin, C, generator=g).to(dtype)
            want = AR.interp_rows_ref(x.float(), Tout, lin, lout)
            xd = x.to(DEV).clone()
            for b, L in enumerate(lin):
                xd[b, L:] = NAN
            got = K.interp_nearest_rows(xd, Tout, torch.tensor(lin, dtype=torch.int32, device=DEV), torch.tensor(lout, dtype=torch.int32, device=DEV))
            res.append((torch.equal(got.float().cpu(), want), f"interp_nearest_rows {str(dtype)[6:]} ({Tin} -> {Tout}, C {C}) lens {lin} -> {lout}: equal"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
_FIX = {}


def _fixture(name):
    """(model on the device in eval(), fixture arrays): built once per fixture and left unchanged."""
    if name not in _FIX:
        cfg, z = AR.load(name)
        model = M.AASVC(**{k: v for k, v in cfg.items() if not k.startswith("__")})
        model.load_state_dict(AR.state_dict_of(cfg))
        _FIX[name] = (model.to(DEV).eval(), cfg, {k: z[k] for k in z.files})
    return _FIX[name]


def _run(name, rows, pad=0.0, dtype=torch.float32):
    """inference_batch on the given rows of the fixture (in that order), the padding of xs / dp_inputs / the noise filled with `pad`."""
    model, cfg, z = _fixture(name)
    Fn.set_compute_dtype(dtype)
    pr = cfg.get("post_encoder_reduction_factor", 1)
    T = [int(z["in.ilens"][b]) for b in rows]
    xs = torch.full((len(rows), max(T), z["in.xs"].shape[2]), pad)
    for i, b in enumerate(rows):
        xs[i, :T[i]] = torch.from_numpy(z["in.xs"][b, :T[i]])
    if "in.sdp_noise" in z:
        tx = [t // pr for t in T]
        n = torch.full((len(rows), 2, max(T) // pr), pad)
        for i, b in enumerate(rows):
            n[i, :, :tx[i]] = torch.from_numpy(z["in.sdp_noise"][b, :, :tx[i]])
        model.duration_predictor.noise = n
    xs = xs.to(DEV)
    try:
        outs, olens, d_outs = model.inference_batch(xs, torch.tensor(T), dp_inputs=xs)
    finally:
        Fn.set_compute_dtype(torch.float32)
    return outs, olens, d_outs


def _against_fixture(res, tag, name, rows, got):
    _, cfg, z = _fixture(name)
    outs, olens, d_outs = got
    want_ol = [int(z["out.olens"][b]) for b in rows]
    tx = [int(z["in.ilens"][b]) // cfg.get("post_encoder_reduction_factor", 1) for b in rows]
    res.append((outs.dtype == torch.float32 and outs.shape == (len(rows), max(want_ol), cfg["odim"]) and isinstance(olens, torch.LongTensor)
                and not olens.is_cuda and olens.tolist() == want_ol, f"{tag}: olens {olens.tolist()} (fixture {want_ol}), outs {tuple(outs.shape)} {outs.dtype}"))
    if olens.tolist() != want_ol:
        return
    for i, b in enumerate(rows):
        res.append(AR.cmp(f"{tag} row {i} (utterance {b}) predicted durations (exact)", d_outs[i, :tx[i]], z["out.d_outs"][b, :tx[i]], 0))
        res.append(AR.cmp(f"{tag} row {i} (utterance {b}) outs[:{want_ol[i]}]", outs[i, :want_ol[i]], z["out.outs"][b, :want_ol[i]], ATOL, l1_tol=L1_TOL))
    beyond = all(bool((outs[i, want_ol[i]:] == 0).all()) and bool((d_outs[i, tx[i]:] == 0).all()) for i in range(len(rows)))
    res.append((beyond, f"{tag}: outs beyond olens and d_outs beyond Tx exactly 0"))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8))


def _batch_cases(name):
    res = []
    B = _fixture(name)[2]["in.xs"].shape[0]
    calls = []
    real = KA.convmod_infer
    KA.convmod_infer = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        fwd = _run(name, list(range(B)))
    finally:
        KA.convmod_infer = real
    res.append((len(calls) > 0, f"{name}: the fused inference core ran {len(calls)} times in one call"))
    _against_fixture(res, f"{name} batch", name, list(range(B)), fwd)
    _against_fixture(res, f"{name} batch, rows reversed", name, list(range(B - 1, -1, -1)), _run(name, list(range(B - 1, -1, -1))))
    nanp = _run(name, list(range(B)), pad=NAN)
    same = [_same_bits(a, b) for a, b in zip(fwd, nanp)]
    res.append((all(same), f"{name}: NaN in the padding of xs / dp_inputs / noise: outs, olens, d_outs bit-identical to the zero-padded call {same}"))
    for b in range(B):
        _against_fixture(res, f"{name} B = 1", name, [b], _run(name, [b]))
    calls = []
    KA.convmod_infer = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    os.environ["S2SVC_NO_CONVMOD_INFER"] = "1"
    try:
        off = _run(name, [0])
    finally:
        del os.environ["S2SVC_NO_CONVMOD_INFER"]
        KA.convmod_infer = real
    res.append((len(calls) == 0, f"{name}: S2SVC_NO_CONVMOD_INFER=1 keeps the separate launches ({len(calls)} fused calls)"))
    _against_fixture(res, f"{name} row 0, separate launches", name, [0], off)
    return res


def aasvc_tiny_inference_batch_fp32():
    """Stochastic duration predictor with its own input (projection + per-row resampling), post-encoder reduction 4 (decoder width 128)."""
    return _batch_cases("aasvc_tiny_inference_batch")


def aasvc_det_tiny_inference_batch_fp32():
    """Deterministic duration predictor on the encoder outputs, Conv1d feed-forward (kernel 3) in every Conformer block."""
    return _batch_cases("aasvc_det_tiny_inference_batch")


def inference_batch_refusals():
    model, cfg, z = _fixture("aasvc_tiny_inference_batch")
    xs = torch.from_numpy(z["in.xs"]).to(DEV)
    il = torch.from_numpy(z["in.ilens"])
    res = []
    for what, kw, exc in (("a target utterance", dict(dp_inputs=xs, tgt_speech=xs[0]), NotImplementedError),
                          ("teacher forcing", dict(dp_inputs=xs, use_teacher_forcing=True), NotImplementedError),
                          ("speaker embeddings", dict(dp_inputs=xs, spembs=xs[:, 0]), NotImplementedError),
                          ("no dp_inputs for a predictor with its own input", dict(), ValueError)):
        try:
            model.inference_batch(xs, il, **kw)
            res.append((False, f"inference_batch accepted {what}"))
        except exc as e:
            res.append((True, f"inference_batch refuses {what}: {type(e).__name__}"))
    try:
        model.inference_batch(xs, il + 1, dp_inputs=xs)
        res.append((False, "inference_batch accepted lengths beyond the batch"))
    except ValueError:
        res.append((True, "inference_batch refuses lengths beyond the batch: ValueError"))
    return res


def aasvc_inference_batch_bf16_structure():
    """bf16 compute: no parity bound -- how often a bf16 encoder flips a predicted duration is not measured, and the fixtures compare
    durations exactly.  Asserted: outputs finite, zero beyond olens, olens = row sums of d_outs after the zero rule, NaN padding gives
    the bits of the zero-padded call.  Reported (not asserted): flipped durations against the fixture and, where no duration of a row
    flipped against it, the distance of the row to its own inference() call in bf16."""
    res = []
    for name in AR.FIXTURES:
        model, cfg, z = _fixture(name)
        B = z["in.xs"].shape[0]
        pr = cfg.get("post_encoder_reduction_factor", 1)
        outs, olens, d_outs = _run(name, list(range(B)), dtype=torch.bfloat16)
        tx = [int(t) // pr for t in z["in.ilens"]]
        res.append((bool(torch.isfinite(outs).all()), f"{name} bf16: outs finite"))
        res.append((all(bool((outs[b, int(olens[b]):] == 0).all()) for b in range(B)), f"{name} bf16: outs zero beyond olens {olens.tolist()}"))
        _, ds, total = AR.durations_finalize_ref(d_outs.cpu().numpy(), tx)
        res.append((olens.tolist() == [int(t) * cfg.get("decoder_reduction_factor", 1) for t in total],
                    f"{name} bf16: olens are the row sums of d_outs after the zero rule"))
        nanp = _run(name, list(range(B)), pad=NAN, dtype=torch.bfloat16)
        same = [_same_bits(a, b) for a, b in zip((outs, olens, d_outs), nanp)]
        res.append((all(same), f"{name} bf16: NaN padding gives the bits of the zero-padded call {same}"))
        flips, dist = 0, []
        for b in range(B):
            flips += int((d_outs[b, :tx[b]].cpu().double() != torch.from_numpy(z["out.d_outs"][b, :tx[b]]).double()).sum())
            x = torch.from_numpy(z["in.xs"][b, :int(z["in.ilens"][b])]).to(DEV)
            if "in.sdp_noise" in z:
                model.duration_predictor.noise = torch.from_numpy(z["in.sdp_noise"][b:b + 1, :, :tx[b]])
            Fn.set_compute_dtype(torch.bfloat16)
            try:
                o1, d1 = model.inference(x, dp_input=x)
            finally:
                Fn.set_compute_dtype(torch.float32)
            if torch.equal(d1.cpu().double(), d_outs[b, :tx[b]].cpu().double()):
                dist.append(float((o1 - outs[b, :o1.shape[0]]).abs().max()))
        res.append((True, f"{name} bf16 (measured, not asserted): {flips} of {sum(tx)} durations differ from the fp32 fixture; max |row - its own "
                          f"inference() call in bf16| over the {len(dist)} of {B} rows whose durations agree with that call: {max(dist) if dist else NAN:.3e}"))
    return res


CASES = [convmod_infer_supported_table, convmod_infer_fp32, convmod_infer_bf16, durations_finalize_exact, interp_nearest_rows_exact,
         aasvc_tiny_inference_batch_fp32, aasvc_det_tiny_inference_batch_fp32, inference_batch_refusals, aasvc_inference_batch_bf16_structure]


if __name__ == "__main__":
    bad = 0
    for c in CASES:
        for ok, msg in c():
            bad += not ok
            print(("ok   " if ok else "FAIL ") + msg, flush=True)
    raise SystemExit(1 if bad else 0)
