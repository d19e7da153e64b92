"""The HuBERT-Soft content encoder on the MI355X: the map-free attention forward (csrc/attn_flash.hip), front-end layer 0 and the unit
log-probs (csrc/hubert.hip) at kernel level, and the model (seq2seq_vc_amd/urhythmic/hubert.py, model.encode / encode_batch) end to end.
  * `python tests/gpu_hubert_check.py [--only a,b]` prints a PASS/FAIL table for all cases and never stops early;
  * tests/test_gpu_hubert.py imports CASES and turns each into a `@pytest.mark.gpu` test.

Floats are compared by the rule of tests/step_kernels_ref.py: ref64 = the float64 restatement of tests/hubert_ref.py on exactly the values
the kernel reads, yard = the same formula in float32 on the CPU (rounded to bf16 where the kernel stores bf16: the probabilities entering
the second product and the output of the bf16 attention kernel, the bf16 output of layer 0), d = max |yard - ref64| over a slice, pass
when |got - ref64| <= 4 d + ulp at every element of the slice.  A slice is one (utterance, head) of the attention, one utterance
elsewhere.  Exact conditions: rows beyond a length are +0 bit for bit, NaN beyond a length changes no bit, sentinel-filled remainders
come back unchanged, a row inside a batch has the bits of its own call."""
import functools
import math
import os
import sys
import traceback

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_kernels_ref as A  # noqa: E402
import gpu_step_kernel_check as S  # noqa: E402  (Tally, sent, same_bits: the idiom of the step-kernel check)
import hubert_ref as HR  # noqa: E402
import step_kernels_ref as R  # noqa: E402
from seq2seq_vc_amd import _lib  # noqa: E402
from seq2seq_vc_amd.ops import functional as Fn  # noqa: E402
from seq2seq_vc_amd.ops import kernels_hubert as KH  # noqa: E402

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = S.SENT
KT = 64                      # key tile of csrc/attn_flash.hip
DK = 64
FLASH_TS = (1, KT - 1, KT, KT + 1, 2 * KT + 1, 577)
# Checks whose kernel is correct and yet takes more than 4 d: 1.5 x the measured margin, with the cause (profiles/AB_LOG.md has the runs).
MEASURED_MARGINS = {}
# bf16 model: (distance of the HIP output from float64) / (distance of the yardstick under torch's CPU bf16 autocast), 1.5 x the ratio
# measured on the first run (profiles/AB_LOG.md: 0.887 for the units, 0.827 for the log-probs; tiny configuration, 16000 samples)
BF16_RATIO_BOUND = {"units": 1.5 * 0.887, "log_probs": 1.5 * 0.827}
sent, same_bits, name_of = S.sent, S.same_bits, S.name_of


class Tally(S.Tally):
    def __init__(self, key=None):
        super().__init__()
        self.margin = MEASURED_MARGINS.get(key, R.MARGIN)

    def slices(self, where, got, ref64, yard, H, out_dtype):
        got = got.detach().cpu()
        for ((b, h), g), (_, r), (_, y) in zip(A.slices(got, H), A.slices(ref64, H), A.slices(yard, H)):
            self.close(f"{where} [b {b}, h {h}]", g, r, y, out_dtype)

    def rows(self, where, got, ref64, yard, out_dtype):
        got = got.detach().cpu()
        for b in range(got.shape[0]):
            self.close(f"{where} [b {b}]", got[b], ref64[b], yard[b], out_dtype)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def zero_bits(x):
    x = x.detach().cpu().contiguous()
    return bool((x.view(torch.int32 if x.dtype == F32 else torch.int16) == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# attention without the map
# ---------------------------------------------------------------------------------------------------------------------------
def flash_inputs(T, H, seed, dtype, B=3):
    """A packed (B, T, 3 D) projection whose scaled scores have a standard deviation of about A.SCORE_STD, in `dtype`, on the CPU."""
    D = H * DK
    q = R.randn(B, T, D, seed=seed, scale=A.SCORE_STD, dtype=dtype)
    k, v = R.randn(B, T, D, seed=seed + 1, dtype=dtype), R.randn(B, T, D, seed=seed + 2, dtype=dtype)
    return torch.cat([q, k, v], dim=-1)


def packed_view(qkv):
    """The projection as the model holds it, inside a sentinel-filled buffer with one more row and 8 more columns."""
    B, T, W = qkv.shape
    buf = sent((B, T + 1, W + 8), qkv.dtype)
    v = buf[:, :T, :W]
    v.copy_(qkv)
    return v


class OutView:
    """A (B, T, D) output as a column block of a sentinel-filled packed buffer."""

    def __init__(self, B, T, D, dtype):
        self.buf = sent((B, T + 1, 2 * D + 8), dtype)
        self.v = self.buf[:, :T, D:2 * D]
        self.T, self.D = T, D

    def rest_untouched(self):
        c = self.buf.clone()
        c[:, :self.T, self.D:2 * self.D] = SENT
        return bool((c == SENT).all())


def run_flash(qkv, H, klen, dtype):
    """-> ctx (B, T, D) on the device, written into a sentinel-filled view; (untouched?) beside it."""
    B, T, W = qkv.shape
    D = W // 3
    pv = packed_view(qkv)
    out = OutView(B, T, D, dtype)
    KH.attn_flash_fwd(pv[..., :D], pv[..., D:2 * D], pv[..., 2 * D:], H, None if klen is None else i32(klen), R.f32(1.0 / math.sqrt(DK)), out=out.v)
    torch.cuda.synchronize()
    return out.v.clone(), out.rest_untouched()


def flash_refs(qkv, H, klen, dtype):
    D = qkv.shape[2] // 3
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    scale = R.f32(1.0 / math.sqrt(DK))
    ref64 = HR.attention_plain(q, k, v, klen, scale, H, F64)
    yard = HR.attention_plain(q, k, v, klen, scale, H, F32) if dtype == F32 else HR.attention_online(q, k, v, klen, scale, H, F32, tile=KT, bf16=True)
    return ref64, yard


def flash_verdict(tx, tag, qkv, H, klen, dtype, nan_check=True, batch_check=True):
    B, T, W = qkv.shape
    D = W // 3
    got, clean = run_flash(qkv, H, klen, dtype)
    ref64, yard = flash_refs(qkv, H, klen, dtype)
    tx.slices(tag, got, ref64, yard, H, dtype)
    tx.exact(tag, clean, "the sentinel-filled remainder of the output changed")
    for b in range(B):
        n = T if klen is None else max(0, min(int(klen[b]), T))
        tx.exact(tag, zero_bits(got[b, n:]), f"rows beyond klen of utterance {b} are not +0")
    if nan_check and klen is not None:
        dirty = qkv.clone()
        for b in range(B):
            n = max(0, min(int(klen[b]), T))
            dirty[b, n:, D:] = float("nan")                     # keys and values beyond klen
        again, _ = run_flash(dirty, H, klen, dtype)
        tx.exact(tag, same_bits(again, got), "NaN in the keys and values beyond klen changed the output")
    if batch_check:
        for b in range(B):
            alone, _ = run_flash(qkv[b:b + 1].contiguous(), H, None if klen is None else [klen[b]], dtype)
            tx.exact(tag, same_bits(alone[0], got[b]), f"utterance {b} alone (B = 1) differs from its bits inside B = {B}")


def _flash_case(name, items):
    res = []
    for dtype in (F32, BF16):
        tx = Tally(f"attn_flash_fwd[{name_of(dtype)}]")
        for tag, make in items:
            qkv, H, klen, kw = make(dtype)
            flash_verdict(tx, tag, qkv, H, klen, dtype, **kw)
        res.append(tx.line(f"{name} [{name_of(dtype)}]"))
    return res


def flash_klen(T):
    return [577, 64, 1] if T == 577 else A.klens(T)


def flash_vs_float64():
    """Every T around the key tile and 577 (ten tiles, the last one partial), H = 2, B = 3 with klen = (T, a cut inside a tile, 1)."""
    return _flash_case("flash attention, T in %s, H 2" % (FLASH_TS,),
                       [(f"T {T}", (lambda T: lambda dt: (flash_inputs(T, 2, 5000 + T, dt), 2, flash_klen(T), {}))(T)) for T in FLASH_TS])


def flash_edge_klens():
    """klen = (0, T + 3, the cut): an utterance without a key is +0, the kernel takes min(klen, T)."""
    return _flash_case("flash attention, klen (0, T + 3, cut)",
                       [(f"T {T}", (lambda T: lambda dt: (flash_inputs(T, 2, 5100 + T, dt), 2, A.edge_klens(T), {}))(T)) for T in (KT + 1, 2 * KT + 1, 577)])


def flash_twelve_heads_and_no_klen():
    return _flash_case("flash attention, H 12; klen None",
                       [("H 12, T 65", lambda dt: (flash_inputs(65, 12, 5200, dt), 12, A.klens(65), dict(batch_check=False))),
                        ("klen None, T 130", lambda dt: (flash_inputs(130, 2, 5207, dt), 2, None, {}))])


def flash_dominant_last_key():
    """One key in the last tile outweighs everything before it: the running maximum moves there and every earlier tile is rescaled."""
    def make(dt):
        T, H = 2 * KT + 1, 2
        qkv = flash_inputs(T, H, 5300, dt).to(F32)
        D = H * DK
        for h in range(H):
            qkv[:, :, h * DK] = qkv[:, :, h * DK].abs() + 2.0                       # q
            qkv[:, T - 1, D + h * DK:D + (h + 1) * DK] = 0.0
            qkv[:, T - 1, D + h * DK] = 64.0                                        # k of the last key: scaled score 8 q0 >= 16
        return qkv.to(dt), H, [T, T, T], {}
    return _flash_case("flash attention, a dominant key in the last tile", [("T 129", make)])


def flash_mean_of_values():
    """q = 0 and small-integer v: every probability is 1 / n, the context is the mean of the first n values.  fp32: within one ulp of the
    float64 mean; bf16: the fp32 quotient rounded to bf16, within one bf16 ulp."""
    res = []
    for dtype in (F32, BF16):
        tx = Tally()
        for T in (KT + 1, 577):
            H, B = 2, 3
            D = H * DK
            qkv = flash_inputs(T, H, 5400 + T, dtype)
            qkv[..., :D] = 0
            qkv[..., 2 * D:] = torch.randint(-8, 9, (B, T, D), generator=R.gen(5400 + T)).to(dtype)
            klen = flash_klen(T)
            got, clean = run_flash(qkv, H, klen, dtype)
            tx.exact(f"T {T}", clean, "the sentinel-filled remainder of the output changed")
            for b, n in enumerate(klen):
                mean = qkv[b, :n, 2 * D:].to(F64).mean(dim=0)
                err = (got[b, :n].cpu().to(F64) - mean[None]).abs()
                tx.exact(f"T {T}, utterance {b}", bool((err <= R.ulp_out(mean, dtype)[None]).all()),
                         f"the context is not the mean of v within one ulp: max err {float(err.max()):.3e}")
                tx.exact(f"T {T}, utterance {b}", zero_bits(got[b, n:]), "rows beyond klen are not +0")
        res.append(tx.line(f"flash attention, q = 0: the mean of v [{name_of(dtype)}]"))
    return res


def flash_supported_table():
    res = []
    ok = (KH.attn_flash_supported(F32, 64, 388, 388, 388, 128) and KH.attn_flash_supported(BF16, 64, 392, 392, 392, 264)
          and not KH.attn_flash_supported(BF16, 32, 392, 392, 392, 264) and not KH.attn_flash_supported(BF16, 64, 388, 392, 392, 264)
          and not KH.attn_flash_supported(F32, 64, 390, 388, 388, 128) and not KH.attn_flash_supported(torch.float16, 64, 392, 392, 392, 264)
          and not KH.attn_flash_supported(F32, 128, 388, 388, 388, 128))
    res.append((ok, f"attn_flash_supported: dk = 64 and whole 16-byte row strides only: {ok}"))
    qkv = sent((1, 4, 3 * 128 + 4), BF16)                                           # a row stride that is no multiple of 8 bf16 elements
    out = sent((1, 4, 128), BF16)
    before = out.clone()
    try:
        KH.attn_flash_fwd(qkv[..., :128], qkv[..., 128:256], qkv[..., 256:384], 2, None, out=out)
        ok, msg = False, "the call was accepted"
    except NotImplementedError as e:
        ok, msg = "unsupported problem" in str(e), str(e)
    torch.cuda.synchronize()
    res.append((ok and same_bits(out, before), f"an unsupported row stride is refused, nothing written: {msg}"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# front-end layer 0
# ---------------------------------------------------------------------------------------------------------------------------
def layer0_params(seed):
    return R.randn(512, 1, 10, seed=seed, scale=0.3), 1.0 + R.randn(512, seed=seed + 1, scale=0.2), R.randn(512, seed=seed + 2, scale=0.2)


def run_layer0(wav, lens, w, gamma, beta, L0max, dtype, pad):
    B = wav.shape[0]
    n = B * L0max * 512
    buf = sent((n + 64,), dtype)
    out = buf[:n].view(B, L0max, 512)
    wd, ld = wav.to(DEV), i32(lens)
    ws = KH.conv0_stats(wd, ld, w.to(DEV), KH.conv0_ws(B, DEV), pad)
    KH.conv0_apply(wd, ld, w.to(DEV), gamma.to(DEV), beta.to(DEV), ws, L0max, dtype, 1e-5, pad, out=out)
    torch.cuda.synchronize()
    return out.clone(), bool((buf[n:] == SENT).all())


def layer0_vs_float64():
    """L0 = 1, 63, 64, 65 frames (pad 0: Hubert.encode) and 400 (pad 40: HubertSoft.units), B = 3 with ragged lengths."""
    res = []
    w, gamma, beta = layer0_params(6000)
    for dtype in (F32, BF16):
        tx = Tally(f"hubert_conv0[{name_of(dtype)}]")
        for L0, pad in ((1, 0), (63, 0), (64, 0), (65, 0), (400, 40)):
            N = 5 * (L0 - 1) + 10 - 2 * pad + 3
            lens = [N, max(12, N // 3), 12 if pad == 0 else 1]
            wav = R.randn(3, N, seed=6100 + L0)
            tag = f"L0 {L0}, pad {pad}, lens {lens}"
            assert KH.frames0(N, pad) == L0
            got, clean = run_layer0(wav, lens, w, gamma, beta, L0, dtype, pad)
            ref64 = HR.layer0(wav, lens, w, gamma, beta, F64, pad=pad, L0max=L0)
            yard = HR.layer0(wav, lens, w, gamma, beta, F32, pad=pad, L0max=L0)
            tx.rows(tag, got, ref64, yard.to(dtype).to(F32), dtype)
            tx.exact(tag, clean, "the sentinel tail behind the output changed")
            for b, n in enumerate(lens):
                tx.exact(tag, zero_bits(got[b, KH.frames0(n, pad):]), f"frames beyond the length of row {b} are not +0")
            dirty = wav.clone()
            for b, n in enumerate(lens):
                dirty[b, n:] = float("nan")
            again, _ = run_layer0(dirty, lens, w, gamma, beta, L0, dtype, pad)
            tx.exact(tag, same_bits(again, got), "NaN in the samples beyond lens changed the output (or two calls differ)")
            twice, _ = run_layer0(wav, lens, w, gamma, beta, L0, dtype, pad)
            tx.exact(tag, same_bits(twice, got), "two calls differ")
            alone, _ = run_layer0(wav[1:2, :lens[1]].contiguous(), lens[1:2], w, gamma, beta, KH.frames0(lens[1], pad), dtype, pad)
            tx.exact(tag, same_bits(alone[0], got[1, :alone.shape[1]]), "row 1 alone differs from its bits inside the batch")
        res.append(tx.line(f"front-end layer 0 [{name_of(dtype)}]"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# logits
# ---------------------------------------------------------------------------------------------------------------------------
def run_logits(units, emb, lens, log_softmax):
    B, L, _ = units.shape
    K = emb.shape[0]
    n = B * L * K
    buf = sent((n + 64,), F32)
    out = buf[:n].view(B, L, K)
    KH.hubert_logits(units.to(DEV), emb.to(DEV), None if lens is None else i32(lens), log_softmax, out=out)
    torch.cuda.synchronize()
    return out.clone(), bool((buf[n:] == SENT).all())


def logits_vs_float64():
    """1 and 65 rows, K = 100 and 256, an all-zero unit row (the eps clamp), fp32 and bf16 units, rows beyond a length."""
    res = []
    for dtype in (F32, BF16):
        tx = Tally(f"hubert_logits[{name_of(dtype)}]")
        for (B, L, lens), K in (((1, 1, None), 100), ((1, 65, None), 256), ((1, 65, None), 100), ((2, 33, [33, 5]), 100)):
            units = R.randn(B, L, 256, seed=7000 + L + K, dtype=dtype)
            if L > 1:
                units[0, 3] = 0
            emb = R.randn(K, 256, seed=7001 + K)
            for ls in (True, False):
                tag = f"rows {B} x {L}, K {K}, lens {lens}, log_softmax {ls}"
                got, clean = run_logits(units, emb, lens, ls)
                ref64, yard = HR.log_probs(units, emb, F64, lens, ls), HR.log_probs(units, emb, F32, lens, ls)
                tx.rows(tag, got, ref64, yard, F32)
                tx.exact(tag, clean, "the sentinel tail behind the output changed")
                if lens is not None:
                    tx.exact(tag, all(zero_bits(got[b, n:]) for b, n in enumerate(lens)), "rows beyond a length are not +0")
        res.append(tx.line(f"unit log-probs [{name_of(dtype)} units]"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
TINY_ARGS = dict(_width=128, _heads=2, _ffn=256, _layers=2)
BATCH_LENS = (192000, 320, 70001)


class _mode:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.prev = Fn.compute_dtype()
        Fn.set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        Fn.set_compute_dtype(self.prev)


@functools.lru_cache(maxsize=None)
def models(kind):
    """-> (yardstick fp32, yardstick float64, the package's model on the GPU) with the same seeded weights."""
    from seq2seq_vc_amd.urhythmic.hubert import HubertSoft
    sizes = HR.TINY if kind == "tiny" else {}
    y32 = HR.seeded(11 if kind == "tiny" else 12, **sizes)
    y64 = HR.seeded(11 if kind == "tiny" else 12, **sizes).double()
    y64.load_state_dict({k: v.double() for k, v in y32.state_dict().items()})
    mine = HubertSoft(**(TINY_ARGS if kind == "tiny" else {}))
    mine.load_state_dict(y32.state_dict())
    return y32, y64, mine.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def batch_wavs():
    return R.randn(3, 1, max(BATCH_LENS), seed=8000, scale=0.3)


@functools.lru_cache(maxsize=None)
def batch_refs():
    """The ragged restatement of the tiny model on BATCH_LENS in float64 and float32, computed once (row 0 is the 600-frame single call)."""
    y32, y64, _ = models("tiny")
    return HR.ragged(y64, batch_wavs().double(), BATCH_LENS), HR.ragged(y32, batch_wavs(), BATCH_LENS)


def _encode_verdict(tx, tag, mine, y32, y64, wav):
    from seq2seq_vc_amd.urhythmic import model as UM
    units, lp = UM.encode(mine, wav.to(DEV))
    torch.cuda.synchronize()
    u64, lp64 = HR.encode(y64, wav.double())
    u32, lp32 = HR.encode(y32, wav)
    tx.exact(tag, tuple(units.shape) == tuple(u64.shape) and tuple(lp.shape) == tuple(lp64.shape) and units.dtype == F32 and lp.dtype == F32,
             f"shapes {tuple(units.shape)}, {tuple(lp.shape)} against {tuple(u64.shape)}, {tuple(lp64.shape)}")
    tx.rows(f"{tag} units", units, u64, u32, F32)
    tx.rows(f"{tag} log_probs", lp, lp64, lp32, F32)


def model_full_size_fp32():
    """HubertSoft() at its upstream sizes, seeded weights: 1 frame (320 samples) and 50 frames (16000)."""
    y32, y64, mine = models("full")
    tx = Tally("hubert_model[fp32]")
    with _mode(F32):
        for N in (320, 16000):
            _encode_verdict(tx, f"full size, N {N}", mine, y32, y64, R.randn(1, 1, N, seed=8100 + N, scale=0.3))
    return [tx.line("HubertSoft full size vs float64 [fp32]")]


def model_tiny_fp32():
    """The tiny configuration (width 128, 2 heads, 2 layers) at 1, 50 and 600 frames: the last one is past 512 keys."""
    y32, y64, mine = models("tiny")
    tx = Tally("hubert_model[fp32]")
    with _mode(F32):
        for N in (320, 16000):
            _encode_verdict(tx, f"tiny, N {N}", mine, y32, y64, R.randn(1, 1, N, seed=8200 + N, scale=0.3))
        from seq2seq_vc_amd.urhythmic import model as UM
        (u64, lp64, fl), (u32, lp32, _) = batch_refs()
        units, lp = UM.encode(mine, batch_wavs()[0:1].to(DEV))
        tx.exact("tiny, N 192000", units.shape[2] == fl[0] == 600, f"{units.shape[2]} frames")
        tx.rows("tiny, N 192000 units", units, u64[0:1], u32[0:1], F32)
        tx.rows("tiny, N 192000 log_probs", lp, lp64[0:1], lp32[0:1], F32)
    return [tx.line("HubertSoft tiny vs float64 [fp32]")]


def model_units_batch_fp32():
    """units_batch / encode_batch on rows of 192000, 320 and 70001 samples: exact frame counts, every valid row within the rule of its own
    single call's float64, +0 beyond, NaN beyond lens changes no bit."""
    from seq2seq_vc_amd.urhythmic import model as UM
    _, _, mine = models("tiny")
    (u64, lp64, fl), (u32, lp32, _) = batch_refs()
    tx = Tally("hubert_model[fp32]")
    wavs = batch_wavs().clone()
    with _mode(F32):
        units, lp, frame_lens = UM.encode_batch(mine, wavs.to(DEV), list(BATCH_LENS))
        ub, fl2 = mine.units_batch(wavs.to(DEV), torch.tensor(BATCH_LENS))
        for b, n in enumerate(BATCH_LENS):
            wavs[b, :, n:] = float("nan")
        units_n, lp_n, _ = UM.encode_batch(mine, wavs.to(DEV), list(BATCH_LENS))
    torch.cuda.synchronize()
    tx.exact("frame_lens", frame_lens.tolist() == fl == [600, 1, 218] and not frame_lens.is_cuda and fl2.tolist() == fl, f"{frame_lens.tolist()} against {fl}")
    tx.exact("units_batch", same_bits(ub.transpose(1, 2), units), "units_batch and encode_batch differ")
    for b, n in enumerate(fl):
        tx.close(f"row {b} units", units[b, :, :n].cpu(), u64[b, :, :n], u32[b, :, :n], F32)
        tx.close(f"row {b} log_probs", lp[b, :n].cpu(), lp64[b, :n], lp32[b, :n], F32)
        tx.exact(f"row {b}", zero_bits(units[b, :, n:]) and zero_bits(lp[b, n:]), "values beyond frame_lens are not +0")
    tx.exact("NaN beyond lens", same_bits(units_n, units) and same_bits(lp_n, lp), "NaN in the samples beyond lens changed the output")
    return [tx.line("units_batch / encode_batch, ragged rows [fp32]")]


def _dist(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def model_bf16():
    """bf16 compute: finite outputs of the same structure; the distance from float64 beside that of the yardstick under torch's CPU bf16
    autocast; the rate at which the most likely unit of a frame differs from float64's is reported, not bounded."""
    from seq2seq_vc_amd.urhythmic import model as UM
    y32, y64, mine = models("tiny")
    res = []
    wav = R.randn(1, 1, 16000, seed=8216, scale=0.3)
    u64, lp64 = HR.encode(y64, wav.double())
    with torch.autocast("cpu", dtype=BF16):
        ua, lpa = HR.encode(y32, wav)
    with _mode(BF16):
        units, lp = UM.encode(mine, wav.to(DEV))
        ub, lpb, fl = UM.encode_batch(mine, batch_wavs().to(DEV), list(BATCH_LENS))
    torch.cuda.synchronize()
    ok = (tuple(units.shape) == tuple(u64.shape) and tuple(lp.shape) == tuple(lp64.shape) and units.dtype == F32 and lp.dtype == F32
          and bool(torch.isfinite(units).all()) and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(ub).all()) and bool(torch.isfinite(lpb).all()))
    res.append((ok, f"bf16: finite units {tuple(units.shape)} and log_probs {tuple(lp.shape)}: {ok}"))
    ok = fl.tolist() == [600, 1, 218] and all(zero_bits(ub[b, :, n:]) and zero_bits(lpb[b, n:]) for b, n in enumerate(fl.tolist()))
    res.append((ok, f"bf16 batch: frame_lens {fl.tolist()}, +0 beyond them: {ok}"))
    for name, got, auto, ref in (("units", units.cpu(), ua.float(), u64), ("log_probs", lp.cpu(), lpa.float(), lp64)):
        dg, da = _dist(got, ref), _dist(auto, ref)
        ratio, bound = dg / da, BF16_RATIO_BOUND[name]
        res.append((ratio <= bound,
                    f"bf16 {name}: distance from float64 {dg:.3e} (HIP) / {da:.3e} (yardstick under CPU bf16 autocast) = {ratio:.3f}, bound {bound:.3f}"))
    flips = float((lp.cpu().argmax(-1) != lp64.argmax(-1)).float().mean())
    flips_a = float((lpa.float().argmax(-1) != lp64.argmax(-1)).float().mean())
    res.append((True, f"bf16: the most likely unit differs from float64's in {flips:.3f} of the frames (yardstick under autocast: {flips_a:.3f}); reported only"))
    return res


def _urhythmic(K):
    import urhythmic_ref as UR
    import vocoder_ref as VR
    from seq2seq_vc_amd import urhythmic as U
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    sound = {c: getattr(U, n) for c, n in UR.SOUND_TYPE_OF_CLUSTER.items()}
    seg = U.Segmenter(gamma=2)
    seg.load_state_dict({"n_clusters_": 3, "labels_": torch.from_numpy(UR.default_labels(K).astype(np.int64)), "n_leaves_": K, "n_features_in_": 8,
                         "children_": torch.zeros(K - 1, 2, dtype=torch.int64), "sound_types": dict(sound)})
    rm = U.RhythmModelFineGrained()
    rm.load_state_dict({"source": {getattr(U, n): v for n, v in UR.RHYTHM_SOURCE.items()},
                        "target": {getattr(U, n): v for n, v in UR.RHYTHM_TARGET.items()}})
    gen = HifiganGenerator(**dict(VR.TINY_CFG, in_channels=256))
    gen.load_state_dict(VR.seed_state_dict(gen.state_dict(), seed=5))
    return U.UrhythmicFine(seg, rm, U.TimeStretcherFineGrained(), gen.to(DEV))


def encode_feeds_urhythmic_and_launches_equal_the_plan():
    """encode -> UrhythmicFine.forward and encode_batch -> convert_batch run; the segmenter sees the log-probs as they are; the library
    launches of a call are launch_plan(), call for call."""
    from seq2seq_vc_amd.urhythmic import model as UM
    _, _, mine = models("tiny")
    res = []
    conv = _urhythmic(100)
    lens = [16000, 4000, 9000]
    wavs = R.randn(3, 1, 16000, seed=8300, scale=0.3).to(DEV)
    with _mode(F32):
        units, lp = UM.encode(mine, wavs[0:1])
        wav = conv(units, lp)
        direct = conv.segmenter(lp[0].clone())
        again = conv.segmenter(UM.encode(mine, wavs[0:1])[1][0])
        res.append((wav.dim() == 3 and bool(torch.isfinite(wav).all()), f"encode -> UrhythmicFine.forward: waveform {tuple(wav.shape)}"))
        res.append((direct == again, "the segmenter's result on encode()'s log_probs equals its result on a copy of them"))
        ub, lpb, fl = UM.encode_batch(mine, wavs, lens)
        outs = conv.convert_batch(ub, lpb, fl)
        rows = conv.segmenter.segment_batch(lpb, fl.to(DEV))[1]
        single = [conv.segmenter(lpb[b, :n].clone()) for b, n in enumerate(fl.tolist())]
        ok = len(outs) == 3 and all(bool(torch.isfinite(o).all()) for o in outs)
        res.append((ok, f"encode_batch -> convert_batch: {[tuple(o.shape) for o in outs]}"))
        same = all([conv.segmenter.sound_types[c] for c in rows[b][0]] == single[b][0] and rows[b][1] == single[b][1] for b in range(3))
        res.append((same, f"convert_batch's segmentation of every row equals the segmenter on that row's log_probs: {same}"))
        for what, dtype, fn in (("model.encode", F32, lambda: UM.encode(mine, wavs[0:1])),
                                ("model.encode batched", F32, lambda: UM.encode_batch(mine, wavs, lens)),
                                ("units", BF16, lambda: mine.units(wavs[0:1]))):
            with _mode(dtype):
                fn()                                                    # derived weights made
                real, names = _lib.check, []

                def counting(rc, what_):
                    names.append(what_)
                    return real(rc, what_)
                _lib.check = counting
                try:
                    fn()
                finally:
                    _lib.check = real
                plan = mine.launch_plan(what.split()[0], batched="batched" in what)
            res.append((names == plan, f"{what} [{name_of(dtype)}]: {len(names)} library launches, launch_plan() lists {len(plan)}"
                        + ("" if names == plan else f"; first difference at {next((i for i, (a, b) in enumerate(zip(names, plan)) if a != b), min(len(names), len(plan)))}")))
    torch.cuda.synchronize()
    return res


def inference_only():
    from seq2seq_vc_amd.urhythmic.hubert import HubertSoft
    _, _, mine = models("tiny")
    res = []
    wav = torch.zeros(1, 1, 400, device=DEV)
    for name, fn, prep in (("train() mode", lambda: mine.units(wav), lambda: mine.train()), ("grad enabled", lambda: mine.encode(wav), lambda: None),
                           ("a CPU tensor", lambda: mine.units(wav.cpu()), lambda: None)):
        prep()
        try:
            fn()
            ok = False
        except NotImplementedError:
            ok = True
        finally:
            mine.eval()
        res.append((ok, f"{name} raises NotImplementedError: {ok}"))
    with torch.no_grad(), _mode(F32):
        x, mask = mine.encode(wav)
        z = mine.logits(mine.units(wav))
    res.append((mask is None and tuple(x.shape) == (1, 1, 128) and tuple(z.shape) == (1, 1, 100), f"encode {tuple(x.shape)}, mask {mask}; logits {tuple(z.shape)}"))
    # Hubert.forward takes the waveform as it is: on the explicitly padded waveform it is logits(units(wav)), bit for bit
    wav = R.randn(2, 1, 1000, seed=8400, scale=0.3).to(DEV)
    with torch.no_grad(), _mode(F32):
        z, mask = mine(torch.nn.functional.pad(wav, (HR.PAD, HR.PAD)))
        want = mine.logits(mine.units(wav))
    res.append((mask is None and same_bits(z, want), f"forward(padded wav) {tuple(z.shape)} equals logits(units(wav)) bit for bit: {same_bits(z, want)}"))
    return res


CASES = [flash_vs_float64, flash_edge_klens, flash_twelve_heads_and_no_klen, flash_dominant_last_key, flash_mean_of_values, flash_supported_table,
         layer0_vs_float64, logits_vs_float64, model_full_size_fp32, model_tiny_fp32, model_units_batch_fp32, model_bf16,
         encode_feeds_urhythmic_and_launches_equal_the_plan, inference_only]


def main():
    only = None
    if "--only" in sys.argv:
        only = set(sys.argv[sys.argv.index("--only") + 1].split(","))
    bad = 0
    for case in CASES:
        if only and case.__name__ not in only:
            continue
        try:
            results = case()
        except Exception:      # noqa: BLE001 -- the table goes on
            results = [(False, f"{case.__name__}: raised\n{traceback.format_exc()}")]
        for ok, msg in results:
            bad += not ok
            print(("PASS  " if ok else "FAIL  ") + msg, flush=True)
        try:
            torch.cuda.synchronize()
        except Exception:      # noqa: BLE001 -- the device reports an error: nothing more is started on it
            print(f"FAIL  {case.__name__}: the device reports an error after the case; stopping\n{traceback.format_exc()}", flush=True)
            return 2
    print(f"{bad} failed", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
