"""Waveform conditioning on the MI355X: the resampler (ops.kernels_audio.resample_poly, audio.resample / resample_batch), the silence
trim (trim_intervals, wav_gather_rows, audio.trim_batch), audio.condition_batch and urhythmic.convert_wavs with conditioning.  Each
case returns [(ok, message)]; tests/test_gpu_audio.py turns them into pytest tests.

The reference is tests/audio_ref.py (float64 restatements, checked on the CPU by tests/test_audio_host.py; parity with torchaudio and
librosa themselves is unpinned: neither is installed).  Exact regime: integer taps and samples, zero tolerance.  Real regime: every
element within 4 x the distance of the restatement's own fp32 evaluation from its float64 evaluation + 1 ulp (step_kernels_ref.compare,
the rule of tests/gpu_griffin_lim_check.py).  Intervals and gathered rows: exact."""
import numpy as np
import torch

import audio_ref as AR
import gpu_urhythmic_plan_check as GP
import step_kernels_ref as R
from seq2seq_vc_amd import _lib
from seq2seq_vc_amd import audio
from seq2seq_vc_amd import urhythmic as U
from seq2seq_vc_amd.ops import kernels_audio as KA

DEV = GP.DEV
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
SENTINEL = -12345.5
GUARD = 4096


def _pad_rows(rows, fill=NAN):
    """list of 1-D fp32 rows -> (B, Nmax) on the device, `fill` beyond every row; lens"""
    rows = [torch.as_tensor(r, dtype=F32) for r in rows]
    lens = [r.numel() for r in rows]
    w = torch.full((len(rows), max(max(lens), 1)), fill, dtype=F32)
    for b, r in enumerate(rows):
        w[b, :lens[b]] = r
    return w.to(DEV), lens


def _guarded(B, M):
    """A (B, M) view in the middle of a sentinel-filled buffer -> (view, check() -> True while the guards are intact)"""
    flat = torch.full((B * M + 2 * GUARD,), SENTINEL, dtype=F32, device=DEV)
    view = flat[GUARD:GUARD + B * M].view(B, M)
    return view, lambda: bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + B * M:] == SENTINEL).all())


def resample_exact_regime():
    """Integer taps and integer samples at every ratio and edge length, in one batch per ratio: the index arithmetic alone."""
    res = []
    L = _lib.lib()
    res.append((L.s2svc_resample_tile() == KA.TILE == AR.TILE and L.s2svc_resample_max_span() == KA.MAX_SPAN,
                f"the library states a tile of {L.s2svc_resample_tile()} outputs and a span cap of {L.s2svc_resample_max_span()} samples"))
    for i, (orig, new) in enumerate(AR.RATIOS):
        band, first, width, rows = AR.exact_case(orig, new, 7100 + i)
        table = KA.make_table(band.numpy(), first, orig, new, width, DEV)
        w, lens = _pad_rows(rows)
        want = [AR.banded_resample(r, orig, new, band, first, width) for r in rows]
        M = max(o.numel() for o in want)
        buf, intact = _guarded(len(rows), M)
        before = KA.LAUNCHES
        out, out_lens = KA.resample_poly(w, lens, table, out=buf)
        n = KA.LAUNCHES - before
        got = out.cpu()
        ok = out_lens == [o.numel() for o in want] and all(torch.equal(got[b, :o.numel()].double(), o) for b, o in enumerate(want))
        zero = all(R.bits_equal(got[b, o.numel():], torch.zeros(M - o.numel())) for b, o in enumerate(want))
        res.append((ok and zero and intact() and n == 1,
                    f"{orig}/{new}: width {width}, Kb {band.shape[0]}, rows of {lens} -> {out_lens}: equal to float64 {ok}, +0 beyond {zero}, "
                    f"guards intact {intact()}, NaN beyond lens, launches {n}"))
    return res


def resample_real_regime():
    """Noise and chirps at every ratio: the comparison rule, a ragged batch against B = 1 calls and against audio.resample."""
    res = []
    for i, (orig, new) in enumerate(AR.RATIOS):
        band, first, width, _ = AR.band_of(orig, new)
        rows = AR.real_rows(orig, new, 7200 + i)
        w, lens = _pad_rows(rows)
        before = KA.LAUNCHES
        out, out_lens = audio.resample_batch(w.unsqueeze(1), lens, orig * 50, new * 50)
        n = KA.LAUNCHES - before
        table = KA.poly_table(orig, new, DEV)
        cached = KA.poly_table(orig * 50, new * 50, DEV) is table
        tb = torch.from_numpy(KA.banded_taps(orig, new)[0]).double()                # the taps the kernel reads
        ratios, oks, same = [], [], []
        for b, x in enumerate(rows):
            ref = AR.banded_resample(x, orig, new, tb, first, width, F64)
            yard = AR.banded_resample(x, orig, new, tb, first, width, F32)
            ok, ratio, d, msg = R.compare(out[b, 0, :out_lens[b]], ref, yard, F32)
            oks.append(ok and out_lens[b] == ref.numel() and not bool(out[b, 0, out_lens[b]:].any()))
            ratios.append(round(ratio, 3))
            one, one_lens = audio.resample_batch(w[b:b + 1, :lens[b]].unsqueeze(1).contiguous(), [lens[b]], orig * 50, new * 50)
            alone = audio.resample(x.to(DEV), orig * 50, new * 50)
            same.append(one_lens == [out_lens[b]] and R.bits_equal(one[0, 0], out[b, 0, :out_lens[b]]) and R.bits_equal(alone, out[b, 0, :out_lens[b]]))
        res.append((all(oks) and all(same) and n == 1 and cached and tuple(out.shape) == (4, 1, max(out_lens)),
                    f"{orig}/{new}: rows {lens} -> {out_lens}: max|got - ref64| / d per row {ratios} (bound 4 d + 1 ulp): {all(oks)}; every row "
                    f"bit-equal to its B = 1 call and to resample() of the row: {all(same)}; launches {n}; table cached: {cached}"))
    x = torch.randn(3, 2, 500, generator=AR.gen(7300)).to(DEV)
    before = KA.LAUNCHES
    y = audio.resample(x, 16000, 16000)
    b2, l2 = audio.resample_batch(x[:, :1], [500, 400, 3], 8000, 8000)
    res.append((y is x and b2.data_ptr() == x[:, :1].data_ptr() and l2 == [500, 400, 3] and KA.LAUNCHES == before, "orig == new returns the input with no launch"))
    y = audio.resample(x, 48000, 16000)
    ok = tuple(y.shape) == (3, 2, 167) and all(R.bits_equal(y[a, c], audio.resample(x[a, c], 48000, 16000)) for a in range(3) for c in range(2))
    res.append((ok, f"resample of (3, 2, 500) -> {tuple(y.shape)}, every row equal to its own call: {ok}"))
    return res


def _trim_case(name, c, mode):
    rows = c["rows"]
    fl, hop, top_db = c["frame_length"], c["hop_length"], c["top_db"]
    want = [AR.trim(y, top_db, fl, hop, mode) for y in rows]
    w, lens = _pad_rows(rows)
    before = KA.LAUNCHES
    out, out_lens, iv = audio.trim_batch(w.unsqueeze(1), lens, top_db, fl, hop, mode)
    n = KA.LAUNCHES - before
    ok_iv = iv.dtype == torch.int32 and not iv.is_cuda and iv.tolist() == [list(t) for t in want] and out_lens == [e - s for s, e in want]
    iv_d = KA.trim_intervals(w, torch.tensor(lens, dtype=torch.int32).to(DEV), 1 + max(lens) // hop, top_db, fl, hop, mode)
    ok_iv = ok_iv and iv_d.is_cuda and torch.equal(iv_d.cpu(), iv)
    got = out.cpu()
    ok_rows = tuple(out.shape) == (len(rows), 1, max(out_lens)) and all(
        R.bits_equal(got[b, 0, :e - s], torch.from_numpy(rows[b][s:e])) and R.bits_equal(got[b, 0, e - s:], torch.zeros(got.shape[2] - (e - s)))
        for b, (s, e) in enumerate(want))
    # every row against its own B = 1 call, and the gain of the gather
    singles = all(audio.trim_batch(w[b:b + 1, :lens[b]].unsqueeze(1).contiguous(), [lens[b]], top_db, fl, hop, mode)[2].tolist() == [list(want[b])]
                  for b in range(len(rows)) if lens[b] > 0)
    gained = KA.wav_gather_rows(w, iv.to(DEV), max(out_lens), 0.7).cpu()
    ok_gain = all(R.bits_equal(gained[b, :e - s], torch.from_numpy(rows[b][s:e] * np.float32(0.7))) and not gained[b, e - s:].any()
                  for b, (s, e) in enumerate(want))
    return (ok_iv and ok_rows and singles and ok_gain and n == (3 if max(out_lens) else 2),        # nothing to gather: no third launch
            f"{name} / {mode}: top_db {top_db}, frame {fl}, hop {hop}, rows {lens} -> intervals {iv.tolist()} (restatement {ok_iv}); rows bit-equal "
            f"to the input's slices, +0 beyond: {ok_rows}; B = 1 calls agree: {singles}; gain 0.7: {ok_gain}; launches {n}")


def trim_cases_vs_restatement():
    return [_trim_case(name, c, mode) for name, c in AR.trim_cases().items() for mode in AR.PAD_MODES]


def condition_batch_runs_the_reference_order():
    res = []
    rows = [AR._burst(12000, 3000, 9000, 8200), AR._burst(7000, 1000, 4000, 8201)]
    w, lens = _pad_rows(rows)
    cfg = dict(sampling_rate=16000, trim_silence=True, trim_threshold_in_db=60, trim_frame_size=2048, trim_hop_size=512, global_gain_scale=0.5)
    before = KA.LAUNCHES
    out, out_lens = audio.condition_batch(w.unsqueeze(1), lens, 24000, cfg)
    n = KA.LAUNCHES - before
    r, rl = audio.resample_batch(w.unsqueeze(1), lens, 24000, 16000)
    t, tl, iv = audio.trim_batch(r, rl, 60, 2048, 512)
    ok = out_lens == tl and R.bits_equal(out, t * 0.5) and n == len(audio.launch_plan("condition", fs=24000, config=cfg)) == 4
    res.append((ok and all(0 < a < b for a, b in zip(tl, rl)), f"24 kHz rows {lens} -> {rl} -> trimmed {tl} (intervals {iv.tolist()}), gain 0.5: equals "
                f"resample_batch -> trim_batch -> * 0.5 bit for bit: {ok}; launches {n}"))
    cfg2 = dict(sampling_rate=16000, trim_silence=False, global_gain_scale=0.25)
    before = KA.LAUNCHES
    g, gl = audio.condition_batch(w.unsqueeze(1), lens, 16000, cfg2)
    n = KA.LAUNCHES - before
    clean = torch.nan_to_num(w, nan=0.0)
    res.append((gl == lens and R.bits_equal(g[:, 0], clean * 0.25) and n == 1, f"gain alone: one gather, zeros beyond every row: launches {n}"))
    before = KA.LAUNCHES
    s, sl = audio.condition_batch(w.unsqueeze(1), lens, 16000, dict(sampling_rate=16000, trim_silence=False, global_gain_scale=0.0))
    res.append((sl == lens and R.bits_equal(s[:, 0], w) and KA.LAUNCHES == before, "nothing to do: the input itself, no launch"))
    return res


class _Recorder:
    """Stands in for the module `_lib` inside ops.kernels_audio: records the name of every library call the wrappers make."""

    def __init__(self):
        self.calls = []
        self.check = _lib.check

    def lib(self):
        real, calls = _lib.lib(), self.calls

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                return lambda *a: (calls.append(name), fn(*a))[1]
        return Proxy()


def _recorded(fn):
    rec = _Recorder()
    orig = KA._lib
    KA._lib = rec
    try:
        before = KA.LAUNCHES
        out = fn()
        return out, rec.calls, KA.LAUNCHES - before
    finally:
        KA._lib = orig


def convert_wavs_with_conditioning():
    """48 kHz waveforms with silence around the speech: convert_wavs(sample_rate=48000, trim=...) against the chain written out."""
    res = []
    hubert, model, up = GP._wav_model()
    rows = [AR._burst(20000, 4000, 16000, 8300), AR._burst(14000, 2000, 11000, 8301)]
    w, lens = _pad_rows(rows)
    w = w.unsqueeze(1)
    trim = dict(top_db=40, frame_length=400, hop_length=160)
    out, calls, n = _recorded(lambda: U.convert_wavs(hubert, model, w, lens, sample_rate=48000, trim=trim))
    cfg = dict(sampling_rate=16000, trim_silence=True, trim_threshold_in_db=40, trim_frame_size=400, trim_hop_size=160)
    plan = audio.launch_plan("condition", fs=48000, config=cfg)
    res.append((calls == plan and n == len(plan) == 4, f"library calls of the conditioning {calls} equal launch_plan() call for call: {calls == plan}"))
    r, rl = audio.resample_batch(w, lens, 48000, 16000)
    t, tl, iv = audio.trim_batch(r, rl, **trim)
    chain, calls0, n0 = _recorded(lambda: U.convert_wavs(hubert, model, t, tl))
    same = len(out) == len(chain) == 2 and all(R.bits_equal(a, b) and a.numel() > 0 and bool(torch.isfinite(a).all()) for a, b in zip(out, chain))
    res.append((same and all(0 < a < b for a, b in zip(tl, rl)),
                f"rows {lens} at 48 kHz -> {rl} at 16 kHz -> trimmed {tl} -> {[o.numel() for o in out]} samples: equals resample_batch -> trim_batch -> "
                f"convert_wavs bit for bit: {same}"))
    res.append((calls0 == [] and n0 == 0, f"convert_wavs with its defaults makes no conditioning launch: {calls0}"))
    only, calls1, _ = _recorded(lambda: U.convert_wavs(hubert, model, w, lens, sample_rate=48000))
    res.append((calls1 == ["s2svc_resample_poly"] and all(R.bits_equal(a, b) for a, b in zip(only, U.convert_wavs(hubert, model, r, rl))),
                f"sample_rate alone: {calls1}, equal to resample_batch -> convert_wavs"))
    return res


CASES = [resample_exact_regime, resample_real_regime, trim_cases_vs_restatement, condition_batch_runs_the_reference_order, convert_wavs_with_conditioning]
