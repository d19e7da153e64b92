"""The stretch plan on the MI355X: the plan kernel (ops.kernels_urhythmic.useg_plan), the three plans of UrhythmicFine.convert_batch and
convert_wavs.  Each case returns [(ok, message)]; tests/test_gpu_urhythmic_plan.py turns them into pytest tests.

No tolerance anywhere: the kernel's tables are compared integer for integer with the host code they replace (rhythm model ->
stretch_plan -> segment_table) and with the numpy restatement of tests/urhythmic_plan_ref.py (pinned to that host code by
tests/test_rhythm_table_host.py); waveforms are compared bit for bit."""
import numpy as np
import torch

import gpu_urhythmic_check as GU
import hubert_ref as HR
import urhythmic_plan_ref as PR
import urhythmic_ref as UR
import vocoder_ref as VR
from seq2seq_vc_amd import _lib
from seq2seq_vc_amd import urhythmic as U
from seq2seq_vc_amd.ops import functional as Fn
from seq2seq_vc_amd.ops import kernels_hubert as KH
from seq2seq_vc_amd.ops import kernels_urhythmic as KU
from seq2seq_vc_amd.ops import kernels_vocoder as KV
from seq2seq_vc_amd.ops.kernels import ptr, stream
from seq2seq_vc_amd.urhythmic.rhythm_model import SHORT_SILENCE
from seq2seq_vc_amd.urhythmic.stretcher import segment_table, stretch_plan
from seq2seq_vc_amd.vocoder import HifiganGenerator

DEV = GU.DEV
SOUND = PR.SOUND
S_, O_, Z_ = PR.SONORANT_ID, PR.OBSTRUENT_ID, PR.SILENCE_ID
TMAX = 130                                       # not a multiple of the kernel's chunk of 64 segments
SENTINEL = -0x5a5a5a5b
GARBAGE = (0x7fffffff, -3)                       # what clusters / cboundaries hold beyond a row's own entries


def _row(nseg, seed, must=()):
    """nseg segments in at most TMAX frames: the (cluster, length) pairs of `must`, the rest one frame each and then grown at random."""
    rng = np.random.default_rng(seed)
    pairs = [(c, n, True) for c, n in must]
    while len(pairs) < nseg:
        pairs.append((int(rng.choice([c for c in (S_, O_, Z_) if not pairs or c != pairs[-1][0]])), 1, False))
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    lengths = [n for _, n, _ in pairs]
    free = [i for i, (_, _, fixed) in enumerate(pairs) if not fixed]
    for _ in range(int(rng.integers(0, TMAX - sum(lengths) + 1)) if free else 0):
        lengths[int(rng.choice(free))] += 1
    assert len(pairs) == nseg and sum(lengths) <= TMAX
    return [c for c, _, _ in pairs], np.concatenate([[0], np.cumsum(lengths)]).astype(int).tolist()


EDGES = ((Z_, 3), (Z_, 4)) + tuple((O_, n) for n in range(1, 9))


def _garbage_tables(rows, Tmax=TMAX):
    cl, cb, ncl = PR.pack_rows(rows, Tmax)
    for b, (c, _) in enumerate(rows):
        tail = np.where(np.arange(Tmax + 1) % 2 == 0, GARBAGE[0], GARBAGE[1]).astype(np.int32)
        cl[b, len(c):] = tail[len(c):Tmax]
        cb[b, len(c) + 1:] = tail[::-1][len(c) + 1:]
    return cl, cb, ncl


def _host_plan(rm, rows):
    """The host code the kernel replaces, on the same rows: (seg (B, Smax, 4), nsegs, totals) as numpy."""
    plans = []
    for cl, cb in rows:
        types_ = [SOUND[c] for c in cl]
        plans.append(stretch_plan(types_, cb, rm(types_, cb) if types_ else []))
    seg, nsegs, totals = segment_table(plans, "cpu")
    return seg.numpy(), nsegs.numpy(), np.array(totals, np.int32)


def _plan(cl, cb, ncl, table_d, silence=Z_):
    out = KU.useg_plan(torch.from_numpy(cl).to(DEV), torch.from_numpy(cb).to(DEV), torch.from_numpy(ncl).to(DEV), table_d, silence, SHORT_SILENCE)
    return {k: v.cpu().numpy() for k, v in out.items()}


def plan_kernel_vs_host_tables():
    """ncl around the edges of the 64-segment chunks in ONE batch, garbage beyond every row's entries, outputs pre-filled."""
    res = []
    rm = PR.rhythm_model()
    table = rm.duration_table(SOUND, KU.MAX_T)
    table_d = torch.from_numpy(table.copy()).to(DEV)
    rows = [_row(0, 1), ([O_], [0, 5]), _row(63, 2, EDGES), _row(64, 3, EDGES[:4]), _row(65, 4, EDGES[4:]), _row(129, 5)]
    cl, cb, ncl = _garbage_tables(rows)
    res.append((ncl.tolist() == [0, 1, 63, 64, 65, 129] and (cl == GARBAGE[0]).any() and (cb < 0).any(), f"rows of {ncl.tolist()} segments, Tmax = {TMAX}"))
    want_seg, want_nsegs, want_totals = _host_plan(rm, rows)
    smax = want_seg.shape[1]
    res.append((want_nsegs[0] == 0 and want_nsegs[1] == 0 and (want_nsegs[2:] > 0).all() and (want_nsegs[2:] < ncl[2:]).all(),
                f"host tables: segments that survive {want_nsegs.tolist()} (rows 0 and 1: none), output frames {want_totals.tolist()}"))

    # the entry point itself, on buffers filled with a sentinel
    B = len(rows)
    d = [torch.from_numpy(a).to(DEV) for a in (cl, cb, ncl)]
    seg = torch.full((B, TMAX, 4), SENTINEL, dtype=torch.int32, device=DEV)
    small = torch.full((3, B), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().s2svc_useg_plan(B, TMAX, table.shape[0], table.shape[1] - 1, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(table_d), Z_, SHORT_SILENCE,
                                          ptr(seg), ptr(small[0]), ptr(small[1]), ptr(small[2]), stream()), "useg_plan")
    seg, small = seg.cpu().numpy(), small.cpu().numpy()
    res.append((not (seg == SENTINEL).any() and not (small == SENTINEL).any(), "every element of seg, nsegs, totals and status was written"))
    ok = np.array_equal(seg[:, :smax], want_seg) and np.array_equal(small[0], want_nsegs) and np.array_equal(small[1], want_totals) and not small[2].any()
    res.append((ok, f"seg, nsegs, totals equal segment_table(stretch_plan(.., rhythm model)) of the host, status 0: {ok}"))
    zero = all(not seg[b, small[0][b]:].any() for b in range(B))
    res.append((zero, f"seg rows at or beyond nsegs are zero: {zero}"))
    again = PR.plan_rows(cl, cb, ncl, table, Z_)
    res.append((all(np.array_equal(a, b) for a, b in zip(again, (seg, small[0], small[1], small[2]))), "... and equal the numpy restatement"))

    # the Python surface: one launch whatever B is, views of one packed buffer, every row equal to its own call
    before = KU.LAUNCHES
    got = _plan(cl, cb, ncl, table_d)
    n6 = KU.LAUNCHES - before
    same = np.array_equal(got["seg"], seg) and np.array_equal(got["packed"], small) and got["packed"].shape == (3, B)
    same = same and all(np.array_equal(got[k], small[i]) for i, k in enumerate(("nsegs", "totals", "status")))
    res.append((same, f"useg_plan returns the same tables, nsegs | totals | status as views of packed (3, B): {same}"))
    singles = []
    for b in range(B):
        before = KU.LAUNCHES
        one = _plan(cl[b:b + 1], cb[b:b + 1], ncl[b:b + 1], table_d)
        singles.append(KU.LAUNCHES - before)
        eq = np.array_equal(one["seg"][0], seg[b]) and np.array_equal(one["packed"][:, 0], small[:, b])
        res.append((eq, f"row {b} ({ncl[b]} segments) equals its own B = 1 call: {eq}"))
    res.append((n6 == 1 and set(singles) == {1}, f"launches of one call: B = 6 {n6}, B = 1 {sorted(set(singles))} (1 whatever B is)"))
    return res


def plan_kernel_flags():
    """Rows the kernel refuses: status, zeroed outputs, and the rows beside them untouched."""
    res = []
    rm = PR.rhythm_model()
    table = rm.duration_table(SOUND, KU.MAX_T)
    table_d = torch.from_numpy(table.copy()).to(DEV)
    ordinary = [_row(20, 11, EDGES), _row(7, 12), _row(40, 13, EDGES[:5])]
    rows = [ordinary[0], ([O_, S_, Z_], [0, 10, 105, 110]), ordinary[1], ([S_, 7, S_], [0, 4, 9, 12]), ordinary[2]]
    cl, cb, ncl = _garbage_tables(rows)
    got = _plan(cl, cb, ncl, table_d)
    res.append((got["status"].tolist() == [0, 1, 0, 2, 0], f"status {got['status'].tolist()} (a sonorant of 95 frames: 1; cluster id 7: 2)"))
    flagged = got["status"] != 0
    ok = (not got["nsegs"][flagged].any() and not got["totals"][flagged].any() and not got["seg"][flagged].any()
          and (got["nsegs"][~flagged] > 0).all() and (got["totals"][~flagged] > 0).all())
    res.append((ok, f"nsegs = totals = 0 and an all-zero seg on exactly the flagged rows: nsegs {got['nsegs'].tolist()}, totals {got['totals'].tolist()}"))
    alone = _plan(*_garbage_tables(ordinary), table_d)
    want_seg, want_nsegs, want_totals = _host_plan(rm, ordinary)
    keep = np.flatnonzero(~flagged)
    same = (np.array_equal(got["seg"][keep], alone["seg"]) and np.array_equal(got["packed"][:, keep], alone["packed"])
            and np.array_equal(alone["seg"][:, :want_seg.shape[1]], want_seg) and np.array_equal(alone["nsegs"], want_nsegs)
            and np.array_equal(alone["totals"], want_totals))
    res.append((same, f"the other rows equal the call without the flagged rows and the host tables, bit for bit: {same}"))
    # every way to be malformed, a short table, and a total beyond int32 (a doctored table): against the restatement
    short = np.array(table[:, :51])
    short[S_, 50] = 2**31 - 1
    rows = [([S_], [0, 60]),                                  # longer than the table (Lmax = 50)
            ([S_, O_], [0, 5, 5]),                            # an empty segment
            ([S_, O_], [0, 9, 4]),                            # boundaries that descend
            ([S_], [0, 131]),                                 # a boundary beyond Tmax
            ([S_], [-2, 5]),                                  # ... and below 0
            ([-1], [0, 5]),                                   # a negative cluster id
            ([S_, O_, S_], [0, 50, 60, 110]),                 # 2 x (2^31 - 1) + 1 output frames
            ([S_, O_], [0, 50, 55]),                          # 2^31 - 1 output frames (the obstruent maps to none): the largest total that fits
            ([S_, 3], [0, 9, 12])]                            # cluster id = n_clusters
    cl, cb, ncl = _garbage_tables(rows)
    got = _plan(cl, cb, ncl, torch.from_numpy(short).to(DEV))
    want = PR.plan_rows(cl, cb, ncl, short, Z_)
    same = all(np.array_equal(got[k], w) for k, w in zip(("seg", "nsegs", "totals", "status"), want))
    res.append((got["status"].tolist() == [2, 2, 2, 2, 2, 2, 3, 0, 2] and same and got["totals"][7] == 2**31 - 1,
                f"malformed rows and overflow: status {got['status'].tolist()}, totals {got['totals'].tolist()}; equal to the restatement: {same}"))
    # ncl itself out of range is clamped to [0, Tmax]
    cl, cb, ncl = _garbage_tables([ordinary[1], ordinary[1]])
    ncl[:] = (-5, 2**31 - 1)
    got = _plan(cl, cb, ncl, table_d)
    want = PR.plan_rows(cl, cb, ncl, table, Z_)
    res.append((got["status"].tolist() == [0, 2] and all(np.array_equal(got[k], w) for k, w in zip(("seg", "nsegs", "totals", "status"), want)),
                f"ncl = -5 and 2^31 - 1: status {got['status'].tolist()} (no segment; garbage entries refused)"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the three plans of convert_batch
# ---------------------------------------------------------------------------------------------------------------------------
def _fixture_batch():
    """The fixture utterance three times, cut to [T, 77, 40] frames, NaN in the padding of units and log-probs."""
    z, gold = np.load(UR.GOLDEN_STRETCH), UR.load_golden()
    name = str(z["names"][0])
    g = gold[name]
    T, K = g["lp"].shape
    units = torch.from_numpy(z[f"{name}/units"]).to(DEV)
    lp = torch.from_numpy(g["lp"]).to(DEV).unsqueeze(0)
    lens = [T, 77, 40]
    ub, lb = units.repeat(3, 1, 1).clone(), lp.repeat(3, 1, 1).clone()
    for b, n in enumerate(lens):
        ub[b, :, n:] = float("nan")
        lb[b, n:] = float("nan")
    return K, units, lp, ub, lb, lens


def _counted(model, fn):
    """fn() -> (result, launches of ops.kernels_urhythmic, launches of the vocoder)"""
    calls = []
    orig = {k: getattr(KV, k) for k in ("hifigan_input", "hifigan_conv1d", "hifigan_tconv1d", "hifigan_conv_out")}
    try:
        for k, f in orig.items():
            setattr(KV, k, (lambda f: lambda *a, **kw: (calls.append(1), f(*a, **kw))[1])(f))
        before = KU.LAUNCHES
        out = fn()
        return out, KU.LAUNCHES - before, len(calls)
    finally:
        for k, f in orig.items():
            setattr(KV, k, f)


def convert_batch_plans_agree():
    res = []
    K, units, lp, ub, lb, lens = _fixture_batch()
    model, up = GU._model(K)
    singles = [model(units[:, :, :n], lp[:, :n]).view(-1) for n in lens]
    lens_d = torch.tensor(lens, dtype=torch.int32).to(DEV)
    host = model.convert_batch(ub, lb, lens_d)
    default = model.convert_batch(ub, lb, lens_d, plan="host")
    res.append((all(torch.equal(a, b) for a, b in zip(host, default)), "plan=\"host\" is the default"))
    voc = len(model.vocoder.launch_plan())
    for plan, launches in (("host", 3), ("table", 3), ("device", 4)):
        counts = {}
        for B in (1, 3):
            wavs, n_ku, n_voc = _counted(model, lambda: model.convert_batch(ub[:B], lb[:B], lens_d[:B], plan=plan))
            counts[B] = (n_ku, n_voc)
        res.append((counts[1] == counts[3] == (launches, voc),
                    f"plan {plan}: launches (search + plan + stretch, vocoder) B = 1 {counts[1]}, B = 3 {counts[3]}; expected {(launches, voc)}"))
        for b, n in enumerate(lens):
            same = (tuple(wavs[b].shape) == tuple(singles[b].shape) and torch.equal(wavs[b], singles[b]) and torch.equal(wavs[b], host[b])
                    and wavs[b].numel() > 0 and wavs[b].numel() % up == 0)
            res.append((same, f"plan {plan}: row {b} ({n} frames -> {wavs[b].numel()} samples) equals plan host and forward() of the row bit for bit: {same}"))
    # lens as a list, and units as the transposed view encode_batch returns
    ut = ub.transpose(1, 2).contiguous().transpose(1, 2)
    wavs = model.convert_batch(ut, lb, lens, plan="device")
    res.append((all(torch.equal(a, b) for a, b in zip(wavs, host)), "plan device: host lens and transposed units give the same bits"))
    return res


def convert_batch_device_raises_like_host():
    """A source distribution whose CDF is exactly 1.0 from two frames on: every plan raises what the host path raises."""
    res = []
    K, units, lp, ub, lb, lens = _fixture_batch()
    model, _ = GU._model(K)
    source = dict(UR.RHYTHM_SOURCE, SONORANT=(1.0, 0.0, 1e-3))
    model.rhythm_model = PR.rhythm_model(source=source)
    cdf = model.rhythm_model.source[U.SONORANT.value].cdf(0.02 * np.arange(1, 5))
    res.append((cdf[0] < 1.0 and (cdf[1:] == 1.0).all(), f"the sonorant source CDF at 1 .. 4 frames: {cdf.tolist()}"))
    lens_d = torch.tensor(lens, dtype=torch.int32).to(DEV)
    for plan in ("host", "table", "device"):
        try:
            model.convert_batch(ub, lb, lens_d, plan=plan)
            raised = None
        except Exception as e:                                   # noqa: BLE001  (the type is what is checked)
            raised = e
        res.append((type(raised) is OverflowError, f"plan {plan}: raises {type(raised).__name__}: {raised}"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# waveform to waveform
# ---------------------------------------------------------------------------------------------------------------------------
TINY_HUBERT = dict(_width=128, _heads=2, _ffn=256, _layers=2)


def _wav_model():
    hubert = U.HubertSoft(**TINY_HUBERT)
    hubert.load_state_dict(HR.seeded(11, **HR.TINY).state_dict())
    hubert = hubert.to(DEV).eval()
    K = hubert.label_embedding.weight.shape[0]
    seg = U.Segmenter(gamma=2)
    seg.load_state_dict({"n_clusters_": 3, "labels_": torch.from_numpy(UR.default_labels(K).astype(np.int64)), "n_leaves_": K, "n_features_in_": KH.UNIT_DIM,
                         "children_": torch.zeros(K - 1, 2, dtype=torch.int64), "sound_types": dict(SOUND)})
    cfg = dict(VR.TINY_CFG, in_channels=KH.UNIT_DIM)
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(VR.seed_state_dict(gen.state_dict(), seed=5))
    return hubert, U.UrhythmicFine(seg, PR.rhythm_model(), U.TimeStretcherFineGrained(), gen.to(DEV)), int(np.prod(cfg["upsample_factors"]))


def _plan_of(model, lp, frame_lens):
    tables = model.segmenter.segment_tables(lp, frame_lens.to(DEV))
    table, silence = model._device_table(lp.device)
    plan = KU.useg_plan(tables["clusters"], tables["cboundaries"], tables["ncl"], table, silence, SHORT_SILENCE)
    return tables, plan["packed"].cpu().numpy()


def convert_wavs_equals_its_parts():
    res = []
    hubert, model, up = _wav_model()
    lens = [16000, 9000]
    g = torch.Generator().manual_seed(8300)
    clean = (0.3 * torch.randn(2, 1, 16000, generator=g)).to(DEV)
    wavs = clean.clone()
    wavs[1, :, lens[1]:] = float("nan")
    prev = Fn.compute_dtype()
    bounds = {}
    try:
        for dtype in (torch.float32, torch.bfloat16):
            Fn.set_compute_dtype(dtype)
            tag = "fp32" if dtype == torch.float32 else "bf16"
            (out, n_ku, n_voc) = _counted(model, lambda: U.convert_wavs(hubert, model, wavs, lens))
            units, lp, frame_lens = U.encode_batch(hubert, wavs, lens)
            tables, (nsegs, totals, status) = _plan_of(model, lp, frame_lens)
            bounds[tag] = [tables["cboundaries"][b, :int(tables["ncl"][b]) + 1].tolist() for b in range(2)]
            res.append((n_ku == 4 and n_voc == len(model.vocoder.launch_plan()) and not status.any(),
                        f"{tag}: convert_wavs: {n_ku} launches of search, plan and stretch (4), {n_voc} of the vocoder; frames {frame_lens.tolist()} -> {totals.tolist()}"))
            ok = (len(out) == 2 and all(o.dim() == 1 and bool(torch.isfinite(o).all()) for o in out) and (totals > 0).all()
                  and [o.numel() for o in out] == (totals * up).tolist())
            res.append((ok, f"{tag}: finite waveforms of totals x {up} samples: {[o.numel() for o in out]}"))
            padded = U.convert_wavs(hubert, model, clean * (torch.arange(16000, device=DEV) < torch.tensor(lens, device=DEV)[:, None, None]), lens)
            same = all(torch.equal(a, b) for a, b in zip(out, padded))
            res.append((same, f"{tag}: NaN and zeros in the padding of the waveforms give the same bits: {same}"))
            if dtype == torch.float32:
                parts = model.convert_batch(units, lp, frame_lens, plan="device")
                host = model.convert_batch(units, lp, frame_lens, plan="host")
                same = all(torch.equal(a, b) for a, b in zip(out, parts)) and all(torch.equal(a, b) for a, b in zip(out, host))
                res.append((same, f"fp32: equals encode_batch + convert_batch(plan=\"device\") and plan=\"host\" bit for bit: {same}"))
    finally:
        Fn.set_compute_dtype(prev)
    moved = [len(set(a) ^ set(b)) / max(len(set(a) | set(b)), 1) for a, b in zip(bounds["fp32"], bounds["bf16"])]
    res.append((True, f"bf16 against fp32: share of cluster boundaries that differ per row {[round(m, 3) for m in moved]}; reported only"))
    return res


CASES = [plan_kernel_vs_host_tables, plan_kernel_flags, convert_batch_plans_agree, convert_batch_device_raises_like_host, convert_wavs_equals_its_parts]
