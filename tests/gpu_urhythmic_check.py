"""Urhythmic on the MI355X.  Each case returns [(ok, message)]; tests/test_gpu_urhythmic.py turns them into pytest tests.

Search: compared BIT FOR BIT, no tolerance -- alpha (as bits), P, codes, boundaries and the merged clusters / boundaries -- against the
numpy restatement in tests/urhythmic_ref.py (pinned to the reference's own output by tests/test_urhythmic_host.py) or, for the
fixture's inputs, against the arrays recorded from the reference.

Stretch: against F.interpolate(mode="linear") on the CPU, per segment.  Yardstick as for the Griffin-Lim vocoder: the CPU run in
float64 is the truth, d = max |float32 run - float64 run| is what fp32 arithmetic costs on this input, and the GPU result must lie
within MARGIN x d of the float64 run, with a floor of FLOOR x the peak.  Nothing here is fitted to what the kernels return."""
import numpy as np
import torch
import torch.nn.functional as F

import urhythmic_ref as UR
import vocoder_ref as VR
from seq2seq_vc_amd import urhythmic as U
from seq2seq_vc_amd.ops import kernels_urhythmic as KU
from seq2seq_vc_amd.urhythmic.stretcher import segment_table, stretch_plan
from seq2seq_vc_amd.vocoder import HifiganGenerator

DEV = "cuda:0"
MARGIN = 4.0
FLOOR = 1e-6
SOUND = {c: getattr(U, n) for c, n in UR.SOUND_TYPE_OF_CLUSTER.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------------
def _search(lps, gamma, labels, Tmax=None, pad=float("nan")):
    """Rows of different lengths in ONE call; padded frames hold `pad`.  Returns the tables on the host."""
    lens = [lp.shape[0] for lp in lps]
    Tmax = max(max(lens), 1) if Tmax is None else Tmax
    K = lps[0].shape[1]
    batch = np.full((len(lps), Tmax, K), pad, np.float32)
    for b, lp in enumerate(lps):
        batch[b, :lens[b]] = lp
    out = KU.useg_segment(torch.from_numpy(batch).to(DEV), torch.tensor(lens, dtype=torch.int32).to(DEV), gamma,
                          labels=torch.from_numpy(np.asarray(labels, np.int32)).to(DEV), want_tables=True)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "packed"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _row_equals(res, tag, got, b, want):
    """Row b of the device tables against a dict of the restatement's / the fixture's arrays: every entry, and zeros behind them."""
    T, ns, nc = len(want["codes"]), len(want["boundaries"]) - 1, len(want["clusters"])
    bad = []
    if not np.array_equal(_bits(got["alpha"][b, :T + 1]), _bits(want["alpha"])):
        bad.append(f"alpha differs at frames {np.flatnonzero(_bits(got['alpha'][b, :T + 1]) != _bits(want['alpha']))[:4].tolist()}")
    if not np.array_equal(got["P"][b, :T + 1], want["P"]):
        bad.append(f"P differs at frames {np.flatnonzero((got['P'][b, :T + 1] != want['P']).any(1))[:4].tolist()}")
    if not np.array_equal(got["codes"][b, :T], want["codes"]):
        bad.append("codes differ")
    if got["nseg"][b] != ns or not np.array_equal(got["boundaries"][b, :ns + 1], want["boundaries"]):
        bad.append(f"boundaries differ ({got['nseg'][b]} segments, {ns} wanted)")
    if got["ncl"][b] != nc or not np.array_equal(got["clusters"][b, :nc], want["clusters"]) or not np.array_equal(got["cboundaries"][b, :nc + 1], want["cboundaries"]):
        bad.append(f"merged clusters / boundaries differ ({got['ncl'][b]} clusters, {nc} wanted)")
    tails = (got["alpha"][b, T + 1:], got["P"][b, T + 1:], got["codes"][b, T:], got["boundaries"][b, ns + 1:], got["clusters"][b, nc:], got["cboundaries"][b, nc + 1:])
    if any(t.size and (t != 0).any() for t in tails):
        bad.append("entries past the row's own are not zero")
    res.append((not bad, f"{tag}: T {T}, {ns} segments, {nc} clusters: " + ("alpha (bits), P, codes, boundaries, clusters equal" if not bad else "; ".join(bad))))


def _against_restatement(res, tag, lp, gamma):
    labels = UR.default_labels(lp.shape[1])
    _row_equals(res, tag, _search([lp], gamma, labels), 0, UR.segment_all(lp, gamma, labels))


def search_chunk_edges_in_T():
    """T around the edges of the 64-candidate chunks of the scan."""
    res = []
    for i, T in enumerate((1, 2, 63, 64, 65, 128, 130)):
        _against_restatement(res, f"T = {T}, K = 100, gamma 2", UR.piecewise_log_probs(T, 100, seed=50 + i), 2.0)
        _against_restatement(res, f"T = {T}, K = 5, gamma 0.7", UR.piecewise_log_probs(T, 5, seed=60 + i, sharp=2.0), 0.7)
    return res


def search_unit_counts():
    """K around the edges of the 64-lane slots of the span kernel."""
    res = []
    for i, K in enumerate((1, 2, 63, 64, 65, 100, 129)):
        gamma = (2.0, 0.7)[i % 2]
        _against_restatement(res, f"K = {K}, T = 70, gamma {gamma}", UR.piecewise_log_probs(70, K, seed=70 + i, sharp=3.0), gamma)
    _against_restatement(res, "K = 256, T = 66, gamma 2", UR.piecewise_log_probs(66, 256, seed=80), 2.0)
    return res


def _against_fixture(names):
    res, gold = [], UR.load_golden()
    for name in names(gold):
        g = gold[name]
        _row_equals(res, name, _search([g["lp"]], float(g["gamma"]), g["labels"]), 0, g)
    return res


def search_piecewise_fixture():
    return _against_fixture(lambda gold: [n for n in gold if n.startswith(("piecewise_", "single_"))])


def search_rounding_family():
    """The running maximum held in float32: 16 inputs on which a plain float64 argmax picks other back-pointers."""
    res = _against_fixture(lambda gold: [n for n in gold if n.startswith("rounding_")])
    res.append((len(res) == 16, f"{len(res)} inputs of the rounding family"))
    return res


def search_ties():
    res = _against_fixture(lambda gold: [n for n in gold if n.startswith("tie_")])
    res.append((len(res) == 4, f"{len(res)} tie inputs"))
    return res


def search_ragged_batch():
    """B = 5 with lengths 0, 1, 64, 65, 130 in one call: every row equals its single call and the restatement; what the padding holds
    (NaN or finite garbage) changes nothing."""
    res = []
    K, gamma = 100, 2.0
    labels = UR.default_labels(K)
    lps = [UR.piecewise_log_probs(T, K, seed=90 + i) if T else np.zeros((0, K), np.float32) for i, T in enumerate((0, 1, 64, 65, 130))]
    before = KU.LAUNCHES
    nan = _search(lps, gamma, labels)
    res.append((KU.LAUNCHES - before == 2, f"launches of one call with B = 5: {KU.LAUNCHES - before} (2 whatever B is)"))
    other = _search(lps, gamma, labels, pad=-3.25)
    same = all(np.array_equal(nan[k], other[k]) if nan[k].dtype.kind != "f" else np.array_equal(_bits(nan[k]), _bits(other[k])) for k in nan)
    res.append((same, f"NaN padding and finite padding give the same tables: {same}"))
    for b, lp in enumerate(lps):
        want = UR.segment_all(lp, gamma, labels)
        _row_equals(res, f"row {b} of the batch", nan, b, want)
        if lp.shape[0]:
            _row_equals(res, f"row {b} alone", _search([lp], gamma, labels), 0, want)
    res.append((nan["nseg"][0] == 0 and nan["ncl"][0] == 0 and nan["boundaries"][0, 0] == 0 and nan["cboundaries"][0, 0] == 0,
                "the row of length 0 has no segment, no cluster and boundaries [0]"))
    # the public surface on the same rows: Segmenter.segment_batch (one host read) and the module function
    seg = U.Segmenter(gamma=gamma)
    seg.load_state_dict({"n_clusters_": 3, "labels_": torch.from_numpy(labels.astype(np.int64)), "n_leaves_": K, "n_features_in_": 8,
                         "children_": torch.zeros(K - 1, 2, dtype=torch.int64), "sound_types": dict(SOUND)})
    batch = np.full((5, 130, K), np.nan, np.float32)
    for b, lp in enumerate(lps):
        batch[b, :lp.shape[0]] = lp
    _, rows = seg.segment_batch(torch.from_numpy(batch).to(DEV), torch.tensor([lp.shape[0] for lp in lps], dtype=torch.int32).to(DEV))
    ok = all(rows[b][0] == UR.segment_all(lp, gamma, labels)["clusters"].tolist() and rows[b][1] == UR.segment_all(lp, gamma, labels)["cboundaries"].tolist()
             for b, lp in enumerate(lps))
    res.append((ok, f"Segmenter.segment_batch host lists equal the restatement: {ok}"))
    want = UR.segment_all(lps[3], gamma, labels)
    types_, bounds = seg(lps[3])
    codes, boundaries = U.segment(torch.from_numpy(lps[3]), gamma)
    res.append((types_ == [SOUND[int(c)] for c in want["clusters"]] and bounds == want["cboundaries"].tolist() and np.array_equal(codes, want["codes"])
                and np.array_equal(boundaries, want["boundaries"]), "Segmenter.__call__ (numpy input) and segment() (CPU tensor) equal the restatement"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the stretcher
# ---------------------------------------------------------------------------------------------------------------------------
def _verdict(res, tag, got, f32, f64):
    got, f32, f64 = (np.asarray(a, np.float64) for a in (got, f32, f64))
    if got.shape != f64.shape:
        res.append((False, f"{tag}: shape {got.shape} vs {f64.shape}"))
        return
    d = float(np.abs(f32 - f64).max())
    peak = float(np.abs(f64).max())
    err = float(np.abs(got - f64).max())
    bar = max(MARGIN * d, FLOOR * peak)
    res.append((bool(np.isfinite(got).all()) and err <= bar,
                f"{tag}: GPU-vs-float64 {err:.3e}, float32-vs-float64 {d:.3e}, ratio {err / max(d, 1e-300):.2f} (bar {MARGIN} x, floor "
                f"{FLOOR * peak:.1e}), peak {peak:.3g}"))


# segments of source length 1, 2 and 7 (and 12); targets 1, shorter, equal, longer; a short silence (dropped) and a zero target (dropped)
S_, O_, Z_ = U.SONORANT, U.OBSTRUENT, U.SILENCE
PLAN_CLUSTERS = [S_, O_, S_, Z_, O_, S_, Z_, O_, S_, O_]
PLAN_BOUNDS = [0, 1, 3, 10, 12, 19, 26, 38, 39, 41, 48]
PLAN_DURATIONS = [4, 1, 7, 3, 0, 30, 1, 2, 11]       # one per segment that is not a short silence (segment 3 is one)


def _units(D, T, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((1, D, T)).astype(np.float32))


def stretch_segments_vs_interpolate():
    res = []
    plan = stretch_plan(PLAN_CLUSTERS, PLAN_BOUNDS, PLAN_DURATIONS)
    res.append((plan == [(0, 1, 4), (1, 2, 1), (3, 7, 7), (12, 7, 3), (26, 12, 30), (38, 1, 1), (39, 2, 2), (41, 7, 11)],
                f"plan (start, length, target) after both filters: {plan}"))
    ts = U.TimeStretcherFineGrained()
    for D in (8, 256):
        x = _units(D, 48, seed=D)
        want32, want64 = (UR.interpolate_segments(x[0], plan, dt).numpy() for dt in (torch.float32, torch.float64))
        y = ts(x.to(DEV), PLAN_CLUSTERS, PLAN_BOUNDS, PLAN_DURATIONS)
        res.append((tuple(y.shape) == (1, D, 59) and y.dtype == torch.float32 and y.is_cuda, f"C = {D}: output {tuple(y.shape)}"))
        _verdict(res, f"C = {D}, (1, D, T) contiguous input", y[0].cpu().numpy(), want32, want64)
        # what encode() returns: a transposed view of (1, T, D)
        xt = x.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
        y2 = ts(xt, PLAN_CLUSTERS, PLAN_BOUNDS, PLAN_DURATIONS)
        res.append((not xt.is_contiguous() and torch.equal(y, y2), f"C = {D}: a transposed view gives the same bits: {torch.equal(y, y2)}"))
        # bf16 units: the same rounding of the input on both sides, fp32 arithmetic
        xb = x.to(torch.bfloat16)
        w32, w64 = (UR.interpolate_segments(xb[0].float(), plan, dt).numpy() for dt in (torch.float32, torch.float64))
        yb = ts(xb.to(DEV), PLAN_CLUSTERS, PLAN_BOUNDS, PLAN_DURATIONS)
        res.append((yb.dtype == torch.float32, f"C = {D}: bf16 units give an fp32 result"))
        _verdict(res, f"C = {D}, bf16 units", yb[0].cpu().numpy(), w32, w64)
    # the fixture recorded from the reference (segmentation, durations and units of two inputs)
    z, gold = np.load(UR.GOLDEN_STRETCH), UR.load_golden()
    for name in z["names"]:
        g = gold[str(name)]
        types_, bounds = [SOUND[int(c)] for c in g["clusters"]], [int(v) for v in g["cboundaries"]]
        x = torch.from_numpy(z[f"{name}/units"])
        plan = stretch_plan(types_, bounds, z[f"{name}/durations"].tolist())
        y = ts(x.to(DEV), types_, bounds, z[f"{name}/durations"].tolist())
        _verdict(res, f"fixture {name}", y[0].cpu().numpy(), z[f"{name}/stretched"][0], UR.interpolate_segments(x[0], plan, torch.float64).numpy())
    return res


def stretch_global_ratios():
    res = []
    z = np.load(UR.GOLDEN_STRETCH)
    tg = U.TimeStretcherGlobal()
    for ratio in (0.5, 1.0, 1.37):
        for D, T in ((8, 37), (256, 50)):
            x = torch.from_numpy(UR.fixture_units(T, D, seed=41))
            want32 = F.interpolate(x, scale_factor=ratio, mode="linear").numpy()
            want64 = F.interpolate(x.double(), scale_factor=ratio, mode="linear").numpy()
            y = tg(x.to(DEV), ratio)
            _verdict(res, f"ratio {ratio}, C = {D}, T = {T} -> {want64.shape[-1]}", y.cpu().numpy(), want32, want64)
            if D == 8:
                res.append((np.array_equal(want32, z[f"global/{ratio}"]), f"ratio {ratio}: the CPU yardstick is the reference's recorded output"))
    x = torch.from_numpy(UR.fixture_units(37, 8, seed=43)).repeat(3, 1, 1)
    y = tg(x.to(DEV), 1.37)
    res.append((tuple(y.shape) == (3, 8, 50) and torch.equal(y[0], y[2]), "a batch of three: every row the same bits"))
    return res


def stretch_batch_rows_equal_single_calls():
    res = []
    ts = U.TimeStretcherFineGrained()
    D, Tmax = 8, 48
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((4, D, Tmax)).astype(np.float32))
    rows = [(PLAN_CLUSTERS, PLAN_BOUNDS, PLAN_DURATIONS),
            ([S_, Z_, O_], [0, 5, 7, 20], [9, 3]),                                   # 20 frames, the short silence dropped
            ([Z_], [0, 2], []),                                                    # nothing is left: an empty row
            ([O_, S_], [0, 30, 31], [2, 5])]
    lens = [48, 20, 2, 31]
    dirty = x.clone()
    for b, n in enumerate(lens):
        dirty[b, :, n:] = float("nan")
    before = KU.LAUNCHES
    out, totals = ts.stretch_batch(dirty.to(DEV), rows)
    res.append((KU.LAUNCHES - before == 1 and totals == [59, 12, 0, 7] and tuple(out.shape) == (4, 59, D),
                f"one launch for the batch ({KU.LAUNCHES - before}), output frames {totals}, {tuple(out.shape)} channel-last"))
    for b, n in enumerate(lens):
        zero = bool((out[b, totals[b]:] == 0).all())
        if totals[b]:
            single = ts(x[b:b + 1, :, :n].to(DEV), *rows[b])
            same = torch.equal(out[b, :totals[b]].t(), single[0])
            alive = bool(torch.isfinite(single).all()) and float(single.abs().max()) > 0
        else:
            same = alive = True
        res.append((same and zero and alive, f"row {b}: equals the single call bit for bit: {same}; frames past {totals[b]} are zero: {zero}"))
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------
def _model(K):
    seg = U.Segmenter(gamma=2)
    seg.load_state_dict({"n_clusters_": 3, "labels_": torch.from_numpy(UR.default_labels(K).astype(np.int64)), "n_leaves_": K, "n_features_in_": 8,
                         "children_": torch.zeros(K - 1, 2, dtype=torch.int64), "sound_types": dict(SOUND)})
    rm = U.RhythmModelFineGrained()
    rm.load_state_dict({"source": {getattr(U, n): v for n, v in UR.RHYTHM_SOURCE.items()},
                        "target": {getattr(U, n): v for n, v in UR.RHYTHM_TARGET.items()}})
    cfg = dict(VR.TINY_CFG, in_channels=8)
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(VR.seed_state_dict(gen.state_dict(), seed=5))
    gen.to(DEV)
    return U.UrhythmicFine(seg, rm, U.TimeStretcherFineGrained(), gen), int(np.prod(cfg["upsample_factors"]))


def urhythmic_fine_end_to_end():
    res = []
    z, gold = np.load(UR.GOLDEN_STRETCH), UR.load_golden()
    name = str(z["names"][0])
    g = gold[name]
    T, K = g["lp"].shape
    model, up = _model(K)
    units = torch.from_numpy(z[f"{name}/units"]).to(DEV)
    lp = torch.from_numpy(g["lp"]).to(DEV).unsqueeze(0)
    types_, bounds = model.segmenter(lp[0])
    durations = model.rhythm_model(types_, bounds)
    ok = types_ == [SOUND[int(c)] for c in g["clusters"]] and bounds == g["cboundaries"].tolist() and durations == z[f"{name}/durations"].tolist()
    res.append((ok, f"{name}: clusters, boundaries and target durations equal the fixture: {ok}"))
    stretched = model.time_stretcher(units, types_, bounds, durations)
    from seq2seq_vc_amd.ops import kernels_vocoder as KV
    wav = model(units, lp)
    direct = model.vocoder(stretched)
    n_out = z[f"{name}/stretched"].shape[-1]
    res.append((tuple(wav.shape) == (1, 1, n_out * up) and torch.equal(wav, direct) and bool(torch.isfinite(wav).all()) and float(wav.std()) > 0,
                f"forward: waveform {tuple(wav.shape)} bit-equal to generator(stretched): {torch.equal(wav, direct)}; std {float(wav.std()):.3f}"))
    # batched: rows of different lengths, NaN in the padding of log_probs and units
    lens = [T, 77, 40]
    ub = units.repeat(3, 1, 1).clone()
    lb = lp.repeat(3, 1, 1).clone()
    for b, n in enumerate(lens):
        ub[b, :, n:] = float("nan")
        lb[b, n:] = float("nan")
    counts = {}
    for B in (1, 3):
        calls = []
        orig = {k: getattr(KV, k) for k in ("hifigan_input", "hifigan_conv1d", "hifigan_tconv1d", "hifigan_conv_out")}
        try:
            for k, fn in orig.items():
                setattr(KV, k, (lambda fn: lambda *a, **kw: (calls.append(1), fn(*a, **kw))[1])(fn))
            before = KU.LAUNCHES
            wavs = model.convert_batch(ub[:B], lb[:B], torch.tensor(lens[:B], dtype=torch.int32).to(DEV))
            counts[B] = (KU.LAUNCHES - before, len(calls))
        finally:
            for k, fn in orig.items():
                setattr(KV, k, fn)
    res.append((counts[1] == counts[3] and counts[1][0] == 3 and counts[1][1] == len(model.vocoder.launch_plan()),
                f"launches of convert_batch (search + stretch, vocoder): B = 1 {counts[1]}, B = 3 {counts[3]}"))
    for b, n in enumerate(lens):
        single = model(units[:, :, :n], lp[:, :n])
        same = tuple(wavs[b].shape) == tuple(single.view(-1).shape) and torch.equal(wavs[b], single.view(-1))
        res.append((same, f"convert_batch row {b} ({n} frames -> {tuple(wavs[b].shape)[0]} samples) equals forward() of the row bit for bit: {same}"))
    return res


CASES = [search_chunk_edges_in_T, search_unit_counts, search_piecewise_fixture, search_rounding_family, search_ties, search_ragged_batch,
         stretch_segments_vs_interpolate, stretch_global_ratios, stretch_batch_rows_equal_single_calls, urhythmic_fine_end_to_end]
