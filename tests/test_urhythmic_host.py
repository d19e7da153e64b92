"""Host-side checks of urhythmic (no GPU): the numpy restatement of the segmentation search against the fixture recorded from the
reference, the rounding family, the host bookkeeping of the segmenter, rhythm model and time stretchers, the refusals and the C ABI."""

import numpy as np
import pytest
import torch

import urhythmic_ref as UR
from seq2seq_vc_amd import urhythmic as U
from seq2seq_vc_amd.ops import kernels_urhythmic as KU
from seq2seq_vc_amd.urhythmic.stretcher import segment_table, stretch_plan

GOLD = UR.load_golden()
KEYS = ("alpha", "P", "codes", "boundaries", "clusters", "cboundaries")
SOUND = {c: getattr(U, n) for c, n in UR.SOUND_TYPE_OF_CLUSTER.items()}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))     # as bits
    return a.shape == b.shape and np.array_equal(a, b)


def test_fixture_holds_the_inputs_the_generator_describes():
    inputs = UR.fixture_inputs()
    assert [n for n, _, _ in inputs] == list(GOLD)
    for name, lp, gamma in inputs:
        assert _same(GOLD[name]["lp"], lp) and float(GOLD[name]["gamma"]) == gamma, name
        assert np.array_equal(GOLD[name]["labels"], UR.default_labels(lp.shape[1])), name
    assert max(g["lp"].shape[0] for g in GOLD.values()) == 130 and max(g["lp"].shape[1] for g in GOLD.values()) == 129
    assert {float(g["gamma"]) for g in GOLD.values()} >= {2.0, 0.7}


@pytest.mark.parametrize("name", list(GOLD))
def test_restatement_equals_the_fixture(name):
    g = GOLD[name]
    got = UR.segment_all(g["lp"], float(g["gamma"]), g["labels"])
    for k in KEYS:
        assert _same(got[k], g[k].astype(got[k].dtype) if g[k].dtype.kind != "f" else g[k]), f"{name}: {k} differs from the reference's"


def test_rounding_family_separates_the_float32_running_maximum_from_a_plain_argmax():
    names = [n for n in GOLD if n.startswith("rounding_")]
    assert len(names) == 16
    for n in names:
        g = GOLD[n]
        assert g["lp"].shape == (6, 2) and float(g["gamma"]) == 0.7
        plain = UR.search_tables(g["lp"], 0.7, rule="argmax")[1]
        assert not np.array_equal(plain, g["P"]), f"{n}: a plain float64 argmax gives the reference's back-pointers: the input no longer tells them apart"
        assert _same(UR.search_tables(g["lp"], 0.7, rule="argmax")[0], g["alpha"]), f"{n}: alpha is float32(max c) under either rule"


def test_tie_inputs_do_tie():
    g = GOLD["tie_twin_columns"]
    assert np.array_equal(g["lp"][:, 5], g["lp"][:, 2]) and (g["codes"] == 2).any() and not (g["codes"] == 5).any()
    g = GOLD["tie_all_equal"]
    assert (g["codes"] == 0).all()
    g = GOLD["tie_across_s_flat"]
    assert np.array_equal(g["boundaries"], np.arange(67))          # equal candidates: the first one (s = 0) stays


def test_module_cluster_merge_is_the_references():
    for name in ("piecewise_130x129_g2", "tie_across_s_flat", "single_frame"):
        g = GOLD[name]
        cl, cb = U.cluster_merge(type("C", (), {"labels_": g["labels"]}), g["codes"][g["boundaries"][:-1]], g["boundaries"])
        assert np.array_equal(cl, g["clusters"]) and np.array_equal(cb, g["cboundaries"])


def _segmenter(K=100):
    s = U.Segmenter(num_clusters=3, gamma=2)
    s.load_state_dict({"n_clusters_": 3, "labels_": torch.from_numpy(UR.default_labels(K).astype(np.int64)), "n_leaves_": K, "n_features_in_": 256,
                       "children_": torch.zeros(K - 1, 2, dtype=torch.int64), "sound_types": dict(SOUND)})
    return s


def test_segmenter_state_dict_round_trip():
    s = _segmenter()
    sd = s.state_dict()
    assert list(sd) == ["n_clusters_", "labels_", "n_leaves_", "n_features_in_", "children_", "sound_types"]
    assert isinstance(sd["labels_"], torch.Tensor) and isinstance(sd["children_"], torch.Tensor)
    s2 = U.Segmenter()
    s2.load_state_dict(sd)
    sd2 = s2.state_dict()
    assert torch.equal(sd2["labels_"], sd["labels_"]) and torch.equal(sd2["children_"], sd["children_"])
    assert sd2["sound_types"] == SOUND and sd2["n_leaves_"] == 100 and sd2["n_features_in_"] == 256 and sd2["n_clusters_"] == 3
    with pytest.raises(RuntimeError):
        U.Segmenter(num_clusters=4).load_state_dict(sd)
    assert (U.Segmenter().gamma, U.Segmenter().clustering.n_clusters) == (2, 3)


def test_segmenter_cluster_fits_sklearn_agglomerative():
    pytest.importorskip("sklearn")
    from sklearn.cluster import AgglomerativeClustering
    codebook = np.random.default_rng(0).standard_normal((40, 6))
    s = U.Segmenter(num_clusters=3)
    s.cluster(codebook)
    want = AgglomerativeClustering(n_clusters=3).fit(codebook)
    sd = s.state_dict()
    assert np.array_equal(sd["labels_"].numpy(), want.labels_) and np.array_equal(sd["children_"].numpy(), want.children_)
    assert sd["n_clusters_"] == 3 and sd["n_leaves_"] == 40 and sd["n_features_in_"] == 6


def test_segmenter_identify():
    s = _segmenter()
    # cluster 2 lies on the marked silence, cluster 0 on the voiced frames
    segments, boundaries = [2, 0, 1, 0, 2], [0, 10, 30, 40, 60, 70]
    silences = np.zeros(71, bool)
    silences[:10] = silences[61:] = True
    voiced = np.zeros(71, bool)
    voiced[12:30] = voiced[42:60] = True
    assert s.identify([(segments, boundaries, silences, voiced)]) == {2: U.SILENCE, 0: U.SONORANT, 1: U.OBSTRUENT}
    s.clustering.n_clusters_ = 4
    with pytest.raises(ValueError):
        s.identify([])


def _rhythm_model():
    rm = U.RhythmModelFineGrained()
    rm.load_state_dict({"source": {getattr(U, n): v for n, v in UR.RHYTHM_SOURCE.items()},
                        "target": {getattr(U, n): v for n, v in UR.RHYTHM_TARGET.items()}})
    return rm


def _stretch_gold():
    return np.load(UR.GOLDEN_STRETCH)


def test_sound_types():
    assert [t.name for t in U.SoundType] == ["VOWEL", "APPROXIMANT", "NASAL", "FRICATIVE", "STOP", "SILENCE"]
    assert U.SONORANT == U.SoundType.VOWEL | U.SoundType.APPROXIMANT | U.SoundType.NASAL
    assert U.OBSTRUENT == U.SoundType.FRICATIVE | U.SoundType.STOP and U.SILENCE == U.SoundType.SILENCE


def test_rhythm_model_durations_and_segment_rate_equal_the_fixture():
    pytest.importorskip("scipy")
    z, rm = _stretch_gold(), _rhythm_model()
    assert rm.hop_rate == 0.02
    for name in z["names"]:
        g = GOLD[str(name)]
        types_, bounds = [SOUND[int(c)] for c in g["clusters"]], [int(v) for v in g["cboundaries"]]
        assert rm(types_, bounds) == z[f"{name}/durations"].tolist()
        assert U.segment_rate(types_, bounds) == float(z[f"{name}/segment_rate"])
    sd = rm.state_dict()
    assert set(sd) == {"source", "target"} and sd["source"][U.SONORANT.value] == (2.2, 0.045)


def test_rhythm_model_fit_ignores_short_silences():
    pytest.importorskip("scipy")
    rm = U.RhythmModelFineGrained(hop_length=160, sample_rate=16000)
    utts = [([U.SONORANT, U.SILENCE, U.OBSTRUENT, U.SILENCE], [0, 5, 8, 12, 30]), ([U.SONORANT, U.OBSTRUENT, U.SONORANT, U.SILENCE], [0, 7, 9, 21, 29])]
    tally = rm._tally_durations(utts)
    assert np.allclose(tally[U.SILENCE], [0.18, 0.08]) and np.allclose(tally[U.SONORANT], [0.05, 0.07, 0.12]) and np.allclose(tally[U.OBSTRUENT], [0.04, 0.02])
    fit = rm._fit(utts)
    assert set(fit) == {U.SONORANT, U.OBSTRUENT, U.SILENCE} and all(len(v) == 3 and v[1] == 0 for v in fit.values())
    rm.fit_source(utts)
    rm.fit_target(utts)
    assert set(rm.state_dict()) == {"source", "target"}


def test_stretch_plan_applies_both_filters_and_matches_the_fixture_lengths():
    z = _stretch_gold()
    for name in z["names"]:
        g = GOLD[str(name)]
        types_, bounds = [SOUND[int(c)] for c in g["clusters"]], [int(v) for v in g["cboundaries"]]
        plan = stretch_plan(types_, bounds, z[f"{name}/durations"].tolist())
        assert sum(d for _, _, d in plan) == z[f"{name}/stretched"].shape[-1]
        assert all(d > 0 and n > 0 for _, n, d in plan)
        # the CPU yardstick on the same plan is the reference's output, bit for bit
        want = UR.interpolate_segments(torch.from_numpy(z[f"{name}/units"][0]), plan, torch.float32)
        assert np.array_equal(want.numpy(), z[f"{name}/stretched"][0])
    S, O, Z = U.SONORANT, U.OBSTRUENT, U.SILENCE
    # silences of <= 3 frames vanish BEFORE the durations are paired up; a duration of 0 (or below) drops its segment
    plan = stretch_plan([S, Z, O, Z, S], [0, 4, 7, 9, 13, 20], [6, 0, 5, -1])
    assert plan == [(0, 4, 6), (9, 4, 5)]
    seg, nsegs, totals = segment_table([plan, [], [(2, 3, 4)]], "cpu")
    assert totals == [11, 0, 4] and nsegs.tolist() == [2, 0, 1] and seg.dtype == torch.int32 and tuple(seg.shape) == (3, 2, 4)
    assert seg[0].tolist() == [[0, 4, 6, 0], [9, 4, 5, 6]] and seg[2, 0].tolist() == [2, 3, 4, 0]


def test_new_entry_points_are_declared_bound_and_exported():
    import abi_header
    from seq2seq_vc_amd import _lib
    names = ["s2svc_useg_ws_bytes", "s2svc_useg_spans", "s2svc_useg_search", "s2svc_useg_stretch"]
    header, declared, L = abi_header.text(), abi_header.declared(), abi_header.library()
    for n in names:
        assert n in declared, f"{n} missing from the header"
        assert n in _lib._FUNCTIONS and n in _lib.exported_symbols(), f"{n} missing from the ctypes binding"
        assert hasattr(L, n), f"{n} not exported by the library"
    assert "urhythmic.hip" in _lib.sources()
    assert "K <= 256" in header and "Tmax <= 4096" in header
    assert L.s2svc_useg_ws_bytes(2, 100, 100) >= 2 * 100 * 100 * 6
    # bad arguments are refused by the entry points themselves, before any launch
    assert L.s2svc_useg_spans(1, 8, 257, None, None, None, None) == -1 and b"K > 256" in L.s2svc_last_error()
    assert L.s2svc_useg_search(1, 4097, 2.0, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"4096" in L.s2svc_last_error()
    assert L.s2svc_useg_stretch(2, 1, 4, 4, None, 0, 0, 0, None, None, 1, 4, 0.0, None, None) == -1


def test_launcher_argument_checks_raise_without_a_gpu_call():
    before = KU.LAUNCHES
    lens = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="units"):
        KU.useg_segment(torch.zeros(1, 4, 257), lens, 2.0)
    with pytest.raises(ValueError, match="frames"):
        KU.useg_segment(torch.zeros(1, 4097, 2), lens, 2.0)
    with pytest.raises(ValueError):
        KU.useg_segment(torch.zeros(4, 3), lens, 2.0)
    with pytest.raises(ValueError):
        KU.useg_segment(torch.zeros(1, 4, 3, dtype=torch.float64), lens, 2.0)
    with pytest.raises(ValueError, match="lens"):
        KU.useg_segment(torch.zeros(2, 4, 3), lens, 2.0)
    with pytest.raises(ValueError, match="lens"):
        KU.useg_segment(torch.zeros(1, 4, 3), lens.long(), 2.0)
    with pytest.raises(ValueError, match="labels"):
        KU.useg_segment(torch.zeros(1, 4, 3), lens, 2.0, labels=torch.zeros(4, dtype=torch.int32))
    seg, nsegs = torch.zeros(1, 1, 4, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="units"):
        KU.useg_stretch(torch.zeros(1, 8, 5, dtype=torch.float16), seg, nsegs, 4)
    with pytest.raises(ValueError, match="seg"):
        KU.useg_stretch(torch.zeros(1, 8, 5), seg.long(), nsegs, 4)
    with pytest.raises(ValueError, match="seg"):
        KU.useg_stretch(torch.zeros(2, 8, 5), seg, nsegs, 4)
    with pytest.raises(ValueError, match="nsegs"):
        KU.useg_stretch(torch.zeros(1, 8, 5), seg, torch.ones(2, dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        U.TimeStretcherGlobal()(torch.zeros(1, 8, 5), 0.1)
    with pytest.raises(ValueError):
        U.TimeStretcherFineGrained().stretch_batch(torch.zeros(1, 8, 5), [([U.SONORANT], [0, 9], [4])])      # a segment past the units
    with pytest.raises(ValueError):
        _segmenter(100).segment_batch(torch.zeros(1, 4, 50), lens)                                            # K differs from the clustering's
    assert KU.LAUNCHES == before
