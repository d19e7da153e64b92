"""Host-side checks of the rhythm model's duration table (no GPU): every entry against the scalar scipy path it replaces,
durations_from_table against __call__, the cache, and the numpy restatement of the plan kernel (tests/urhythmic_plan_ref.py) against
the host code that ships.  Every comparison is equality of integers."""
import numpy as np
import pytest
import torch

pytest.importorskip("scipy")

import urhythmic_plan_ref as PR
import urhythmic_ref as UR
from seq2seq_vc_amd import urhythmic as U
from seq2seq_vc_amd.ops import kernels_urhythmic as KU
from seq2seq_vc_amd.urhythmic import rhythm_model as RM
from seq2seq_vc_amd.urhythmic.rhythm_model import transform
from seq2seq_vc_amd.urhythmic.stretcher import segment_table, stretch_plan

SOUND = PR.SOUND
N_CHECKED = 300


def _scalar(rm, sound_type, n):
    """The per-segment path of __call__ for one segment of n frames: (duration, None) or (None, the exception's type)."""
    try:
        return round(transform(rm.source[sound_type.value], rm.target[sound_type.value], rm.hop_rate * np.int64(n)) / rm.hop_rate), None
    except (OverflowError, ValueError) as e:
        return None, type(e)


def test_table_entries_equal_the_scalar_path():
    rm = PR.rhythm_model()
    table = rm.duration_table(SOUND, N_CHECKED)
    assert RM.UNMAPPED == -2**31 and table.dtype == np.int32 and table.shape == (3, N_CHECKED + 1)
    first_unmapped = {}
    for c, sound_type in SOUND.items():
        for n in range(1, N_CHECKED + 1):
            want, raised = _scalar(rm, sound_type, n)
            if raised is None:
                assert table[c, n] == want, f"{sound_type} {n} frames: table {table[c, n]}, scalar path {want}"
            else:
                assert table[c, n] == RM.UNMAPPED, f"{sound_type} {n} frames: the scalar path raises {raised.__name__}, table {table[c, n]}"
                first_unmapped.setdefault(c, n)
    # derived from the scalar path above, not assumed: every type of the fixture stops being mappable inside the checked range
    assert set(first_unmapped) == set(SOUND), f"first unmapped length per cluster: {first_unmapped}"
    for c, n in first_unmapped.items():
        assert (table[c, n:] == RM.UNMAPPED).all() and (table[c, :n] != RM.UNMAPPED).all()
    # the fixture's obstruent target maps short segments to no frame at all: the stretcher's second filter has work to do
    assert (table[PR.OBSTRUENT_ID, 1:8] == 0).all() and table[PR.OBSTRUENT_ID, 8] > 0
    # the table the conversion uses is the same one, longer
    full = rm.duration_table(SOUND, KU.MAX_T)
    assert full.shape == (3, KU.MAX_T + 1) and np.array_equal(full[:, :N_CHECKED + 1], table) and (full[:, N_CHECKED:] == RM.UNMAPPED).all()


def test_table_of_another_hop_rate_and_parameter_set():
    rm = U.RhythmModelFineGrained(hop_length=256, sample_rate=22050)
    rm.load_state_dict({"source": {U.SONORANT: (3.1, 0.0, 0.02), U.OBSTRUENT: (1.7, 0.0, 0.05), U.SILENCE: (0.9, 0.0, 0.3)},
                        "target": {U.SONORANT: (2.4, 0.0, 0.03), U.OBSTRUENT: (2.2, 0.0, 0.03), U.SILENCE: (1.2, 0.0, 0.2)}})
    table = rm.duration_table(SOUND, 120)
    for c, sound_type in SOUND.items():
        for n in range(1, 121):
            want, raised = _scalar(rm, sound_type, n)
            assert table[c, n] == (want if raised is None else RM.UNMAPPED), (sound_type, n)


def _random_rows(count, seed, edge_every=2):
    rng = np.random.default_rng(seed)
    return [PR.random_row(rng, int(rng.integers(0, 30)), edge=i % edge_every == 0) for i in range(count)]


def test_durations_from_table_equal_call():
    rm = PR.rhythm_model()
    table = rm.duration_table(SOUND, KU.MAX_T)
    seen = set()
    for clusters, bounds in _random_rows(100, seed=11):
        types_ = [SOUND[c] for c in clusters]
        want = rm(types_, bounds) if types_ else []
        assert rm.durations_from_table(table, clusters, bounds) == want
        seen |= {(c, n) for c, n in zip(clusters, np.diff(bounds).tolist())}
    assert {(PR.SILENCE_ID, 3), (PR.SILENCE_ID, 4)} <= seen and {(PR.OBSTRUENT_ID, n) for n in range(1, 9)} <= seen


def test_durations_from_table_raise_what_call_raises():
    rm = PR.rhythm_model()
    table = rm.duration_table(SOUND, KU.MAX_T)
    clusters, bounds = [PR.OBSTRUENT_ID, PR.SONORANT_ID, PR.SILENCE_ID], [0, 10, 105, 110]      # a sonorant of 95 frames
    with pytest.raises(Exception) as host:
        rm([SOUND[c] for c in clusters], bounds)
    assert host.type is OverflowError
    with pytest.raises(host.type, match=str(host.value)):
        rm.durations_from_table(table, clusters, bounds)
    with pytest.raises(ValueError, match="duration_table"):
        rm.durations_from_table(table.copy(), clusters, bounds)          # not the model's own table


def test_cache_and_its_invalidation():
    rm = PR.rhythm_model()
    table = rm.duration_table(SOUND, 64)
    assert rm.duration_table(dict(SOUND), 64) is table and not table.flags.writeable
    longer = rm.duration_table(SOUND, 65)
    assert longer is not table and rm.durations_from_table(longer, [0], [0, 5]) == rm([U.SONORANT], [0, 5])
    with pytest.raises(ValueError, match="duration_table"):
        rm.durations_from_table(table, [0], [0, 5])                       # one table is kept: the last one built
    assert np.array_equal(rm.duration_table(SOUND, 64), table)
    rm.load_state_dict({"target": {getattr(U, n): (a, loc, 2 * scale) for n, (a, loc, scale) in UR.RHYTHM_TARGET.items()}})
    fresh = rm.duration_table(SOUND, 64)
    assert fresh is not table and not np.array_equal(fresh, table)
    with pytest.raises(ValueError, match="duration_table"):
        rm.durations_from_table(table, [0], [0, 5])                       # a table from before the change
    utts = [([U.SONORANT, U.SILENCE, U.OBSTRUENT, U.SILENCE], [0, 5, 8, 12, 30]), ([U.SONORANT, U.OBSTRUENT, U.SONORANT, U.SILENCE], [0, 7, 9, 21, 29])]
    for fit in (rm.fit_source, rm.fit_target):
        before = rm.duration_table(SOUND, 64)
        fit(utts)
        assert rm.duration_table(SOUND, 64) is not before


def test_missing_distribution_gives_an_unmapped_row():
    rm = PR.rhythm_model(target={n: v for n, v in UR.RHYTHM_TARGET.items() if n != "OBSTRUENT"})
    table = rm.duration_table(SOUND, 50)
    assert (table[PR.OBSTRUENT_ID] == RM.UNMAPPED).all() and (table[PR.SONORANT_ID, :50] != RM.UNMAPPED).all()
    with pytest.raises(KeyError):
        rm([U.OBSTRUENT], [0, 9])
    with pytest.raises(KeyError):
        rm.durations_from_table(table, [PR.OBSTRUENT_ID], [0, 9])
    # a cluster id without a sound type: its row exists and is unmapped
    sparse = PR.rhythm_model().duration_table({0: U.SONORANT, 2: U.SILENCE}, 50)
    assert sparse.shape == (3, 51) and (sparse[1] == RM.UNMAPPED).all()
    assert (U.RhythmModelFineGrained().duration_table(SOUND, 10) == RM.UNMAPPED).all()       # nothing fitted or loaded


def test_filters_that_disagree_are_refused():
    # hop * n > 3 * hop and n > 3 agree for every positive finite hop rate (hop * 3 is one product, hop * 4 is exact); a hop rate of
    # zero is where they part: no duration exceeds 3 * 0, so __call__ drops every silence and the stretcher only the short ones
    rm = U.RhythmModelFineGrained(hop_length=0)
    with pytest.raises(ValueError, match="disagree at 4 frames"):
        rm.duration_table(SOUND, 16)
    for hop, rate in ((320, 16000), (200, 16000), (256, 22050), (300, 24000), (256, 24000)):
        assert U.RhythmModelFineGrained(hop, rate).duration_table(SOUND, KU.MAX_T).shape == (3, KU.MAX_T + 1)


def test_restatement_of_the_plan_kernel_equals_the_host_code():
    rm = PR.rhythm_model()
    table = rm.duration_table(SOUND, KU.MAX_T)
    rows = _random_rows(200, seed=23, edge_every=3)
    Tmax = max(max(b[-1] for _, b in rows), max(len(c) for c, _ in rows), 1)
    clusters, cboundaries, ncl = PR.pack_rows(rows, Tmax, fill=(0x7fffffff, -5))
    seg, nsegs, totals, status = PR.plan_rows(clusters, cboundaries, ncl, table, PR.SILENCE_ID)
    assert not status.any()
    plans = [stretch_plan([SOUND[c] for c in cl], cb, rm([SOUND[c] for c in cl], cb) if cl else []) for cl, cb in rows]
    want_seg, want_nsegs, want_totals = segment_table(plans, "cpu")
    smax = want_seg.shape[1]
    assert np.array_equal(seg[:, :smax], want_seg.numpy()) and not seg[:, smax:].any()
    assert np.array_equal(nsegs, want_nsegs.numpy()) and totals.tolist() == want_totals
    assert (nsegs == 0).any() and (nsegs < ncl).any() and nsegs.max() > 10
    # the flags of the restatement: an unmapped length, a malformed row, a total beyond int32
    cl, cb, n = PR.pack_rows([([0], [0, 95]), ([7], [0, 5]), ([0, 1], [0, 5, 5]), ([0], [0, 60])], 100)
    assert PR.plan_rows(cl, cb, n, table[:, :101], PR.SILENCE_ID)[3].tolist() == [1, 2, 2, 0]
    cl2, cb2, n2 = PR.pack_rows([([0, 1, 0], [0, 60, 70, 130])], 130)
    big = np.array(table[:, :131])
    big[0, 60] = 2**31 - 1
    seg, nsegs, totals, status = PR.plan_rows(cl2, cb2, n2, big, PR.SILENCE_ID)
    assert status.tolist() == [3] and nsegs.tolist() == [0] and totals.tolist() == [0] and not seg.any()


def test_plan_launcher_argument_checks_raise_without_a_gpu_call():
    before = KU.LAUNCHES
    cl, cb, n = (torch.from_numpy(a) for a in PR.pack_rows([([0], [0, 5])], 8))
    table = torch.zeros(3, 9, dtype=torch.int32)
    with pytest.raises(ValueError, match="clusters"):
        KU.useg_plan(cl.long(), cb, n, table, 2)
    with pytest.raises(ValueError, match="cboundaries"):
        KU.useg_plan(cl, cb[:, :-1].contiguous(), n, table, 2)
    with pytest.raises(ValueError, match="ncl"):
        KU.useg_plan(cl, cb, torch.zeros(2, dtype=torch.int32), table, 2)
    with pytest.raises(ValueError, match="table"):
        KU.useg_plan(cl, cb, n, table.float(), 2)
    with pytest.raises(ValueError, match="frames"):
        KU.useg_plan(torch.zeros(1, 4097, dtype=torch.int32), torch.zeros(1, 4098, dtype=torch.int32), n, table, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        KU.useg_plan(cl, cb, n, table, 2)
    model = U.UrhythmicFine(U.Segmenter(), PR.rhythm_model(), U.TimeStretcherFineGrained(), None)
    with pytest.raises(ValueError, match="plan"):
        model.convert_batch(torch.zeros(1, 8, 5), torch.zeros(1, 5, 3), [5], plan="gpu")
    assert KU.LAUNCHES == before


def test_plan_entry_point_is_declared_bound_and_refuses_bad_arguments():
    import abi_header
    from seq2seq_vc_amd import _lib
    L = abi_header.library()
    assert "s2svc_useg_plan" in abi_header.declared() and "s2svc_useg_plan" in _lib.exported_symbols() and hasattr(L, "s2svc_useg_plan")
    nulls = (None,) * 4
    assert L.s2svc_useg_plan(1, 4097, 3, 10, *nulls, 2, 3, *nulls, None) == -1 and b"4096" in L.s2svc_last_error()
    assert L.s2svc_useg_plan(65536, 8, 3, 10, *nulls, 2, 3, *nulls, None) == -1 and b"65535" in L.s2svc_last_error()
    assert L.s2svc_useg_plan(1, 8, 3, 10, *nulls, 2, 3, *nulls, None) == -1 and b"null" in L.s2svc_last_error()
    assert L.s2svc_useg_plan(1, 8, 0, 10, *nulls, 2, 3, *nulls, None) == -1 and b"shape" in L.s2svc_last_error()


def _fine(sound_types=None):
    seg = U.Segmenter()
    seg.sound_types = dict(SOUND if sound_types is None else sound_types)
    return U.UrhythmicFine(seg, PR.rhythm_model(), U.TimeStretcherFineGrained(), None)


def test_rows_the_plan_kernel_flags_raise_as_documented():
    """UrhythmicFine._refuse_plan on host copies of the tables (it only reads them): the error path of plan="device"."""
    model = _fine()
    rows = [([PR.SONORANT_ID, PR.OBSTRUENT_ID], [0, 9, 20]), ([PR.OBSTRUENT_ID, PR.SONORANT_ID, PR.SILENCE_ID], [0, 10, 105, 110])]
    tables = dict(zip(("clusters", "cboundaries", "ncl"), (torch.from_numpy(a) for a in PR.pack_rows(rows, 110))))
    with pytest.raises(OverflowError):                                    # status 1 on the row with the 95-frame sonorant: the host path's own
        model._refuse_plan(tables, np.array([0, 1], np.int32))
    with pytest.raises(RuntimeError, match="row 0.*disagree"):            # status 1 on a row the host path maps
        model._refuse_plan(tables, np.array([1, 0], np.int32))
    with pytest.raises(ValueError, match="row 1.*malformed"):
        model._refuse_plan(tables, np.array([0, 2], np.int32))
    with pytest.raises(ValueError, match="row 0.*2\\^31"):
        model._refuse_plan(tables, np.array([3, 1], np.int32))            # the first flagged row decides
    unknown = dict(tables, clusters=tables["clusters"].clone())
    unknown["clusters"][0, 0] = 5
    with pytest.raises(KeyError):                                         # a cluster without a sound type: the host path's KeyError
        model._refuse_plan(unknown, np.array([1, 0], np.int32))


def test_plan_device_alone_needs_a_single_silence_cluster():
    two = _fine({0: U.SONORANT, 1: U.SILENCE, 2: U.SILENCE})
    with pytest.raises(ValueError, match="plan=\"device\""):
        two._device_table("cpu")
    table = two.rhythm_model.duration_table(two.segmenter.sound_types, 40)           # what plan="table" uses: no such limit
    assert two.rhythm_model.durations_from_table(table, [1, 0, 2], [0, 3, 9, 14]) == two.rhythm_model([U.SILENCE, U.SONORANT, U.SILENCE], [0, 3, 9, 14])
    with pytest.raises(ValueError, match="plan=\"device\""):
        _fine({})._device_table("cpu")
    dev_table, silence = _fine()._device_table("cpu")
    assert silence == PR.SILENCE_ID and dev_table.dtype == torch.int32 and tuple(dev_table.shape) == (3, KU.MAX_T + 1)
    assert _fine({0: U.SONORANT, 1: U.OBSTRUENT})._device_table("cpu")[1] == -1
