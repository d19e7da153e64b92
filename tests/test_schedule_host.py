"""Host side of the gradient batches (ops.kernels.GradBatch / recording / disjoint_waves): no GPU and no built library needed.

The expected waves below are literals.  They were obtained by running the three wave loops of the commit before the single helper
(flush_grouped, flush_colreduce, conv1d_wgrad_grouped) on the same lists, their launches replaced by recorders."""
import types

import pytest

from seq2seq_vc_amd.ops import kernels as K

# (C, a_rowsum) of weight-gradient GEMMs, (out_sum, out_dot) of column reductions, dw of Conv1d weight gradients
GEMMS = [(10, None), (20, 21), (10, None), (30, 21), (40, None), (10, 41), (50, 40), (20, None)]
GEMM_WAVES = [[(10, None), (20, 21), (40, None)], [(10, None), (30, 21), (50, 40), (20, None)], [(10, 41)]]
REDUCTIONS = [(1, 2), (3, None), (2, None), (4, 1), (3, 5), (6, None), (1, None)]
REDUCTION_WAVES = [[(1, 2), (3, None), (6, None)], [(2, None), (4, 1), (3, 5)], [(1, None)]]
CONV1D = [7, 8, 7, 9, 7, 8]
CONV1D_WAVES = [[7, 8, 9], [7, 8], [7]]


def _pair(t):
    return {t[0]} | ({t[1]} if t[1] else set())


def _waves_of_objects(pairs):
    """The pairs as distinct objects (the flushes pass descriptors, and equal descriptors must stay apart) -> waves of pairs."""
    items = [types.SimpleNamespace(pair=p) for p in pairs]
    waves = list(K.disjoint_waves(items, lambda it: _pair(it.pair)))
    assert sorted(id(it) for w in waves for it in w) == sorted(id(it) for it in items)      # every item exactly once
    return [[it.pair for it in w] for w in waves]


def test_waves_are_those_of_the_three_loops_they_replace():
    assert _waves_of_objects(GEMMS) == GEMM_WAVES
    assert _waves_of_objects(REDUCTIONS) == REDUCTION_WAVES
    assert [list(w) for w in K.disjoint_waves(CONV1D, lambda dw: {dw})] == CONV1D_WAVES


def test_conflicting_items_take_successive_waves_in_their_order():
    assert _waves_of_objects([(5, None)] * 3) == [[(5, None)], [(5, None)], [(5, None)]]
    assert _waves_of_objects([(5, None), (6, None), (5, None), (6, None)]) == [[(5, None), (6, None)], [(5, None), (6, None)]]


def test_disjoint_items_share_the_first_wave_in_their_order():
    assert _waves_of_objects([(3, 4), (1, None), (2, 9)]) == [[(3, 4), (1, None), (2, 9)]]


def test_an_empty_list_gives_no_wave():
    assert list(K.disjoint_waves([], lambda it: {it})) == []


def test_an_item_with_two_addresses_conflicts_through_either():
    assert _waves_of_objects([(1, 2), (1, 3)]) == [[(1, 2)], [(1, 3)]]            # through C / out_sum
    assert _waves_of_objects([(1, 2), (3, 2)]) == [[(1, 2)], [(3, 2)]]            # through a_rowsum / out_dot
    assert _waves_of_objects([(1, 2), (2, None)]) == [[(1, 2)], [(2, None)]]      # one's second address is the other's first


def test_an_inner_batch_restores_the_outer_one():
    assert K._BATCH is None and not K.in_capped_batch()
    outer, inner = K.GradBatch(cap=64), K.GradBatch()
    with K.recording(outer) as got:
        assert got is outer and K._BATCH is outer and K.in_capped_batch()
        with K.recording(inner):
            assert K._BATCH is inner and not K.in_capped_batch()
        assert K._BATCH is outer
        with pytest.raises(ZeroDivisionError):
            with K.recording(inner):
                1 / 0
        assert K._BATCH is outer
    assert K._BATCH is None
    with pytest.raises(ZeroDivisionError):
        with K.recording(outer):
            1 / 0
    assert K._BATCH is None
    assert (outer.gemms, outer.colreduces, outer.conv1d, outer.cap, inner.cap) == ([], [], [], 64, 0)
