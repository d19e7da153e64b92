"""Host side of the one-launch refresh of the derived weight copies: the path and the work units the library plans for a job
(s2svc_derived_refresh_plan, host arithmetic, no device), and the registry the cached getters fill."""
import os

import pytest
import torch

from seq2seq_vc_amd import _lib
from seq2seq_vc_amd.ops import kernels as K

ELEMENT, TILE, SLAB, TCONV = 0, 1, 2, 3
BF16, F32 = torch.bfloat16, torch.float32


class _Stub:
    """What ops.kernels.derived_jobs reads of a tensor: an address and a shape (the plan dereferences nothing)."""

    def __init__(self, shape=()):
        self.shape = shape

    def data_ptr(self):
        return 256


def _plan(gathers=(), tconvs=()):
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library(verbose=False)
    return K.derived_refresh_plan([(_Stub(), (n, st, off, dt), _Stub()) for n, st, off, dt in gathers],
                                  [(_Stub((O, C, 3, 3)), _Stub()) for O, C in tconvs])


def _cdiv(a, b):
    return -(-a // b)


def test_plan_of_the_vtn_copies():
    """The copies of a full-size VTN step: all of them go through LDS, and the units are the tiles the kernel walks."""
    got = _plan([((384, 9, 384), (3456, 1, 9), 0, BF16),            # Conv2d taps (O, 9, C)
                 ((384, 19, 384), (7296, 1, 19), 0, BF16),          # permuted Linear (D, F, C)
                 ((19, 384, 384), (1, 19, 7296), 0, BF16),          # ... its data-gradient layout (F, C, D)
                 ((512, 5, 80), (400, 1, 5), 0, BF16),              # Conv1d forward (O, k, C)
                 ((80, 5, 512), (5, -1, 400), 4, BF16)],            # Conv1d flipped (C, k, O)
                [(384, 384)])
    # slab chunks: 256 columns x 9 floats, 128 x 19, and the 80 columns of the Postnet's last layer in one chunk of 128
    assert got == [(SLAB, 384 * 2), (SLAB, 384 * 3), (TILE, 114 * 6), (SLAB, 512), (TILE, _cdiv(400, 64) * 8), (TCONV, 54 * 6)]


@pytest.mark.parametrize("n, st, off, path, units", [
    ((64, 9, 32), (288, 1, 9), 0, SLAB, 64),                        # one partial chunk of 64 columns per slab
    ((3, 40, 70), (2800, 1, 40), 7, SLAB, 3 * 2),                   # 128 columns x 40 floats do not fit the LDS tile: chunks of 64
    ((5, 3, 300), (900, 1, 3), 0, SLAB, 5),                         # chunks of 512: no larger than n2 needs
    ((2, 3, 1100), (3300, 1, 3), 0, SLAB, 2 * 2),                   # chunks of 1024, the largest
    ((1536, 3, 1536), (4608, 1, 3), 0, SLAB, 1536 * 2),
    ((3, 70, 70), (4900, 1, 70), 0, TILE, 4 * 2),                   # a per-slab transpose whose 64 columns do not fit a slab: tiles
    ((3, 70, 70), (4900, 2, 70), 0, ELEMENT, _cdiv(3 * 70 * 70, 4096)),   # no unit-stride row index and s2 < s0
    ((130, 3, 200), (3, 1, 390), 0, TILE, 7 * 4),
    ((19, 40, 24), (1, 19, 760), 0, ELEMENT, _cdiv(19 * 40 * 24, 4096)),  # n2 < 32
    ((48, 5, 80), (5, -1, 240), 4, TILE, 4 * 2),
    ((7, 3, 5), (15, 5, 1), 0, ELEMENT, 1),
])
def test_plan_paths_and_units(n, st, off, path, units):
    assert _plan([(n, st, off, F32)]) == [(path, units)]


def test_plan_class_matrices_and_bad_jobs():
    assert _plan(tconvs=[(64, 32), (32, 64), (40, 24), (32, 1)]) == [(TCONV, 5), (TCONV, 9), (TCONV, 4), (TCONV, 1)]
    with pytest.raises(RuntimeError, match="bad job"):
        _plan([((0, 3, 5), (15, 5, 1), 0, F32)])
    assert _plan() == []


def test_registry_keeps_class_jobs_beside_the_gathers():
    """PermRegistry stays the list of (weight, gather3 key, buffer) triples; the class matrices have a list of their own."""
    reg = K.PermRegistry()
    assert list(reg) == [] and reg.tconv == [] and reg.covered is None and reg.tconv_covered is None
    reg.append(("w", "key", "buf"))
    other = K.PermRegistry()
    other.tconv.append(("w", "buf"))
    assert len(reg) == 1 and reg.tconv == [] and len(other) == 0 and len(other.tconv) == 1
