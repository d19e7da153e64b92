"""Host-side checks of AASVC.inference_batch (no GPU): the float64 restatements of tests/aasvc_batch_ref.py against stock torch and the
reference's rule, the lengths of the two fixtures, the C ABI of the new launchers and the supported set of the fused inference core."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aasvc_batch_ref as AR
import abi_header
from seq2seq_vc_amd import _lib

NEW = ("s2svc_convmod_infer", "s2svc_convmod_infer_supported", "s2svc_durations_finalize", "s2svc_interp_nearest_rows")


@pytest.mark.parametrize("shape,vlens", AR.CONVMOD_CASES, ids=[f"{s}-{'full' if v is None else v}" for s, v in AR.CONVMOD_CASES])
def test_fused_core_restatement_equals_stock_torch_on_the_cropped_row(shape, vlens):
    B, Tn, C, ks = shape
    p = AR.convmod_problem(shape, seed=7)
    y2 = p["y2"].clone()
    if vlens is not None:
        for b in range(B):
            y2[b, vlens[b]:] = float("nan")          # never touched
    out = AR.convmod_infer_ref(y2, p["w"], p["bias"], p["mean"], p["var"], p["gamma"], p["beta"], p["eps"], vlens)
    d = lambda t: t.double()
    for b in range(B):
        L = Tn if vlens is None else vlens[b]
        x = F.glu(d(p["y2"][b, :L]).t()[None], dim=1)
        x = F.conv1d(x, d(p["w"]), d(p["bias"]), padding=(ks - 1) // 2, groups=C)
        x = F.batch_norm(x, d(p["mean"]), d(p["var"]), d(p["gamma"]), d(p["beta"]), training=False, eps=p["eps"])
        x = (x * torch.sigmoid(x))[0].t()
        assert x.shape == (L, C)
        assert float((out[b, :L] - x).abs().max()) <= 1e-12 * max(1.0, float(x.abs().max())), (b, L)
        assert (out[b, L:] == 0).all() and torch.isfinite(out[b]).all()


def _reference_rule(d_row):
    """modules/length_regulator.py:127-135 on the single-utterance tensor (1, Tx), after the clamp of models/aas_vc.py:393."""
    d_outs = torch.clamp(torch.as_tensor(d_row)[None], max=AR.MAX_DP_OUTPUT)
    ds = d_outs.float().clone()
    if ds.sum() == 0:
        ds[ds.sum(dim=1).eq(0)] = 1
    return d_outs[0].numpy(), ds[0].numpy(), int(ds.sum())


@pytest.mark.parametrize("dtype", [np.float32, np.int64])
def test_durations_finalize_restatement_equals_the_reference_rule_row_by_row(dtype):
    rows = [[3, 0, 11, 10, 2, 0, 1], [0, 0, 0, 0], [12], [0], [0, 5, 0]]
    Tx = max(len(r) for r in rows)
    d = np.full((len(rows), Tx), 7, dtype)                # padding entries hold 7: they must come out 0
    for b, r in enumerate(rows):
        d[b, :len(r)] = r
    lens = [len(r) for r in rows]
    d_outs, ds, total = AR.durations_finalize_ref(d, lens)
    assert d_outs.dtype == dtype and ds.dtype == np.float32 and total.dtype == np.int32
    for b, r in enumerate(rows):
        want_d, want_ds, want_total = _reference_rule(np.asarray(r, dtype))
        assert np.array_equal(d_outs[b, :lens[b]], want_d) and np.array_equal(ds[b, :lens[b]], want_ds) and total[b] == want_total, b
        assert (d_outs[b, lens[b]:] == 0).all() and (ds[b, lens[b]:] == 0).all()
    assert total.tolist() == [3 + 10 + 10 + 2 + 1, 4, 10, 1, 5]


@pytest.mark.parametrize("name", AR.FIXTURES)
def test_fixture_lengths_are_the_test(name):
    cfg, z = AR.load(name)
    res = AR.fixture_conditions(cfg, z)
    assert all(ok for ok, _ in res), "\n".join(m for ok, m in res if not ok)
    assert ("in.sdp_noise" in z.files) == (cfg["duration_predictor_type"] == "stochastic")
    sd = AR.state_dict_of(cfg)
    assert any(k.startswith("duration_predictor.") for k in sd) and not [k for k in z.files if k.startswith("sd.")]
    assert os.path.getsize(os.path.join(AR.GOLD, name + ".npz")) < 256 * 1024


def test_header_declares_and_the_library_exports_the_new_launchers():
    header, declared, L = abi_header.text(), abi_header.declared(), abi_header.library()
    for n in NEW:
        assert n in declared, f"{n} not declared in include/s2svc_hip.h"
        assert n in _lib._FUNCTIONS and n in _lib.exported_symbols(), f"{n} missing from the ctypes binding"
        assert hasattr(L, n), f"{n} not exported by the library"
    assert "convmod_infer.hip" in _lib.sources()
    assert "replaces: modules/conformer/convolution.py:68-75" in header and "modules/length_regulator.py:127-135" in header


def test_aasvc_has_inference_batch():
    from seq2seq_vc_amd import models as M
    import inspect
    sig = inspect.signature(M.AASVC.inference_batch)
    assert list(sig.parameters)[:6] == ["self", "xs", "ilens", "dp_inputs", "dplens", "spembs"]


def test_supported_table_of_the_fused_inference_core():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_library(verbose=False)
    L = _lib.lib()
    for C in (32, 128, 384, 1536):
        for ks in (7, 15, 31):
            assert L.s2svc_convmod_infer_supported(C, ks) == 1, (C, ks)
    for C, ks in ((30, 7), (32, 8), (384, 14), (384, 33), (0, 7), (32, 0), (32, -1)):
        assert L.s2svc_convmod_infer_supported(C, ks) == 0, (C, ks)


def test_per_row_lens_reach_the_time_mixing_modules_only_when_asked():
    """modules.Lens.per_row: crop_dev / rows_dev give the per-row vector; a plain Lens keeps giving None (existing paths unchanged)."""
    from seq2seq_vc_amd import modules as Mo
    plain = Mo.Lens([5, 3], "cpu")
    rows = plain.per_row()
    assert Mo.crop_dev(plain) is None and Mo.rows_dev(plain) is None and Mo.crop_dev(None) is None and Mo.rows_dev(None) is None
    assert Mo.crop_dev(rows).tolist() == [5, 3] and Mo.rows_dev(rows).tolist() == [5, 3]
    half = rows.map(lambda v: v // 2).clamp(2)
    assert half.rows and half.host == (2, 1) and not plain.map(lambda v: v // 2).rows
