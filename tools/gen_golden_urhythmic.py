"""Generate tests/golden/urhythmic_search.npz and urhythmic_stretch.npz by IMPORTING the reference's urhythmic/segmenter.py,
rhythm_model.py and stretcher.py.

Runs only where the reference tree exists (never on the GPU box).  The reference's search is numba-JIT; numba is not installed, so a
stand-in `numba` module whose njit() returns the function unchanged is put in sys.modules first and the routine runs as plain Python
over numpy scalars.  `gamma` is passed as np.float64, so that numpy's promotion (float32 + float64 -> float64, the store rounds to
float32) equals numba's typing of the same lines.  Parity unpinned in numba's typing (numba is not installed; its promotion rule is
restated by the cast).

Recorded for every input of tests/urhythmic_ref.fixture_inputs(): the input, alpha, P, codes, boundaries, and the merged clusters and
boundaries for a fixed labels_; for the first two inputs also the target durations of a fixed pair of gamma dictionaries and the
stretched units (D = 8).

    python tools/gen_golden_urhythmic.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("S2SVC_REFERENCE", "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import urhythmic_ref as UR  # noqa: E402


def import_reference():
    nb = types.ModuleType("numba")
    nb.njit = lambda *a, **k: (lambda f: f)
    sys.modules["numba"] = nb
    sys.path.insert(0, REF)
    import seq2seq_vc.urhythmic.rhythm_model as R
    import seq2seq_vc.urhythmic.segmenter as S
    import seq2seq_vc.urhythmic.stretcher as St
    import seq2seq_vc.urhythmic.utils as U
    return S, R, St, U


def main():
    S, R, St, U = import_reference()
    arrays, names = {}, []
    segmented = {}
    for name, lp, gamma in UR.fixture_inputs():
        labels = UR.default_labels(lp.shape[1])
        alpha, P = S._segment(lp, np.float64(gamma))
        assert alpha.dtype == np.float32 and P.dtype == np.int32
        codes, boundaries = S._backtrack(alpha, P)
        clusters, cboundaries = S.cluster_merge(types.SimpleNamespace(labels_=labels), codes[boundaries[:-1]], boundaries)
        rec = dict(lp=lp, gamma=np.float64(gamma), labels=labels, alpha=alpha, P=P, codes=codes, boundaries=boundaries,
                   clusters=clusters.astype(np.int32), cboundaries=cboundaries)
        names.append(name)
        arrays.update({f"{name}/{k}": v for k, v in rec.items()})
        segmented[name] = rec
        print(f"{name}: T {lp.shape[0]}, K {lp.shape[1]}, gamma {gamma}: {len(boundaries) - 1} segments, {len(clusters)} after the merge")
    arrays["names"] = np.array(names)
    out = UR.GOLDEN
    np.savez_compressed(out, **arrays)
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.0f} KiB)")

    # rhythm model and time stretcher on the first two inputs
    sound = {c: getattr(U, n) for c, n in UR.SOUND_TYPE_OF_CLUSTER.items()}
    rm = R.RhythmModelFineGrained()
    rm.load_state_dict({"source": {getattr(U, n): v for n, v in UR.RHYTHM_SOURCE.items()},
                        "target": {getattr(U, n): v for n, v in UR.RHYTHM_TARGET.items()}})
    stretch, seen_short, seen_zero = {}, 0, 0
    for i, name in enumerate(names[:2]):
        rec = segmented[name]
        types_ = [sound[int(c)] for c in rec["clusters"]]
        bounds = [int(v) for v in rec["cboundaries"]]
        durations = rm(types_, bounds)
        units = torch.from_numpy(UR.fixture_units(rec["lp"].shape[0], seed=31 + i))
        stretched = St.TimeStretcherFineGrained()(units, types_, bounds, durations)
        short = sum(1 for c, a, b in zip(rec["clusters"], bounds[:-1], bounds[1:]) if c == 2 and b - a <= 3)
        print(f"{name}: {len(types_)} clusters, {short} short silences dropped, {len(durations)} durations, {sum(d <= 0 for d in durations)} of them "
              f"<= 0, {bounds[-1]} -> {stretched.shape[-1]} frames, segment rate {R.segment_rate(types_, bounds):.4f}")
        seen_short, seen_zero = seen_short + short, seen_zero + sum(d <= 0 for d in durations)
        stretch.update({f"{name}/units": units.numpy(), f"{name}/durations": np.array(durations, np.int64), f"{name}/stretched": stretched.numpy(),
                        f"{name}/segment_rate": np.float64(R.segment_rate(types_, bounds))})
    assert seen_short > 0 and seen_zero > 0, "the fixture must exercise both filters"
    for ratio in (0.5, 1.0, 1.37):
        units = torch.from_numpy(UR.fixture_units(37, seed=41))
        stretch[f"global/{ratio}"] = St.TimeStretcherGlobal()(units, ratio).numpy()
    stretch["names"] = np.array(names[:2])
    out = UR.GOLDEN_STRETCH
    np.savez_compressed(out, **stretch)
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.0f} KiB)")
    total = os.path.getsize(UR.GOLDEN) + os.path.getsize(UR.GOLDEN_STRETCH)
    assert total < 200 * 1024, f"fixtures too large: {total} bytes"


if __name__ == "__main__":
    main()
