#!/usr/bin/env python3
"""Timing of urhythmic on the HIP kernels: Segmenter.segment_batch and UrhythmicFine.convert_batch.

    python tools/bench_urhythmic.py [--repeats 5] [--target-s 0.25] [--no-cpu]

Two shapes -- one utterance of 500 frames (10 s at 50 Hz) and a batch of 16 x 750 frames -- with K = 100 units, D = 256 and the
HiFi-GAN generator in its default configuration (seeded weights, fp32).  Per shape: ms per call of segment_batch (two launches and
the one host read), of its two kernels alone (span scores; span scores + search, no host read), of convert_batch (search, host
durations through scipy, stretch, vocoder) and of the vocoder alone on the stretched units.  Device events around back-to-back calls,
warmed; `repeats` timed groups of about `target-s` seconds; median [min, max] over the groups.  Beside it, once, as context: the numpy
restatement of the search (tests/urhythmic_ref.py) on ONE CPU thread at 1 x 500 -- a restatement in Python, NOT the reference's
numba-JIT routine, which is not installed here and was not run.  No speed bar: there is no earlier implementation to compare with.
Prints ONE JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 500), (16, 750)]
K, D, GAMMA = 100, 256, 2.0


def timed_group(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(fn, repeats, target_s):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    iters = max(2, math.ceil(target_s * 1e3 / max(timed_group(fn, 2), 1e-3)))
    ts = [timed_group(fn, iters) for _ in range(repeats)]
    return {"ms_per_call": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "calls_per_group": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.25)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    import urhythmic_ref as UR
    import vocoder_ref as VR
    from seq2seq_vc_amd import _lib
    from seq2seq_vc_amd import urhythmic as U
    from seq2seq_vc_amd.ops import kernels_urhythmic as KU
    from seq2seq_vc_amd.ops.kernels import ptr, stream
    from seq2seq_vc_amd.vocoder import HifiganGenerator

    dev = "cuda:0"
    labels = UR.default_labels(K)
    seg = U.Segmenter(gamma=GAMMA)
    seg.load_state_dict({"n_clusters_": 3, "labels_": torch.from_numpy(labels.astype(np.int64)), "n_leaves_": K, "n_features_in_": D,
                         "children_": torch.zeros(K - 1, 2, dtype=torch.int64),
                         "sound_types": {c: getattr(U, n) for c, n in UR.SOUND_TYPE_OF_CLUSTER.items()}})
    rm = U.RhythmModelFineGrained()
    rm.load_state_dict({"source": {getattr(U, n): v for n, v in UR.RHYTHM_SOURCE.items()},
                        "target": {getattr(U, n): v for n, v in UR.RHYTHM_TARGET.items()}})
    gen = HifiganGenerator(in_channels=D)
    gen.load_state_dict(VR.seed_state_dict(gen.state_dict(), seed=5))
    gen.to(dev)
    model = U.UrhythmicFine(seg, rm, U.TimeStretcherFineGrained(), gen)

    res = {"metric": f"urhythmic on HIP, K = {K} units, D = {D}, gamma = {GAMMA}, HiFi-GAN default configuration, fp32", "repeats": a.repeats,
           "timed": "device events around back-to-back calls; median [min, max] over the repeats", "shapes": {}}
    for B, T in SHAPES:
        lp = torch.from_numpy(np.stack([UR.piecewise_log_probs(T, K, seed=100 + b) for b in range(B)])).to(dev)
        units = torch.randn(B, T, D, generator=torch.Generator().manual_seed(B)).to(dev).transpose(1, 2)      # what encode() returns
        lens = torch.full((B,), T, dtype=torch.int32).to(dev)
        labels_d = torch.from_numpy(labels).to(dev)
        ws = torch.empty(_lib.lib().s2svc_useg_ws_bytes(B, T, K) // 8 + 1, dtype=torch.int64, device=dev)
        _, rows = seg.segment_batch(lp, lens)
        plan_rows = []
        for clusters, bounds in rows:
            types_ = [seg.sound_types[c] for c in clusters]
            plan_rows.append((types_, bounds, rm(types_, bounds)))
        stretched, totals = model.time_stretcher.stretch_batch(units, plan_rows)
        out_lens = torch.tensor(totals, dtype=torch.int32).to(dev)
        before = KU.LAUNCHES
        wavs = model.convert_batch(units, lp, lens)
        entry = {"utterances": B, "frames": T, "segments_per_row_after_merge": statistics.mean(len(c) for c, _ in rows),
                 "frames_after_stretch": totals[:4], "samples_row_0": int(wavs[0].numel()), "search_and_stretch_launches_per_call": KU.LAUNCHES - before,
                 "vocoder_launches_per_call": len(gen.launch_plan()), "workspace_MB": ws.numel() * 8 / 1e6}
        legs = {
            "span_scores_kernel": lambda: _lib.check(_lib.lib().s2svc_useg_spans(B, T, K, ptr(lp), ptr(lens), ptr(ws), stream()), "spans"),
            "search_kernels_no_host_read": lambda: KU.useg_segment(lp, lens, GAMMA, labels=labels_d),
            "segment_batch": lambda: seg.segment_batch(lp, lens),
            "stretch_kernel": lambda: model.time_stretcher.stretch_batch(units, plan_rows),
            "vocoder_forward_batch": lambda: gen.forward_batch(stretched, out_lens, host_lens=totals),
            "convert_batch": lambda: model.convert_batch(units, lp, lens),
        }
        for name, fn in legs.items():
            entry[name] = measure(fn, a.repeats, a.target_s)
        t0 = time.perf_counter()
        for types_, bounds, _ in plan_rows:
            rm(types_, bounds)
        entry["host_durations_scipy_ms"] = (time.perf_counter() - t0) * 1e3
        entry["search_share_of_convert_batch"] = entry["segment_batch"]["ms_per_call"] / entry["convert_batch"]["ms_per_call"]
        res["shapes"][f"{B}x{T}"] = entry
        if (B, T) == SHAPES[0]:
            first_row = rows[0]
    if not a.no_cpu:
        torch.set_num_threads(1)
        lp = UR.piecewise_log_probs(500, K, seed=100)
        t0 = time.perf_counter()
        want = UR.segment_all(lp, GAMMA, labels)
        res["cpu_numpy_restatement_one_thread_1x500_s"] = time.perf_counter() - t0
        res["gpu_equals_restatement_1x500"] = bool(first_row[0] == want["clusters"].tolist() and first_row[1] == want["cboundaries"].tolist())
        res["cpu_leg_is"] = "the numpy restatement of tests/urhythmic_ref.py (Python loops over numpy rows), not the reference's numba-JIT routine"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
