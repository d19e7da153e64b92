#!/usr/bin/env python3
"""Timing of urhythmic on the HIP kernels: Segmenter.segment_batch and UrhythmicFine.convert_batch.

    python tools/bench_urhythmic.py [--repeats 5] [--target-s 0.25] [--no-cpu] [--dtype fp32|bf16] [--no-wavs]

Two shapes -- one utterance of 500 frames (10 s at 50 Hz) and a batch of 16 x 750 frames -- with K = 100 units, D = 256 and the
HiFi-GAN generator in its default configuration (seeded weights, fp32).  Per shape: ms per call of segment_batch (two launches and
the one host read), of its two kernels alone (span scores; span scores + search, no host read), of convert_batch (search, host
durations through scipy, stretch, vocoder) and of the vocoder alone on the stretched units.  Device events around back-to-back calls,
warmed; `repeats` timed groups of about `target-s` seconds; median [min, max] over the groups.  Beside it, once, as context: the numpy
restatement of the search (tests/urhythmic_ref.py) on ONE CPU thread at 1 x 500 -- a restatement in Python, NOT the reference's
numba-JIT routine, which is not installed here and was not run.

The three plans of convert_batch: "host" (the leg `convert_batch`: durations through scipy per segment, the code before the duration
table existed) is the opponent; `convert_batch_table` replaces the scipy calls by the rhythm model's duration table in the same host
loop; `convert_batch_device` keeps the segment tables on the device (`plan_kernel`: ops.kernels_urhythmic.useg_plan alone).  Each
comparison gets a verdict from the medians and the [min, max] of the timed groups: WINS / LOSES when the two ranges do not overlap,
"within the spread" otherwise.  `duration_table_build_ms`: the host build of the table, once per model.  `convert_wavs` (waveform in,
plan "device") against `encode_batch_then_convert_batch_host` on a HuBERT-Soft at its upstream sizes (seeded weights, noise as input;
a rhythm model with 40 x wider distributions, since a seeded HuBERT's segments are as long as they like).  --dtype bf16 sets the
compute dtype of HuBERT-Soft and the vocoder; search, plan and stretch are fp32 / integer either way.  Prints ONE JSON line."""
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


def verdict(mine, opponent):
    """`mine` against `opponent` (two results of measure): the medians, and whether the [min, max] ranges of the timed groups overlap."""
    if mine["ms_max"] < opponent["ms_min"]:
        word = "WINS"
    elif mine["ms_min"] > opponent["ms_max"]:
        word = "LOSES"
    else:
        word = "within the spread"
    return {"verdict": word, "ms": mine["ms_per_call"], "range": [mine["ms_min"], mine["ms_max"]], "opponent_ms": opponent["ms_per_call"],
            "opponent_range": [opponent["ms_min"], opponent["ms_max"]], "ratio_of_medians": opponent["ms_per_call"] / mine["ms_per_call"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.25)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--no-wavs", action="store_true", help="skip the waveform-to-waveform legs (they build a full-size HuBERT-Soft)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import urhythmic_ref as UR
    import vocoder_ref as VR
    from seq2seq_vc_amd import _lib
    from seq2seq_vc_amd import urhythmic as U
    from seq2seq_vc_amd.ops import functional as Fn
    from seq2seq_vc_amd.ops import kernels_urhythmic as KU
    from seq2seq_vc_amd.ops.kernels import ptr, stream
    from seq2seq_vc_amd.vocoder import HifiganGenerator

    dev = "cuda:0"
    Fn.set_compute_dtype(torch.float32 if a.dtype == "fp32" else torch.bfloat16)
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
    t0 = time.perf_counter()
    table = rm.duration_table(seg.sound_types, KU.MAX_T)
    table_build_ms = (time.perf_counter() - t0) * 1e3
    table_d, silence = model._device_table(dev)
    if not a.no_wavs:
        import hubert_ref as HR
        hubert = U.HubertSoft()
        hubert.load_state_dict(HR.seeded(12).state_dict())
        hubert = hubert.to(dev).eval()
        wide = U.RhythmModelFineGrained()
        wide.load_state_dict({side: {getattr(U, n): (k, loc, 40 * scale) for n, (k, loc, scale) in d.items()}
                              for side, d in (("source", UR.RHYTHM_SOURCE), ("target", UR.RHYTHM_TARGET))})
        model_w = U.UrhythmicFine(seg, wide, U.TimeStretcherFineGrained(), gen)

    res = {"metric": f"urhythmic on HIP, K = {K} units, D = {D}, gamma = {GAMMA}, HiFi-GAN default configuration, {a.dtype}", "dtype": a.dtype,
           "repeats": a.repeats, "timed": "device events around back-to-back calls; median [min, max] over the repeats",
           "duration_table_build_ms": table_build_ms, "duration_table_shape": list(table.shape), "shapes": {}}
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
        tables = seg.segment_tables(lp, lens)
        before = KU.LAUNCHES
        wavs_host = model.convert_batch(units, lp, lens)
        entry = {"utterances": B, "frames": T, "segments_per_row_after_merge": statistics.mean(len(c) for c, _ in rows),
                 "frames_after_stretch": totals[:4], "samples_row_0": int(wavs_host[0].numel()), "search_and_stretch_launches_per_call": KU.LAUNCHES - before,
                 "vocoder_launches_per_call": len(gen.launch_plan()), "workspace_MB": ws.numel() * 8 / 1e6}
        legs = {
            "span_scores_kernel": lambda: _lib.check(_lib.lib().s2svc_useg_spans(B, T, K, ptr(lp), ptr(lens), ptr(ws), stream()), "spans"),
            "search_kernels_no_host_read": lambda: KU.useg_segment(lp, lens, GAMMA, labels=labels_d),
            "segment_batch": lambda: seg.segment_batch(lp, lens),
            "stretch_kernel": lambda: model.time_stretcher.stretch_batch(units, plan_rows),
            "vocoder_forward_batch": lambda: gen.forward_batch(stretched, out_lens, host_lens=totals),
            "convert_batch": lambda: model.convert_batch(units, lp, lens),
            "plan_kernel": lambda: KU.useg_plan(tables["clusters"], tables["cboundaries"], tables["ncl"], table_d, silence),
            "convert_batch_table": lambda: model.convert_batch(units, lp, lens, plan="table"),
            "convert_batch_device": lambda: model.convert_batch(units, lp, lens, plan="device"),
        }
        if not a.no_wavs:
            wavs = (0.3 * torch.randn(B, 1, T * 320, generator=torch.Generator().manual_seed(7 + B))).to(dev)
            wav_lens = [T * 320] * B

            def parts_host():
                u, l, fl = U.encode_batch(hubert, wavs, wav_lens)
                return model_w.convert_batch(u, l, fl, plan="host")
            legs["encode_batch_then_convert_batch_host"] = parts_host
            legs["convert_wavs"] = lambda: U.convert_wavs(hubert, model_w, wavs, wav_lens)
            try:
                entry["convert_wavs_equals_its_parts"] = all(torch.equal(x, y) for x, y in zip(parts_host(), legs["convert_wavs"]()))
            except (OverflowError, ValueError, KeyError) as e:     # a segment the rhythm model cannot map: reported, not timed
                entry["convert_wavs_error"] = repr(e)
                del legs["encode_batch_then_convert_batch_host"], legs["convert_wavs"]
        for plan in ("table", "device"):
            before = KU.LAUNCHES
            same = all(torch.equal(x, y) for x, y in zip(wavs_host, model.convert_batch(units, lp, lens, plan=plan)))
            entry[f"plan_{plan}_launches_per_call"] = KU.LAUNCHES - before
            entry[f"plan_{plan}_equals_plan_host_bit_for_bit"] = same
        for name, fn in legs.items():
            entry[name] = measure(fn, a.repeats, a.target_s)
        entry["verdicts"] = {"convert_batch_table vs convert_batch": verdict(entry["convert_batch_table"], entry["convert_batch"]),
                             "convert_batch_device vs convert_batch": verdict(entry["convert_batch_device"], entry["convert_batch"]),
                             "convert_batch_device vs convert_batch_table": verdict(entry["convert_batch_device"], entry["convert_batch_table"])}
        if "convert_wavs" in entry:
            entry["verdicts"]["convert_wavs vs encode_batch_then_convert_batch_host"] = verdict(entry["convert_wavs"], entry["encode_batch_then_convert_batch_host"])
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
