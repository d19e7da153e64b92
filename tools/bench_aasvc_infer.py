#!/usr/bin/env python3
"""Timing of AAS-VC inference (seq2seq_vc_amd/models/aas_vc.py): one padded batch through AASVC.inference_batch against the same
utterances one at a time through AASVC.inference.

    python tools/bench_aasvc_infer.py [--repeats 5] [--target-s 0.12] [--out profiles/aasvc_infer_bench.json]

Configuration: AAS-VC vc2 (bench.AASVC_VC2, 157 M parameters), seeded init, eval().  Input: 16 utterances of 128-256 frames drawn as in
SURVEY section 8(d) (ilens = randint(128, 257), ilens[0] = 256, xs = randn, dp_inputs = xs), and one utterance of 256 frames.  The draw of
the stochastic duration predictor is fixed and injected into every call (row b of the batch and single call b get the same columns), so
that all legs predict the same durations and produce the same number of frames.  fp32 and bf16, per leg:
    batch            one inference_batch call on the 16 utterances
    batch_unfused    the same with S2SVC_NO_CONVMOD_INFER=1 (the convolution modules on their separate launches)
    singles          16 inference calls (the path this library had before inference_batch; unchanged by it)
    one_batch / one_single    1 x 256 frames through both methods
ms_per_call: device events around back-to-back calls, warmed (3 calls), `repeats` timed groups of about `target-s` seconds each, the legs
alternated, median and min / max over the groups.  Every call ends with its result on the device; inference_batch reads B ints back in
the middle (the output's size), inference stops the stream twice.  launches: calls into the HIP library during one call (ATen's own
launches -- casts, the slices of the single path -- are not in it).  Prints ONE JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 1234


def timed_group(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def count_launches(fn):
    from seq2seq_vc_amd import _lib
    real, n = _lib.check, [0]

    def counting(rc, what):
        n[0] += 1
        return real(rc, what)

    _lib.check = counting
    try:
        fn()
    finally:
        _lib.check = real
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from seq2seq_vc_amd import models as M
    from seq2seq_vc_amd.ops import functional as Fn
    dev = "cuda"
    torch.manual_seed(SEED)
    model = M.AASVC(**bench.AASVC_VC2).to(dev).eval()
    pr = bench.AASVC_VC2["post_encoder_reduction_factor"]
    g = torch.Generator().manual_seed(SEED)
    B = 16
    ilens = torch.randint(128, 257, (B,), generator=g)
    ilens[0] = 256
    xs = torch.randn(B, 256, 80, generator=g)
    for b in range(B):
        xs[b, ilens[b]:] = 0
    noise = torch.randn(B, 2, 256 // pr, generator=g).to(dev)
    xs = xs.to(dev)
    rows = [xs[b, : int(ilens[b])].contiguous() for b in range(B)]
    noises = [noise[b:b + 1, :, : int(ilens[b]) // pr].contiguous() for b in range(B)]
    sdp = model.duration_predictor

    def batch(idx, dtype, fused=True):
        x, il, n = xs[idx].contiguous(), ilens[idx], noise[idx].contiguous()
        x, n = x[:, : int(il.max())].contiguous(), n[:, :, : int(il.max()) // pr].contiguous()

        def run():
            Fn.set_compute_dtype(dtype)
            if not fused:
                os.environ["S2SVC_NO_CONVMOD_INFER"] = "1"
            try:
                sdp.noise = n
                return model.inference_batch(x, il, dp_inputs=x)
            finally:
                os.environ.pop("S2SVC_NO_CONVMOD_INFER", None)
                Fn.set_compute_dtype(torch.float32)
        return run

    def singles(idx, dtype):
        def run():
            Fn.set_compute_dtype(dtype)
            try:
                out = []
                for b in idx:
                    sdp.noise = noises[b]
                    out.append(model.inference(rows[b], dp_input=rows[b]))
                return out
            finally:
                Fn.set_compute_dtype(torch.float32)
        return run

    every, first = list(range(B)), [0]
    res = {"metric": "AAS-VC vc2 inference, seeded init, 16 utterances of 128-256 frames (SURVEY 8(d)) and 1 x 256", "repeats": a.repeats,
           "timed": "device events around back-to-back calls; median [min, max] over the repeats, legs alternated",
           "ilens": ilens.tolist(), "dtypes": {}}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        legs = {"batch": batch(every, dtype), "batch_unfused": batch(every, dtype, fused=False), "singles": singles(every, dtype),
                "one_batch": batch(first, dtype), "one_batch_unfused": batch(first, dtype, fused=False), "one_single": singles(first, dtype)}
        iters, times = {}, {k: [] for k in legs}
        for k, fn in legs.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[k] = max(2, math.ceil(a.target_s * 1e3 / timed_group(fn, 2)))
        for _ in range(a.repeats):
            for k, fn in legs.items():
                times[k].append(timed_group(fn, iters[k]))
        outs, olens, _ = legs["batch"]()
        single_frames = [int(o[0].shape[0]) for o in legs["singles"]()]
        entry = {"frames_out_batch": olens.tolist(), "frames_out_singles": single_frames,
                 "audio_seconds": float(olens.sum()) * bench.HOP / bench.SR}
        for k, ts in times.items():
            med = statistics.median(ts)
            n_utt = 1 if k.startswith("one") else B
            entry[k] = {"ms_per_call": med, "ms_min": min(ts), "ms_max": max(ts), "calls_per_group": iters[k], "utterances": n_utt,
                        "hip_library_launches": count_launches(legs[k])}
        entry["batch_vs_singles_speedup"] = entry["singles"]["ms_per_call"] / entry["batch"]["ms_per_call"]
        entry["fused_core_vs_separate_launches_speedup"] = entry["batch_unfused"]["ms_per_call"] / entry["batch"]["ms_per_call"]
        entry["one_fused_core_vs_separate_launches_speedup"] = entry["one_batch_unfused"]["ms_per_call"] / entry["one_batch"]["ms_per_call"]
        entry["one_batch_vs_one_single_speedup"] = entry["one_single"]["ms_per_call"] / entry["one_batch"]["ms_per_call"]
        entry["rtf_batch"] = entry["batch"]["ms_per_call"] * 1e-3 / entry["audio_seconds"]
        res["dtypes"][name] = entry
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
