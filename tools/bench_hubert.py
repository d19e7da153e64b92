#!/usr/bin/env python3
"""Timing of the HuBERT-Soft content encoder on the HIP kernels: urhythmic.model.encode, and the map-free attention kernel alone.

    python tools/bench_hubert.py [--repeats 5] [--target-s 0.2] [--out profiles/hubert_bench.json]

Workloads: encode() of 1 x 10 s, 1 x 30 s (1500 frames) and 16 x 5 s of 16 kHz audio with HubertSoft at its upstream sizes (seeded
weights), in fp32 and bf16 compute.  The opponent is the yardstick of tests/hubert_ref.py -- upstream's architecture in stock torch
modules -- on the same card with the same weights, under torch.autocast(bfloat16) for the bf16 rows.  Beside it the attention kernel
alone (bf16, H = 12, dk = 64, one utterance): T = 500 against the one-launch attention map with its second product (csrc/attn_map.hip),
T = 1500 against what the package ran beyond 512 keys before (scores GEMM, softmax launch, P.V GEMM through memory).  Device events
around back-to-back calls, warmed; `repeats` timed groups of about `target-s` seconds; median [min, max] over the groups.  A row is
"WINS" / "LOSES" when the two [min, max] intervals do not overlap, else "within the spread".  Prints ONE JSON line (and writes --out)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = [("1x10s", 1, 160000), ("1x30s", 1, 480000), ("16x5s", 16, 80000)]


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


def verdict(ours, theirs):
    if ours["ms_max"] < theirs["ms_min"]:
        return "WINS"
    if ours["ms_min"] > theirs["ms_max"]:
        return "LOSES"
    return "within the spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import hubert_ref as HR
    from seq2seq_vc_amd.ops import functional as Fn
    from seq2seq_vc_amd.ops import functional_attn as FAttn
    from seq2seq_vc_amd.ops import kernels_hubert as KH
    from seq2seq_vc_amd.urhythmic import model as UM
    from seq2seq_vc_amd.urhythmic.hubert import HubertSoft

    dev = "cuda:0"
    yard = HR.seeded(12)
    mine = HubertSoft()
    mine.load_state_dict(yard.state_dict())
    mine.to(dev).eval()
    yard.to(dev)
    res = {"metric": "urhythmic.model.encode with HubertSoft (upstream sizes, seeded weights) on HIP against the stock-torch yardstick, same card",
           "repeats": a.repeats, "timed": "device events around back-to-back calls; median [min, max] over the repeats", "encode": {}, "attention": {}}
    for name, B, N in WORKLOADS:
        wav = (torch.randn(B, 1, N, generator=torch.Generator().manual_seed(N)) * 0.3).to(dev)
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            Fn.set_compute_dtype(dtype)
            try:
                units, lp = UM.encode(mine, wav)
                ours = measure(lambda: UM.encode(mine, wav), a.repeats, a.target_s)
            finally:
                Fn.set_compute_dtype(torch.float32)

            def stock():
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                    return HR.encode(yard, wav)
            u_ref, lp_ref = stock()
            theirs = measure(stock, a.repeats, a.target_s)
            res["encode"][f"{name}_{tag}"] = {
                "utterances": B, "samples": N, "frames": int(units.shape[2]), "launches_per_call": len(mine.launch_plan("model.encode", dtype=dtype)),
                "hip": ours, "stock_torch": theirs, "speedup": theirs["ms_per_call"] / ours["ms_per_call"], "verdict": verdict(ours, theirs),
                "max_abs_units_difference": float((units - u_ref.float()).abs().max()), "max_abs_units": float(u_ref.float().abs().max())}
    H, D = 12, 768
    for T, rival in ((500, "attn_map forward with its second product"), (1500, "scores GEMM + softmax + P.V GEMM")):
        qkv = (torch.randn(1, T, 3 * D, generator=torch.Generator().manual_seed(T))).to(dev).to(torch.bfloat16)
        qkv[..., :D] *= 3.0
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        out = torch.empty(1, T, D, dtype=torch.bfloat16, device=dev)
        with torch.no_grad():
            ours = measure(lambda: KH.attn_flash_fwd(q, k, v, H, None, out=out), a.repeats, a.target_s)
            theirs = measure(lambda: FAttn._attn_fwd_views(q, k, v, None, False, H, 0.0), a.repeats, a.target_s)
            other = FAttn._attn_fwd_views(q, k, v, None, False, H, 0.0)[0]
        res["attention"][f"T{T}_H{H}_dk64_bf16"] = {"flash": ours, "rival": rival, "rival_time": theirs, "speedup": theirs["ms_per_call"] / ours["ms_per_call"],
                                                    "verdict": verdict(ours, theirs), "max_abs_difference": float((out.float() - other.float()).abs().max())}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
