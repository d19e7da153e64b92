#!/usr/bin/env python3
"""Timing of the Griffin-Lim vocoder (seq2seq_vc_amd/vocoder/griffin_lim.py): linear spectrogram -> waveform, 64 iterations,
n_fft 1024 / hop 256.

    python tools/bench_griffin_lim.py [--repeats 5] [--target-s 0.25] [--leg-timeout 240] [--no-torch] [--no-cpu]

Two shapes a user runs -- one utterance of 300 frames and a batch of 16 x 150 frames.  Per shape: ms_per_call of the HIP path and of
the comparison leg, the same loop written with stock torch.stft / torch.istft ON THE SAME CARD (tests/griffin_lim_ref.py:
torch_griffin_lim).  Device events around back-to-back calls, warmed; `repeats` timed groups of about `target-s` seconds per leg,
HIP and torch groups alternated; median [min, max] over the groups.  Every leg warms up first in a child process of its own under
`leg-timeout` seconds (first-use library initialisation happens there); a leg whose child fails or times out is reported as
unavailable and is not run here.  The CPU float64 numpy restatement (one utterance, what the reference's librosa path does on one
thread) is timed once as context.  The bar: HIP is not slower than the torch leg beyond the larger min-max spread of the two.
Prints ONE JSON line."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 300), (16, 150)]
N_FFT, HOP, N_ITER, FS = 1024, 256, 64, 16000


def inputs(device):
    import numpy as np
    import torch

    import griffin_lim_ref as GR
    out = {}
    for B, T in SHAPES:
        rows = []
        for b in range(B):
            y = GR.make_signal((T - 1) * HOP / FS + 0.001, FS, seed=b)
            rows.append(np.abs(GR.stft(y, N_FFT, HOP))[:T])
        S = torch.from_numpy(np.stack(rows).astype(np.float32))
        u = torch.rand(S.shape, generator=torch.Generator().manual_seed(B))
        out[(B, T)] = (S.to(device), u.to(device))
    return out


def legs(S, u):
    import torch

    import griffin_lim_ref as GR
    from seq2seq_vc_amd.vocoder.griffin_lim import griffin_lim_batch

    def hip():
        return griffin_lim_batch(S, None, N_FFT, HOP, n_iter=N_ITER, init_phase=u)[0]

    def stock():
        with torch.no_grad():
            return GR.torch_griffin_lim(S, u, N_FFT, HOP, n_iter=N_ITER)
    return {"hip": hip, "torch": stock}


def timed_group(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def warm_only(name):
    import torch
    for S, u in inputs("cuda").values():
        fn = legs(S, u)[name]
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
    print(f"{name} leg warmed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.25)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--warm-only", choices=["hip", "torch"])
    a = ap.parse_args()
    if a.warm_only:
        return warm_only(a.warm_only)
    errors = {}
    for name in ("hip", "torch"):                 # fresh children, one after the other, before this process touches the GPU
        if name == "torch" and a.no_torch:
            errors[name] = "skipped (--no-torch)"
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--warm-only", name], capture_output=True, text=True,
                               timeout=a.leg_timeout)
            if r.returncode != 0:
                errors[name] = f"warm-up exited {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
        except subprocess.TimeoutExpired:
            errors[name] = f"warm-up did not finish in {a.leg_timeout:.0f} s"
        if name in errors and r"exited -" in errors[name]:
            break                                  # a child killed by a signal: start nothing more on the card
    import numpy as np
    import torch

    import griffin_lim_ref as GR
    from seq2seq_vc_amd.ops import kernels_griffin_lim as KG
    res = {"metric": f"Griffin-Lim, n_fft {N_FFT} / hop {HOP}, {N_ITER} iterations, fp32", "repeats": a.repeats,
           "timed": "device events around back-to-back calls; median [min, max] over the repeats, HIP and stock-torch groups alternated",
           "shapes": {}}
    for name, err in errors.items():
        res[f"{name}_leg"], res[f"{name}_leg_error"] = "unavailable", err
    if "hip" not in errors:
        data = inputs("cuda")
        for (B, T), (S, u) in data.items():
            fns = {k: f for k, f in legs(S, u).items() if k not in errors}
            iters, times = {}, {k: [] for k in fns}
            for k, fn in fns.items():
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                iters[k] = max(2, math.ceil(a.target_s * 1e3 / timed_group(fn, 2)))
            for _ in range(a.repeats):
                for k, fn in fns.items():
                    times[k].append(timed_group(fn, iters[k]))
            before = KG.LAUNCHES
            y = fns["hip"]()
            entry = {"utterances": B, "frames": T, "audio_seconds": B * HOP * (T - 1) / FS, "hip_launches_per_call": KG.LAUNCHES - before}
            if "torch" in fns:
                yt = fns["torch"]()
                entry["hip_vs_torch_max_abs"] = float((y - yt).abs().max())
                entry["waveform_peak"] = float(yt.abs().max())
            for k, ts in times.items():
                med = statistics.median(ts)
                entry[k] = {"ms_per_call": med, "ms_min": min(ts), "ms_max": max(ts), "calls_per_group": iters[k],
                            "rtf": med * 1e-3 / entry["audio_seconds"]}
            res["shapes"][f"{B}x{T}"] = entry
    if not a.no_cpu:
        S, u = inputs("cpu")[SHAPES[0]]
        t0 = time.perf_counter()
        GR.griffin_lim(S[0].numpy(), u[0].numpy(), N_FFT, HOP, None, N_ITER, dtype=np.float64)
        res["cpu_float64_restatement_1x300_s"] = time.perf_counter() - t0
    bar = {"rule": "per shape: HIP is not slower than the stock-torch leg beyond the larger min-max spread of the two"}
    if errors:
        bar["met"] = "not measured"
    else:
        met = {}
        for k, e in res["shapes"].items():
            spread = max(e[leg]["ms_max"] - e[leg]["ms_min"] for leg in ("hip", "torch"))
            met[k] = {"hip_ms": e["hip"]["ms_per_call"], "torch_ms": e["torch"]["ms_per_call"], "spread_ms": spread,
                      "met": bool(e["hip"]["ms_per_call"] <= e["torch"]["ms_per_call"] + spread)}
        bar["shapes"], bar["met"] = met, all(v["met"] for v in met.values())
    res["speed_bar"] = bar
    print(json.dumps(res))


if __name__ == "__main__":
    main()
