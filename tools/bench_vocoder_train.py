#!/usr/bin/env python3
"""Timing of one fine-tuning step's generator part -- forward plus backward of HifiganGenerator.trainable() -- at the default
configuration and the reference's fine-tuning shape (urhythmic_fine_tune_vocoder.py:39-41: 8 x 26 frames -> 8 x 8320 samples), and
at 8 x 104 frames.

    python tools/bench_vocoder_train.py [--repeats 5] [--target-s 0.2] [--torch-warm-timeout 300] [--no-torch] [--out profiles/vocoder_train_bench.json]

Per shape, in fp32 and bf16: ms per forward + backward (device events around back-to-back steps, warmed; median and min / max over
`repeats` groups), launches, and a per-kind time split of ONE step (device events around every launch; the sum is larger than the
back-to-back step, which overlaps launch overhead; in bf16 mode the forward runs in fp32 and `hifigan_input` counts the casts of
the stored activations to bf16).  The weight-gradient kernel's FLOPs (2 B T C_out C_in k per layer) over its time
give its achieved TFLOP/s.  The stock-torch leg is autograd over tests/vocoder_ref.generator_forward ON THE SAME CARD in fp32 and
under torch.autocast("cuda", bfloat16), its groups alternated with the HIP groups; a child process runs it first under a time limit
(the convolution library searches algorithms on first use).  Also prints the worst relL2 of HIP's fp32 gradients against stock
torch's fp32 gradients.  Prints ONE JSON line and writes it to --out."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(8, 26), (8, 104)]
CFG = dict()
SEED = 20240807


def timed_group(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def loss_of(y):
    return 0.5 * (y.float() ** 2).mean() + y.float().mean()


def make(device):
    import torch

    import vocoder_ref as VR
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    gen = HifiganGenerator(**CFG)
    sd = VR.seed_state_dict(gen.state_dict(), SEED)
    gen.load_state_dict(sd)
    gen.to(device).trainable()
    g = torch.Generator().manual_seed(0)
    xs = {s: torch.randn(s[0], gen.in_channels, s[1], generator=g).to(device) for s in SHAPES}
    leaves = {k: v.to(device).requires_grad_(True) for k, v in sd.items()}
    return gen, leaves, xs


def torch_legs(leaves, x):
    import torch

    import vocoder_ref as VR

    def step(amp):
        def run():
            for p in leaves.values():
                p.grad = None
            if amp:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = VR.generator_forward(leaves, CFG, x)
            else:
                y = VR.generator_forward(leaves, CFG, x)
            loss_of(y).backward()
        return run
    return {"torch_fp32": step(False), "torch_bf16_autocast": step(True)}


def warm_torch_only():
    import torch
    _, leaves, xs = make("cuda")
    for s in SHAPES:
        for fn in torch_legs(leaves, xs[s]).values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
    print("torch legs warmed")


def kind_split(step):
    """device time of ONE step by launcher: events around every call of the ops/kernels_vocoder.py wrappers"""
    import torch

    from seq2seq_vc_amd.ops import kernels_vocoder as KV
    names = [n for n in dir(KV) if n.startswith("hifigan_") and callable(getattr(KV, n))]
    orig, marks = {n: getattr(KV, n) for n in names}, []

    def wrap(n):
        def f(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig[n](*a, **kw)
            e1.record()
            marks.append((n, e0, e1))
            return out
        return f
    try:
        for n in names:
            setattr(KV, n, wrap(n))
        step()
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(KV, n, orig[n])
    split, count = {}, {}
    for n, e0, e1 in marks:
        split[n] = split.get(n, 0.0) + e0.elapsed_time(e1)
        count[n] = count.get(n, 0) + 1
    return {n: {"ms": split[n], "launches": count[n]} for n in sorted(split)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.2)
    ap.add_argument("--torch-warm-timeout", type=float, default=300.0)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--warm-torch-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_train_bench.json"))
    a = ap.parse_args()
    if a.warm_torch_only:
        return warm_torch_only()
    torch_err = "skipped (--no-torch)" if a.no_torch else None
    if not a.no_torch:               # a fresh child, before this process touches the GPU, under its own time limit
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--warm-torch-only"], capture_output=True, text=True,
                               timeout=a.torch_warm_timeout)
            if r.returncode != 0:
                torch_err = f"warm-up exited {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
        except subprocess.TimeoutExpired:
            torch_err = f"warm-up did not finish in {a.torch_warm_timeout:.0f} s"
    import torch

    from seq2seq_vc_amd.ops import functional as Fn
    gen, leaves, xs = make("cuda")
    fwd, bwd = gen.launch_plan(), gen.backward_plan()
    nleaves = len(gen._leaves())
    res = {"metric": "HiFi-GAN generator forward + backward (parameter gradients), default configuration",
           "launches": {"forward": len(fwd), "fold (per step, from the live parameters)": 2 * nleaves - 2, "backward": len(bwd),
                        "casts of the stored fp32 activations (bf16 mode only)": sum(1 for e in gen.train_plan(torch.bfloat16) if e["kind"] == "cast")},
           "repeats": a.repeats, "timed": "device events around back-to-back steps; median [min, max] over the repeats, HIP and stock-torch "
           "groups alternated", "shapes": {}}
    if torch_err:
        res["torch_leg"], res["torch_leg_error"] = "unavailable", torch_err
    wgrad_flops = lambda B, N: sum(2.0 * B * N * e["mul"] * e["cout"] * e["cin"] * e["k"] for e in fwd if e["kind"] in ("conv1d", "tconv1d"))   # noqa: E731
    for s in SHAPES:
        B, N = s
        x = xs[s]

        def hip(dtype):
            def run():
                Fn.set_compute_dtype(dtype)
                try:
                    gen.zero_grad(set_to_none=True)
                    loss_of(gen(x)).backward()
                finally:
                    Fn.set_compute_dtype(torch.float32)
            return run
        legs = {"hip_fp32": hip(torch.float32), "hip_bf16": hip(torch.bfloat16)}
        if not torch_err:
            legs.update(torch_legs(leaves, x))
        iters, times = {}, {k: [] for k in legs}
        for k, fn in legs.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[k] = max(2, math.ceil(a.target_s * 1e3 / timed_group(fn, 2)))
        for _ in range(a.repeats):
            for k, fn in legs.items():
                times[k].append(timed_group(fn, iters[k]))
        entry = {"utterances": B, "frames": N, "samples": N * math.prod(gen.upsample_factors)}
        if not torch_err:
            legs["hip_fp32"]()
            legs["torch_fp32"]()
            worst = 0.0
            for k, p in gen.named_parameters():
                t = leaves[k].grad
                worst = max(worst, float((p.grad - t).norm() / t.norm().clamp_min(1e-30)))
            entry["hip_fp32_vs_torch_fp32_grads_worst_relL2"] = worst
        for k, ts in times.items():
            med = statistics.median(ts)
            entry[k] = {"ms_per_step": med, "ms_min": min(ts), "ms_max": max(ts), "steps_per_group": iters[k]}
            if k.startswith("hip"):
                split = kind_split(legs[k])
                entry[k]["split_ms_one_step"] = split
                wg = split["hifigan_wgrad"]["ms"]
                entry[k]["wgrad_flops"] = wgrad_flops(B, N)
                entry[k]["wgrad_achieved_TFLOPs"] = wgrad_flops(B, N) / wg / 1e9
        if not torch_err:
            for k, t in (("hip_fp32", "torch_fp32"), ("hip_bf16", "torch_bf16_autocast")):
                entry[k]["vs_" + t] = entry[t]["ms_per_step"] / entry[k]["ms_per_step"]
        res["shapes"][f"{B}x{N}"] = entry
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
