#!/usr/bin/env python3
"""Timing of the mel L1 loss of HiFi-GAN generator fine-tuning (seq2seq_vc_amd/urhythmic/dataset.py: LogMelSpectrogram.l1_loss).

    python tools/bench_mel_loss.py [--repeats 5] [--target-s 0.25] [--leg-timeout 240] [--out profiles/mel_loss_bench.json]

Shapes: 8 x 8320 samples, the reference's training batch (loss forward + backward), and 1 x 64000 samples, a validation utterance
(forward only, under no_grad).  Legs per shape: `hip`, the kernels of csrc/melspec.hip, and `torch`, the restatement of
tests/mel_loss_ref.py in float32 ON THE SAME CARD under stock torch autograd (filterbank and window built once, on the device).  A third
pair at 8 x 26 frames: generator(units) -> mel loss -> backward with the default HiFi-GAN generator on HIP in both legs, the loss on HIP
(`step_hip`) against the stock-torch loss (`step_torch`): what the change is worth inside a step; reported, not bounded.
Device events around back-to-back calls, warmed; `repeats` timed groups of about `target-s` seconds per leg, the legs alternated; median
[min, max] over the groups.  Every leg warms up first in a child process of its own under `leg-timeout` seconds (first-use library
initialisation happens there); a leg whose child fails or times out is reported as unavailable and is not run here.  launches: calls
into the HIP library during one call (ATen's own launches are not in it).  The bar: per shape, HIP is not slower than the torch leg
beyond the larger min-max spread of the two.  Prints ONE JSON line and writes it to --out."""
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

TRAIN, VALID, STEP = (8, 8320), (1, 64000), (8, 26)
SEED = 20240807
LEGS = ("hip", "torch", "step")


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


def timed_group(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def make(device, which):
    """-> {leg name: callable}: `which` in LEGS selects what is built (a warm-up child builds its own leg only)"""
    import torch

    import mel_loss_ref as MR
    from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram
    mod = LogMelSpectrogram()
    consts = MR.constants(MR.DEFAULT, torch.float32, device)
    g = torch.Generator().manual_seed(SEED)
    data = {}
    for B, N in (TRAIN, VALID):
        wav = (0.3 * torch.randn(B, 1, N, generator=g)).to(device)
        with torch.no_grad():
            lm = MR.logmel(wav[:, 0], torch.float32, consts).unsqueeze(1)
        data[(B, N)] = (wav, (lm + 0.5 * torch.randn(lm.shape, generator=g).to(device)).contiguous())
    legs = {}
    wav_t, tgt_t = data[TRAIN]
    wav_v, _ = data[VALID]

    def hip_train():
        x = wav_t.detach().requires_grad_(True)
        loss, _ = mod.l1_loss(x, tgt_t)
        loss.backward()
        return loss.detach(), x.grad

    def torch_train():
        x = wav_t.detach().requires_grad_(True)
        loss = MR.l1(x[:, 0], tgt_t[:, 0], torch.float32, consts)
        loss.backward()
        return loss.detach(), x.grad

    def hip_valid():
        with torch.no_grad():
            return mod(wav_v)

    def torch_valid():
        with torch.no_grad():
            return MR.logmel(wav_v[:, 0], torch.float32, consts).unsqueeze(1)
    if which in ("hip", "all"):
        legs["hip"] = {TRAIN: hip_train, VALID: hip_valid}
    if which in ("torch", "all"):
        legs["torch"] = {TRAIN: torch_train, VALID: torch_valid}
    if which in ("step", "all"):
        import vocoder_ref as VR
        from seq2seq_vc_amd.vocoder import HifiganGenerator
        gen = HifiganGenerator()
        gen.load_state_dict(VR.seed_state_dict(gen.state_dict(), SEED))
        gen.to(device).trainable()
        units = torch.randn(STEP[0], gen.in_channels, STEP[1], generator=g).to(device)

        def step(hip_loss):
            def run():
                gen.zero_grad(set_to_none=True)
                wav = gen(units)
                loss = mod.l1_loss(wav, tgt_t)[0] if hip_loss else MR.l1(wav[:, 0], tgt_t[:, 0], torch.float32, consts)
                loss.backward()
                return loss.detach()
            return run
        legs["step_hip"], legs["step_torch"] = {STEP: step(True)}, {STEP: step(False)}
    return legs


def warm_only(name):
    import torch
    for fns in make("cuda", name).values():
        for fn in fns.values():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
    print(f"{name} leg warmed")


def measure(fns, repeats, target_s):
    """fns {name: callable} -> {name: {ms_per_call, ms_min, ms_max, calls_per_group}}, the groups of the legs alternated"""
    import torch
    iters, times = {}, {k: [] for k in fns}
    for k, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(2, math.ceil(target_s * 1e3 / timed_group(fn, 2)))
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(timed_group(fn, iters[k]))
    return {k: {"ms_per_call": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "calls_per_group": iters[k]} for k, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.25)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_loss_bench.json"))
    ap.add_argument("--warm-only", choices=LEGS)
    a = ap.parse_args()
    if a.warm_only:
        return warm_only(a.warm_only)
    errors = {}
    for name in LEGS:                             # fresh children, one after the other, before this process touches the GPU
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--warm-only", name], capture_output=True, text=True,
                               timeout=a.leg_timeout)
            if r.returncode != 0:
                errors[name] = f"warm-up exited {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
        except subprocess.TimeoutExpired:
            errors[name] = f"warm-up did not finish in {a.leg_timeout:.0f} s"
        if name in errors:
            break                                  # a child that failed or hung: start nothing more on the card
    res = {"metric": "mel L1 loss of HiFi-GAN fine-tuning (LogMelSpectrogram.l1_loss), fp32, n_fft 1024 / hop 320 / 80 mels",
           "repeats": a.repeats,
           "timed": "device events around back-to-back calls; median [min, max] over the repeats, the legs' groups alternated",
           "shapes": {}}
    for name, err in errors.items():
        res[f"{name}_leg"], res[f"{name}_leg_error"] = "unavailable", err
    bar = {"rule": "per shape: HIP is not slower than the stock-torch leg beyond the larger min-max spread of the two"}
    if errors:
        bar["met"] = "not measured"
    else:
        import torch
        legs = make("cuda", "all")
        met = {}
        for shape, what in ((TRAIN, "l1_loss forward + backward"), (VALID, "forward under no_grad")):
            fns = {k: legs[k][shape] for k in ("hip", "torch")}
            entry = {"rows": shape[0], "samples": shape[1], "what": what, "hip_library_launches_per_call": count_launches(fns["hip"])}
            entry.update(measure(fns, a.repeats, a.target_s))
            yh, yt = fns["hip"](), fns["torch"]()
            if shape == TRAIN:
                entry["loss_hip"], entry["loss_torch"] = float(yh[0]), float(yt[0])
                entry["dwav_hip_vs_torch_max_abs"], entry["dwav_peak"] = float((yh[1] - yt[1]).abs().max()), float(yt[1].abs().max())
            else:
                entry["logmel_hip_vs_torch_max_abs"] = float((yh - yt).abs().max())
            spread = max(entry[k]["ms_max"] - entry[k]["ms_min"] for k in ("hip", "torch"))
            met[f"{shape[0]}x{shape[1]}"] = {"hip_ms": entry["hip"]["ms_per_call"], "torch_ms": entry["torch"]["ms_per_call"], "spread_ms": spread,
                                             "met": bool(entry["hip"]["ms_per_call"] <= entry["torch"]["ms_per_call"] + spread)}
            res["shapes"][f"{shape[0]}x{shape[1]}"] = entry
        fns = {k: legs[k][STEP] for k in ("step_hip", "step_torch")}
        step = {"what": "generator(units) -> mel loss -> backward, default generator on HIP in both legs, fp32; reported, not bounded",
                "rows": STEP[0], "frames": STEP[1], "hip_library_launches_per_step": {k: count_launches(fn) for k, fn in fns.items()}}
        step.update(measure(fns, a.repeats, a.target_s))
        step["gain_ms"] = step["step_torch"]["ms_per_call"] - step["step_hip"]["ms_per_call"]
        step["loss_step_hip"], step["loss_step_torch"] = float(fns["step_hip"]()), float(fns["step_torch"]())
        res["step_8x26"] = step
        torch.cuda.synchronize()
        bar["shapes"], bar["met"] = met, all(v["met"] for v in met.values())
    res["speed_bar"] = bar
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
