#!/usr/bin/env python3
"""Timing of the HiFi-GAN multi-scale discriminator alone and of the whole HifiganDiscriminator (seq2seq_vc_amd/urhythmic/vocoder.py)
at the fine-tuning shape.  Method and output shape of tools/bench_disc.py, one block of workloads per net.

    python tools/bench_msd.py [--repeats 5] [--target-s 0.5] [--leg-timeout 400] [--out profiles/msd_bench.json]

Shape: 8 x 8320 samples, fp32 (urhythmic_fine_tune_vocoder.py's training batch).  Workloads:
  forward      D(x) under no_grad
  disc_step    D(real), D(generated.detach()), discriminator_loss, backward: parameter gradients only
  gen_step     D(real), D(generated) with `generated` requiring grad, feature_loss + generator_loss, backward: parameter gradients and dx
Nets: `msd` (MultiScaleDiscriminator) and `whole` (HifiganDiscriminator = mpd + msd).  Legs: `hip`, the kernels of csrc/hifigan_msd.hip
and csrc/hifigan_disc.hip, and `torch`, the restatements tests/msd_ref.py (+ tests/disc_ref.py) as stock torch (conv1d / conv2d and
autograd, the power iteration of the spectrally normed scale per call as torch.nn.utils.spectral_norm runs it) ON THE SAME CARD with
the same seeded weights; both legs are in train() mode.  The losses are the same stock torch code in both legs.  Device events around
back-to-back calls, warmed; `repeats` timed groups of about `target-s` seconds per leg, the legs alternated; median [min, max] over the
groups.  Every leg warms up first in a child process of its own under `leg-timeout` seconds; a leg whose child fails or times out is
reported as unavailable and nothing more is started on the card.  launches: calls into the HIP library during one call (the zero
fills of the operand buffers included; ATen's own launches -- the losses, gradient accumulation -- are not in it); plan: the length of
launch_plan() / backward_plan().
No threshold is set: the verdict line says which leg is faster.  Prints ONE JSON line and writes it to --out."""
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

SHAPE = (8, 8320)
SEED = 13
NETS = ("msd", "whole")
LEGS = ("hip", "torch")
WORKLOADS = ("forward", "disc_step", "gen_step")


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


def make(device, which, net):
    """-> {leg: {workload: callable}} of one net; every callable returns (a scalar or score, dx or None, one parameter gradient or None)"""
    import torch

    import disc_ref as DR
    import msd_ref as MR
    sd = {"msd." + k: v for k, v in MR.seeded_state_dict(SEED).items()}
    if net == "whole":
        sd.update({"mpd." + k: v for k, v in DR.seeded_state_dict(DR.SEED).items()})
    g = torch.Generator().manual_seed(SEED)
    real = (0.3 * torch.randn(SHAPE[0], 1, SHAPE[1], generator=g)).to(device)
    fake = (0.3 * torch.randn(SHAPE[0], 1, SHAPE[1], generator=g)).to(device)
    probe = "msd.discriminators.1.convs.3.weight_v"
    legs = {}

    def workloads(call, params, zero):
        def forward():
            with torch.no_grad():
                return call(fake)[0][0], None, None

        def disc_step():
            zero()
            sr, _ = call(real)
            sg, _ = call(fake.detach())
            loss = sum(torch.mean((1 - r) ** 2) + torch.mean(q ** 2) for r, q in zip(sr, sg))
            loss.backward()
            return loss.detach(), None, params()[probe].grad

        def gen_step():
            zero()
            x = fake.detach().requires_grad_(True)
            _, fr = call(real)
            sg, fg = call(x)
            loss = sum(torch.mean(torch.abs(a - b)) for fa, fb in zip(fr, fg) for a, b in zip(fa, fb)) + sum(torch.mean((1 - q) ** 2) for q in sg)
            loss.backward()
            return loss.detach(), x.grad, params()[probe].grad
        return {"forward": forward, "disc_step": disc_step, "gen_step": gen_step}

    if which in ("hip", "all"):
        from seq2seq_vc_amd.urhythmic.vocoder import HifiganDiscriminator, MultiScaleDiscriminator

        class _Msd(torch.nn.Module):                  # the same key prefix for both nets
            def __init__(self):
                super().__init__()
                self.msd = MultiScaleDiscriminator()

            def launch_plan(self):
                return self.msd.launch_plan()

            def backward_plan(self, need_dx=False):
                return self.msd.backward_plan(need_dx)

            def forward(self, x):
                return self.msd(x)
        mpd = HifiganDiscriminator() if net == "whole" else _Msd()
        mpd.load_state_dict(sd)
        mpd.to(device).train()
        legs["hip"] = workloads(mpd, lambda: dict(mpd.named_parameters()), lambda: mpd.zero_grad(set_to_none=True))
        legs["hip_plans"] = {"forward": len(mpd.launch_plan()), "disc_step": 2 * len(mpd.launch_plan()) + 2 * len(mpd.backward_plan(False)),
                             "gen_step": 2 * len(mpd.launch_plan()) + len(mpd.backward_plan(False)) + len(mpd.backward_plan(True))}
    if which in ("torch", "all"):
        prm = {k: v.to(device).requires_grad_(k.startswith("mpd.") or not MR.is_buffer(k[4:])) for k, v in sd.items()}
        msd_sd = {k[4:]: v for k, v in prm.items() if k.startswith("msd.")}
        mpd_sd = {k[4:]: v for k, v in prm.items() if k.startswith("mpd.")}

        def zero():
            for v in prm.values():
                v.grad = None

        def call(x):
            moved = {}
            s, f = MR.msd_forward(msd_sd, x, True, moved)
            msd_sd.update(moved)                      # the power iteration's buffers, written back as the module does
            if net == "whole":
                s0, f0 = DR.mpd_forward(mpd_sd, x)
                s, f = s0 + s, f0 + f
            return s, f
        legs["torch"] = workloads(call, lambda: prm, zero)
    return legs


def warm_only(name):
    import torch
    for net in NETS:
        for fn in make("cuda", name, net)[name].values():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
    print(f"{name} leg warmed")


def measure(fns, repeats, target_s):
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
    ap.add_argument("--target-s", type=float, default=0.5)
    ap.add_argument("--leg-timeout", type=float, default=400.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msd_bench.json"))
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
    res = {"metric": "HiFi-GAN multi-scale discriminator (3 scales, 29.6 M values) and the whole HifiganDiscriminator (mpd + msd), fp32, train() mode",
           "rows": SHAPE[0], "samples": SHAPE[1], "repeats": a.repeats,
           "timed": "device events around back-to-back calls; median [min, max] over the repeats, the legs' groups alternated",
           "yardstick": "tests/msd_ref.py (+ tests/disc_ref.py) as stock torch (conv1d / conv2d + autograd) on the same card, the same seeded weights",
           "workloads": {}}
    for name, err in errors.items():
        res[f"{name}_leg"], res[f"{name}_leg_error"] = "unavailable", err
    if not errors:
        import torch
        for net in NETS:
            res["workloads"][net] = {}
            legs = make("cuda", "all", net)
            for wl in WORKLOADS:
                fns = {k: legs[k][wl] for k in LEGS}
                entry = {"hip_library_launches_per_call": count_launches(fns["hip"]), "hip_plan_launches": legs["hip_plans"][wl]}
                entry.update(measure(fns, a.repeats, a.target_s))
                yh, yt = fns["hip"](), fns["torch"]()
                entry["value_hip"], entry["value_torch"] = float(yh[0].flatten()[0]), float(yt[0].flatten()[0])
                for tag, i in (("dx", 1), ("grad_probe", 2)):
                    if yh[i] is not None:
                        diff, peak = (yh[i] - yt[i]).abs(), float(yt[i].abs().max())
                        entry[f"{tag}_hip_vs_torch_max_abs"], entry[f"{tag}_peak"] = float(diff.max()), peak
                        # two fp32 runs disagree on the sign of a few pre-activations out of 10^7 (a leaky-relu mask, the sign in |a - b|); each
                        # one moves the gradient inside that unit's receptive field only -- the median says what the rest agrees to
                        entry[f"{tag}_hip_vs_torch_median_abs"] = float(diff.median())
                        entry[f"{tag}_elements_beyond_1e-3_of_peak"] = f"{int((diff > 1e-3 * peak).sum())} of {diff.numel()}"
                h, t = entry["hip"]["ms_per_call"], entry["torch"]["ms_per_call"]
                spread = max(entry[k]["ms_max"] - entry[k]["ms_min"] for k in LEGS)
                entry["torch_over_hip"] = t / h
                entry["verdict"] = "HIP WINS" if h + spread < t else ("HIP LOSES" if h > t + spread else "within the spread")
                res["workloads"][net][wl] = entry
        torch.cuda.synchronize()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
