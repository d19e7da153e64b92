#!/usr/bin/env python3
"""Timing of the vocoder fine-tuning step (seq2seq_vc_amd/urhythmic/fine_tune.py) at the reference's batch, and of its new pieces alone.
Method and output shape of tools/bench_msd.py.

    python tools/bench_finetune.py [--repeats 5] [--target-s 0.5] [--leg-timeout 400] [--out profiles/finetune_bench.json]

Shape: 8 x 26 unit frames -> 8 x 8320 samples, the default generator, fp32 (urhythmic_fine_tune_vocoder.py's training batch).  Legs, all
on the same card from the same seeded weights:
  step_lean        VocoderFineTuner.step, mode="lean"
  step_reference   VocoderFineTuner.step, mode="reference"
  step_parent      the INTEGRATION.md loop as it stood before this package had the losses and the optimiser: the HIP nets, stock-torch
                   feature_loss / discriminator_loss (its 16 .item() calls kept) / generator_loss, F.l1_loss, torch.optim.AdamW
  losses_hip / losses_torch      the three losses alone, forward + backward, on the scores and feature lists of one discriminator call
  adamw_multi / adamw_torch_fused / adamw_torch_default      one optimiser step over the discriminator's 154 parameters
Device events around back-to-back calls, warmed; `repeats` timed groups of about `target-s` seconds per leg, the legs of a row
alternated; median [min, max] over the groups.  Every leg warms up first in a child process of its own under `leg-timeout` seconds; a
leg whose child fails or times out is reported as unavailable and nothing more is started on the card.  launches: calls into the HIP
library during one step, counted as tools/bench_msd.py counts them (ATen's own launches are not in it).  At most 16 CPU threads.
No threshold is set: the verdict lines say which leg is faster.  Prints ONE JSON line and writes it to --out."""
import argparse
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_msd import count_launches, measure  # noqa: E402

ROWS, FRAMES, SEED = 8, 26, 13
STEP_LEGS = ("step_lean", "step_reference", "step_parent")
LOSS_LEGS = ("losses_hip", "losses_torch")
ADAMW_LEGS = ("adamw_multi", "adamw_torch_fused", "adamw_torch_default")
LEGS = STEP_LEGS + LOSS_LEGS + ADAMW_LEGS
HYPER = dict(lr=5e-5, betas=(0.8, 0.99), weight_decay=1e-2)


def _base(device):
    """the seeded nets (built once per process) and one batch"""
    import torch

    import disc_ref as DR
    import msd_ref as MR
    from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram
    from seq2seq_vc_amd.urhythmic.vocoder import HifiganDiscriminator
    from seq2seq_vc_amd.vocoder import HifiganGenerator
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.manual_seed(SEED)
    gen = HifiganGenerator().to(device)
    disc = HifiganDiscriminator()
    disc.load_state_dict({**{"mpd." + k: v for k, v in DR.seeded_state_dict(DR.SEED).items()},
                          **{"msd." + k: v for k, v in MR.seeded_state_dict(SEED).items()}})
    disc.to(device)
    mel = LogMelSpectrogram().to(device)
    g = torch.Generator().manual_seed(SEED)
    T = FRAMES * 320
    wavs = (0.3 * torch.randn(ROWS, 1, T, generator=g)).to(device)
    units = torch.randn(ROWS, gen.in_channels, FRAMES, generator=g).to(device)
    tgts = torch.randn(mel.output_shape((ROWS, 1, T)), generator=g).to(device)
    return gen, disc, mel, (wavs, units, tgts)


def stock_feature_loss(features_real, features_generated):
    loss = 0
    for r, g in zip(features_real, features_generated):
        for rl, gl in zip(r, g):
            loss += torch_mean_abs(rl, gl)
    return loss


def torch_mean_abs(a, b):
    import torch
    return torch.mean(torch.abs(a - b))


def stock_discriminator_loss(real, generated):
    import torch
    loss, real_losses, generated_losses = 0, [], []
    for r, g in zip(real, generated):
        r_loss, g_loss = torch.mean((1 - r) ** 2), torch.mean(g ** 2)
        loss += r_loss + g_loss
        real_losses.append(r_loss.item())                 # the loop's 16 stream stops
        generated_losses.append(g_loss.item())
    return loss, real_losses, generated_losses


def stock_generator_loss(outputs):
    import torch
    loss, parts = 0, []
    for x in outputs:
        part = torch.mean((1 - x) ** 2)
        parts.append(part)
        loss += part
    return loss, parts


def make(device, which, base=None):
    """-> {leg: callable} for the legs named in `which`; every callable returns a tensor to read a value from"""
    import torch
    import torch.nn.functional as F

    from seq2seq_vc_amd.optim import MultiAdamW
    from seq2seq_vc_amd.urhythmic.fine_tune import VocoderFineTuner
    from seq2seq_vc_amd.urhythmic.vocoder import discriminator_loss, feature_loss, generator_loss
    gen0, disc0, mel, batch = base if base is not None else _base(device)
    wavs, units, tgts = batch
    legs, extra = {}, {}
    for leg, mode in (("step_lean", "lean"), ("step_reference", "reference")):
        if leg in which:
            tuner = VocoderFineTuner(copy.deepcopy(gen0), copy.deepcopy(disc0), mel, mode=mode)
            legs[leg] = (lambda t: lambda: t.step(wavs, units, tgts)["loss_generator"])(tuner)
            extra[leg + "_plan"] = len(tuner.launch_plan())
    if "step_parent" in which:
        G, D = copy.deepcopy(gen0).trainable().train(), copy.deepcopy(disc0).train()
        opt_g, opt_d = torch.optim.AdamW(G.parameters(), **HYPER), torch.optim.AdamW(D.parameters(), **HYPER)

        def parent():
            opt_d.zero_grad()
            wavs_ = G(units)
            mels_ = mel(wavs_)
            scores, _ = D(wavs)
            scores_, _ = D(wavs_.detach())
            loss_discriminator, _, _ = stock_discriminator_loss(scores, scores_)
            loss_discriminator.backward()
            opt_d.step()
            opt_g.zero_grad()
            scores, features = D(wavs)
            scores_, features_ = D(wavs_)
            loss_mel = F.l1_loss(mels_, tgts)
            loss_features = stock_feature_loss(features, features_)
            loss_adv, _ = stock_generator_loss(scores_)
            loss_generator = 45 * loss_mel + 2 * loss_features + loss_adv
            loss_generator.backward()
            opt_g.step()
            return loss_generator.detach()
        legs["step_parent"] = parent
    if any(leg in which for leg in LOSS_LEGS):
        D = copy.deepcopy(disc0).train()                  # train(): the power iteration gives the first scale its sigma
        with torch.no_grad():
            sr, fr = D(wavs)
            sg, fg = D(0.5 * wavs.flip(0))

        def leaves(lists):
            return [[t.detach().requires_grad_(True) for t in fl] for fl in lists]
        fr_l, fg_l, (sr_l,), (sg_l,) = leaves(fr), leaves(fg), leaves([sr]), leaves([sg])

        def losses(feat, dl, gl):
            def run():
                for t in [x for fl in fr_l + fg_l for x in fl] + sr_l + sg_l:
                    t.grad = None
                total = dl(sr_l, sg_l)[0] + 2 * feat(fr_l, fg_l) + gl(sg_l)[0]
                total.backward()
                return total.detach()
            return run
        if "losses_hip" in which:
            legs["losses_hip"] = losses(feature_loss, lambda a, b: discriminator_loss(a, b, detail=False), generator_loss)
        if "losses_torch" in which:
            legs["losses_torch"] = losses(stock_feature_loss, stock_discriminator_loss, stock_generator_loss)
    for leg, ctor in (("adamw_multi", lambda p: MultiAdamW(p, **HYPER)), ("adamw_torch_fused", lambda p: torch.optim.AdamW(p, fused=True, **HYPER)),
                      ("adamw_torch_default", lambda p: torch.optim.AdamW(p, **HYPER))):
        if leg in which:
            D = copy.deepcopy(disc0)
            g = torch.Generator().manual_seed(SEED + 1)
            for p in D.parameters():
                p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(device)
            opt = ctor(list(D.parameters()))
            probe = next(iter(D.parameters()))
            legs[leg] = (lambda o, q: lambda: (o.step(), q.detach().flatten()[0])[1])(opt, probe)
    return legs, extra


def warm_only(name):
    import torch
    legs, _ = make("cuda", (name,))
    for _ in range(2):
        legs[name]()
    torch.cuda.synchronize()
    print(f"{name} leg warmed")


def verdict(entry, ours, others):
    spread = max(entry[k]["ms_max"] - entry[k]["ms_min"] for k in (ours,) + tuple(others))
    out = {}
    for k in others:
        h, t = entry[ours]["ms_per_call"], entry[k]["ms_per_call"]
        out[f"{ours} vs {k}"] = "HIP WINS" if h + spread < t else ("HIP LOSES" if h > t + spread else "within the spread")
        out[f"{k}_over_{ours}"] = t / h
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.5)
    ap.add_argument("--leg-timeout", type=float, default=400.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_bench.json"))
    ap.add_argument("--warm-only", choices=LEGS)
    ap.add_argument("--rows", default="step,losses,adamw", help="comma-separated rows of legs to run (step, losses, adamw)")
    a = ap.parse_args()
    rows = [r for r in a.rows.split(",") if r]
    table = {"step": (STEP_LEGS, "step_lean"), "losses": (LOSS_LEGS, "losses_hip"), "adamw": (ADAMW_LEGS, "adamw_multi")}
    if any(r not in table for r in rows):
        ap.error("--rows takes step, losses, adamw")
    if a.warm_only:
        return warm_only(a.warm_only)
    errors = {}
    for name in [leg for r in rows for leg in table[r][0]]:          # fresh children, one after the other, before this process touches the GPU
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--warm-only", name], capture_output=True, text=True,
                               timeout=a.leg_timeout)
            if r.returncode != 0:
                errors[name] = f"warm-up exited {r.returncode}: {(r.stderr or r.stdout)[-400:]}"
        except subprocess.TimeoutExpired:
            errors[name] = f"warm-up did not finish in {a.leg_timeout:.0f} s"
        if name in errors:
            break                                  # a child that failed or hung: start nothing more on the card
    res = {"metric": "HiFi-GAN vocoder fine-tuning step (default generator, full discriminator, mel loss, three GAN losses, two AdamW), fp32, train() mode",
           "rows": ROWS, "unit_frames": FRAMES, "samples": FRAMES * 320, "repeats": a.repeats,
           "timed": "device events around back-to-back calls; median [min, max] over the repeats, the legs' groups of a row alternated",
           "rows_of_legs": {}}
    for name, err in errors.items():
        res[f"{name}_leg"], res[f"{name}_leg_error"] = "unavailable", err
    if not errors:
        import torch
        base = _base("cuda")
        for row, (names, ours) in ((r, table[r]) for r in rows):
            legs, extra = make("cuda", names, base)
            entry = dict(extra)
            entry.update(measure(legs, a.repeats, a.target_s))
            if row != "adamw":
                entry["library_launches_per_call"] = {k: count_launches(fn) for k, fn in legs.items()}
            entry["values"] = {k: float(fn().flatten()[0]) for k, fn in legs.items()}
            entry["verdict"] = verdict(entry, ours, tuple(k for k in names if k != ours))
            if row == "step":
                entry["verdict"].update(verdict(entry, "step_reference", ("step_parent",)))
                entry["lean_saves_ms_against_parent"] = entry["step_parent"]["ms_per_call"] - entry["step_lean"]["ms_per_call"]
            res["rows_of_legs"][row] = entry
            del legs
            torch.cuda.empty_cache()
        torch.cuda.synchronize()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
