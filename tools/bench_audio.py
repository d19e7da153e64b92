#!/usr/bin/env python3
"""Timing of the waveform conditioning on the HIP kernels: audio.resample_batch, audio.trim_batch and urhythmic.convert_wavs with
and without conditioning.

    python tools/bench_audio.py [--repeats 5] [--target-s 0.25] [--no-wavs]

Two batches -- one utterance of 10 s and 16 of 5 s -- of seeded noise.  resample_batch at 48 000 -> 16 000 Hz and 22 050 -> 16 000 Hz
against the DENSE form of the same filter as stock torch on the same card (F.pad + F.conv1d(stride=orig) in fp32 with the 2 width +
orig taps per phase torchaudio builds: tests/audio_ref.py's restatement moved to the GPU; never the code under test).  trim_batch on
the same batches at 16 kHz against a stock-torch statement of librosa.effects.trim (pad, unfold, mean of squares, log10, nonzero; one
host read as well).  convert_wavs on 48 kHz input with sample_rate=48000 and trim= against convert_wavs on the same audio conditioned
beforehand (a HuBERT-Soft at its upstream sizes, seeded; the rhythm model of tools/bench_urhythmic.py).  Device events around
back-to-back calls, warmed; `repeats` timed groups of about `target-s` seconds; median [min, max] over the groups; a verdict per row:
WINS / LOSES when the two ranges do not overlap, "within the spread" otherwise.  Prints ONE JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BATCHES = [(1, 10.0), (16, 5.0)]
RATES = [(48000, 16000), (22050, 16000)]
TRIM = dict(top_db=60, frame_length=2048, hop_length=512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-s", type=float, default=0.25)
    ap.add_argument("--no-wavs", action="store_true", help="skip the convert_wavs legs (they build a full-size HuBERT-Soft)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    import audio_ref as AR
    from bench_urhythmic import measure, verdict
    from seq2seq_vc_amd import audio
    from seq2seq_vc_amd.ops import kernels_audio as KA

    dev = "cuda:0"
    res = {"metric": "waveform conditioning on HIP: resample_batch, trim_batch, convert_wavs; fp32, seeded noise", "repeats": a.repeats,
           "timed": "device events around back-to-back calls; median [min, max] over the repeats", "rows": {}}

    def dense_stock(w, kernel, orig, new, width, M):
        """torchaudio's _apply_sinc_resample_kernel on a (B, 1, N) batch of full-length rows, fp32 on the device"""
        y = F.conv1d(F.pad(w, (width, width + orig)), kernel, stride=orig)
        return y.transpose(1, 2).reshape(w.shape[0], -1)[:, :M]

    def trim_stock(w, lens, top_db, frame_length, hop_length):
        """librosa.effects.trim of a (B, 1, N) batch of full-length rows with stock torch ops: intervals on the host, rows gathered"""
        n = w.shape[2]
        p = F.pad(w[:, 0], (frame_length // 2, frame_length - frame_length // 2)).unfold(1, frame_length, hop_length)[:, :1 + n // hop_length]
        power = p.double().pow(2).mean(2)
        db = 10 * torch.log10(power.clamp(min=1e-10)) - 10 * torch.log10(power.max(1, keepdim=True)[0].clamp(min=1e-10))
        loud = (db > -top_db).cpu()
        out = []
        for b in range(w.shape[0]):
            nz = torch.nonzero(loud[b])[:, 0]
            s, e = (int(nz[0]) * hop_length, min(n, (int(nz[-1]) + 1) * hop_length)) if nz.numel() else (0, 0)
            out.append(w[b, 0, s:e])
        return torch.nn.utils.rnn.pad_sequence(out, batch_first=True)

    for B, secs in BATCHES:
        for fs, target in RATES:
            n = int(fs * secs)
            w = (0.3 * torch.randn(B, 1, n, generator=torch.Generator().manual_seed(B + fs))).to(dev)
            lens = [n] * B
            orig, new = KA.reduced(fs, target)
            _, taps, width = AR.dense_kernel(orig, new)
            kernel = taps.to(torch.float32).view(new, 1, -1).to(dev)
            M = KA.out_length(n, orig, new)
            table = KA.poly_table(fs, target, dev)
            mine = measure(lambda: audio.resample_batch(w, lens, fs, target), a.repeats, a.target_s)
            stock = measure(lambda: dense_stock(w, kernel, orig, new, width, M), a.repeats, a.target_s)
            got, want = audio.resample_batch(w, lens, fs, target)[0][:, 0], dense_stock(w, kernel, orig, new, width, M)
            row = verdict(mine, stock)
            row.update(dense_taps=int(kernel.shape[2]), band_taps=table.Kb, samples_out=M,
                       max_abs_difference_from_the_dense_fp32_conv=float((got - want).abs().max()))
            res["rows"][f"resample_batch {B} x {secs:g} s {fs} -> {target}"] = row
        n = int(16000 * secs)
        w = (0.3 * torch.randn(B, 1, n, generator=torch.Generator().manual_seed(40 + B))).to(dev)
        w[:, :, :n // 5] *= 1e-4
        w[:, :, -n // 8:] *= 1e-4
        lens = [n] * B
        mine = measure(lambda: audio.trim_batch(w, lens, **TRIM), a.repeats, a.target_s)
        stock = measure(lambda: trim_stock(w, lens, **TRIM), a.repeats, a.target_s)
        out, out_lens, iv = audio.trim_batch(w, lens, **TRIM)
        row = verdict(mine, stock)
        row.update(interval_row_0=iv[0].tolist(), equals_stock_torch=bool(torch.equal(out[:, 0], trim_stock(w, lens, **TRIM))))
        res["rows"][f"trim_batch {B} x {secs:g} s at 16 kHz"] = row

    if not a.no_wavs:
        import hubert_ref as HR
        import urhythmic_ref as UR
        import vocoder_ref as VR
        from seq2seq_vc_amd import urhythmic as U
        from seq2seq_vc_amd.vocoder import HifiganGenerator
        K, D = 100, 256
        seg = U.Segmenter(gamma=2.0)
        seg.load_state_dict({"n_clusters_": 3, "labels_": torch.from_numpy(UR.default_labels(K).astype(np.int64)), "n_leaves_": K, "n_features_in_": D,
                             "children_": torch.zeros(K - 1, 2, dtype=torch.int64),
                             "sound_types": {c: getattr(U, n) for c, n in UR.SOUND_TYPE_OF_CLUSTER.items()}})
        wide = U.RhythmModelFineGrained()
        wide.load_state_dict({side: {getattr(U, n): (k, loc, 40 * scale) for n, (k, loc, scale) in d.items()}
                              for side, d in (("source", UR.RHYTHM_SOURCE), ("target", UR.RHYTHM_TARGET))})
        gen = HifiganGenerator(in_channels=D)
        gen.load_state_dict(VR.seed_state_dict(gen.state_dict(), seed=5))
        hubert = U.HubertSoft()
        hubert.load_state_dict(HR.seeded(12).state_dict())
        hubert = hubert.to(dev).eval()
        model = U.UrhythmicFine(seg, wide, U.TimeStretcherFineGrained(), gen.to(dev))
        for B, secs in BATCHES:
            n = int(48000 * secs)
            w = (0.3 * torch.randn(B, 1, n, generator=torch.Generator().manual_seed(70 + B))).to(dev)
            w[:, :, :n // 5] *= 1e-4
            lens = [n] * B
            cfg = dict(sampling_rate=16000, trim_silence=True, trim_threshold_in_db=60, trim_frame_size=2048, trim_hop_size=512)
            ready, ready_lens = audio.condition_batch(w, lens, 48000, cfg)
            key = f"convert_wavs {B} x {secs:g} s"
            try:
                same = all(torch.equal(x, y) for x, y in zip(U.convert_wavs(hubert, model, w, lens, sample_rate=48000, trim=TRIM),
                                                             U.convert_wavs(hubert, model, ready, ready_lens)))
            except (OverflowError, ValueError, KeyError) as e:       # a segment the rhythm model cannot map: reported, not timed
                res["rows"][key] = {"error": repr(e)}
                continue
            cond = measure(lambda: U.convert_wavs(hubert, model, w, lens, sample_rate=48000, trim=TRIM), a.repeats, a.target_s)
            bare = measure(lambda: U.convert_wavs(hubert, model, ready, ready_lens), a.repeats, a.target_s)
            alone = measure(lambda: audio.condition_batch(w, lens, 48000, cfg), a.repeats, a.target_s)
            res["rows"][key] = {"from_48_kHz_with_resample_and_trim": cond, "from_conditioned_16_kHz": bare, "condition_batch_alone": alone,
                                "conditioning_share": (cond["ms_per_call"] - bare["ms_per_call"]) / cond["ms_per_call"],
                                "samples_in": n, "samples_conditioned": ready_lens[0], "equal_bit_for_bit": same}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
