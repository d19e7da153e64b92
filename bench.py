#!/usr/bin/env python3
"""Headline benchmark of the MI355X-native seq2seq-vc hot path.

    python bench.py --gpus N --steps K --warmup W [--workload vtn|aasvc]

Headline workload (BASELINE.json configs[1], SURVEY.md section 8d "C2"): one optimiser step of VTN
(egs/arctic/vc1/conf/vtn.v1.yaml: 6+6 layers, d=384, r=4, postnet 5x256xk5; 30.48 M params) on a synthetic ARCTIC-shaped batch
of 32 utterance pairs PER GPU (T_src = T_tgt padded to 256, 80-dim mel), bf16 compute with fp32 master weights: forward +
Seq2SeqLoss + backward + grad-clip + Adam + WarmupLR.  Metric: mel-frames/sec = valid target frames consumed per step over all
ranks / step wall time.  `--workload aasvc` runs configuration C3 instead (AAS-VC, egs/arctic/vc2/conf/aas_vc.melmelmel.v1.yaml,
157.5 M params, 16 utterance pairs per GPU) through the same data-parallel machinery.

One process per GPU (torch.distributed, backend nccl == RCCL).  Data parallel = the staged backward pass of
seq2seq_vc_amd.distributed.OverlappedBackward: every stage of model.dp_plan() is one captured hipGraph, and the all-reduce of
the gradients a stage has finished is issued (asynchronously, on RCCL's stream) before the next stage's graph is replayed.

Rank 0 prints ONE JSON line.  A plain run measures the headline only: set-up, warm-up, the timed steps, the line.  With --full the
line is extended with
  "roofline":     the workload's dominant kernel (MFMA GEMM) timed live with HIP events against the bf16 MFMA peak
  "cpu_baseline": the CPU oracle (fp32 restatement of the reference) timed on this box's host cores
and, at N = 1 with the default workload, sub-objects measured in the same run:
  "aasvc":        configuration C3 (one rank), with its own roofline (4096 x 1536 x 1536 GEMM) and cpu_baseline
  "decode":       configuration C5 (VTN autoregressive decode, 16 utterances, captured step graph): RTF, with the CPU baseline
                  the recipe prescribes (16 single-thread processes, egs/arctic/vc1/run.sh:284-286)
  "tts", "trainer", "alignment", "memory_bound" (see main())

--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (float32; see dump_outputs()), so that two builds
can be compared output for output: the inputs, initial weights and dropout seeds are fixed, identical from run to run.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

VTN_VC1 = dict(idim=80, odim=80, dprenet_layers=2, dprenet_units=256, adim=384, aheads=4, elayers=6, eunits=1536, dlayers=6,
               dunits=1536, postnet_layers=5, postnet_filts=5, postnet_chans=256, use_batch_norm=True,
               encoder_normalize_before=True, decoder_normalize_before=False, encoder_concat_after=False,
               decoder_concat_after=False, decoder_reduction_factor=4)
AASVC_VC2 = dict(
    idim=80, odim=80, adim=384, aheads=2, elayers=4, eunits=1536, dlayers=4, dunits=1536, positionwise_layer_type="linear",
    positionwise_conv_kernel_size=1, duration_predictor_use_encoder_outputs=False, duration_predictor_input_dim=80,
    duration_predictor_layers=2, duration_predictor_chans=256, duration_predictor_kernel_size=3, postnet_layers=5,
    postnet_filts=5, postnet_chans=256, use_masking=True, encoder_normalize_before=True, decoder_normalize_before=True,
    encoder_reduction_factor=1, post_encoder_reduction_factor=4, decoder_reduction_factor=1, encoder_type="conformer",
    decoder_type="conformer", duration_predictor_type="stochastic", encoder_input_layer="linear",
    conformer_pos_enc_layer_type="rel_pos", conformer_self_attn_layer_type="rel_selfattn",
    use_macaron_style_in_conformer=True, use_cnn_in_conformer=True, conformer_enc_kernel_size=15, conformer_dec_kernel_size=15,
    init_type="xavier_uniform", transformer_enc_dropout_rate=0.2, transformer_enc_positional_dropout_rate=0.2,
    transformer_enc_attn_dropout_rate=0.2, transformer_dec_dropout_rate=0.2, transformer_dec_positional_dropout_rate=0.2,
    transformer_dec_attn_dropout_rate=0.2)
TTS_V1 = dict(idim=78, odim=80, dprenet_layers=2, dprenet_units=256, adim=384, aheads=4, elayers=6, eunits=1536, dlayers=6,
              dunits=1536, postnet_layers=5, postnet_filts=5, postnet_chans=256, use_batch_norm=True,
              encoder_normalize_before=True, decoder_normalize_before=False, encoder_concat_after=False,
              decoder_concat_after=False, decoder_reduction_factor=2)   # egs/ljspeech/tts1/conf/transformer_tts.v1.yaml:23-42
FWD_BWD_GFLOP = {"vtn": 715.9, "aasvc": 4777.0}   # BASELINE.md section 2 (matmul/conv FLOPs of one fwd+bwd at the canonical shapes)
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: ~2.5 PFLOP/s dense bf16
F32_MFMA_PEAK_TFLOPS = 157.3
DECODE_ARGS = {"threshold": 2.0, "minlenratio": 0.0, "maxlenratio": 6.0}   # threshold 2.0 never fires: 94 steps = 376 frames
HOP, SR = 256, 16000


def canonical_batch(B_total, T=256, idim=80, odim=80, seed=1234):
    """draw order ilens, olens, xs, ys; lens in [128,256], element 0 forced to 256."""
    g = torch.Generator().manual_seed(seed)
    ilens = torch.randint(128, T + 1, (B_total,), generator=g)
    ilens[0] = T
    olens = torch.randint(128, T + 1, (B_total,), generator=g)
    olens[0] = T
    xs = torch.randn(B_total, T, idim, generator=g)
    ys = torch.randn(B_total, T, odim, generator=g)
    ar = torch.arange(T)[None, :]
    xs[(ar >= ilens[:, None])] = 0.0
    ys[(ar >= olens[:, None])] = 0.0
    labels = (ar >= (olens[:, None] - 1)).float()
    return xs, ilens, ys, labels, olens


def canonical_batch_T(B_total, T, idim=80, odim=80, seed=1234):
    """canonical_batch's draw at another padded length T: lens in [T / 2, T], element 0 forced to T (bench.py --frames)."""
    g = torch.Generator().manual_seed(seed)
    ilens = torch.randint(T // 2, T + 1, (B_total,), generator=g)
    ilens[0] = T
    olens = torch.randint(T // 2, T + 1, (B_total,), generator=g)
    olens[0] = T
    xs = torch.randn(B_total, T, idim, generator=g)
    ys = torch.randn(B_total, T, odim, generator=g)
    ar = torch.arange(T)[None, :]
    xs[(ar >= ilens[:, None])] = 0.0
    ys[(ar >= olens[:, None])] = 0.0
    labels = (ar >= (olens[:, None] - 1)).float()
    return xs, ilens, ys, labels, olens


def canonical_tts_batch(B_total, seed=1234):
    """SURVEY.md section 8(d), C4 (LJSpeech TTS pre-training, egs/ljspeech/tts1): ilens in [60, 150] tokens in [1, 77) padded with 0,
    olens in [300, 640] frames, ys randn(B, 640, 80); element 0 fills both padded shapes (the batch of tests' tts_full_size_c4)."""
    g = torch.Generator().manual_seed(seed)
    ilens = torch.randint(60, 151, (B_total,), generator=g)
    ilens[0] = 150
    olens = torch.randint(300, 641, (B_total,), generator=g)
    olens[0] = 640
    xs = torch.randint(1, 77, (B_total, 150), generator=g)
    ys = torch.randn(B_total, 640, 80, generator=g)
    xs[torch.arange(150)[None] >= ilens[:, None]] = 0
    ar = torch.arange(640)[None]
    ys[ar >= olens[:, None]] = 0.0
    labels = (ar >= (olens[:, None] - 1)).float()
    return xs, ilens, ys, labels, olens


# =====================================================================================================================
# CPU baselines (the oracle = "port" of the reference, proven equal to it by tests/golden) -- rank 0, N = 1 only
# =====================================================================================================================
def _oracle_params(sd):
    names = [k for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k]
    for k in names:
        sd[k].requires_grad_(True)
    params = [sd[k] for k in names]
    return params, [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]


def cpu_info():
    """CPU model string, logical CPUs and physical cores of this box (/proc/cpuinfo)."""
    model, cores, logical = "unknown", set(), 0
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "model name":
                    model = v
                elif k == "processor":
                    logical += 1
                elif k == "physical id":
                    phys = v
                elif k == "core id":
                    core = v
                    cores.add((phys, core))
    except OSError:
        pass
    logical = logical or (os.cpu_count() or 1)
    return {"cpu_model": model, "logical_cpus": logical, "physical_cores": len(cores) or logical}


def _thread_candidates(info):
    """Thread counts for the sweep: 8, 16, 32 and the physical core count (capped by what the box has)."""
    phys = max(1, min(info["physical_cores"], info["logical_cpus"]))
    return sorted({min(8, phys), min(16, phys), min(32, phys), phys})


def _slice_batch(batch, n):
    return tuple(t[:n] for t in batch)


def _vtn_cpu_step(sd, params, state, batch, it):
    from oracle import models as OM
    xs, ilens, ys, labels, olens = batch
    t0 = time.perf_counter()
    o = OM.vtn_forward(sd, VTN_VC1, xs, ilens, ys, labels, olens, training=True, drop=True)
    l1, bce = OM.seq2seq_loss(o[0], o[1], o[2], o[3], o[4], o[5])
    grads = torch.autograd.grad(l1 + bce, params, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, params)]
    with torch.no_grad():
        OM.adam_step(params, grads, state, OM.warmup_lr(8e-5, it + 1), it + 1)
    return time.perf_counter() - t0


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def cpu_baseline_vtn(batch, steps=3):
    """fwd + loss + bwd + clip + Adam at the same shapes, fp32, train-mode dropout on: the oracle on the host cores at the best
    of three thread counts (a box with 128 hardware threads is SLOWER with all of them than with 16-32: VERDICT r2 weak #10), and
    on ONE thread -- the recipes export OMP_NUM_THREADS=1 (egs/arctic/vc1/path.sh:16) -- over a quarter of the batch."""
    from seq2seq_vc_amd.models import VTN
    info = cpu_info()
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in VTN(**VTN_VC1).state_dict().items()}
    params, state = _oracle_params(sd)
    olens = batch[4]
    keep = torch.get_num_threads()
    sweep = {}
    try:
        for nt in _thread_candidates(info):
            torch.set_num_threads(nt)
            _vtn_cpu_step(sd, params, state, batch, 0)                         # warm-up at this thread count
            sweep[nt] = _vtn_cpu_step(sd, params, state, batch, 1)
        best = min(sweep, key=sweep.get)
        torch.set_num_threads(best)                                            # the reported figure: MEDIAN of `steps` further steps
        runs = [sweep[best]] + [_vtn_cpu_step(sd, params, state, batch, 2 + i) for i in range(steps - 1)]
        sweep[best] = _median(runs)
        torch.set_num_threads(1)
        small = _slice_batch(batch, 8)
        t1 = _vtn_cpu_step(sd, params, state, small, 9)
    finally:
        torch.set_num_threads(keep)
    t = sweep[best]
    return {"value": float(olens.sum()) / t, "unit": "mel-frames/sec", "cores": best, "kind": "port",
            "sample": f"median of {steps} optimiser steps (after 1 warm-up) of the same VTN-vc1 B=32 batch, fp32, {t:.2f} s/step at {best} threads",
            "ms_per_step": t * 1e3, "steps_timed": steps, "s_per_step_runs": [round(r, 3) for r in runs], **info,
            "thread_sweep_s_per_step": {str(k): round(v, 3) for k, v in sweep.items()},
            "one_thread": {"value": float(small[4].sum()) / t1, "unit": "mel-frames/sec", "cores": 1,
                           "sample": f"1 optimiser step of the first 8 of the 32 utterance pairs, {t1:.2f} s (OMP_NUM_THREADS=1 as in egs/arctic/vc1/path.sh:16)"}}


def _tts_cpu_step(sd, params, state, batch, it):
    from oracle import models as OM
    xs, ilens, ys, labels, olens = batch
    t0 = time.perf_counter()
    o = OM.tts_forward(sd, TTS_V1, xs, ilens, ys, labels, olens, training=True, drop=True)
    l1, bce = OM.seq2seq_loss(o[0], o[1], o[2], o[3], o[4], o[5])
    grads = torch.autograd.grad(l1 + bce, params, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, params)]
    with torch.no_grad():
        OM.adam_step(params, grads, state, OM.warmup_lr(8e-4, it + 1), it + 1)
    return time.perf_counter() - t0


def cpu_baseline_tts(batch, steps=3):
    """The TransformerTTS training step of trainers/ar_tts.py:45-100 on the oracle (forward + Seq2SeqLoss + backward + clip + Adam,
    fp32, dropout on) over the same 8-utterance batch: the better of 16 and 32 host threads, median of `steps` steps."""
    from seq2seq_vc_amd.models import TransformerTTS
    info = cpu_info()
    cands = sorted({min(16, info["physical_cores"]), min(32, info["physical_cores"])})
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in TransformerTTS(**TTS_V1).state_dict().items()}
    params, state = _oracle_params(sd)
    keep = torch.get_num_threads()
    sweep = {}
    try:
        for nt in cands:
            torch.set_num_threads(nt)
            _tts_cpu_step(sd, params, state, batch, 0)
            sweep[nt] = _tts_cpu_step(sd, params, state, batch, 1)
        nt = min(sweep, key=sweep.get)
        torch.set_num_threads(nt)
        runs = [sweep[nt]] + [_tts_cpu_step(sd, params, state, batch, 2 + i) for i in range(steps - 1)]
        t = sweep[nt] = _median(runs)
    finally:
        torch.set_num_threads(keep)
    return {"value": float(batch[4].sum()) / t, "unit": "mel-frames/sec", "cores": nt, "kind": "port",
            "sample": f"median of {steps} optimiser steps (after 1 warm-up) of the same TransformerTTS-tts1 B={batch[0].shape[0]} batch, fp32, {t:.2f} s/step at {nt} threads",
            "ms_per_step": t * 1e3, "steps_timed": steps, "s_per_step_runs": [round(r, 3) for r in runs], **info,
            "thread_sweep_s_per_step": {str(k): round(v, 3) for k, v in sweep.items()}}


def _aasvc_cpu_step(sd, params, state, batch, it):
    from oracle import models as OM
    xs, ilens, ys, _, olens = batch
    t0 = time.perf_counter()
    noise = torch.randn(xs.shape[0], 2, 64)
    r = OM.aasvc_forward(sd, AASVC_VC2, xs, ilens, ys, olens, dp_inputs=xs, noise=noise, training=True, drop=True)
    l1 = OM.l1_loss(r["after_outs"], r["before_outs"], r["ys"], r["olens"])
    fs = OM.forward_sum_loss(r["log_p_attn"], r["ilens"], r["olens_reduced"])
    loss = l1 + 2.0 * (fs + r["bin_loss"]) + r["dur_nll"].sum()
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, params)]
    with torch.no_grad():
        OM.adam_step(params, grads, state, OM.warmup_lr(8e-5, it + 1), it + 1)
    return time.perf_counter() - t0


def cpu_baseline_aasvc(batch, steps=3, threads=None):
    """The AAS-VC training step of trainers/aas_vc.py:56-164 on the oracle: forward (incl. the C alignment search) + L1 +
    lambda*(forward-sum + bin) + duration NLL + backward + clip + Adam, fp32, dropout on; the better of 16 and 32 host threads (or
    `threads`) and ONE thread over two of the 16 utterance pairs."""
    from seq2seq_vc_amd.models import AASVC
    info = cpu_info()
    cands = [threads] if threads else sorted({min(16, info["physical_cores"]), min(32, info["physical_cores"])})
    olens = batch[4]
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in AASVC(**AASVC_VC2).state_dict().items()}
    params, state = _oracle_params(sd)
    keep = torch.get_num_threads()
    sweep = {}
    try:
        for nt in cands:
            torch.set_num_threads(nt)
            _aasvc_cpu_step(sd, params, state, batch, 0)
            sweep[nt] = _aasvc_cpu_step(sd, params, state, batch, 1)
        nt = min(sweep, key=sweep.get)
        torch.set_num_threads(nt)
        runs = [sweep[nt]] + [_aasvc_cpu_step(sd, params, state, batch, 2 + i) for i in range(steps - 1)]
        t = sweep[nt] = _median(runs)
        torch.set_num_threads(1)
        small = _slice_batch(batch, 2)
        t1 = _aasvc_cpu_step(sd, params, state, small, 9)
    finally:
        torch.set_num_threads(keep)
    return {"value": float(olens.sum()) / t, "unit": "mel-frames/sec", "cores": nt, "kind": "port",
            "sample": f"median of {steps} optimiser steps (after 1 warm-up) of the same AAS-VC-vc2 B=16 batch, fp32, {t:.2f} s/step at {nt} threads",
            "ms_per_step": t * 1e3, "steps_timed": steps, "s_per_step_runs": [round(r, 3) for r in runs], **info, "thread_sweep_s_per_step": {str(k): round(v, 3) for k, v in sweep.items()},
            "one_thread": {"value": float(small[4].sum()) / t1, "unit": "mel-frames/sec", "cores": 1,
                           "sample": f"1 optimiser step of the first 2 of the 16 utterance pairs, {t1:.2f} s"}}


def _decode_cpu_worker(seed):
    """One of the recipe's 16 decoding jobs: a single-thread process generating one utterance with the reference's
    schedule (the whole prefix is recomputed every step; prenet dropout on).  Returns the seconds spent generating."""
    torch.set_num_threads(1)
    from oracle import models as OM
    from seq2seq_vc_amd.models import VTN
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in VTN(**VTN_VC1).state_dict().items()}
    x = torch.randn(256, 80, generator=torch.Generator().manual_seed(1234 + seed))
    t0 = time.perf_counter()
    with torch.no_grad():
        outs, _, _ = OM.vtn_inference(sd, VTN_VC1, x, drop=True, **DECODE_ARGS)
    return time.perf_counter() - t0, int(outs.shape[0])


def cpu_baseline_decode(jobs=16):
    """egs/arctic/vc1/run.sh:284-286: n_jobs=16 CPU processes (CUDA_VISIBLE_DEVICES=""), OMP_NUM_THREADS=1 (path.sh:16),
    one utterance each here.  RTF = slowest job's generation time / audio seconds of ONE utterance is what a user waits
    per utterance; the aggregate RTF (comparable to the GPU's batch-aggregate number) divides by all 16 utterances."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    with ctx.Pool(jobs) as pool:
        res = pool.map(_decode_cpu_worker, range(jobs))
    wall = max(t for t, _ in res)
    frames = sum(n for _, n in res)
    return {"value": wall / (frames * HOP / SR), "unit": "RTF (wall s / audio s, aggregate over the jobs)", "cores": jobs, "kind": "port",
            "sample": f"{jobs} single-thread processes x one 256-frame utterance -> {frames // jobs} frames each, slowest job {wall:.2f} s "
                      f"(per-utterance RTF {wall / (frames // jobs * HOP / SR):.3f})"}


# =====================================================================================================================
# dominant-kernel rooflines
# =====================================================================================================================
def _time_graph_loop(launch, iters):
    """`iters` launches replayed from one hipGraph, HIP events on the stream they run on: events around a Python launch
    loop would time the host's ~10 us per ctypes launch, not the kernel (rocprofv3's per-dispatch average is the cross-check)."""
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    timed = "hipGraph replay"
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                for _ in range(iters):
                    launch()
            g.replay()
            side.synchronize()
            # three timed replays, the MEDIAN reported: one replay of a 50-launch graph was once seen 45 x slower than the
            # others (785 vs 17 us per launch, profiles/r03 collection: a stall on the host box, not the kernel)
            ms = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                g.replay()
                e1.record(side)
                side.synchronize()
                ms.append(e0.elapsed_time(e1))
            torch.cuda.current_stream().wait_stream(side)
            return sorted(ms)[1] / iters, timed + " (median of 3 replays)"
    except Exception as e:  # noqa: BLE001 -- report it and time a plain launch loop instead
        print(f"[bench] roofline graph capture failed ({type(e).__name__}: {e}); timing a Python launch loop", file=sys.stderr)
        timed = "python launch loop"
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            for _ in range(iters):
                launch()
            e1.record(side)
            side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    return e0.elapsed_time(e1) / iters, timed


def _pmc_traffic(key):
    """HBM-side bytes per launch come from rocprofv3 PMC passes of exactly this loop (they cannot be read from inside the
    process): profiles/roofline_pmc.json holds (2*FETCH_SIZE + WRITE_SIZE)*1024 as MI355X_MICROARCH.md prescribes."""
    pmc = os.path.join(ROOT, "profiles", "roofline_pmc.json")
    if not os.path.exists(pmc):
        return None
    with open(pmc) as f:
        d = json.load(f)
    if key == "vtn":
        return d.get("hbm_bytes_per_launch")
    return (d.get(key) or {}).get("hbm_bytes_per_launch")


def dominant_kernel_roofline(dtype, iters=100, workload="vtn"):
    """vtn:   the FLOP-heaviest launch of the VTN step, the implicit-GEMM 3x3 stride-2 Conv2d of the encoder front-end
              (M = 32*63*19, N = 384, K = 9*384; subsampling.py:60);
       aasvc: the GEMM shape that carries the AAS-VC step, 4096 x 1536 x 1536 (B*T = 16*256 rows, d = 1536: the decoder's
              attention / feed-forward / pointwise-conv projections, 60+ launches per step).
    Timed with HIP events on the stream the kernel is launched on and rated against the MFMA peak of its dtype."""
    from seq2seq_vc_amd.ops import kernels as K
    peak = BF16_MFMA_PEAK_TFLOPS if dtype == torch.bfloat16 else F32_MFMA_PEAK_TFLOPS
    if workload in ("aasvc", "aasvc_qkv"):
        # aasvc_qkv: the packed Q|K|V projection of the decoder's relative-position attention (attention.py:262-305; north_star
        # names the QKV GEMMs): 4096 x 4608 x 1536 = 256 workgroups of 256 x 288 (gemm_8ph_kernel_n96<3>)
        M, N, Kd = (4096, 1536, 1536) if workload == "aasvc" else (4096, 4608, 1536)
        x = torch.randn(M, Kd, device="cuda").to(dtype)
        w = (torch.randn(N, Kd, device="cuda") * 0.02).to(dtype)
        b = torch.zeros(N, device="cuda")
        y = torch.empty(M, N, dtype=dtype, device="cuda")

        def launch():
            K.gemm(K.operand(x, Kd), K.operand(w, Kd), M, N, Kd, y, in_dtype=dtype, bias=b)
        shape = "dense GEMM M=%d N=%d K=%d (+bias)" % (M, N, Kd)
    else:
        B, T1, F1, C, O = 32, 127, 39, 384, 384
        T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
        M, N, Kd = B * T2 * F2, O, 9 * C
        x = torch.randn(B, T1, F1, C, device="cuda").to(dtype)
        w = (torch.randn(O, 9 * C, device="cuda") * 0.02).to(dtype)
        b = torch.zeros(O, device="cuda")
        y = torch.empty(B, T2, F2, O, dtype=dtype, device="cuda")

        def launch():
            K.gemm(K.operand(x, C, mode=K.CONV2D_S2, C=C, T1=T1, F1=F1, T2=T2, F2=F2), K.operand(w, 9 * C), M, N, Kd, y,
                   in_dtype=dtype, bias=b, act="relu")
        shape = "conv2d-3x3-s2 implicit GEMM M=%d N=%d K=%d" % (M, N, Kd)
    ms, timed = _time_graph_loop(launch, iters)
    flops = 2.0 * M * N * Kd
    ach = flops / (ms * 1e-3) / 1e12
    if dtype != torch.bfloat16:
        kernel = "gemm_fast_kernel<float,128,128,32> (exact-fp32 MFMA)"
    elif workload == "aasvc_qkv":
        kernel = "gemm_8ph_kernel_n96<3> (bf16, 8 waves, 256x288 tile = one round of 256 workgroups, 3 phases per K tile)"
    elif workload == "aasvc":
        kernel = "gemm_8ph_kernel_128<DENSE> (bf16, 8 waves, 256x128 tile, 2 phases per K tile, LDS-DMA + counted vmcnt)"
    else:
        kernel = "gemm_8ph_kernel_q<CONV2D,4,2> (bf16, 8 waves, 512x128 tile, 4 phases per K tile, LDS-DMA + counted vmcnt)"
    alg_bytes = float((x.numel() + w.numel() + y.numel()) * x.element_size())
    traffic = _pmc_traffic(workload) if dtype == torch.bfloat16 and workload != "aasvc_qkv" else None
    return {"bound": "mfma", "kernel": f"{kernel} {shape}", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
            "traffic": traffic, "algorithmic_bytes": alg_bytes,
            # `achieved` / `avg_launch_us` are measured in THIS process; `traffic` and `by_time_*` cannot be (PMC counters need rocprofv3
            # around the process): they are read from the committed collection of the same loop / the same step
            "traffic_source": "profiles/roofline_pmc.json (replayed from the committed rocprofv3 --pmc collection, not measured in this "
                              "process)" if traffic is not None else None,
            "avg_launch_us": ms * 1e3, "flops_per_launch": flops, "timed": f"{iters} launches, {timed}, HIP events",
            "by_time": _by_time(workload) if dtype == torch.bfloat16 and workload != "aasvc_qkv" else None}


# =====================================================================================================================
# training workloads
# =====================================================================================================================
class Workload:
    """Model + fused optimiser + criterion on the canonical synthetic batch of this rank."""

    def __init__(self, name, dev, dtype, batch, world, rank, frames=None):
        from seq2seq_vc_amd import losses as L
        from seq2seq_vc_amd import models as M
        from seq2seq_vc_amd.ops import functional as Fn
        from seq2seq_vc_amd.optim import FlatAdam
        self.name, self.dev, self.Fn = name, dev, Fn
        if frames and name != "tts":            # --frames: the same draw at another padded length (lens in [T / 2, T]); NOT the canonical workload
            xs, ilens, ys, labels, olens = canonical_batch_T(batch * world, int(frames))
        else:
            xs, ilens, ys, labels, olens = (canonical_tts_batch if name == "tts" else canonical_batch)(batch * world)
        sl = slice(rank * batch, (rank + 1) * batch)
        xs, ilens, ys, labels, olens = xs[sl], ilens[sl], ys[sl], labels[sl], olens[sl]
        Ti, To = xs.shape[1], ys.shape[1]
        if int(ilens.max()) < Ti:  # keep the padded shape canonical on every rank
            ilens[0] = Ti
        if int(olens.max()) < To:
            olens[0] = To
        self.T_src, self.T_tgt = Ti, To
        self.frames = float(olens.sum())
        self.cpu_batch = (xs.clone(), ilens.clone(), ys.clone(), labels.clone(), olens.clone())
        self.xs, self.ys, self.labels, self.ilens, self.olens = xs.to(dev), ys.to(dev), labels.to(dev), ilens, olens
        torch.manual_seed(0)  # identical initial weights on every rank (the trainers broadcast rank 0's instead)
        lr = 8e-5
        if name == "vtn":
            self.model = M.VTN(**VTN_VC1).to(dev).train()
            self.crit = L.Seq2SeqLoss(bce_pos_weight=10.0)
            self.loss_names = ["l1", "bce"]
            self.desc = "VTN egs/arctic/vc1 (vtn.v1.yaml) training step: fwd+Seq2SeqLoss+bwd+clip+Adam+WarmupLR"
        elif name == "tts":
            self.model = M.TransformerTTS(**TTS_V1).to(dev).train()
            self.crit = L.Seq2SeqLoss(bce_pos_weight=10.0)
            self.loss_names = ["l1", "bce"]
            lr = 8e-4               # egs/ljspeech/tts1/conf/transformer_tts.v1.yaml optimizer_params
            self.desc = ("TransformerTTS egs/ljspeech/tts1 (transformer_tts.v1.yaml) pre-training step: text-enc -> mel-dec, "
                         "fwd+Seq2SeqLoss+bwd+clip+Adam+WarmupLR")
        else:
            self.model = M.AASVC(**AASVC_VC2).to(dev).train()
            self.l1, self.fs = L.L1Loss(), L.ForwardSumLoss()
            self.model.forward_sum_prefetch = self.fs.prefetch          # as trainers.AASVCTrainer does
            self.loss_names = ["l1", "forward_sum", "bin", "dur_nll"]
            self.desc = ("AAS-VC egs/arctic/vc2 (aas_vc.melmelmel.v1.yaml) training step: fwd (incl. alignment search)"
                         "+L1+2*(forward-sum+bin)+duration NLL+bwd+clip+Adam+WarmupLR")
        self.opt = FlatAdam(self.model, lr=lr, grad_norm=1.0, warmup_steps=4000, bf16_shadow=(dtype == torch.bfloat16))
        self.loss_buf = torch.zeros(len(self.loss_names), device=dev)
        self.params_m = sum(p.numel() for p in self.model.parameters()) / 1e6
        self.keep_outputs = False       # --dump-outputs: hold the model outputs of the forward pass (a captured graph rewrites them on every replay)
        self.outputs = {}

    def forward(self, staged=True):
        """One forward pass -> the loss split by the keys of model.dp_plan() (their sum is the training loss); staged=False: one key."""
        from seq2seq_vc_amd.ops import kernels as K
        if self.name in ("vtn", "tts"):
            after, before, logits, ys_, labels_, olens_, _ = self.model(self.xs, self.ilens, self.ys, self.labels, self.olens)
            if self.keep_outputs:
                self.outputs = {"after_outs": after.detach(), "before_outs": before.detach(), "logits": logits.detach()}
            l1, bce = self.crit(after, before, logits, ys_, labels_, olens_)
            K.scalars_axpy([(l1.detach(), 1.0), (bce.detach(), 1.0)], self.loss_buf, beta=0.0)     # (logging: one launch of the library)
            return {"loss": self.Fn.weighted_sum([(l1, 1.0), (bce, 1.0)])}
        ret = self.model(self.xs, self.ilens, self.ys, self.olens, self.xs, dp_lengths=self.ilens)
        if self.keep_outputs:
            self.outputs = {k: ret[k].detach() for k in ("after_outs", "before_outs", "ds", "log_p_attn") if ret.get(k) is not None}
        l1 = self.l1(ret["after_outs"], ret["before_outs"], ret["ys"], ret["olens"])
        fs = self.fs(ret["log_p_attn"], ret["ilens"], ret["olens_reduced"])
        dur = ret["dur_nll"]          # (B,): summed inside the launches below
        K.scalars_axpy([(l1.detach(), 1.0), (fs.detach(), 1.0), (ret["bin_loss"].detach(), 1.0), (dur.detach(), 1.0)], self.loss_buf, beta=0.0)
        if not staged:
            return {"loss": self.Fn.weighted_sum([(l1, 1.0), (fs, 2.0), (ret["bin_loss"], 2.0), (dur, 1.0)])}
        return {"decoder": l1, "align": self.Fn.weighted_sum([(fs, 2.0), (ret["bin_loss"], 2.0), (dur, 1.0)])}


def build_step(wl, dist, world, staged, force_dist, payload, use_graph, warmup_eager=2, collective="allreduce", stage_mode="flush",
               min_bucket_mb=16.0):
    """Returns (step(), info).  Unstaged: graph 1 = zero + forward + loss + backward, graph 2 = clip + Adam + WarmupLR.
    Data parallel, stage_mode "flush" (round 6, the default): the UNCUT backward pass in one graph with an event-record node behind
    every flushed gradient batch (distributed.FlushExchange); after the replay's launch every bucket of the flat gradient buffer is
    all-reduced from the communication stream behind the mark of the flush that finished it, beside the rest of the same graph.
    stage_mode "marks": the stages of model.dp_plan() in ONE graph with a mark behind each (the stage joins stay);
    stage_mode "graphs" (rounds 2-5): one graph per stage, the exchange issued between the replays.  The optimiser graph follows
    the join."""
    from seq2seq_vc_amd.distributed import FlushExchange, OverlappedBackward, allreduce_mean_
    from seq2seq_vc_amd.ops import kernels as K
    Fn, opt, dev = wl.Fn, wl.opt, wl.dev
    fx = None
    if staged and stage_mode == "flush":       # the UNCUT backward pass, the exchange behind the flushes of its gradient batches
        staged = False
        fx = FlushExchange(opt, dist, world, payload=payload, force=force_dist, min_bucket_numel=int(min_bucket_mb * 262144))
    ob = OverlappedBackward(wl.model, opt, dist, world, payload=payload, force=force_dist, collective=collective) if staged else None
    stage16 = None
    if not staged and (dist is not None or force_dist) and payload == "bf16":
        stage16 = torch.empty(opt.numel, dtype=torch.bfloat16, device=dev)
    held = {}

    def begin():
        K.reset_op_counter()
        K.advance_seed(dev)
        opt.begin_step()            # zero_grad + the refresh of the derived weight copies, beside the forward pass

    def fwd_bwd(record=True):
        begin()
        (total,) = wl.forward(staged=False).values()
        opt.join_prologue()
        if fx is not None and record:
            with fx.recording():                # a mark behind every flushed gradient batch
                Fn.root_backward(total, fx.scale)
                Fn.side_join()
        else:
            Fn.root_backward(total, fx.scale if fx is not None else 1.0)
            Fn.side_join()
        if fx is not None:
            fx.mark_end()

    def stage(i):
        if i == 0:
            begin()
            with ob.forward_context():
                held["losses"] = wl.forward()
        ob.run_stage(i, held["losses"])

    n_stages = len(ob.plan) if staged else 1

    def step_eager():
        if staged:
            for i in range(n_stages):
                stage(i)
                ob.begin_reduce(i)
            ob.finish()
        elif fx is not None:
            fwd_bwd()
            fx.issue()
            fx.finish()
        else:
            fwd_bwd()
            if (dist is not None or force_dist):
                allreduce_mean_(opt.flat_g, dist, world, force=force_dist, stage_bf16=stage16)
        opt.step()

    if fx is not None:              # which slices of the flat gradient buffer are final behind which flush: one instrumented eager pass
        fx.learn(lambda: fwd_bwd(record=False))
        opt.zero_grad()
    side = torch.cuda.Stream()      # warm-up on a side stream so that a later capture sees a quiet default stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup_eager):
            step_eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graphs, g_opt = [], None
    if use_graph:
        try:
            if staged and stage_mode == "marks":
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    for i in range(n_stages):
                        stage(i)
                        ob.mark(i)               # an event-record node: "stage i's gradients are final" of THIS replay
                graphs.append(g)
            else:
                for i in range(n_stages):
                    g = torch.cuda.CUDAGraph()
                    kw = {"pool": graphs[0].pool()} if graphs else {}
                    # thread_local: RCCL's watchdog thread polls events while this thread captures (N > 1)
                    with torch.cuda.graph(g, capture_error_mode="thread_local", **kw):
                        stage(i) if staged else fwd_bwd()
                    graphs.append(g)
            g_opt = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_opt, capture_error_mode="thread_local"):
                opt.step()
        except Exception as e:  # noqa: BLE001 -- report and fall back to eager launches, loudly
            print(f"[bench] hipGraph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
            use_graph = False
            torch.cuda.synchronize()

    post_reduce = (dist is not None or force_dist) and not staged and fx is None

    def step():
        if not use_graph:
            step_eager()
            return
        if staged and stage_mode == "marks":
            graphs[0].replay()
            for i in range(n_stages):
                ob.begin_reduce(i, after_mark=True)      # behind mark i of this replay, beside the later stages of the same graph
            ob.finish()
        elif staged:
            for i, g in enumerate(graphs):
                g.replay()
                ob.begin_reduce(i)       # this stage's gradients travel while the next stage's graph runs
            ob.finish()
        elif fx is not None:
            graphs[0].replay()
            fx.issue()                   # every bucket behind the mark of the flush that finished it, beside the rest of the same graph
            fx.finish()
        else:
            graphs[0].replay()
            if post_reduce:
                allreduce_mean_(opt.flat_g, dist, world, force=force_dist, stage_bf16=stage16)
        g_opt.replay()

    def probe(reps=20):
        """Milliseconds of each piece of the staged step run ALONE (device-synchronised between pieces, so nothing overlaps):
        the stage graphs, the gradient exchange issued after each, the join, the optimiser graph."""
        if not (use_graph and staged) or stage_mode == "marks":
            return None
        names = [f"graph{i}" for i in range(n_stages)] + [f"reduce{i}" for i in range(n_stages)] + ["finish", "opt"]
        acc = dict.fromkeys(names, 0.0)

        def timed(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc[name] += (time.perf_counter() - t0) * 1e3 / reps

        for _ in range(reps):
            for i, g in enumerate(graphs):
                timed(f"graph{i}", g.replay)
                timed(f"reduce{i}", lambda i=i: ob.begin_reduce(i))
            timed("finish", ob.finish)
            timed("opt", g_opt.replay)
        return {k: round(v, 3) for k, v in acc.items()}

    def check_exchange():
        """Flush mode: the overlapped exchange of ONE replayed (or eager) pass against a blocking all-reduce of the same local gradients
        (the dropout seed is pinned so that both passes draw the same masks) -> max |difference| over the flat gradient buffer, and
        whether the plan covers every element exactly once."""
        if fx is None:
            return None
        seed = K.SEED.tensor(dev)
        s0 = seed.clone()
        rng = torch.cuda.get_rng_state(dev)          # (the stochastic duration predictor draws its noise with torch.randn)

        def local_pass():
            seed.copy_(s0)
            torch.cuda.set_rng_state(rng, dev)
            if use_graph:
                graphs[0].replay()
            else:
                fwd_bwd()
        torch.cuda.synchronize()
        local_pass()
        torch.cuda.synchronize()
        ref = opt.flat_g.clone()
        if dist is not None:
            dist.all_reduce(ref)
        torch.cuda.synchronize()
        local_pass()
        fx.issue()
        fx.finish()
        torch.cuda.synchronize()
        diff = float((opt.flat_g - ref).abs().max())
        cover = torch.zeros(opt.numel, dtype=torch.int32, device=dev)
        per_bucket = []
        for _, rs in fx.plan:
            m = 0.0
            for lo, hi in rs:
                cover[lo:hi] += 1
                m = max(m, float((opt.flat_g[lo:hi] - ref[lo:hi]).abs().max()))
            per_bucket.append(m)
        return {"max_abs_diff": diff, "per_bucket_max_abs_diff": per_bucket, "covered_once": bool((cover == 1).all()), "buckets": len(fx.plan), "flushes": fx.n_flushes,
                "grad_abs_max": float(ref.abs().max())}

    info = {"hip_graph": bool(use_graph), "backward_stages": n_stages, "_check": check_exchange, "stage_mode": stage_mode if (staged or fx is not None) else None, "_probe": probe,
            "grad_buckets_MB": [round(b / 1e6, 1) for b in ob.bucket_bytes()] if staged else [round(b / 1e6, 1) for b in fx.bucket_bytes()] if fx is not None else
                               ([round(opt.numel * (2 if stage16 is not None else 4) / 1e6, 1)] if post_reduce else None),
            "grad_payload": payload if (staged or post_reduce or fx is not None) else None,
            "collective": collective if staged else ("allreduce" if (post_reduce or fx is not None) else None)}
    return step, info


def time_steps(step, steps, warmup, dist=None, dev=None):
    for _ in range(warmup):
        step()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    return dt


def step_mfma(workload, ms):
    if workload not in FWD_BWD_GFLOP:
        return None
    gf = FWD_BWD_GFLOP[workload]
    return {"gflop_per_step_per_gpu": gf, "achieved_tflops_per_gpu": gf / ms, "frac_of_bf16_peak": gf / ms / BF16_MFMA_PEAK_TFLOPS}


DUMP_MAX_ELEMS = 1 << 21        # per array (8 MB of float32): params, grads, <= 4 model outputs + two tiny arrays -> < 64 MB per dump
DUMP_SAMPLE_SEED = 20240531


def _dump_sample(t):
    """t as float32 on the host; above DUMP_MAX_ELEMS a fixed, seeded sample of its flattened elements (sorted indices drawn from a
    CPU generator seeded by DUMP_SAMPLE_SEED: the same positions in every run, and in every array of the same size)."""
    t = t.detach()
    if t.numel() > DUMP_MAX_ELEMS:
        g = torch.Generator().manual_seed(DUMP_SAMPLE_SEED)
        idx = torch.randint(0, t.numel(), (DUMP_MAX_ELEMS,), generator=g).sort().values
        t = t.reshape(-1)[idx.to(t.device)]
    return t.float().cpu().numpy()


def dump_outputs(wl, out_dir):
    """What the last timed step handed back, as out_dir/<name>.npy (float32):
      losses          the logged loss terms of the step (wl.loss_names order)
      opt_state       [step, lr, grad_norm, clip_coef] of the fused optimiser after the step
      params / grads  the flat fp32 master weights after the update and the flat gradient buffer the step filled
                      (a seeded sample of DUMP_MAX_ELEMS elements, the same positions in both)
      <model output>  the forward pass's outputs (vtn / tts: after_outs, before_outs, logits; aasvc: after_outs, before_outs, ds,
                      log_p_attn), sampled the same way above DUMP_MAX_ELEMS elements
    -> {name: shape} of what was written."""
    import numpy as np
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    arrays = {"losses": wl.loss_buf, "opt_state": wl.opt.state, "params": wl.opt.flat_p, "grads": wl.opt.flat_g, **wl.outputs}
    os.makedirs(out_dir, exist_ok=True)
    written, total = {}, 0
    for name, t in arrays.items():
        a = np.ascontiguousarray(_dump_sample(t), dtype=np.float32)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name], total = list(a.shape), total + a.nbytes
    assert total <= 64 << 20, f"--dump-outputs wrote {total} bytes"
    return written


# =====================================================================================================================
# sub-benchmarks reported beside the headline (N = 1)
# =====================================================================================================================
def bench_aasvc_single(dev, dtype, steps=40, warmup=8, cpu=True, batch=16):
    from seq2seq_vc_amd.ops import functional as Fn
    # the schedule AASVCTrainer ships (trainers.AASVCTrainer.GRADIENT_WORK)
    Fn.enable_side_streams(0, inline_batches=True)
    wl = Workload("aasvc", dev, dtype, batch, 1, 0)
    step, info = build_step(wl, None, 1, False, False, "fp32", True)
    info.pop("_probe", None)
    info.pop("_check", None)
    dt = time_steps(step, steps, warmup)
    ms = dt / steps * 1e3
    lb = wl.loss_buf.tolist()
    out = {"metric": "mel-frames/sec (train)", "value": wl.frames / (dt / steps), "unit": "mel-frames/sec", "n_gpus": 1, "steps": steps,
           "warmup": warmup, "ms_per_step": ms, "dtype": "bf16" if dtype == torch.bfloat16 else "fp32", "data": "synthetic",
           "config": {"workload": wl.desc, "batch_per_gpu": batch, "T_src": 256, "T_tgt": 256, "params_M": round(wl.params_m, 2),
                      **info},
           "final_losses": dict(zip(wl.loss_names, lb), **wl.opt.last_stats()), "step_mfma": step_mfma("aasvc", ms)}
    if not all(v == v and abs(v) < 1e6 for v in lb):
        raise SystemExit(f"bench: non-finite AAS-VC loss {lb}")
    out["roofline"] = dominant_kernel_roofline(dtype, workload="aasvc")
    if dtype == torch.bfloat16:
        q = dominant_kernel_roofline(dtype, workload="aasvc_qkv")
        out["qkv_gemm"] = {k: q[k] for k in ("kernel", "achieved", "peak", "unit", "frac", "avg_launch_us", "flops_per_launch", "timed")}
    if cpu:
        out["cpu_baseline"] = cpu_baseline_aasvc(wl.cpu_batch)
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    del wl, step
    torch.cuda.empty_cache()
    return out


def bench_tts_single(dev, dtype, steps=40, warmup=8, cpu=True, batch=8):
    """C4 (BASELINE.json configs[3]): TransformerTTS tts1, one rank's share (8 utterances) of the global batch of 64."""
    from seq2seq_vc_amd.ops import functional as Fn
    Fn.enable_side_streams(4)               # the schedule ARTTSTrainer ships (trainers.Trainer.GRADIENT_WORK)
    wl = Workload("tts", dev, dtype, batch, 1, 0)
    step, info = build_step(wl, None, 1, False, False, "fp32", True)
    info.pop("_probe", None)
    info.pop("_check", None)
    dt = time_steps(step, steps, warmup)
    ms = dt / steps * 1e3
    lb = wl.loss_buf.tolist()
    out = {"metric": "mel-frames/sec (train)", "value": wl.frames / (dt / steps), "unit": "mel-frames/sec", "n_gpus": 1, "steps": steps,
           "warmup": warmup, "ms_per_step": ms, "dtype": "bf16" if dtype == torch.bfloat16 else "fp32", "data": "synthetic",
           "config": {"workload": wl.desc, "batch_per_gpu": batch, "global_batch_of_the_recipe": 64, "T_text": wl.T_src, "T_tgt": wl.T_tgt,
                      "params_M": round(wl.params_m, 2), **info},
           "final_losses": dict(zip(wl.loss_names, lb), **wl.opt.last_stats())}
    if not all(v == v and abs(v) < 1e6 for v in lb):
        raise SystemExit(f"bench: non-finite TTS loss {lb}")
    if cpu:
        out["cpu_baseline"] = cpu_baseline_tts(wl.cpu_batch)
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    del wl, step
    torch.cuda.empty_cache()
    return out


def bench_decode(dev, dtype, batch=16, iters=5, poll=32, cpu=True):
    """C5: encoder + source K/V projection + 94 replays of the captured step graph + postnet, all inside the timed region."""
    from seq2seq_vc_amd import decode as D
    from seq2seq_vc_amd.models import VTN
    from seq2seq_vc_amd.ops import functional as Fn
    from seq2seq_vc_amd.ops import kernels as K
    torch.manual_seed(0)
    K.manual_seed(1234)
    model = VTN(**VTN_VC1).to(dev).eval()
    xs = torch.randn(batch, 256, 80, generator=torch.Generator().manual_seed(1234)).to(dev)
    ilens = torch.full((batch,), 256)

    def run():
        with torch.no_grad():
            lens = D.Mo.Lens.of(ilens, xs.device)
            hs, hlens = model.encoder(Fn.to_compute(xs), lens, exact_lens=True)
            return D.decode(model, hs, list(hlens.host), DECODE_ARGS, poll=poll, use_graph=True)

    res = run()            # builds the session + captures the step graph
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):             # host-paced (a poll every `poll` steps): the median batch, not the mean, is reported
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    frames = sum(r[0].shape[0] for r in res)
    nsteps = frames // (batch * VTN_VC1["decoder_reduction_factor"])
    out = {"metric": "RTF (AR decode, batch aggregate)", "value": t / (frames * HOP / SR), "unit": "wall s / audio s",
           "higher_is_better": False, "n_gpus": 1, "dtype": "bf16" if dtype == torch.bfloat16 else "fp32", "data": "synthetic",
           "ms_per_batch": t * 1e3, "us_per_step": t * 1e6 / nsteps, "frames_per_sec": frames / t,
           "config": {"workload": "VTN egs/arctic/vc1 AR decode (C5): encoder + 94 steps x r=4 + postnet, prenet dropout 0.5 on",
                      "batch": batch, "T_src": 256, "steps": nsteps, "frames_per_utt": frames // batch, "hip_graph": True, "poll": poll},
           "finite": bool(all(torch.isfinite(r[0]).all() for r in res))}
    if cpu:
        out["cpu_baseline"] = cpu_baseline_decode(batch)
        out["speedup_vs_cpu_baseline"] = out["cpu_baseline"]["value"] / out["value"]
    return out


# =====================================================================================================================
def bench_alignment_kernels(dev, cpu=True):
    """SURVEY 8(d) / BASELINE.md 4.4: the two dependency-latency-bound kernels of the AAS path at the C3 shape (16 utterances,
    256 target frames x 64 source positions), us per utterance: the alignment search (modules/alignments.py:63-93, numba JIT in
    the reference) beside the C -O3 restatement on ONE host thread, and the forward-sum (CTC) loss with its gradient
    (losses/forward_sum_loss.py:58-76) beside torch.nn.functional.ctc_loss -- the reference's own call -- on ONE host thread."""
    from seq2seq_vc_amd.ops import kernels as K
    from seq2seq_vc_amd.ops import kernels_aas as KA
    B, Tf, Tx = 16, 256, 64
    g = torch.Generator().manual_seed(11)
    lp = torch.log_softmax(torch.randn(B, Tf, Tx, generator=g), dim=-1)
    tl = torch.randint(Tx // 2, Tx + 1, (B,), generator=g)
    fl = torch.randint(Tf // 2, Tf + 1, (B,), generator=g)
    tl[0], fl[0] = Tx, Tf
    lp_d, tl_d, fl_d = lp.to(dev), tl.to(dev, torch.int32), fl.to(dev, torch.int32)
    out = {}
    us, timed = _time_graph_loop(lambda: K.mas(lp_d, tl_d, fl_d), 50)
    out["mas"] = {"metric": "monotonic alignment search + durations + bin-loss gather", "shape": [B, Tf, Tx], "us_per_batch": us * 1e3,
                  "us_per_utterance": us * 1e3 / B, "bound": "dependency latency (T_mel sequential steps per utterance, one wavefront each)",
                  "timed": f"50 launches, {timed}, HIP events"}
    prior = KA.betabinom_prior(B, Tf, Tx, tl_d, fl_d, dev)
    us, timed = _time_graph_loop(lambda: KA.forward_sum(lp_d, prior, tl_d, fl_d), 50)
    out["forward_sum"] = {"metric": "forward-sum (CTC) loss + gradient", "shape": [B, Tf, Tx], "us_per_batch": us * 1e3,
                          "us_per_utterance": us * 1e3 / B, "bound": "dependency latency (alpha / beta recursions over T_mel steps)",
                          "timed": f"50 launches, {timed}, HIP events"}
    if cpu:
        keep = torch.get_num_threads()
        try:
            torch.set_num_threads(1)
            from oracle import cmas
            lpn, tln, fln = lp.numpy(), tl.numpy(), fl.numpy()
            cmas.viterbi_decode(lpn, tln, fln)
            t0 = time.perf_counter()
            reps = 20
            for _ in range(reps):
                cmas.viterbi_decode(lpn, tln, fln)
            tc = (time.perf_counter() - t0) / reps
            out["mas"]["cpu_baseline"] = {"us_per_utterance": tc / B * 1e6, "cores": 1, "kind": "port",
                                          "sample": f"{reps} x 16 utterances, oracle/mas.c (gcc -O3), one thread", **cpu_info()}
            import torch.nn.functional as F
            from oracle import models as OM
            prior_c = torch.full((B, Tf, Tx), -float("inf"))      # the reference caches its priors by (T, N): not part of the timed call
            for b in range(B):
                prior_c[b, : int(fl[b]), : int(tl[b])] = torch.from_numpy(OM.betabinom_logprior(int(fl[b]), int(tl[b]))).float()

            def ctc_ref():
                x = lp.clone().requires_grad_(True)
                cur_all = F.pad(x + prior_c, (1, 0, 0, 0, 0, 0), value=-1.0)
                total = 0.0
                for b in range(B):                                   # forward_sum_loss.py:58-76: one ctc_loss call per utterance
                    T, N = int(fl[b]), int(tl[b])
                    total = total + F.ctc_loss(cur_all[b, :T, : N + 1].unsqueeze(1), torch.arange(1, N + 1).unsqueeze(0), torch.tensor([T]),
                                               torch.tensor([N]), zero_infinity=True)
                (total / B).backward()
            ctc_ref()
            t0 = time.perf_counter()
            reps = 5
            for _ in range(reps):
                ctc_ref()
            tc = (time.perf_counter() - t0) / reps
            out["forward_sum"]["cpu_baseline"] = {"us_per_utterance": tc / B * 1e6, "cores": 1, "kind": "reference",
                                                  "sample": f"{reps} x 16 utterances, torch.nn.functional.ctc_loss forward + backward (the reference's own call), one thread"}
        finally:
            torch.set_num_threads(keep)
    return out


def bench_memory_bound(dev):
    """SURVEY 8(d) "state per kernel": the HBM-bound kernels at their AAS-VC vc2 shapes (4096 rows x 1536 channels bf16; 16 x 2 x 256
    x 256 attention scores; 157.5 M parameters), achieved bytes/s over the ALGORITHMIC traffic (one read of every input, one write
    of every output) and its fraction of the 8 TB/s HBM3E peak (MI355X_MICROARCH.md; a plain copy reaches 6.3 TB/s)."""
    from seq2seq_vc_amd.ops import kernels as K
    rows, D = 4096, 1536
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, D, generator=g).to(dev, torch.bfloat16)
    res_ = torch.randn(rows, D, generator=g).to(dev, torch.bfloat16)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    items = []
    # what a dependent launch costs whatever it does (a kernel of 256 / 2048 workgroups that store one word each, same graph loop):
    # every figure below is bytes / (launch time), so an 8 us kernel that moves 12 MB can never show more than ~20 % of the HBM peak --
    # the floor-corrected rate (bytes / (time - floor * launches)) says what the kernel does while it runs
    sink = torch.zeros(1024, dtype=torch.int32, device=dev)
    floor = {wgs: _time_graph_loop(lambda wgs=wgs: K.launch_floor(sink, wgs, 256), 50)[0] * 1e3 for wgs in (256, 2048)}

    def add(name, nbytes, launch, note, launches=1):
        ms, timed = _time_graph_loop(launch, 50)
        us = ms * 1e3
        body = max(us - launches * floor[256], 1e-3)
        items.append({"kernel": name, "algorithmic_bytes": nbytes, "us_per_launch": us, "achieved_TBs": nbytes / (ms * 1e-3) / 1e12,
                      "frac_of_8TBs": nbytes / (ms * 1e-3) / 8e12, "launches": launches, "launch_floor_us": floor[256],
                      "frac_of_8TBs_excl_launch_floor": nbytes / (body * 1e-6) / 8e12,
                      "shape": note, "timed": f"50 launches, {timed}, HIP events"})
    seed = K.new_seed(dev)
    add("ln_fwd_vec (residual + dropout + LayerNorm)", 4 * rows * D * 2 + 8 * rows,
        lambda: K.layernorm_fwd(x, gamma, beta, 1e-12, res=res_, p=0.1, seed=seed), f"{rows} x {D} bf16: h, res in; s, y out")
    mean, rstd = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    from seq2seq_vc_amd.ops import kernels_aas as KA
    add("bn_swish_apply (BatchNorm apply + Swish of the Conformer convolution module, csrc/convmod.hip)", 2 * rows * D * 2,
        lambda: KA.bn_swish_apply(x, mean, rstd, gamma, beta), f"{rows} x {D} bf16 in, out")
    y2 = torch.randn(16, 256, 2 * D, generator=g).to(dev, torch.bfloat16)
    dww, dwb = torch.randn(D, 1, 15, generator=g).to(dev) * 0.2, torch.zeros(D, device=dev)
    add("convmod_fwd (GLU + depthwise conv k15 + batch statistics, csrc/convmod.hip; 2 launches)", 3 * rows * D * 2,
        lambda: KA.convmod_fwd(y2, dww, dwb, 15, 1e-5, 0.1), f"16 x 256 x {2 * D} bf16 in, 16 x 256 x {D} out", launches=2)
    B, H, T = 16, 2, 256
    sc = torch.randn(B, H, T, T, generator=g).to(dev)
    klen = torch.full((B,), T, dtype=torch.int32, device=dev)
    add("softmax_fwd (scale + mask + softmax)", B * H * T * T * (4 + 2), lambda: K.attn_softmax_fwd(sc, torch.bfloat16, 0.07, klen=klen),
        f"{B} x {H} x {T} x {T}: fp32 scores in, bf16 probabilities out")
    n = 157_530_000 // 64 * 64
    p_, g_, m_, v_ = (torch.zeros(n, device=dev) for _ in range(4))
    g_.normal_(generator=None)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    state, partial = torch.zeros(4, device=dev), torch.empty(1024, dtype=torch.float64, device=dev)
    add("sumsq + adam_prepare + adam_update (clip + Adam + WarmupLR + bf16 shadow)", n * (4 + 16 + 12 + 2),
        lambda: K.adam_step(p_, g_, m_, v_, sh, state, partial, 8e-5), f"{n / 1e6:.1f} M parameters: g (norm pass); p, g, m, v in; p, m, v, shadow out",
        launches=3)
    items.append({"kernel": "launch floor (s2svc_launch_floor: one word stored per workgroup, dependent launches of one graph)",
                  "us_per_launch_256_workgroups": floor[256], "us_per_launch_2048_workgroups": floor[2048]})
    return items


def bench_product_trainer(dev, dtype, steps=40):
    """The same VTN step through the PRODUCT trainer (seq2seq_vc_amd.trainers.ARVCTrainer) on host batches whose lengths differ
    from batch to batch: eager launches against config["hip_graph"] (captured steps, lengths as data of the graph).  The
    host-to-device copy of every batch is inside the timed region (tools/bench_trainer.py)."""
    from tools import bench_trainer as BT
    try:
        data = BT.make_batches("vtn", steps + 6, 32)
        res = [BT.run("vtn", mode, data, dtype, dev) for mode in (False, True)]
        return {"workload": "ARVCTrainer, VTN vc1, B = 32, lengths vary per batch, H2D inside",
                "eager_ms_per_step": res[0]["ms_per_step"], "hip_graph_ms_per_step": res[1]["ms_per_step"],
                "hip_graph_mel_frames_per_s": res[1]["mel_frames_per_s"], "steps": res[1]["steps"]}
    finally:
        Fn_reset()


def _by_time(workload):
    """The kernel family the STEP spends most of its time in (profiles/step_by_time.json, written by tools/step_by_time.py from the
    rocprofv3 kernel trace + SQ counter pass of whole steps): the FLOP-heaviest launch above is a few percent of the VTN step, so the
    headline roofline also names where the time goes and how busy the MFMA pipe is there."""
    path = os.path.join(ROOT, "profiles", "step_by_time.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f).get(workload)


def _get(obj, *path):
    for p in path:
        if not isinstance(obj, dict) or p not in obj:
            return None
        obj = obj[p]
    return obj if isinstance(obj, (int, float, str, bool)) else None


def _shape_line(out):
    """Shape of the ONE JSON line.  The driver's record keeps the scalar fields of `config`, `roofline` and `cpu_baseline`, the
    top-level scalars, only the NAMES of other nested objects, and the last 2 000 characters of the line.  So: the C3 (AAS-VC) / C5
    (decode) / trainer figures are scalars INSIDE `config`, the by-time kernel family's share and MFMA-busy are scalars inside
    `roofline`, the other CPU baselines scalars inside `cpu_baseline`; the verbose objects (memory_bound, alignment, the full
    sub-benchmark objects, roofline.by_time's top-5 list) come FIRST and the line ENDS with the same figures as flat scalars."""
    cfg, roof, cpu = out.get("config", {}), out.get("roofline") or {}, out.get("cpu_baseline")
    extra = {
        "aasvc_ms_per_step": _get(out, "aasvc", "ms_per_step"),
        "aasvc_mel_frames_per_s": _get(out, "aasvc", "value"),
        "aasvc_roofline_frac": _get(out, "aasvc", "roofline", "frac"),
        "aasvc_roofline_kernel_us": _get(out, "aasvc", "roofline", "avg_launch_us"),
        "aasvc_qkv_gemm_frac": _get(out, "aasvc", "qkv_gemm", "frac"),
        "aasvc_qkv_gemm_us": _get(out, "aasvc", "qkv_gemm", "avg_launch_us"),
        "aasvc_step_mfma_frac": _get(out, "aasvc", "step_mfma", "frac_of_bf16_peak"),
        "aasvc_cpu_frames_per_s": _get(out, "aasvc", "cpu_baseline", "value"),
        "aasvc_cpu_cores": _get(out, "aasvc", "cpu_baseline", "cores"),
        "aasvc_speedup_vs_cpu": _get(out, "aasvc", "speedup_vs_cpu_baseline"),
        "aasvc_by_time_family": _get(out, "aasvc", "roofline", "by_time", "family"),
        "aasvc_by_time_mfma_busy": _get(out, "aasvc", "roofline", "by_time", "mfma_busy"),
        "aasvc_by_time_source": _get(out, "aasvc", "roofline", "by_time", "source"),
        "aasvc_traffic_source": _get(out, "aasvc", "roofline", "traffic_source"),
        "tts_ms_per_step": _get(out, "tts", "ms_per_step"),
        "tts_mel_frames_per_s": _get(out, "tts", "value"),
        "tts_cpu_frames_per_s": _get(out, "tts", "cpu_baseline", "value"),
        "tts_cpu_cores": _get(out, "tts", "cpu_baseline", "cores"),
        "tts_speedup_vs_cpu": _get(out, "tts", "speedup_vs_cpu_baseline"),
        "decode_rtf": _get(out, "decode", "value"),
        "decode_us_per_step": _get(out, "decode", "us_per_step"),
        "decode_cpu_rtf": _get(out, "decode", "cpu_baseline", "value"),
        "trainer_hip_graph_ms_per_step": _get(out, "trainer", "hip_graph_ms_per_step"),
        "trainer_eager_ms_per_step": _get(out, "trainer", "eager_ms_per_step"),
        "mas_us_per_utterance": _get(out, "alignment", "mas", "us_per_utterance"),
        "forward_sum_us_per_utterance": _get(out, "alignment", "forward_sum", "us_per_utterance"),
        "step_mfma_frac": _get(out, "step_mfma", "frac_of_bf16_peak"),
        "launch_floor_us": next((it.get("us_per_launch_256_workgroups") for it in (out.get("memory_bound") or [])
                                 if isinstance(it, dict) and "us_per_launch_256_workgroups" in it), None),
    }
    extra = {k: v for k, v in extra.items() if v is not None}
    cfg.update(extra)
    by_time = roof.pop("by_time", None) if isinstance(roof, dict) else None
    if isinstance(by_time, dict):
        roof["by_time_family"] = by_time.get("family")
        roof["by_time_share"] = by_time.get("share_of_kernel_time")
        roof["by_time_mfma_busy"] = by_time.get("mfma_busy")
        roof["by_time_launches_per_step"] = by_time.get("launches_per_step")
        roof["by_time_source"] = by_time.get("source")
    if isinstance(cpu, dict):
        for k_src, k_dst in (("aasvc_cpu_frames_per_s", "aasvc_value"), ("aasvc_cpu_cores", "aasvc_cores"), ("decode_cpu_rtf", "decode_rtf"),
                             ("tts_cpu_frames_per_s", "tts_value"), ("tts_cpu_cores", "tts_cores")):
            if k_src in extra:
                cpu[k_dst] = extra[k_src]
    head = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data")
    line = {k: out[k] for k in head if k in out}
    for k in ("memory_bound", "alignment", "aasvc", "tts", "decode", "trainer"):          # verbose objects first
        if k in out:
            line[k] = out[k]
    if by_time is not None:
        line["roofline_by_time"] = by_time
    for k, v in out.items():
        if k not in line and k not in ("config", "roofline", "cpu_baseline"):
            line[k] = v
    line["config"] = cfg
    if roof:
        line["roofline"] = roof
    if cpu is not None:
        line["cpu_baseline"] = cpu
    tail = {"roofline_frac": _get(roof, "frac"), "roofline_kernel_us": _get(roof, "avg_launch_us"),
            "roofline_by_time_family": _get(roof, "by_time_family"), "roofline_by_time_share": _get(roof, "by_time_share"),
            "roofline_by_time_mfma_busy": _get(roof, "by_time_mfma_busy"),
            "cpu_baseline_value": _get(cpu, "value"), "cpu_baseline_cores": _get(cpu, "cores"),
            **{k: v for k, v in extra.items() if not k.endswith("_source")}}          # (the *_source labels stay inside config / roofline)
    for k, v in tail.items():                                                     # ... and the line ends with the flat scalars
        if v is not None:
            line[k] = v
    return line


def Fn_reset():
    from seq2seq_vc_amd.ops import functional as Fn
    Fn.enable_side_streams(0)


def spawn_ranks(n, argv=None):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script on this node (RANK = LOCAL_RANK = 0..N-1,
    WORLD_SIZE = N, rendezvous on a free port of 127.0.0.1 -- the env contract of torch.distributed.run and of the reference's
    distributed/launch.py:119-173), wait for all of them and return the first non-zero exit code.  Rank 0 prints the JSON line."""
    argv = list(sys.argv[1:] if argv is None else argv)
    rc = 0
    for attempt in range(3):           # the free port is found, released, then bound by rank 0: another process can take it in between
        rc = _spawn_ranks_once(n, argv)
        if rc != RC_RENDEZVOUS:
            break
        print(f"bench.py: rendezvous port was taken (attempt {attempt + 1}), retrying on another port", file=sys.stderr)
    return rc


RC_RENDEZVOUS = 75        # exit code of a rank whose init_process_group could not bind / reach the rendezvous port (EX_TEMPFAIL)


def _spawn_ranks_once(n, argv):
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), S2SVC_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: RCCL between processes needs it on this driver
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in pending:                            # a dead rank leaves the others waiting in a collective
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def _init_group(dist, backend, rank, world, **kw):
    """init_process_group; under spawn_ranks a bind failure of the rendezvous port exits with RC_RENDEZVOUS so that the launcher retries."""
    try:
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    except Exception as e:       # noqa: BLE001 -- torch raises RuntimeError / DistNetworkError with the errno in its text
        if os.environ.get("S2SVC_BENCH_SPAWNED") and ("EADDRINUSE" in str(e) or "address already in use" in str(e).lower()):
            raise SystemExit(RC_RENDEZVOUS)
        raise


def dist_dry_run(world, rank):
    """The launcher contract without a GPU (CPU test): join a gloo group, sum a 1 over the ranks, rank 0 prints what it saw."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")       # a bare one-rank run only: launchers (torchrun, spawn_ranks) always set it
    _init_group(dist, "gloo", rank, world)
    one = torch.ones(1)
    dist.all_reduce(one)
    ranks = torch.zeros(world)
    ranks[rank] = 1.0
    dist.all_reduce(ranks)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": int(one.item()), "world_size": world, "ranks_present": int(ranks.sum().item())}),
              flush=True)
    dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks of the job (default: WORLD_SIZE when a launcher set it, else 1)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="vtn", choices=["vtn", "aasvc", "tts"])
    ap.add_argument("--batch", type=int, default=None, help="utterance pairs per GPU (default: 32 for vtn, 16 for aasvc, 8 for tts)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-graph", action="store_true", help="launch kernels eagerly instead of replaying hipGraphs")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline also measure the dominant-kernel roofline, the CPU baseline and (N = 1, vtn) the sub-benchmarks "
                         "(aasvc, tts, decode, trainer, alignment, memory_bound); a plain run times the headline step only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed to DIR/<name>.npy (float32, < 64 MB; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="--full, N = 1: skip the sub-benchmarks (aasvc, tts, decode, trainer, ...)")
    ap.add_argument("--roofline-only", action="store_true", help="only run the dominant-kernel loop (for rocprofv3)")
    ap.add_argument("--split-backward", action="store_true",
                    help="N = 1: run the staged backward pass of the data-parallel path without collectives")
    ap.add_argument("--stage-times", action="store_true",
                    help="staged runs: also report the milliseconds of every stage graph / gradient exchange / optimiser graph run alone")
    ap.add_argument("--force-dist", action="store_true",
                    help="take the N > 1 code path (RCCL process group, staged backward, overlapped all-reduces) at world size 1")
    ap.add_argument("--grad-payload", default=None, choices=["fp32", "bf16"],
                    help="dtype of the gradient exchange (default: the trainers' default, <Trainer>.DP_GRAD_PAYLOAD = fp32; bf16 is the "
                         "opt-in config['dp_grad_payload']; reported in config.grad_payload)")
    ap.add_argument("--stage-mode", default="flush", choices=["flush", "marks", "graphs"],
                    help="data parallel: flush = the uncut backward pass, every gradient bucket exchanged behind the flush of the gradient batch "
                         "that finished it (event-record nodes inside ONE graph); marks = the stages of model.dp_plan() in one graph with a mark "
                         "behind each; graphs = one graph per stage, the exchange between the replays (rounds 2-5)")
    ap.add_argument("--min-bucket-mb", type=float, default=16.0, help="--stage-mode flush: smallest gradient bucket (MB of fp32)")
    ap.add_argument("--check-exchange", action="store_true",
                    help="--stage-mode flush: compare the overlapped exchange of one pass with a blocking all-reduce of the same gradients")
    ap.add_argument("--dp-decoder-stages", type=int, default=0,
                    help="aasvc: this many decoder layers get a backward stage (gradient bucket) of their own")
    ap.add_argument("--collective", default="allreduce", choices=["allreduce", "rs_ag"],
                    help="data parallel: one all-reduce per bucket, or reduce-scatter + all-gather")
    ap.add_argument("--inline-batches", action="store_true", help="with --side-streams 0: queue the gradient work and run it in batches on its own stream")
    ap.add_argument("--frames", type=int, default=None, help="vtn / aasvc: padded utterance length in frames instead of the canonical 256 (a side measurement: "
                                                              "the line's config.T_src / T_tgt say so; lengths in [T / 2, T])")
    ap.add_argument("--grad-batch", type=int, default=None, help="closures per parameter-gradient batch (default: 16 forked / 64 inline, ops.functional.enable_side_streams)")
    ap.add_argument("--side-streams", type=int, default=None, help="HIP side streams for parameter-gradient kernels (default: 4 for vtn, 0 + inline batches for aasvc)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend of the N > 1 path (nccl == RCCL; gloo: test aid, the same code path without RCCL)")
    ap.add_argument("--one-device", action="store_true",
                    help="test aid for a 1-GPU box: every rank runs on GPU 0 (RCCL refuses two ranks per device: use --dist-backend gloo)")
    ap.add_argument("--dist-dry-run", action="store_true",
                    help="launcher check without a GPU: every rank joins a gloo group, all-reduces a 1 and rank 0 prints the rank count")
    args = ap.parse_args()

    # --gpus N is the number of ranks of the job.  Launched by torch.distributed.run (the driver's N > 1 command) the environment
    # carries WORLD_SIZE = N already; launched bare (`python bench.py --gpus 4`) this process becomes the launcher of N ranks --
    # one process per GPU, env rendezvous on 127.0.0.1, like the reference's distributed/launch.py:119-173.  A WORLD_SIZE that
    # disagrees with --gpus is an error, never a silent 1-rank run.
    if args.gpus is None:                     # `torchrun --nproc-per-node 8 bench.py` without --gpus: the launcher's world size
        args.gpus = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} (or without a launcher: "
              f"`python bench.py --gpus {args.gpus}` starts the ranks itself)", file=sys.stderr)
        raise SystemExit(2)
    if args.dist_dry_run:
        raise SystemExit(dist_dry_run(world, rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    if args.one_device:
        if args.dist_backend == "nccl" and world > 1:
            raise SystemExit("bench.py: --one-device puts every rank on GPU 0, which RCCL refuses: add --dist-backend gloo")
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} wants GPU {local_rank}, this node has {torch.cuda.device_count()}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    dp = world > 1 or args.force_dist          # the data-parallel code path (also reachable at world size 1 for testing)
    ranks_seen = 1
    if dp:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", str(rank))
        os.environ.setdefault("WORLD_SIZE", str(world))
        if args.dist_backend == "nccl":
            _init_group(dist, "nccl", rank, world, device_id=dev)
        else:
            _init_group(dist, "gloo", rank, world)
        one = torch.ones(1, device=dev)
        dist.all_reduce(one)                   # n_gpus of the line = the ranks RCCL actually summed over
        ranks_seen = int(one.item())
        if ranks_seen != world:
            raise SystemExit(f"bench.py: RCCL reduced over {ranks_seen} ranks, WORLD_SIZE is {world}")

    from seq2seq_vc_amd.ops import functional as Fn
    from seq2seq_vc_amd.ops import kernels as K

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if args.roofline_only:
        print(json.dumps(dominant_kernel_roofline(dtype, iters=200, workload=args.workload)))
        return
    Fn.set_compute_dtype(dtype)
    if args.side_streams is None:
        n_side, inline = (4, args.inline_batches) if args.workload in ("vtn", "tts") else (0, True)
    else:
        n_side, inline = args.side_streams, args.inline_batches
    Fn.enable_side_streams(n_side, inline_batches=inline, batch=args.grad_batch)
    K.manual_seed(1234 + rank)

    B = args.batch or {"vtn": 32, "aasvc": 16, "tts": 8}[args.workload]
    wl = Workload(args.workload, dev, dtype, B, world, rank, frames=args.frames)
    # Data parallel: backward in the stages of model.dp_plan(), one captured graph per stage, the all-reduce of a finished stage's
    # slice of the flat gradient buffer issued between the replays (overlap).  N = 1 keeps one graph (the cuts cost ~0.2 ms).
    staged = dp or args.split_backward
    if args.grad_payload is None:
        from seq2seq_vc_amd import trainers as TR      # what the workload's product trainer defaults to (fp32 = the reference's DDP)
        args.grad_payload = (TR.AASVCTrainer if args.workload == "aasvc" else TR.ARVCTrainer).DP_GRAD_PAYLOAD
    if args.dp_decoder_stages:
        wl.model.dp_decoder_stages = args.dp_decoder_stages      # AAS-VC: decoder layers with a stage (= a bucket) of their own
    wl.keep_outputs = bool(args.dump_outputs) and rank == 0
    def build(stage_mode):
        return build_step(wl, dist, world, staged, args.force_dist, args.grad_payload, not args.no_graph, collective=args.collective,
                          warmup_eager=max(2, args.warmup if args.no_graph else 2), stage_mode=stage_mode, min_bucket_mb=args.min_bucket_mb)
    err = None
    try:
        step, info = build(args.stage_mode)
    except Exception as e:  # noqa: BLE001 -- the flush exchange has only ever run on one GPU: fall back to the stage graphs of rounds 2-5, loudly
        if not (staged and args.stage_mode == "flush"):
            raise
        err = e
    failed = err is not None
    if dp and staged and args.stage_mode == "flush":      # the ranks fall back TOGETHER (a rank on another exchange would hang the rest)
        flag = torch.tensor([1 if failed else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        failed = bool(flag.item())
    if failed:
        why = f"{type(err).__name__}: {err}" if err is not None else "another rank failed"
        print(f"[bench] --stage-mode flush failed ({why}); falling back to --stage-mode graphs", file=sys.stderr)
        torch.cuda.synchronize()
        wl.Fn._Side.on_flush = None
        step, info = build("graphs")
        info["stage_mode_fallback_from"] = "flush"
    probe = info.pop("_probe")
    check = info.pop("_check")
    dt = time_steps(step, args.steps, args.warmup, dist if dp else None, dev)
    if args.dump_outputs and rank == 0:
        print(f"[bench] outputs of the last timed step in {args.dump_outputs}: {dump_outputs(wl, args.dump_outputs)}", file=sys.stderr)
    if args.check_exchange:
        info["exchange_check"] = check()
    if args.stage_times:
        info["stage_ms_alone"] = probe()
    if dp:
        ft = torch.tensor([wl.frames], device=dev)
        dist.all_reduce(ft)
        frames = float(ft.item())
    else:
        frames = wl.frames
    ms = dt / args.steps * 1e3
    losses = wl.loss_buf.tolist()
    stats = wl.opt.last_stats()
    if not all(map(lambda v: v == v and abs(v) < 1e6, losses)):
        raise SystemExit(f"bench: non-finite loss {losses}")

    if rank == 0:
        out = {
            "metric": "mel-frames/sec (train)", "value": frames / (dt / args.steps), "unit": "mel-frames/sec",
            "n_gpus": ranks_seen, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": wl.desc, "batch_per_gpu": B, "global_batch": B * world, "T_src": wl.T_src, "T_tgt": wl.T_tgt, "mel_dim": 80,
                       "params_M": round(wl.params_m, 2), "parallelism": f"dp{world}", "split_backward": bool(staged),
                       **({"dist_backend": args.dist_backend, "one_device": bool(args.one_device)} if dp else {}),
                       "valid_target_frames_per_step": frames, **info},
            "final_losses": dict(zip(wl.loss_names, losses), grad_norm=stats["grad_norm"], opt_steps=stats["step"]),
            "step_mfma": step_mfma(args.workload, ms),
        }
        if args.full:
            out["roofline"] = dominant_kernel_roofline(dtype, workload="vtn" if args.workload == "tts" else args.workload)
        single = world == 1 and not args.force_dist
        if args.full and single and not args.no_cpu_baseline:
            out["cpu_baseline"] = {"vtn": cpu_baseline_vtn, "aasvc": cpu_baseline_aasvc, "tts": cpu_baseline_tts}[args.workload](wl.cpu_batch)
            out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
        if args.full and single and args.workload == "vtn" and not args.no_extras:
            del step
            wl.model = wl.opt = None
            torch.cuda.empty_cache()
            # the sub-objects must never cost the headline line: a failure is reported in place
            for key, fn in (("aasvc", lambda: bench_aasvc_single(dev, dtype, cpu=not args.no_cpu_baseline)),
                            ("tts", lambda: bench_tts_single(dev, dtype, cpu=not args.no_cpu_baseline)),
                            ("decode", lambda: bench_decode(dev, dtype, cpu=not args.no_cpu_baseline)),
                            ("trainer", lambda: bench_product_trainer(dev, dtype)),
                            ("alignment", lambda: bench_alignment_kernels(dev, cpu=not args.no_cpu_baseline)),
                            ("memory_bound", lambda: bench_memory_bound(dev))):
                try:
                    out[key] = fn()
                except Exception as e:  # noqa: BLE001
                    out[key] = {"error": f"{type(e).__name__}: {e}"}
                    print(f"[bench] sub-benchmark '{key}' failed: {type(e).__name__}: {e}", file=sys.stderr)
                Fn.enable_side_streams(0)
        out = _shape_line(out)
        # RCCL writes its version banner to the C-level stdout; flush that buffer first so the JSON line stays the last line
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        print(json.dumps(out), flush=True)
    if dp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
