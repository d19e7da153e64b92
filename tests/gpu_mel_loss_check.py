"""LogMelSpectrogram and its fused L1 loss on the MI355X (csrc/melspec.hip, seq2seq_vc_amd/urhythmic/dataset.py) against the plain-torch
restatement in tests/mel_loss_ref.py.  Each case returns [(ok, message)]; tests/test_gpu_mel_loss.py turns them into pytest tests.

Yardstick: step_kernels_ref.compare, unchanged -- |got - ref64| <= 4 d + ulp_out at every element, d = max |yard - ref64| (the restatement
in float32 against itself in float64, gradients by torch autograd).  The scalar loss: mel_loss_ref.loss_bound.  Inputs, references and
the conditions they satisfy are those of tests/test_mel_loss_host.py.  Every kernel writes into buffers pre-filled with NaN, so an
element it leaves out fails.  Nothing here is fitted to what the kernels return."""
import torch

import mel_loss_ref as MR
import step_kernels_ref as R
import vocoder_ref as VR
from seq2seq_vc_amd import _lib
from seq2seq_vc_amd.ops import functional as Fn
from seq2seq_vc_amd.ops import kernels_melspec as KM
from seq2seq_vc_amd.urhythmic.dataset import LogMelSpectrogram
from seq2seq_vc_amd.vocoder import HifiganGenerator

DEV = "cuda:0"
F32 = torch.float32


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def _held(res, tag, got, pair):
    ok, ratio, d, msg = R.compare(got.cpu(), pair[0], pair[1], F32)
    res.append((ok, f"{tag}: {msg}"))


def _kernel_level(inp, fused):
    """The launchers themselves on NaN-filled outputs -> (logmel, loss or None, frames, dwav)"""
    cfg = inp["cfg"]
    wav, hop, pad, nm = inp["wav"].to(DEV), cfg["hop_length"], inp["pad"], cfg["n_mels"]
    B, N = wav.shape
    T = inp["T"]
    tab = KM.tables(torch.device(DEV), cfg["sample_rate"], cfg["n_fft"], nm)
    mel, logmel, frames, dwav = _nan(B, nm, T), _nan(B, nm, T), _nan(B, T, KM.N_FFT), _nan(B, N)
    loss = None
    if fused:
        tgt = inp["tgt"].to(DEV)
        _, _, partials = KM.melspec_fwd(wav, tab, hop, pad, nm, tgt=tgt, mel=mel, logmel=logmel)
        loss = KM.melspec_loss_finish(partials, B * nm * T, loss=_nan(1))
        KM.melspec_bwd_frames(wav, tab, hop, pad, mel, logmel=logmel, tgt=tgt, gout=torch.ones(1, device=DEV), gscale=1.0 / (B * nm * T),
                              frames=frames)
    else:
        KM.melspec_fwd(wav, tab, hop, pad, nm, mel=mel, logmel=logmel)
        KM.melspec_bwd_frames(wav, tab, hop, pad, mel, g_logmel=inp["g_logmel"].to(DEV), frames=frames)
    KM.melspec_bwd_ola(frames, N, hop, pad, dwav=dwav)
    return logmel, loss, frames, dwav


def _table_case(name):
    res = []
    inp, ref = MR.inputs(name), MR.reference(name)
    cfg = inp["cfg"]
    B, N = inp["wav"].shape
    nm, T = cfg["n_mels"], inp["T"]
    res.append((KM.melspec_supported(cfg["n_fft"], cfg["win_length"], nm), "the library takes this configuration"))
    logmel, _, frames, dwav = _kernel_level(inp, fused=False)
    _held(res, f"{name}: log-mel", logmel, ref["logmel"])
    _held(res, f"{name}: dwav, generic path", dwav, ref["dwav"])
    logmel_f, loss, frames_f, dwav_f = _kernel_level(inp, fused=True)
    _held(res, f"{name}: dwav, fused loss", dwav_f, ref["dwav_l1"])
    res.append((R.bits_equal(logmel_f, logmel), f"{name}: the forward with a target writes the same log-mel bits"))
    err, bar = abs(float(loss.double().cpu()) - float(ref["loss"][0])), MR.loss_bound(name)
    res.append((err <= bar, f"{name}: loss {float(loss):.9g} vs float64 {float(ref['loss'][0]):.12g}: |diff| {err:.3e}, bound {bar:.3e} "
                            f"(float32 restatement: {abs(float(ref['loss'][1]) - float(ref['loss'][0])):.3e})"))
    fin = all(bool(torch.isfinite(t).all()) for t in (frames, dwav, frames_f, dwav_f, logmel))
    res.append((fin, f"{name}: every frame gradient and every dwav element is written and finite (silent frames included)"))
    # the module: same bits as the launchers, the reference's layouts, one autograd node
    mod = LogMelSpectrogram(**cfg)
    x = inp["wav"].to(DEV).unsqueeze(1).requires_grad_(True)
    y = mod(x)
    node_ok = y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_LogMelFunction") and tuple(y.shape) == (B, 1, nm, T)
    y.backward(inp["g_logmel"].to(DEV).unsqueeze(1))
    res.append((node_ok and R.bits_equal(y.detach(), logmel.unsqueeze(1)) and R.bits_equal(x.grad, dwav.unsqueeze(1)),
                f"{name}: forward(wav (B, 1, N)) -> {tuple(y.shape)}, one node {type(y.grad_fn).__name__}; log-mel and dwav equal the launchers' bits"))
    x2 = inp["wav"].to(DEV).requires_grad_(True)
    y2 = mod(x2)
    res.append((tuple(y2.shape) == (B, nm, T) and R.bits_equal(y2.detach(), logmel), f"{name}: forward(wav (B, N)) -> {tuple(y2.shape)}, the same bits"))
    for shape_tag, xin, tg in (("(B, 1, N)", inp["wav"].to(DEV).unsqueeze(1), inp["tgt"].to(DEV).unsqueeze(1)), ("(B, N)", inp["wav"].to(DEV), inp["tgt"].to(DEV))):
        xin = xin.requires_grad_(True)
        l, lm = mod.l1_loss(xin, tg)
        shape_ok = l.dim() == 0 and tuple(lm.shape) == (B, 1, nm, T) and not lm.requires_grad and type(l.grad_fn).__name__.startswith("_MelL1Function")
        l.backward()
        res.append((shape_ok and R.bits_equal(l.detach().reshape(1), loss) and R.bits_equal(lm, logmel.unsqueeze(1))
                    and R.bits_equal(xin.grad.reshape(B, N), dwav_f),
                    f"{name}: l1_loss(wav {shape_tag}) -> 0-d loss and {tuple(lm.shape)} log-mel, one node; loss, log-mel and dwav equal the launchers' bits"))
    return res


def case_one_frame():
    return _table_case("one_frame")


def case_ragged_tail():
    return _table_case("ragged_tail")


def case_silence():
    return _table_case("silence")


def case_finetune():
    return _table_case("finetune")


def case_other_cfg():
    return _table_case("other_cfg")


def case_quiet_frame():
    return _table_case("quiet_frame")


def bits():
    res = []
    for name in ("finetune", "one_frame", "other_cfg"):
        inp = MR.inputs(name)
        cfg = inp["cfg"]
        mod = LogMelSpectrogram(**cfg)
        wav, tgt, g = inp["wav"].to(DEV), inp["tgt"].to(DEV), inp["g_logmel"].to(DEV)

        def run():
            x = wav.clone().requires_grad_(True)
            y = mod(x)
            y.backward(g)
            xl = wav.clone().requires_grad_(True)
            l, lm = mod.l1_loss(xl, tgt)
            l.backward()
            return y.detach(), x.grad, l.detach(), lm, xl.grad
        a, b = run(), run()
        res.append((all(R.bits_equal(p, q) for p, q in zip(a, b)), f"{name}: two calls are bit-equal (log-mel, dwav, loss, dwav of the loss)"))
        with torch.no_grad():
            y0 = mod(wav.unsqueeze(1))
        res.append((y0.grad_fn is None and R.bits_equal(y0, a[3]), f"{name}: forward under no_grad equals the log-mel l1_loss returns, bit for bit"))
        same = []
        for b_ in range(wav.shape[0]):
            x1 = wav[b_:b_ + 1].clone().requires_grad_(True)
            y1 = mod(x1)
            y1.backward(g[b_:b_ + 1])
            same.append(R.bits_equal(y1.detach(), a[0][b_:b_ + 1]) and R.bits_equal(x1.grad, a[1][b_:b_ + 1]))
        res.append((all(same), f"{name}: every batch row equals its own B = 1 call bit for bit (log-mel and generic-path dwav): {same}"))
    return res


def _count_launches(fn):
    """Calls into the HIP library during fn (tools/bench_aasvc_infer.py: every launcher returns through _lib.check)"""
    real, n = _lib.check, [0]

    def counting(rc, what):
        n[0] += 1
        return real(rc, what)
    _lib.check = counting
    try:
        out = fn()
    finally:
        _lib.check = real
    return n[0], out


def launch_budget():
    res = []
    inp = MR.inputs("finetune")
    mod = LogMelSpectrogram(**inp["cfg"])
    wav, tgt, g = inp["wav"].to(DEV).unsqueeze(1), inp["tgt"].to(DEV).unsqueeze(1), inp["g_logmel"].to(DEV).unsqueeze(1)
    mod(wav)                                                                     # tables built

    def no_grad():
        with torch.no_grad():
            return mod(wav)
    n, _ = _count_launches(no_grad)
    res.append((n == 1, f"forward under no_grad: {n} launch(es) (budget 1)"))
    x = wav.clone().requires_grad_(True)
    n, y = _count_launches(lambda: mod(x))
    res.append((n == 1, f"forward under grad mode: {n} launch(es) (budget 1)"))
    n, _ = _count_launches(lambda: y.backward(g))
    res.append((n == 2, f"its backward: {n} launches (budget 2)"))
    x = wav.clone().requires_grad_(True)
    n, (l, _) = _count_launches(lambda: mod.l1_loss(x, tgt))
    res.append((n == 2, f"l1_loss forward: {n} launches (budget 2)"))
    n, _ = _count_launches(l.backward)
    res.append((n == 2, f"l1_loss backward: {n} launches (budget 2)"))
    return res


def through_the_generator():
    """loss = mel.l1_loss(generator(units), tgt); loss.backward(): the parameter gradients equal, bit for bit, those of
    generator(units).backward(gradient=dwav) with dwav from the same loss on a detached leaf copy of the waveform (the generator's
    backward is deterministic, so this pins the autograd plumbing and nothing else)."""
    res = []
    cfg, sd, _, _, _ = VR.load_fixture()
    gen = HifiganGenerator(**cfg)
    gen.load_state_dict(sd)
    gen.to(DEV).trainable()
    mod = LogMelSpectrogram()
    units = R.randn(2, 80, 12, seed=77).to(DEV)                                  # -> 2 x 768 samples, two frames
    prev = Fn.compute_dtype()
    Fn.set_compute_dtype(F32)
    try:
        with torch.no_grad():
            wav0 = gen(units)
            lm0 = mod(wav0)
            off = (torch.rand(lm0.shape, generator=R.gen(78)) * 0.9 + 0.1) * (torch.randint(0, 2, lm0.shape, generator=R.gen(79)) * 2 - 1)
            tgt = lm0 + off.to(DEV)
        gen.zero_grad(set_to_none=True)
        wav = gen(units)
        loss, _ = mod.l1_loss(wav, tgt)
        loss.backward()
        ga = {k: p.grad.detach().clone() for k, p in gen.named_parameters()}
        leaf = gen(units).detach().clone().requires_grad_(True)
        loss2, _ = mod.l1_loss(leaf, tgt)
        loss2.backward()
        gen.zero_grad(set_to_none=True)
        gen(units).backward(gradient=leaf.grad)
        gb = {k: p.grad.detach().clone() for k, p in gen.named_parameters()}
    finally:
        Fn.set_compute_dtype(prev)
    res.append((tuple(wav.shape) == (2, 1, 768) and wav.grad_fn is not None and R.bits_equal(loss.detach(), loss2.detach()),
                f"generator(units) {tuple(wav.shape)} with a grad_fn; loss {float(loss.detach()):.6f}"))
    bad = [k for k, v in ga.items() if not bool(torch.isfinite(v).all()) or not bool((v != 0).any())]
    res.append((len(ga) > 100 and not bad, f"{len(ga)} parameters, every gradient finite and not all zero (offenders: {bad[:5]})"))
    diff = [k for k in ga if not R.bits_equal(ga[k], gb[k])]
    res.append((not diff, f"gradients through the loss node equal those of generator(units).backward(gradient=dwav) bit for bit (differing: {diff[:5]})"))
    return res


CASES = [case_one_frame, case_ragged_tail, case_silence, case_finetune, case_other_cfg, case_quiet_frame, bits, launch_budget,
         through_the_generator]
