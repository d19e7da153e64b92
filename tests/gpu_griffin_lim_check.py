"""Griffin-Lim vocoder on the MI355X against the numpy restatement in tests/griffin_lim_ref.py.  Each case returns [(ok, message)];
tests/test_gpu_griffin_lim.py turns them into pytest tests.

Yardstick (every numeric case): the restatement is run on the same input in float64 (the truth) and in float32; their distance
d = max |f32 - f64| is what fp32 arithmetic costs on this input.  The GPU result must lie within MARGIN x d of the float64 run, with
a floor of FLOOR x the signal's peak.  The margin covers a different FFT factorisation and table rounding than pocketfft's (errors
of the same order, not the same bits); a wrong window, envelope, trim or momentum term is three or more orders above it.
One quantity is held per bin instead of globally, the projected spectrum X of a single iteration: see _verdict_projected (measured
on the MI355X: literal global ratios 0.43 - 2.72 on seven of the eight inputs, 10.41 on the 2048 / 300 / 1200 reflect first-iteration
input where the projection's gain reaches 1.1e5; R on the same input 1.58).  Nothing here is fitted to what the kernels return."""
import numpy as np
import torch

import griffin_lim_ref as GR
from seq2seq_vc_amd import frontend
from seq2seq_vc_amd.ops import kernels_griffin_lim as KG
from seq2seq_vc_amd.vocoder import Spectrogram2Waveform, griffin_lim, istft, logmel2linear

DEV = "cuda:0"
MARGIN = 4.0
FLOOR = 1e-6
CONVERGENCE_SLACK = 1.02
GEOMETRIES = [(512, 128, None), (1024, 256, None), (2048, 300, 1200), (2048, 512, None)]
FS, N_MELS, FMIN, FMAX = 16000, 80, 80, 7600


def _verdict(res, tag, got, f32, f64):
    got, f32, f64 = (np.asarray(a) for a in (got, f32, f64))
    if got.shape != f64.shape:
        res.append((False, f"{tag}: shape {got.shape} vs {f64.shape}"))
        return
    d = float(np.abs(f32 - f64).max())
    peak = float(np.abs(f64).max())
    err = float(np.abs(got - f64).max())
    bar = max(MARGIN * d, FLOOR * peak)
    res.append((bool(np.isfinite(got).all()) and err <= bar,
                f"{tag}: GPU-vs-float64 {err:.3e}, float32-vs-float64 {d:.3e}, ratio {err / max(d, 1e-300):.2f} (bar {MARGIN} x, floor "
                f"{FLOOR * peak:.1e}), peak {peak:.3g}"))


def _verdict_projected(res, tag, got, f32, f64, S, A64, d_R):
    """The projected spectrum X = S A / (|A| + tiny) of one iteration.  The map A -> A / |A| has the local gain k = S / |A|, and a
    spectrum of ~1e5 bins always has a few bins where A nearly vanishes (k of 1e3 .. 1e5 here, from the float64 run): there an
    error in R far BELOW the R bar moves X by more than MARGIN x the global float32-vs-float64 distance of X, and the float32 leg's
    own error at such a bin is one draw of noise, not a yardstick (on the 2048 / 300 / 1200 reflect first-iteration input torch's CPU
    fp32 stft / istft lands 40.6 x the numpy float32 leg's distance, at frame 0, bin 868, k = 1.1e5).  So the bar is per bin:
    max(MARGIN d_X, floor, MARGIN k_bin d_R) -- the issue's rule wherever k_bin <= d_X / d_R, and what an R error of the size the R bar
    admits amounts to where the projection is singular.  k, d_X and d_R come from the restatement alone.  The literal global ratio
    is printed beside it."""
    got, f32, f64 = (np.asarray(a) for a in (got, f32, f64))
    d = float(np.abs(f32 - f64).max())
    peak = float(np.abs(f64).max())
    gain = np.asarray(S, np.float64) / np.maximum(np.abs(A64), np.finfo(np.float64).tiny)
    bar = np.maximum(max(MARGIN * d, FLOOR * peak), MARGIN * gain * d_R)
    err = np.abs(got - f64)
    over = err > bar
    i = np.unravel_index(err.argmax(), err.shape)
    res.append((bool(np.isfinite(got).all()) and not over.any(),
                f"{tag}: bins over the per-bin bar: {int(over.sum())} of {over.size}; GPU-vs-float64 {float(err.max()):.3e} at frame {i[0]} bin {i[1]} "
                f"(gain S/|A| there {float(gain[i]):.3g}, largest gain {float(gain.max()):.3g}), float32-vs-float64 {d:.3e}, literal global ratio "
                f"{float(err.max()) / max(d, 1e-300):.2f}, bins with gain above d_X / d_R: {int((gain * d_R > d).sum())}"))


def _c(t):
    """device (.., 2) real -> numpy complex"""
    a = t.detach().cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _spectrogram(n_fft, hop, wl, seconds=2.0, seed=0):
    y = GR.make_signal(seconds, FS, seed)
    S = np.abs(GR.stft(y, n_fft, hop, wl, "constant"))
    u = np.random.default_rng(seed + 100).uniform(0, 1, S.shape).astype(np.float32)
    return S.astype(np.float32), u


def istft_alone():
    res = []
    for i, (n_fft, hop, wl) in enumerate(GEOMETRIES):
        rng = np.random.default_rng(10 + i)
        T = 23
        X = (rng.standard_normal((T, n_fft // 2 + 1)) + 1j * rng.standard_normal((T, n_fft // 2 + 1))).astype(np.complex64)
        y = istft(torch.from_numpy(X).to(DEV), n_fft, hop, wl)
        y2 = istft(torch.view_as_real(torch.from_numpy(X)).to(DEV), n_fft, hop, wl)
        res.append((tuple(y.shape) == (hop * (T - 1),) and y.dtype == torch.float32 and torch.equal(y, y2),
                    f"istft {n_fft}/{hop}/{wl}: {tuple(y.shape)} samples, complex and (.., 2) inputs agree bit for bit"))
        _verdict(res, f"istft {n_fft}/{hop}/{wl}", y.cpu().numpy(), GR.istft(X, n_fft, hop, wl, np.float32), GR.istft(X, n_fft, hop, wl, np.float64))
    return res


def one_iteration():
    res = []
    for n_fft, hop, wl in ((1024, 256, None), (2048, 300, 1200)):
        S, u = _spectrogram(n_fft, hop, wl, seconds=1.0, seed=3)
        X0 = GR.initial(S, u, np.float64)
        X1, R1 = GR.gl_iteration(X0, None, S, n_fft, hop, wl, 0.99, "constant", np.float64)
        for pad_mode in ("constant", "reflect"):
            for tag, X, Rp in (("first iteration (no R_prev)", X0, None), ("with R_prev", X1, R1)):
                X = X.astype(np.complex64)
                Rp = None if Rp is None else Rp.astype(np.complex64)
                want64 = GR.gl_iteration(X, Rp, S, n_fft, hop, wl, 0.99, pad_mode, np.float64)
                want32 = GR.gl_iteration(X, Rp, S, n_fft, hop, wl, 0.99, pad_mode, np.float32)
                tab = KG.tables(torch.device(DEV), n_fft, wl)
                Xd = torch.view_as_real(torch.from_numpy(X)).to(DEV).unsqueeze(0).contiguous()
                Pd = torch.full_like(Xd, float("nan")) if Rp is None else torch.view_as_real(torch.from_numpy(Rp)).to(DEV).unsqueeze(0).contiguous()
                Sd = torch.from_numpy(S).to(DEV).unsqueeze(0)
                frames = KG.gl_synth(Xd, n_fft, tab)
                KG.gl_analyse(frames, Sd, Xd, Pd, n_fft, hop, tab, 0.99 / 1.99, have_prev=Rp is not None, reflect=pad_mode == "reflect")
                name = f"iteration {n_fft}/{hop}/{wl} {pad_mode}, {tag}"
                _verdict(res, name + ": R", _c(Pd[0]), want32[1], want64[1])
                A64 = want64[1] if Rp is None else want64[1] - 0.99 / 1.99 * Rp.astype(np.complex128)
                _verdict_projected(res, name + ": X", _c(Xd[0]), want32[0], want64[0], S, A64, float(np.abs(want32[1] - want64[1]).max()))
    return res


def griffin_lim_few_iterations():
    res = []
    n_fft, hop, wl = 1024, 256, None
    S, u = _spectrogram(n_fft, hop, wl)
    for n_iter in (4, 8):
        y = griffin_lim(torch.from_numpy(S).to(DEV), n_fft, hop, wl, n_iter=n_iter, init_phase=torch.from_numpy(u))
        res.append((tuple(y.shape) == (hop * (S.shape[0] - 1),) and y.is_cuda, f"n_iter {n_iter}: {tuple(y.shape)} samples on the device"))
        _verdict(res, f"griffin_lim {n_fft}/{hop} n_iter {n_iter}", y.cpu().numpy(),
                 GR.griffin_lim(S, u, n_fft, hop, wl, n_iter, dtype=np.float32), GR.griffin_lim(S, u, n_fft, hop, wl, n_iter, dtype=np.float64))
    # the other geometries and the reflect padding, 4 iterations
    for (n_fft, hop, wl), pad_mode in (((2048, 300, 1200), "constant"), ((512, 128, None), "reflect"), ((2048, 512, None), "reflect")):
        S, u = _spectrogram(n_fft, hop, wl, seconds=1.0, seed=5)
        y = griffin_lim(torch.from_numpy(S).to(DEV), n_fft, hop, wl, n_iter=4, init_phase=u, pad_mode=pad_mode)
        _verdict(res, f"griffin_lim {n_fft}/{hop}/{wl} {pad_mode} n_iter 4", y.cpu().numpy(),
                 GR.griffin_lim(S, u, n_fft, hop, wl, 4, pad_mode=pad_mode, dtype=np.float32),
                 GR.griffin_lim(S, u, n_fft, hop, wl, 4, pad_mode=pad_mode, dtype=np.float64))
    return res


def griffin_lim_64_iterations():
    res = []
    n_fft, hop, wl, n_iter = 1024, 256, None, 64
    S, u = _spectrogram(n_fft, hop, wl)
    before = KG.LAUNCHES
    y = griffin_lim(torch.from_numpy(S).to(DEV), n_fft, hop, wl, n_iter=n_iter, init_phase=u).cpu().numpy()
    launches = KG.LAUNCHES - before
    res.append((launches == 2 * n_iter + 3, f"launches of one call with n_iter {n_iter}: {launches} (2 n_iter + 3 = {2 * n_iter + 3})"))
    y64 = GR.griffin_lim(S, u, n_fft, hop, wl, n_iter, dtype=np.float64)
    y32 = GR.griffin_lim(S, u, n_fft, hop, wl, n_iter, dtype=np.float32)
    _verdict(res, f"griffin_lim {n_fft}/{hop} n_iter {n_iter}", y, y32, y64)
    c, c64, c32 = (GR.spectral_convergence(v, S, n_fft, hop, wl) for v in (y, y64, y32))
    res.append((c <= CONVERGENCE_SLACK * c64, f"spectral convergence after {n_iter} iterations: GPU {c:.6f}, float64 {c64:.6f}, float32 {c32:.6f} "
                f"(bar: no more than {CONVERGENCE_SLACK} x the float64 run's)"))
    return res


def batch_rows_equal_single_calls():
    res = []
    n_fft, hop = 1024, 256
    S, u = _spectrogram(n_fft, hop, None, seconds=0.7, seed=7)
    lens = [S.shape[0], 27, 13, 2]
    B, Tmax, nb = len(lens), S.shape[0], S.shape[1]
    rng = np.random.default_rng(8)
    spcs = np.stack([S * rng.uniform(0.5, 1.5) for _ in lens]).astype(np.float32)
    us = rng.uniform(0, 1, (B, Tmax, nb)).astype(np.float32)
    dirty, dirty_u = spcs.copy(), us.copy()
    for b, n in enumerate(lens):                              # garbage in the padded frames: the kernels never read them
        dirty[b, n:], dirty_u[b, n:] = np.nan, np.nan
    voc = Spectrogram2Waveform(n_fft, hop, griffin_lim_iters=6, take_norm_feat=False, fs=FS)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ys, ns, fs = voc.decode_batch(torch.from_numpy(dirty).to(DEV), lens_d, init_phase=torch.from_numpy(dirty_u).to(DEV))
    ys2, _, _ = voc.decode_batch(torch.from_numpy(dirty).to(DEV), lens, init_phase=torch.from_numpy(dirty_u).to(DEV))
    res.append((tuple(ys.shape) == (B, hop * (Tmax - 1)) and fs == FS and ns.tolist() == [hop * (n - 1) for n in lens] and ns.is_cuda,
                f"decode_batch: ys {tuple(ys.shape)}, n_samples {ns.tolist()} on the device, fs {fs}"))
    res.append((torch.equal(ys, ys2), "two identical calls (device lengths / host lengths) are bit-equal"))
    for b, n in enumerate(lens):
        y1, _ = voc.decode(torch.from_numpy(spcs[b, :n]).to(DEV), init_phase=us[b, :n])
        m = hop * (n - 1)
        same = tuple(y1.shape) == (m,) and torch.equal(ys[b, :m], y1)
        zero = bool((ys[b, m:] == 0).all())
        alive = bool(torch.isfinite(y1).all()) and float(y1.abs().max()) > 0
        res.append((same and zero and alive, f"row {b} ({n} frames): equals the single decode bit for bit: {same}; samples past {m} are zero: {zero}; "
                                             f"finite and non-zero: {alive}"))
    a, _, _ = voc.decode_batch(torch.from_numpy(spcs).to(DEV), lens, seed=11)
    b_, _, _ = voc.decode_batch(torch.from_numpy(spcs).to(DEV), lens, seed=11)
    c, _, _ = voc.decode_batch(torch.from_numpy(spcs).to(DEV), lens, seed=12)
    res.append((torch.equal(a, b_) and not torch.equal(a, c) and bool(torch.isfinite(a).all()),
                f"the same seed gives the same waveform: {torch.equal(a, b_)}; another seed another one: {not torch.equal(a, c)}"))
    return res


def decode_normalised_logmel():
    res = []
    n_fft, hop = 1024, 256
    S, u = _spectrogram(n_fft, hop, None, seconds=1.5, seed=9)
    basis = frontend.mel_basis(FS, n_fft, N_MELS, FMIN, FMAX)
    lmspc = np.log10(np.maximum(1e-10, S.astype(np.float64) @ basis.astype(np.float64).T))
    stats = dict(mean=lmspc.mean(0), scale=lmspc.std(0) + 0.1)
    norm = ((lmspc - stats["mean"]) / stats["scale"]).astype(np.float32)
    lm32 = lmspc.astype(np.float32)
    lin = logmel2linear(torch.from_numpy(lm32).to(DEV), FS, n_fft, N_MELS, FMIN, FMAX)
    res.append((tuple(lin.shape) == (S.shape[0], n_fft // 2 + 1) and lin.dtype == torch.float32 and lin.is_cuda and float(lin.min()) >= 1e-10,
                f"logmel2linear: {tuple(lin.shape)} fp32 on the device, min {float(lin.min()):.1e}"))
    _verdict(res, "logmel2linear", lin.cpu().numpy(), GR.logmel2linear(lm32, basis, np.float32), GR.logmel2linear(lm32, basis, np.float64))
    voc = Spectrogram2Waveform(n_fft, hop, stats=stats, fs=FS, n_mels=N_MELS, fmin=FMIN, fmax=FMAX, griffin_lim_iters=8)
    x = torch.from_numpy(norm).to(DEV).to(torch.float64)
    y, fs = voc.decode(x, init_phase=u)
    res.append((fs == FS and y.dtype == torch.float64 and y.device == x.device and tuple(y.shape) == (hop * (S.shape[0] - 1),),
                f"decode: wav {tuple(y.shape)} in the input's dtype {y.dtype} on its device, fs {fs}"))
    _verdict(res, "Spectrogram2Waveform.decode, normalised log-mel, n_iter 8", y.cpu().numpy(),
             GR.decode(norm, basis, stats, u, n_fft, hop, None, 8, dtype=np.float32), GR.decode(norm, basis, stats, u, n_fft, hop, None, 8, dtype=np.float64))
    yc, _ = voc.decode(torch.from_numpy(norm), init_phase=u)
    res.append((yc.device.type == "cpu" and yc.dtype == torch.float32 and np.array_equal(yc.numpy(), y.float().cpu().numpy()),
                "decode of a CPU tensor returns the same waveform on the CPU"))
    return res


CASES = [istft_alone, one_iteration, griffin_lim_few_iterations, griffin_lim_64_iterations, batch_rows_equal_single_calls,
         decode_normalised_logmel]
