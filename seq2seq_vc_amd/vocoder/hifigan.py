"""HiFi-GAN generator on the HIP kernels of csrc/hifigan.hip: mel -> waveform, single and batched; with `trainable()` also the
backward pass with respect to its parameters (csrc/hifigan_bwd.hip), for fine-tuning.

Drop-in surface of the reference's `seq2seq_vc/urhythmic/vocoder.py` HifiganGenerator (constructor keywords, defaults and
`state_dict` keys, with and without weight norm) and of `seq2seq_vc/vocoder/vocoder.py` Vocoder.decode.  Every convolution is one
launch; activation, residual, the MRF sum / average, tanh and the input transposition / normalisation / cast ride in the kernels'
prologues and epilogues, so a call of the default configuration is 79 launches (`launch_plan()`).  There is no CPU path.

Fine-tuning (reference: urhythmic_fine_tune_vocoder.py:191-222): `generator.trainable()` makes forward() return a tensor with a
grad_fn; one autograd Function takes every parameter as an input, so `.grad`, accumulation, zero_grad and DDP hooks work as on any
module.  The input never gets a gradient (units / mels are data).  One training forward is `train_plan()` (the folds, the
convolutions and, in bf16 mode, the casts of the stored activations), one backward pass `backward_plan()`.

The three lists are walked through one table from `kind` to handler (vocoder/plan.py) and built once per module."""
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from ..ops import functional as Fn
from ..ops import kernels_vocoder as KV
from .plan import Layer, PlanExecutor, WNConv, fold_calls, handles

LRELU_SLOPE = 0.1
POST_SLOPE = 0.01        # vocoder.py:103 applies F.leaky_relu with torch's DEFAULT slope in front of conv_post
KINDS = ("input", "conv1d", "tconv1d", "conv_out")   # the input launch + the kernel families a call may launch ("fold" runs at load)
TRAIN_KINDS = ("fold", "fold_bwd") + KINDS + ("cast",)     # a training forward folds from the live parameters and keeps its buffers
BWD_KINDS = ("conv_out_bwd", "wgrad", "finish", "conv1d_dgrad", "tconv1d_dgrad")    # the launches of one backward pass


# ---------------------------------------------------------------------------------------------------------------------------
# host logic of the transposed convolution as one GEMM (the kernel's addressing, stated once; tests evaluate it with plain torch)
# ---------------------------------------------------------------------------------------------------------------------------
def tconv1d_geometry(k, u):
    """(pad, ntaps) of ConvTranspose1d(kernel k, stride u, padding (k - u) / 2): output length is exactly u * T_in."""
    if u < 1 or k < u or (k - u) % 2:
        raise ValueError(f"ConvTranspose1d kernel {k} / stride {u}: needs k >= u and (k - u) even (padding (k - u) / 2)")
    return (k - u) // 2, -(-k // u)


def tconv1d_rows(t_in, k, u):
    """GEMM rows per utterance: i = 0 .. T_in + ceil(pad / u) - 1 (the last rows hold the tail taps of the last frames)."""
    pad, _ = tconv1d_geometry(k, u)
    return t_in + -(-pad // u)


def tconv1d_out_frame(i, p, k, u):
    """Row i, phase p is output frame u * i + p - pad (stored when it lies inside [0, u * T_in))."""
    return u * i + p - tconv1d_geometry(k, u)[0]


def tconv1d_operand(w, u, cin_padded=None):
    """w (C_in, C_out, k) -> [u * C_out, ntaps * Cp] with element [p * C_out + o][n * Cp + c] = w[c, o, p + u * n] (zero where
    p + u * n >= k or c >= C_in): row (i, :) of the GEMM reads input frames i - n, n = 0 .. ntaps - 1."""
    cin, cout, k = w.shape
    _, ntaps = tconv1d_geometry(k, u)
    cp = cin if cin_padded is None else cin_padded
    op = w.new_zeros(u, cout, ntaps, cp)
    for p in range(u):
        for n in range(ntaps):
            if p + u * n < k:
                op[p, :, n, :cin] = w[:, :, p + u * n].t()
    return op.reshape(u * cout, ntaps * cp)


def stage_lengths(lens, factors):
    """Frames of every utterance at the input of stage i (i = 0 .. len(factors)): lens * prod(factors[:i])."""
    out, m = [], 1
    for f in list(factors) + [None]:
        out.append([int(n) * m for n in lens])
        if f is not None:
            m *= int(f)
    return out


class ResBlock(nn.Module):
    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        mk = lambda: WNConv((channels, channels, kernel_size))   # noqa: E731
        self.convs1 = nn.ModuleList([mk() for _ in dilation])
        self.convs2 = nn.ModuleList([mk() for _ in dilation])


class _GeneratorFunction(torch.autograd.Function):
    """forward(x) of a trainable generator as ONE autograd node over all its parameters (x gets no gradient)."""

    @staticmethod
    def forward(ctx, gen, x, taps, *params):
        B, _, N = x.shape
        ctx.gen, ctx.state = gen, gen._run(x, B, N, (x.stride(0), x.stride(2), x.stride(1)), train=True, taps=taps)
        y = ctx.state.y.view(B, 1, -1)
        ctx.save_for_backward(y, *params)       # the parameters: autograd refuses a backward after an in-place update of one
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y = ctx.saved_tensors[0]
        return (None, None, None) + tuple(ctx.gen._backward(ctx.state, y, dy))


class HifiganGenerator(PlanExecutor):
    """HiFi-GAN generator (reference urhythmic/vocoder.py:23-114).  x (B, in_channels, N) -> (B, 1, N * prod(factors)).  Inference
    only until `trainable()` is called; then forward() under grad mode carries the parameter gradients."""

    def __init__(self, in_channels=256, resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), resblock_kernel_sizes=(3, 7, 11),
                 upsample_kernel_sizes=(20, 16, 4, 4), upsample_channels=512, upsample_factors=(10, 8, 2, 2), sample_rate=16000):
        super().__init__()
        if len(upsample_kernel_sizes) != len(upsample_factors) or len(resblock_kernel_sizes) != len(resblock_dilation_sizes):
            raise ValueError("upsample_kernel_sizes / upsample_factors and resblock_kernel_sizes / resblock_dilation_sizes pair up")
        for k, u in zip(upsample_kernel_sizes, upsample_factors):
            tconv1d_geometry(k, u)
        for k, ds in zip(resblock_kernel_sizes, resblock_dilation_sizes):
            if k % 2 == 0 or k > 11 or any(d < 1 or d > 5 for d in ds):
                raise ValueError("ResBlock kernels: odd k <= 11, dilations 1..5 (csrc/hifigan.hip)")
        if upsample_channels % (2 ** len(upsample_factors)) or not 1 <= in_channels <= 512 or upsample_channels > 512:
            raise ValueError("upsample_channels must halve cleanly at every stage; channels <= 512")
        self.in_channels, self.upsample_channels, self.sample_rate = in_channels, upsample_channels, sample_rate
        self.upsample_factors, self.upsample_kernel_sizes = tuple(upsample_factors), tuple(upsample_kernel_sizes)
        self.resblock_kernel_sizes = tuple(resblock_kernel_sizes)
        self.resblock_dilation_sizes = tuple(tuple(d) for d in resblock_dilation_sizes)
        self.num_kernels, self.num_upsamples = len(resblock_kernel_sizes), len(upsample_factors)
        self.conv_pre = WNConv((upsample_channels, in_channels, 5))
        self.ups = nn.ModuleList()
        self.resblocks = nn.ModuleList()
        for i, (u, k) in enumerate(zip(upsample_factors, upsample_kernel_sizes)):
            cin, cout = upsample_channels // 2 ** i, upsample_channels // 2 ** (i + 1)
            self.ups.append(WNConv((cin, cout, k), cout))
        for i in range(self.num_upsamples):
            ch = upsample_channels // 2 ** (i + 1)
            for k, d in zip(resblock_kernel_sizes, resblock_dilation_sizes):
                self.resblocks.append(ResBlock(ch, k, d))
        self.conv_post = WNConv((1, ch, 7))
        self._ops = {}            # compute dtype -> {layer name: Layer(operand, bias fp32)}: the inference path's cache
        self._trainable = False

    def trainable(self, mode=True):
        """Switch the backward pass on (or off again; off is the default and changes nothing).  On: forward() under grad mode
        returns a tensor with a grad_fn whose backward fills the .grad of every parameter, and EVERY call -- under no_grad and
        the batched ones too -- folds its operands from the live parameters, so an optimiser's in-place update is seen by the
        next call.  An input that requires grad is refused in either mode.  Under Fn.set_compute_dtype(bfloat16) the backward runs in
        bf16 (fp32 accumulation, fp32 parameter gradients) while the training forward keeps fp32 activations (train_plan)."""
        self._trainable = bool(mode)
        self._drop_cache()
        return self

    # ---- checkpoint forms -------------------------------------------------------------------------------------------------
    def _leaves(self):
        return [(n, m) for n, m in self.named_modules() if isinstance(m, WNConv)]

    def _drop_cache(self):
        self._ops = {}

    def load_state_dict(self, state_dict, strict=True, **kw):
        for name, m in self._leaves():
            if name + ".weight_v" in state_dict:
                m.set_form(True)
            elif name + ".weight" in state_dict:
                m.set_form(False)
        self._drop_cache()
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _apply(self, fn, *a, **kw):
        self._drop_cache()
        return super()._apply(fn, *a, **kw)

    def remove_weight_norm(self):
        """Replace (weight_g, weight_v) by the folded weight -- the fp32 values the kernels' operands were laid out from, so no
        output changes."""
        for name, m in self._leaves():
            if not m.normed:
                continue
            if m.weight_v.is_cuda:
                w = self._fold(name, m, None, want_op=False)[0]
            else:
                v = m.weight_v.detach()
                w = v * (m.weight_g.detach() / v.flatten(1).norm(dim=1).view(-1, 1, 1))
            m.set_form(False, w.to(m.bias.dtype))
        self._drop_cache()

    # ---- operands ---------------------------------------------------------------------------------------------------------
    def _layer_mode(self, name):
        if name.startswith("ups."):
            return 1, self.upsample_factors[int(name.split(".")[1])]
        return (2, 1) if name == "conv_post" else (0, 1)

    def _fold(self, name, m, dtype, want_w32=True, want_op=True):
        mode, u = self._layer_mode(name)
        with torch.no_grad():
            v, g = m.vg()
            return KV.hifigan_fold(mode, v, g, torch.float32 if dtype is None else dtype, u=u, want_w32=want_w32, want_op=want_op)

    def _operands(self, dtype):
        """Folded weights in the kernels' layouts for `dtype`: built once per load / device move, on the device."""
        if dtype not in self._ops:
            self._ops[dtype] = {name: Layer(None, None, m.bias.detach().float().contiguous(), op=self._fold(name, m, dtype, want_w32=False)[1])
                                for name, m in self._leaves()}
        return self._ops[dtype]

    # ---- the launch list --------------------------------------------------------------------------------------------------
    def launch_plan(self):
        """What one call launches, in order: dicts with `kind` in KINDS, the layer, source / destination buffers and the fused
        prologue / epilogue options.  forward() executes exactly this list."""
        uc = self.upsample_channels
        plan = [dict(kind="input", dst="x", cout=self.in_channels, mul=1),
                dict(kind="conv1d", layer="conv_pre", src="x", dst="pre", k=5, dil=1, cin=self.in_channels, cout=uc, slope=0.0, mul=1,
                     tap="conv_pre")]
        cur, mul = "pre", 1
        for i, (u, k) in enumerate(zip(self.upsample_factors, self.upsample_kernel_sizes)):
            cin, ch = uc // 2 ** i, uc // 2 ** (i + 1)
            plan.append(dict(kind="tconv1d", layer=f"ups.{i}", src=cur, dst=f"up{i}", k=k, u=u, cin=cin, cout=ch, slope=LRELU_SLOPE,
                             mul=mul, tap=f"ups.{i}"))
            mul *= u
            for j, (rk, dils) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)):
                x = f"up{i}"
                rb = f"resblocks.{i * self.num_kernels + j}"
                for q, d in enumerate(dils):
                    last = q == len(dils) - 1
                    plan.append(dict(kind="conv1d", layer=f"{rb}.convs1.{q}", src=x, dst=f"t{i}", k=rk, dil=d, cin=ch, cout=ch,
                                     slope=LRELU_SLOPE, mul=mul))
                    e = dict(kind="conv1d", layer=f"{rb}.convs2.{q}", src=f"t{i}", res=x, k=rk, dil=1, cin=ch, cout=ch, slope=LRELU_SLOPE,
                             mul=mul)
                    if last:      # x = xt + x is the block's output: it goes straight into the MRF average of the stage
                        e.update(dst=f"s{i}", accumulate=j > 0, scale=1.0 / self.num_kernels)
                        if j == self.num_kernels - 1:
                            e["tap"] = f"stage.{i}"
                    else:
                        x = f"a{i}" if x != f"a{i}" else f"b{i}"
                        e.update(dst=x)
                    plan.append(e)
            cur = f"s{i}"
        plan.append(dict(kind="conv_out", layer="conv_post", src=cur, k=7, cin=ch, slope=POST_SLOPE, mul=mul))
        return plan

    def train_plan(self, dtype=None):
        """What one training forward launches, in order: dicts with `kind` in TRAIN_KINDS.  Per leaf the fold from the live parameters
        (`op`: it lays out the operand too) and, for every layer whose input gets a gradient, the data gradient's operand; then
        launch_plan() with every convolution's output in a buffer of its own (the backward reads them all): the ping-pong buffers
        t{i} / a{i} / b{i} become `<layer>.out`; then, in bf16 mode (dtype: the compute dtype, None = the current one), one cast
        launch per kept buffer.  _run(train=True) executes exactly this list.
        The training forward keeps fp32 activations in EITHER compute mode: a leaky-relu mask is the sign of a stored
        pre-activation, and a bf16 forward's error flips hundreds of them (370 of 170 880 on the tests' tiny model, which alone
        puts every gradient 5 - 20 % from the exact one).  In bf16 mode the backward's GEMMs run in bf16 over copies of the stored
        tensors that one cast launch each (the input kernel) rounds to bf16 -- a rounding keeps the sign, so no mask flips."""
        plan, cur, kept = [], {}, []
        for name, _ in self._leaves():
            mode, u = self._layer_mode(name)
            plan.append(dict(kind="fold", layer=name, mode=mode, u=u, op=True))
            if mode != 2 and name != "conv_pre":
                plan.append(dict(kind="fold_bwd", layer=name, mode=mode, u=u))
        for e in self.launch_plan():
            e = dict(e)
            for key in ("src", "res"):
                if key in e:
                    e[key] = cur.get(e[key], e[key])
            dst = e.get("dst")
            if dst is not None and dst[0] in "tab" and dst[1:].isdigit():
                cur[dst] = e["dst"] = e["layer"] + ".out"
            if dst is not None and e["dst"] not in kept:
                kept.append(e["dst"])
            plan.append(e)
        if (Fn.compute_dtype() if dtype is None else dtype) != torch.float32:
            plan += [dict(kind="cast", src=name) for name in kept]
        return plan

    def backward_plan(self):
        """What one backward pass launches, in order: dicts with `kind` in BWD_KINDS.  `d:<buffer>` names the gradient of a forward
        buffer of train_plan().  Per convolution: the weight / bias partials ("wgrad"; conv_post's come from "conv_out_bwd"), the
        "finish" launch that writes the parameters' gradients, and -- except for conv_pre, whose input is data -- the data gradient.
        Every gradient buffer is written by one launch; d:up{i} is accumulated by the first unit of every ResBlock of the stage.
        The residual x' = conv2(..) + x is the `res` of conv1's data gradient, and the 1 / num_kernels of the MRF average is the
        `scale` of the launch that produces d:s{i}.  _backward() executes exactly this list."""
        nk = self.num_kernels
        plan, pending, written = [], {}, set()
        for e in reversed(self.train_plan(torch.float32)):
            kind, layer = e["kind"], e.get("layer")
            if kind not in KINDS[1:]:
                continue
            if kind == "conv_out":
                plan.append(dict(kind="conv_out_bwd", layer=layer, src=e["src"], dst="d:" + e["src"], k=e["k"], cin=e["cin"], slope=e["slope"],
                                 scale=1.0 / nk))
                plan.append(dict(kind="finish", layer=layer, mode=2, u=1))
                continue
            dy = "d:" + e["dst"]
            if kind == "tconv1d":
                plan.append(dict(kind="wgrad", layer=layer, conv=1, dy=dy, src=e["src"], k=e["k"], step=e["u"], slope=e["slope"]))
                plan.append(dict(kind="finish", layer=layer, mode=1, u=e["u"]))
                plan.append(dict(kind="tconv1d_dgrad", layer=layer, dy=dy, mask=e["src"], dst="d:" + e["src"], k=e["k"], u=e["u"], cin=e["cin"],
                                 slope=e["slope"], scale=1.0 if e["src"] == "pre" else 1.0 / nk))
                continue
            plan.append(dict(kind="wgrad", layer=layer, conv=0, dy=dy, src=e["src"], k=e["k"], step=e["dil"], slope=e["slope"]))
            plan.append(dict(kind="finish", layer=layer, mode=0, u=1))
            if layer == "conv_pre":
                continue
            d = dict(kind="conv1d_dgrad", layer=layer, dy=dy, mask=e["src"], dst="d:" + e["src"], k=e["k"], dil=e["dil"], cin=e["cin"],
                     slope=e["slope"], scale=1.0, accumulate=False)
            if "res" in e:                       # convs2: the residual's share of d:x waits for convs1's data gradient
                pending[e["res"]] = dy
            else:                                # convs1
                d.update(res=pending.pop(e["src"]), accumulate=e["src"] in written)
                written.add(e["src"])
            plan.append(d)
        return plan

    # ---- execution --------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_input(x, grad_refusal):
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError(grad_refusal)
        if not x.is_cuda:
            raise RuntimeError("HifiganGenerator needs GPU tensors (there is no CPU path)")
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("HifiganGenerator input: float32 or bfloat16")

    def _run(self, x, B, N, strides, train=False, **fields):
        """One forward call -> its state, `c` of the handlers: the input with its (batch, frame, channel) strides, ops: layer -> Layer,
        dtype of the activations, bufs: name -> activation, y = the waveform, and in `fields` what forward_batch (vlens, a, b) and the
        tests (taps) pass.  train: walk train_plan() -- the operands are folded from the live parameters, the activations are fp32 in
        either compute mode, bwd_dtype is the backward's, and w32 is the folded weight a fold hands the launch after it."""
        dtype = Fn.compute_dtype()
        if not train:
            self._check_input(x, "HifiganGenerator is inference only: no backward pass (call it under torch.no_grad() or detach the input)")
            if self._trainable:                  # an optimiser updates the parameters in place: fold from the live values
                self._drop_cache()
        c = SimpleNamespace(x=x.detach(), B=B, N=N, strides=strides, ops={} if train else self._operands(dtype), bufs={}, y=None, w32=None,
                            dtype=torch.float32 if train else dtype, bwd_dtype=dtype, vlens=None, a=None, b=None, taps=None)
        c.__dict__.update(fields, leaves=dict(self._leaves()) if train else None)
        self._walk(self._plan("train_plan", dtype) if train else self._plan("launch_plan"), c)
        return c

    def _backward(self, state, y, dy):
        """Gradients of every parameter, in named_parameters() order, from dy (B, 1, L): executes backward_plan().  The state of the
        pass: the forward's ops and bufs, y and dy as (B, L), grads: `d:<buffer>` -> gradient, parts = the partials one launch hands
        the finish launch, out: layer -> (grad_weight, grad_g, grad_bias)."""
        B, L = y.shape[0], y.shape[-1]
        c = SimpleNamespace(ops=state.ops, bufs=state.bufs, y=y.detach().reshape(B, L).contiguous(),
                            dy=dy.detach().float().reshape(B, L).contiguous(), grads={}, parts=None, out={})
        self._walk(self._plan("backward_plan"), c)
        return self._param_grads(c.out)

    # ---- the handlers: `calls` names the library calls each makes ---------------------------------------------------------------
    @handles("fold", fold_calls)
    def _do_fold(self, c, e):
        leaf = c.leaves[e["layer"]]
        v, g = leaf.vg()
        c.w32, op = KV.hifigan_fold(e["mode"], v, g, torch.float32, u=e["u"], want_op=e["op"])
        c.ops[e["layer"]] = Layer(v, g, leaf.bias.detach().float().contiguous(), op=op)

    @handles("fold_bwd", "fill_zero", "hifigan_fold_bwd")
    def _do_fold_bwd(self, c, e):
        c.ops[e["layer"]].opT = KV.hifigan_fold_bwd(e["mode"], c.w32, c.bwd_dtype, u=e["u"])

    @handles("input", "hifigan_input")
    def _do_input(self, c, e):
        c.bufs[e["dst"]] = KV.hifigan_input(c.x, c.B, c.N, e["cout"], c.strides, c.dtype, a=c.a, b=c.b, vlens=c.vlens)

    @handles("cast", "hifigan_input")
    def _do_cast(self, c, e):
        v = c.bufs[e["src"]]
        c.bufs[e["src"]] = KV.hifigan_input(v, v.shape[0], v.shape[1], v.shape[2], (v.stride(0), v.stride(1), v.stride(2)), c.bwd_dtype)

    def _store(self, c, e, t):
        c.bufs[e["dst"]] = t
        if c.taps is not None and "tap" in e:
            c.taps[e["tap"]] = t

    @handles("conv1d", "hifigan_conv1d")
    def _do_conv1d(self, c, e):
        o = c.ops[e["layer"]]
        self._store(c, e, KV.hifigan_conv1d(c.bufs[e["src"]], o.op, o.bias, e["k"], e["dil"], e["cout"], slope=e["slope"],
                                            res=c.bufs[e["res"]] if "res" in e else None, accumulate=e.get("accumulate", False),
                                            scale=e.get("scale", 1.0), out=c.bufs.get(e["dst"]), vlens=c.vlens, vmul=e["mul"]))

    @handles("tconv1d", "hifigan_tconv1d")
    def _do_tconv1d(self, c, e):
        o = c.ops[e["layer"]]
        self._store(c, e, KV.hifigan_tconv1d(c.bufs[e["src"]], o.op, o.bias, e["k"], e["u"], e["cout"], slope=e["slope"],
                                             out=c.bufs.get(e["dst"]), vlens=c.vlens, vmul=e["mul"]))

    @handles("conv_out", "hifigan_conv_out")
    def _do_conv_out(self, c, e):
        o = c.ops[e["layer"]]
        c.y, pre = KV.hifigan_conv_out(c.bufs[e["src"]], o.op, o.bias, e["k"], slope=e["slope"], tanh=True, want_pre=c.taps is not None,
                                       vlens=c.vlens, vmul=e["mul"])
        if c.taps is not None:
            c.taps["conv_post"] = pre

    @handles("conv_out_bwd", "hifigan_conv_out_bwd")
    def _do_conv_out_bwd(self, c, e):
        c.grads[e["dst"]], wp, bp = KV.hifigan_conv_out_bwd(c.bufs[e["src"]], c.ops[e["layer"]].op, c.y, c.dy, e["k"], slope=e["slope"],
                                                            scale=e["scale"])
        c.parts = (wp, bp)

    @handles("wgrad", "hifigan_wgrad")
    def _do_wgrad(self, c, e):
        c.parts = KV.hifigan_wgrad(e["conv"], c.grads[e["dy"]], c.bufs[e["src"]], e["k"], e["step"], slope=e["slope"])

    @handles("tconv1d_dgrad", "hifigan_tconv1d_dgrad")
    def _do_tconv1d_dgrad(self, c, e):
        c.grads[e["dst"]] = KV.hifigan_tconv1d_dgrad(c.grads[e["dy"]], c.ops[e["layer"]].opT, e["k"], e["u"], e["cin"],
                                                     mask_src=c.bufs[e["mask"]], slope=e["slope"], scale=e["scale"])

    @handles("conv1d_dgrad", "hifigan_conv1d_dgrad")
    def _do_conv1d_dgrad(self, c, e):
        c.grads[e["dst"]] = KV.hifigan_conv1d_dgrad(c.grads[e["dy"]], c.ops[e["layer"]].opT, e["k"], e["dil"], e["cin"],
                                                    mask_src=c.bufs[e["mask"]], slope=e["slope"], res=c.grads[e["res"]] if e.get("res") else None,
                                                    accumulate=e["accumulate"], scale=e["scale"], out=c.grads.get(e["dst"]))

    def forward(self, x, taps=None):
        """x (B, in_channels, N) -> (B, 1, N * prod(upsample_factors)) fp32.  taps: a dict that receives the channel-last outputs of
        conv_pre, every ups[i], every stage (after the MRF average) and conv_post before tanh (tests)."""
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError(f"HifiganGenerator: x (B, {self.in_channels}, N) expected, got {tuple(x.shape)}")
        B, _, N = x.shape
        if self._trainable and torch.is_grad_enabled():
            self._check_input(x, "HifiganGenerator computes no input gradient: the units / mel are data (detach the input)")
            return _GeneratorFunction.apply(self, x, taps, *[p for _, p in self.named_parameters()])
        return self._run(x, B, N, (x.stride(0), x.stride(2), x.stride(1)), taps=taps).y.view(B, 1, -1)

    def forward_batch(self, xs, lens, a=None, b=None, host_lens=None):
        """xs (B, Nmax, in_channels) channel-last, zero-padded (whatever the padding holds is never read); lens (B) mel frames ->
        list of B waveforms of lens[b] * prod(upsample_factors) samples, each what the utterance gets alone.
        lens: a list / CPU tensor, or an int32 device tensor (what the kernels read).  Only the slicing of the result needs the
        lengths on the host: pass them as host_lens beside a device tensor and the call never waits for the device; without
        host_lens a device tensor is read back AFTER every launch has been queued.
        Inference only, also after trainable(): the result has no grad_fn (ragged batches are not trained on)."""
        if xs.dim() != 3 or xs.shape[2] != self.in_channels:
            raise ValueError(f"HifiganGenerator: xs (B, Nmax, {self.in_channels}) expected, got {tuple(xs.shape)}")
        B, N, _ = xs.shape
        on_device = isinstance(lens, torch.Tensor) and lens.is_cuda
        if on_device and (lens.dtype != torch.int32 or not lens.is_contiguous() or lens.numel() != B):
            raise ValueError("forward_batch: device lengths are a contiguous int32 tensor with one value per row")
        host = host_lens if on_device else lens
        if host is not None:
            host = [int(n) for n in (host.tolist() if isinstance(host, torch.Tensor) else host)]
            if len(host) != B or any(n < 0 or n > N for n in host):
                raise ValueError("forward_batch: one length per row, 0 <= lens[b] <= Nmax")
        vlens = lens if on_device else torch.tensor(host, dtype=torch.int32).to(xs.device)
        y = self._run(xs, B, N, (xs.stride(0), xs.stride(1), xs.stride(2)), vlens=vlens, a=a, b=b).y
        if host is None:
            host = [min(max(int(n), 0), N) for n in lens.tolist()]
        total = stage_lengths(host, self.upsample_factors)[-1]
        return [y[i, :total[i]] for i in range(B)]


class HifiganVocoder:
    """The call shape of the reference's Vocoder (vocoder/vocoder.py:10-61) over a HifiganGenerator whose in_channels = n_mels:
    decode(c) de-normalises c (T, n_mels) with the target statistics, normalises with the vocoder's and generates.  The two
    affine maps are one per-bin a * c + b applied by the input launch.  stats / trg_stats: dicts of arrays `mean`, `scale`."""

    def __init__(self, generator, stats, trg_stats=None, take_norm_feat=True):
        if take_norm_feat and trg_stats is None:
            raise ValueError("trg_stats must be given if take_norm_feat=True")
        self.generator, self.take_norm_feat = generator, take_norm_feat
        mean, scale = np.asarray(stats["mean"], np.float64), np.asarray(stats["scale"], np.float64)
        if take_norm_feat:
            tm, ts = np.asarray(trg_stats["mean"], np.float64), np.asarray(trg_stats["scale"], np.float64)
            a, b = ts / scale, (tm - mean) / scale
        else:
            a, b = 1.0 / scale, -mean / scale
        if a.shape != (generator.in_channels,):
            raise ValueError("statistics must have one value per input channel of the generator")
        self._a, self._b = torch.from_numpy(a).float(), torch.from_numpy(b).float()

    def _affine(self, device):
        if self._a.device != device:
            self._a, self._b = self._a.to(device), self._b.to(device)
        return self._a, self._b

    def decode(self, c):
        y, sr = self.decode_batch(c.unsqueeze(0), [c.shape[0]])
        return y[0], sr

    def decode_batch(self, cs, lens, host_lens=None):
        """Inference only, also over a generator that is trainable(): the waveforms have no grad_fn."""
        a, b = self._affine(cs.device)
        return self.generator.forward_batch(cs, lens, a=a, b=b, host_lens=host_lens), self.generator.sample_rate
