"""HiFi-GAN discriminator on the HIP kernels of csrc/hifigan_disc.hip and csrc/hifigan_msd.hip, forward and backward, fp32: the
multi-period half, the multi-scale half and HifiganDiscriminator, which holds both.

Drop-in surface of the reference's `seq2seq_vc/urhythmic/vocoder.py` PeriodDiscriminator / MultiPeriodDiscriminator (:211-327),
ScaleDiscriminator / MultiScaleDiscriminator (:330-402) and HifiganDiscriminator (:405-425): the constructor arguments, the
`state_dict` keys and shapes (`discriminators.{i}.convs.{j}.{bias,weight_g,weight_v}`, `conv_post.*`, weights (O, C, k, 1) in the
period discriminators and (O, C / groups, k) in the scale discriminators; the spectrally normed first scale holds `bias, weight_orig`
and the buffers `weight_u, weight_v`) and the call `forward(x (B, 1, T)) -> (scores, feats)`; a reference checkpoint of the whole
discriminator, or its `mpd.*` / `msd.*` subtree, loads as it is.  The three loss functions of the reference (:428-465) are at the end
of this file, one autograd node and one table-driven launch sequence each (csrc/gan_loss.hip); the optimiser is optim.MultiAdamW and
the whole loop body is urhythmic/fine_tune.py.

PeriodDiscriminator and ScaleDiscriminator are one executor, `_Discriminator`, over vocoder/plan.py (the weight-norm leaf, the
cached lists, the walk through one table from `kind` to handler, `calls()`), which the generator runs on too: `launch_plan()` /
`backward_plan()` list the launches of one call as dicts, built once per module and mode.  The launches both halves share (the
weight-norm fold, the 5-tap convolution, conv_post, their backward) have one handler each, written for the period half's 4-D
buffers; a class says how its stored buffers become that view (`_four` / `_stored`: the identity there, `unsqueeze(2)` /
`squeeze(2)` in the scale half, whose layer 6 and conv_post are the period kernels at p = 1) and defines the handlers of the kinds it
has alone.  The three containers add `calls(stage, backward)`: the library calls of one forward or one backward of theirs, in the
order they run, which is what urhythmic/fine_tune.py concatenates into the plan of a step.

Activations are channel-last, (B, L, p, C) or (B, L, C); the features handed out are strided (B, C, L, p) / (B, C, L) views of them
and the score is the flattening of the last one.  Under grad mode a call is ONE autograd node whose inputs are x and the parameters
(18 per period; 16, or 24 under spectral norm, per scale) and whose outputs are the score and the six or eight features; its backward
takes whichever of the gradients arrive, in any strides (channel-last-strided ones are read in place, others go through one copy),
and returns the parameter gradients and -- when x requires grad -- dx, which flows on into `HifiganGenerator.trainable()`.  The
average pool between the scales is a small node of its own.  The spectrally normed scale runs one power iteration per call in
train() mode (under no_grad too) and writes u, v back into its buffers, as torch.nn.utils.spectral_norm does; the state kept for
the backward holds copies of the u, v and sigma that the call used.  There is no CPU path and no bf16 path: a bf16 forward flips
leaky-relu masks, which alone puts the gradients several per cent off."""
import math
from types import SimpleNamespace

import torch
from torch import nn

from ..ops import kernels_disc as KD
from ..ops import kernels_ganloss as KG
from ..ops import kernels_msd as KM
from ..ops import kernels_vocoder as KV
from ..vocoder.plan import Layer, PlanExecutor, WNConv, fold_calls, handles

LRELU_SLOPE = 0.1
PERIODS = (2, 3, 5, 7, 11)
CHANNELS = (1, 32, 128, 512, 1024, 1024)          # convs[j]: CHANNELS[j] -> CHANNELS[j + 1]
STRIDES = (3, 3, 3, 3, 1)
KINDS = ("fold", "input", "conv", "post")
BWD_KINDS = ("post_bwd", "wgrad", "input_wgrad", "finish", "fold_bwd", "dgrad", "input_dgrad")


def layer_lengths(T, p):
    """[L0, L1, .., L5]: rows along L of the folded input and of the output of convs[0..4] (conv_post keeps L5)."""
    L = [KD.folded_len(T, p)[0]]
    for s in STRIDES:
        L.append(KD.out_len(L[-1], s))
    return L


class _DiscFunction(torch.autograd.Function):
    """One discriminator call as ONE autograd node: inputs x and the parameters, outputs the score and the features."""

    @staticmethod
    def forward(ctx, disc, x, *params):
        ctx.set_materialize_grads(False)
        score, feats, state = disc._run(x, keep=True)
        ctx.disc, ctx.state = disc, state
        ctx.save_for_backward(*params)           # autograd refuses a backward after an in-place update of one of them
        return (score,) + tuple(feats)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gscore, *gfeats):
        ctx.saved_tensors                        # the version check of the parameters
        need_dx, need_params = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        dx, grads = ctx.disc._backward(ctx.state, gscore, gfeats, need_dx, need_params)
        return (None, dx) + tuple(grads)


class _PeriodFunction(_DiscFunction):
    """One PeriodDiscriminator call: inputs x and the 18 parameters, outputs the score and the six features."""


class _ScaleFunction(_DiscFunction):
    """One ScaleDiscriminator call: inputs x and the 16 or 24 parameters, outputs the score and the eight features."""


def _flat(g, B):
    return None if g is None else g.detach().float().reshape(B, -1).contiguous()


class _Discriminator(PlanExecutor):
    """The executor of both discriminator halves.  A subclass has `convs`, `conv_post`, `launch_plan()` and `backward_plan()`, names
    its autograd node (`_FUNCTION`), the permutations between its stored buffers and the caller's features (`_TO_CALLER`,
    `_FROM_CALLER`), `_four` / `_stored`, and defines the `@handles` methods of the kinds of its own.  A handler is `f(self, c, e)`: c = the
    state of the call (ops: layer -> Layer, bufs: index -> stored activation, x (B, T), keep; in the backward also gf = the features'
    gradients channel-last, gscore, glast, out: layer -> (gw, gg, gb), and parts, dpre, opT, dx = what one launch hands the next)."""
    _MIN_T = 0

    def _leaf(self, name):
        return self.conv_post if name == "conv_post" else self.convs[int(name.split(".")[1])]

    def _check(self, x):
        name = type(self).__name__
        if x.dim() != 3 or x.shape[1] != 1 or x.shape[2] < self._MIN_T:
            raise ValueError(f"{name}: x (B, 1, T) expected, got {tuple(x.shape)}")
        dtypes = {x.dtype} | {p.dtype for p in self.parameters()} | {b.dtype for b in self.buffers()}
        if torch.bfloat16 in dtypes or torch.float16 in dtypes:
            raise NotImplementedError(f"{name} runs in fp32 only: a 16-bit forward flips leaky-relu masks, which alone puts the "
                                      "gradients several per cent off (DESIGN.md section 8)")
        if dtypes != {torch.float32}:
            raise TypeError(f"{name}: float32 input and parameters")
        if not x.is_cuda or not self.conv_post.bias.is_cuda:
            raise RuntimeError(f"{name} needs GPU tensors and GPU parameters (there is no CPU path)")

    def _run(self, x, keep=False):
        """-> (score, feats, state): executes launch_plan().  keep: the state also holds what the backward reads (the folded weights,
        the parameters' views, the input, and copies of the u, v, sigma this call used)."""
        B, _, T = x.shape
        with torch.no_grad():
            c = SimpleNamespace(ops={}, bufs={}, x=x.detach().reshape(B, T).contiguous(), keep=keep)
            self._walk(self._plan("launch_plan"), c)
            n = len(self.convs)
            feats = [c.bufs[j].permute(*self._TO_CALLER) for j in range(n + 1)]
            score = c.bufs[n].view(B, -1)
        return score, feats, (c if keep else None)

    def _backward(self, state, gscore, gfeats, need_dx, need_params):
        """(dx or None, the parameter gradients in named_parameters() order or Nones) from whichever of the output gradients
        arrived: executes backward_plan()."""
        n = len(self.convs)

        def channel_last(g):
            """a feature's gradient as a contiguous stored buffer: in place when it already is channel-last-strided, else one copy"""
            if g is None:
                return None
            g = g.detach().float().permute(*self._FROM_CALLER)
            return g if g.is_contiguous() else g.contiguous()

        c = SimpleNamespace(ops=state.ops, bufs=state.bufs, x=state.x, gf=[channel_last(g) for g in gfeats[:n]], gscore=gscore,
                            glast=gfeats[n], out={}, parts=None, dpre=None, opT=None, dx=None)
        self._walk(self._plan("backward_plan", bool(need_dx), bool(need_params)), c)
        return c.dx, self._param_grads(c.out) if need_params else [None] * len(list(self.parameters()))

    def forward(self, x):
        self._check(x)
        params = [prm for _, prm in self.named_parameters()]
        if torch.is_grad_enabled() and (x.requires_grad or any(prm.requires_grad for prm in params)):
            res = self._FUNCTION.apply(self, x, *params)
            return res[0], list(res[1:])
        score, feats, _ = self._run(x)
        return score, feats

    # ---- the launches both halves have: the period half's launchers on the 4-D view of the buffers ---------------------------
    @handles("fold", fold_calls)
    def _do_fold(self, c, e):
        leaf = self._leaf(e["layer"])
        v, g = leaf.vg()                          # the input layer reads the folded weight itself (`op` False), the others the operand
        w32, op = KV.hifigan_fold(e["mode"], v, g, torch.float32, want_w32=not e["op"] or (c.keep and e["mode"] == 0), want_op=e["op"])
        c.ops[e["layer"]] = Layer(v, g, leaf.bias.detach().contiguous(), w32, op)

    @handles("conv", "hifigan_disc_conv")
    def _do_conv(self, c, e):
        o = c.ops[e["layer"]]
        c.bufs[e["dst"]] = self._stored(KD.disc_conv(self._four(c.bufs[e["src"]]), o.op, o.bias, e["cout"], e["stride"], slope=LRELU_SLOPE))

    @handles("post", "hifigan_disc_post")
    def _do_post(self, c, e):
        o, src = c.ops[e["layer"]], c.bufs[e["src"]]
        c.bufs[e["dst"]] = KD.disc_post(self._four(src), o.op, o.bias).view(src.shape[:-1] + (1,))

    @handles("post_bwd", "hifigan_disc_post_bwd")
    def _do_post_bwd(self, c, e):
        B = c.x.shape[0]
        dpre, wp, bp = KD.disc_post_bwd(self._four(c.bufs[e["src"]]), c.ops[e["layer"]].op, dy1=_flat(c.gscore, B), dy2=_flat(c.glast, B),
                                        add=self._four(c.gf[e["src"]]), slope=LRELU_SLOPE)
        c.dpre, c.parts = self._stored(dpre), (wp, bp)

    @handles("wgrad", "hifigan_disc_wgrad")
    def _do_wgrad(self, c, e):
        c.parts = KD.disc_wgrad(self._four(c.dpre), self._four(c.bufs[e["src"]]), e["stride"])

    @handles("fold_bwd", "fill_zero", "hifigan_fold_bwd")
    def _do_fold_bwd(self, c, e):
        c.opT = KV.hifigan_fold_bwd(0, c.ops[e["layer"]].w32, torch.float32)

    @handles("dgrad", "hifigan_disc_dgrad")
    def _do_dgrad(self, c, e):
        mask = c.bufs[e["mask"]]
        c.dpre = self._stored(KD.disc_dgrad(self._four(c.dpre), c.opT, mask.shape[1], e["cin"], e["stride"], mask_src=self._four(mask),
                                            add=self._four(c.gf[e["mask"]]), slope=LRELU_SLOPE))
        c.opT = None


class PeriodDiscriminator(_Discriminator):
    """HiFi-GAN period discriminator (reference urhythmic/vocoder.py:211-293).  x (B, 1, T) fp32 on the device ->
    (score (B, L5 * p), [six features (B, C, L, p)])."""
    _FUNCTION = _PeriodFunction
    _TO_CALLER, _FROM_CALLER = (0, 3, 1, 2), (0, 2, 3, 1)

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False):
        super().__init__()
        if use_spectral_norm:
            raise NotImplementedError("PeriodDiscriminator: spectral norm is not implemented (the multi-period discriminator never sets it)")
        if kernel_size != KD.TAPS or stride != KD.STRIDE:
            raise ValueError(f"PeriodDiscriminator: the kernels are built for kernel_size {KD.TAPS}, stride {KD.STRIDE} (csrc/hifigan_disc.hip)")
        if int(period) < 1:
            raise ValueError("PeriodDiscriminator: period >= 1")
        self.period = int(period)
        self.convs = nn.ModuleList([WNConv((CHANNELS[j + 1], CHANNELS[j], kernel_size, 1)) for j in range(len(STRIDES))])
        self.conv_post = WNConv((1, CHANNELS[-1], KD.POST_TAPS, 1))

    # ---- the launch lists -------------------------------------------------------------------------------------------------
    def launch_plan(self):
        """What one forward call launches, in order: dicts with `kind` in KINDS: 12 per period, 60 per MultiPeriodDiscriminator call.
        forward() executes exactly this list.  ("fold" is the fold kernel; hifigan_fold zero-fills each of the five operand buffers with
        one more library launch beside it, and hifigan_fold_bwd does the same in the backward: 17 and 25 / 24 launches per period.)"""
        plan = [dict(kind="fold", layer=f"convs.{j}", mode=0, op=j > 0) for j in range(len(STRIDES))] + [dict(kind="fold", layer="conv_post", mode=2, op=True)]
        plan.append(dict(kind="input", layer="convs.0", dst=0, cout=CHANNELS[1], stride=STRIDES[0]))
        for j in range(1, len(STRIDES)):
            plan.append(dict(kind="conv", layer=f"convs.{j}", src=j - 1, dst=j, cin=CHANNELS[j], cout=CHANNELS[j + 1], stride=STRIDES[j]))
        plan.append(dict(kind="post", layer="conv_post", src=len(STRIDES) - 1, dst=len(STRIDES), cin=CHANNELS[-1]))
        return plan

    def backward_plan(self, need_dx=False, need_params=True):
        """What one backward pass launches, in order: dicts with `kind` in BWD_KINDS.  Per layer from the top: the weight / bias
        partials and their finish launch (when a parameter needs a gradient), then the data gradient, whose epilogue adds the gradient
        of the feature below and applies its leaky_relu'.  The input layer's data gradient runs only when x requires grad.
        _backward() executes exactly this list."""
        n = len(STRIDES)
        plan = [dict(kind="post_bwd", layer="conv_post", src=n - 1)]
        if need_params:
            plan.append(dict(kind="finish", layer="conv_post", mode=2))
        for j in range(n - 1, 0, -1):
            if need_params:
                plan += [dict(kind="wgrad", layer=f"convs.{j}", src=j - 1, stride=STRIDES[j]), dict(kind="finish", layer=f"convs.{j}", mode=0)]
            plan += [dict(kind="fold_bwd", layer=f"convs.{j}"),
                     dict(kind="dgrad", layer=f"convs.{j}", mask=j - 1, cin=CHANNELS[j], stride=STRIDES[j])]
        if need_params:
            plan += [dict(kind="input_wgrad", layer="convs.0"), dict(kind="finish", layer="convs.0", mode=0)]
        if need_dx:
            plan.append(dict(kind="input_dgrad", layer="convs.0"))
        return plan

    # ---- execution: the buffers are (B, L, p, C) as the launchers take them ---------------------------------------------------
    def _check(self, x):
        super()._check(x)
        KD.folded_len(x.shape[2], self.period)

    def _four(self, t):
        return t

    _stored = _four

    @handles("input", "hifigan_disc_input")
    def _do_input(self, c, e):
        o = c.ops[e["layer"]]
        c.bufs[e["dst"]] = KD.disc_input(c.x, o.w32, o.bias, self.period, slope=LRELU_SLOPE)

    @handles("input_wgrad", "hifigan_disc_input_wgrad")
    def _do_input_wgrad(self, c, e):
        c.parts = KD.disc_input_wgrad(c.dpre, c.x, self.period)

    @handles("input_dgrad", "hifigan_disc_input_dgrad")
    def _do_input_dgrad(self, c, e):
        B, T = c.x.shape
        c.dx = KD.disc_input_dgrad(c.dpre, c.ops[e["layer"]].w32, T, self.period).view(B, 1, T)


class MultiPeriodDiscriminator(nn.Module):
    """HiFi-GAN multi-period discriminator (reference urhythmic/vocoder.py:296-327): five PeriodDiscriminators, periods 2, 3, 5, 7, 11.
    x (B, 1, T) -> ([five scores], [five lists of six features])."""

    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([PeriodDiscriminator(p) for p in PERIODS])

    def launch_plan(self):
        return [dict(e, period=d.period) for d in self.discriminators for e in d.launch_plan()]

    def backward_plan(self, need_dx=False, need_params=True):
        return [dict(e, period=d.period) for d in self.discriminators for e in d.backward_plan(need_dx, need_params)]

    def calls(self, stage, backward=None):
        """The library calls of one forward (PlanExecutor.calls of launch_plan()) or, with backward = (need_dx, need_params), of one
        backward in the order autograd runs the nodes: the last one made first."""
        ds = self.discriminators if backward is None else reversed(self.discriminators)
        return [c for d in ds for c in d.calls([dict(e, period=d.period) for e in (d.backward_plan(*backward) if backward else d.launch_plan())], stage)]

    def forward(self, x):
        scores, feats = [], []
        for d in self.discriminators:
            score, feat = d(x)
            scores.append(score)
            feats.append(feat)
        return scores, feats


# ---------------------------------------------------------------------------------------------------------------------------
# the multi-scale half (csrc/hifigan_msd.hip)
# ---------------------------------------------------------------------------------------------------------------------------
# convs[j]: (C_in, C_out, kernel size, stride, groups); the last entry is conv_post
MSD_LAYERS = ((1, 128, 15, 1, 1), (128, 128, 41, 2, 4), (128, 256, 41, 2, 16), (256, 512, 41, 4, 16), (512, 1024, 41, 4, 16),
              (1024, 1024, 41, 1, 16), (1024, 1024, 5, 1, 1), (1024, 1, 3, 1, 1))
MSD_KINDS = ("sn_power", "sn_scale", "fold", "input", "gconv", "conv", "post")
MSD_BWD_KINDS = ("post_bwd", "wgrad", "gconv_wgrad", "input_wgrad", "finish", "sn_finish", "fold_bwd", "gfold_bwd", "dgrad", "gconv_dgrad",
                 "input_dgrad")


def scale_lengths(T):
    """[L0 .. L7]: rows of the output of convs[0..6] of a ScaleDiscriminator on T samples (conv_post keeps L6)."""
    L, out = T, []
    for _, _, _, s, _ in MSD_LAYERS[:-1]:
        L = KM.out_len(L, s)
        out.append(L)
    return out + [L]


class _SNConv1d(nn.Module):
    """Parameters and buffers of torch.nn.utils.spectral_norm(Conv1d(cin, cout, k, groups=groups)) (the hook form: dim 0, one power
    iteration, eps 1e-12) in the reference's checkpoint form; u and v are normalised normal draws."""

    def __init__(self, cin, cout, k, groups=1):
        super().__init__()
        bound = 1.0 / math.sqrt(cin // groups * k)
        self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        self.weight_orig = nn.Parameter(torch.empty(cout, cin // groups, k).uniform_(-bound, bound))
        self.register_buffer("weight_u", torch.nn.functional.normalize(torch.randn(cout), dim=0, eps=KM.SN_EPS))
        self.register_buffer("weight_v", torch.nn.functional.normalize(torch.randn(cin // groups * k), dim=0, eps=KM.SN_EPS))


class _PoolFunction(torch.autograd.Function):
    """AvgPool1d(4, 2, padding=2) on (B, 1, T): the HIP forward and its adjoint, one library call each (`CALLS`)."""
    CALLS = ("hifigan_msd_pool", "hifigan_msd_pool_bwd")

    @staticmethod
    def forward(ctx, x):
        B, _, T = x.shape
        ctx.T = T
        return KM.msd_pool(x.detach().reshape(B, T).contiguous()).view(B, 1, -1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        B = gy.shape[0]
        return KM.msd_pool_bwd(gy.detach().float().reshape(B, -1).contiguous(), ctx.T).view(B, 1, ctx.T)


class _MeanPool(nn.Module):
    """AvgPool1d(4, 2, padding=2) between the scales (no parameters, as in the reference's `meanpools`)."""

    def forward(self, x):
        return _PoolFunction.apply(x)


class ScaleDiscriminator(_Discriminator):
    """HiFi-GAN scale discriminator (reference urhythmic/vocoder.py:330-365).  x (B, 1, T) fp32 on the device ->
    (score (B, L), [eight features (B, C, L)])."""
    _FUNCTION = _ScaleFunction
    _TO_CALLER = _FROM_CALLER = (0, 2, 1)
    _MIN_T = 1

    def __init__(self, use_spectral_norm=False):
        super().__init__()
        self.use_spectral_norm = bool(use_spectral_norm)

        def leaf(cin, cout, k, groups=1):
            return _SNConv1d(cin, cout, k, groups) if self.use_spectral_norm else WNConv((cout, cin // groups, k))

        self.convs = nn.ModuleList([leaf(cin, cout, k, g) for cin, cout, k, _, g in MSD_LAYERS[:-1]])
        self.conv_post = leaf(*MSD_LAYERS[-1][:3])

    # ---- the launch lists -------------------------------------------------------------------------------------------------
    def launch_plan(self):
        """What one forward call launches, in order: dicts with `kind` in MSD_KINDS; forward() executes exactly this list.  Weight norm:
        one fold per layer (the input layer needs the folded weight alone, `op` False).  Spectral norm: the power iteration (or, in
        eval() mode, sigma from the stored u, v), W / sigma, and the fold of that with g = None.  ("sn_power" is 4 small kernels with
        `iterate`, 2 without; hifigan_fold zero-fills each operand buffer with one more library launch beside it.)"""
        plan, n = [], len(MSD_LAYERS) - 1
        for j in range(n + 1):
            layer = f"convs.{j}" if j < n else "conv_post"
            if self.use_spectral_norm:
                plan += [dict(kind="sn_power", layer=layer, iterate=self.training), dict(kind="sn_scale", layer=layer)]
                if j == 0:
                    continue
            plan.append(dict(kind="fold", layer=layer, mode=2 if j == n else 0, op=j > 0))
        for j, (cin, cout, k, s, g) in enumerate(MSD_LAYERS[:-1]):
            kind = "input" if j == 0 else ("gconv" if k == KM.TAPS else "conv")
            plan.append(dict(kind=kind, layer=f"convs.{j}", src=j - 1, dst=j, cin=cin, cout=cout, stride=s, groups=g))
        plan.append(dict(kind="post", layer="conv_post", src=n - 1, dst=n, cin=MSD_LAYERS[-1][0]))
        return plan

    def backward_plan(self, need_dx=False, need_params=True):
        """What one backward pass launches, in order: dicts with `kind` in MSD_BWD_KINDS.  Per layer from the top: the weight / bias
        partials, their finish launch and -- under spectral norm -- the backward of the division by sigma (when a parameter needs a
        gradient), then the transposed operand and the data gradient, whose epilogue adds the gradient of the feature below and applies
        its leaky_relu'.  The input layer's data gradient runs only when x requires grad.  _backward() executes exactly this list."""
        n = len(MSD_LAYERS) - 1
        sn = [dict(kind="sn_finish")] if self.use_spectral_norm else []

        def params(layer, first, mode=0):
            return [first, dict(kind="finish", layer=layer, mode=mode)] + [dict(e, layer=layer) for e in sn] if need_params else []

        plan = [dict(kind="post_bwd", layer="conv_post", src=n - 1)]
        plan += params("conv_post", None, 2)[1:]
        for j in range(n - 1, 0, -1):
            cin, cout, k, s, g = MSD_LAYERS[j]
            grouped = k == KM.TAPS
            layer = f"convs.{j}"
            plan += params(layer, dict(kind="gconv_wgrad" if grouped else "wgrad", layer=layer, src=j - 1, stride=s, groups=g))
            plan += [dict(kind="gfold_bwd" if grouped else "fold_bwd", layer=layer, groups=g),
                     dict(kind="gconv_dgrad" if grouped else "dgrad", layer=layer, mask=j - 1, cin=cin, stride=s, groups=g)]
        plan += params("convs.0", dict(kind="input_wgrad", layer="convs.0"))
        if need_dx:
            plan.append(dict(kind="input_dgrad", layer="convs.0"))
        return plan

    # ---- execution: the buffers are (B, L, C); the shared launchers take them as (B, L, 1, C) ----------------------------------
    def _four(self, t):
        return None if t is None else t.unsqueeze(2)

    def _stored(self, t):
        return t.squeeze(2)

    @handles("sn_power", "hifigan_msd_sn_power")
    def _do_sn_power(self, c, e):
        leaf = self._leaf(e["layer"])
        W = leaf.weight_orig.detach().contiguous()
        sigma = KM.msd_sn_power(W, leaf.weight_u, leaf.weight_v, e["iterate"])
        c.ops[e["layer"]] = Layer(W, None, leaf.bias.detach().contiguous(), sigma=sigma,
                                   uv=(leaf.weight_u.clone(), leaf.weight_v.clone()) if c.keep else None)

    @handles("sn_scale", "hifigan_msd_sn_scale")
    def _do_sn_scale(self, c, e):
        o = c.ops[e["layer"]]
        o.w32 = KM.msd_sn_scale(o.v, o.sigma)

    @handles("fold", fold_calls)
    def _do_fold(self, c, e):
        if not self.use_spectral_norm:
            return super()._do_fold(c, e)
        o = c.ops[e["layer"]]
        o.op = KV.hifigan_fold(e["mode"], o.w32, None, torch.float32, want_w32=False)[1]

    @handles("input", "hifigan_msd_input")
    def _do_input(self, c, e):
        o = c.ops[e["layer"]]
        c.bufs[e["dst"]] = KM.msd_input(c.x, o.w32, o.bias, slope=LRELU_SLOPE)

    @handles("gconv", "hifigan_msd_gconv")
    def _do_gconv(self, c, e):
        o = c.ops[e["layer"]]
        c.bufs[e["dst"]] = KM.msd_gconv(c.bufs[e["src"]], o.op, o.bias, e["cout"], e["groups"], e["stride"], slope=LRELU_SLOPE)

    @handles("gconv_wgrad", "hifigan_msd_gconv_wgrad")
    def _do_gconv_wgrad(self, c, e):
        c.parts = KM.msd_gconv_wgrad(c.dpre, c.bufs[e["src"]], e["groups"], e["stride"])

    @handles("input_wgrad", "hifigan_msd_input_wgrad")
    def _do_input_wgrad(self, c, e):
        c.parts = KM.msd_input_wgrad(c.dpre, c.x)

    @handles("sn_finish", "hifigan_msd_sn_finish")
    def _do_sn_finish(self, c, e):
        o = c.ops[e["layer"]]
        gw, _, gb = c.out[e["layer"]]
        c.out[e["layer"]] = (KM.msd_sn_finish(gw, o.v, o.uv[0], o.uv[1], o.sigma), None, gb)

    @handles("gfold_bwd", "hifigan_msd_fold_bwd")
    def _do_gfold_bwd(self, c, e):
        c.opT = KM.msd_fold_bwd(c.ops[e["layer"]].w32, e["groups"])

    @handles("gconv_dgrad", "hifigan_msd_gconv_dgrad")
    def _do_gconv_dgrad(self, c, e):
        mask = c.bufs[e["mask"]]
        c.dpre = KM.msd_gconv_dgrad(c.dpre, c.opT, mask.shape[1], e["cin"], e["groups"], e["stride"], mask_src=mask, add=c.gf[e["mask"]],
                                    slope=LRELU_SLOPE)
        c.opT = None

    @handles("input_dgrad", "hifigan_msd_input_dgrad")
    def _do_input_dgrad(self, c, e):
        B, T = c.x.shape
        c.dx = KM.msd_input_dgrad(c.dpre, c.ops[e["layer"]].w32).view(B, 1, T)


class MultiScaleDiscriminator(nn.Module):
    """HiFi-GAN multi-scale discriminator (reference urhythmic/vocoder.py:368-402): three ScaleDiscriminators, the first spectrally
    normed, on x, pool(x) and pool(pool(x)).  x (B, 1, T) -> ([three scores], [three lists of eight features])."""

    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([ScaleDiscriminator(use_spectral_norm=True), ScaleDiscriminator(), ScaleDiscriminator()])
        self.meanpools = nn.ModuleList([_MeanPool(), _MeanPool()])

    def launch_plan(self):
        plan = []
        for i, d in enumerate(self.discriminators):
            plan += ([dict(kind="pool", scale=i)] if i else []) + [dict(e, scale=i) for e in d.launch_plan()]
        return plan

    def backward_plan(self, need_dx=False, need_params=True):
        plan = []
        for i, d in enumerate(self.discriminators):
            plan += [dict(e, scale=i) for e in d.backward_plan(need_dx, need_params)]
        return plan + ([dict(kind="pool_bwd", scale=2), dict(kind="pool_bwd", scale=1)] if need_dx else [])

    def calls(self, stage, backward=None):
        """As MultiPeriodDiscriminator.calls; in a backward the adjoint of a pool runs after the scale it feeds."""
        fwd, bwd = _PoolFunction.CALLS
        out = []
        for i, d in enumerate(self.discriminators):
            if backward is None:
                out += ([dict(kind="pool", scale=i, stage=stage, call=fwd)] if i else []) + d.calls([dict(e, scale=i) for e in d.launch_plan()], stage)
            else:
                pool = [dict(kind="pool_bwd", scale=i, stage=stage, call=bwd)] if backward[0] and i else []
                out = d.calls([dict(e, scale=i) for e in d.backward_plan(*backward)], stage) + pool + out
        return out

    def forward(self, x):
        scores, feats = [], []
        for i, d in enumerate(self.discriminators):
            if i:
                d._check(x)
                x = self.meanpools[i - 1](x)
            score, feat = d(x)
            scores.append(score)
            feats.append(feat)
        return scores, feats


class HifiganDiscriminator(nn.Module):
    """The reference's HifiganDiscriminator (urhythmic/vocoder.py:405-425): `mpd` + `msd`; forward returns the concatenated lists
    (eight scores, eight lists of features)."""

    def __init__(self):
        super().__init__()
        self.mpd = MultiPeriodDiscriminator()
        self.msd = MultiScaleDiscriminator()

    def launch_plan(self):
        return self.mpd.launch_plan() + self.msd.launch_plan()

    def backward_plan(self, need_dx=False, need_params=True):
        return self.mpd.backward_plan(need_dx, need_params) + self.msd.backward_plan(need_dx, need_params)

    def calls(self, stage, backward=None):
        """As the halves' `calls`: mpd then msd in a forward, the reverse in a backward."""
        halves = (self.mpd, self.msd) if backward is None else (self.msd, self.mpd)
        return [c for h in halves for c in h.calls(stage, backward)]

    def forward(self, x):
        scores, feats = self.mpd(x)
        scores_, feats_ = self.msd(x)
        return scores + scores_, feats + feats_


# ---------------------------------------------------------------------------------------------------------------------------
# the three losses (csrc/gan_loss.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(name, tensors):
    """The checks of the discriminators' `_check`, on every tensor of a loss call."""
    if not tensors:
        raise ValueError(f"{name}: no tensors")
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: tensors expected, got {type(t).__name__}")
        if t.dtype in (torch.bfloat16, torch.float16):
            raise NotImplementedError(f"{name} runs in fp32 only, as the discriminators do (DESIGN.md section 8)")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: float32 tensors")
        if not t.is_cuda:
            raise RuntimeError(f"{name} needs GPU tensors (there is no CPU path)")


class _FeatureLossFunction(torch.autograd.Function):
    """feature_loss as ONE autograd node.  launch plan: forward 2 library launches (chunk sums of every pair, finish), backward 1
    (sign and fl(upstream / numel) recomputed from the saved inputs: nothing is stored between the passes but the inputs)."""

    @staticmethod
    def forward(ctx, n, *tensors):
        pairs = []
        for r, g in zip(tensors[:n], tensors[n:]):
            r, g = r.detach(), g.detach()
            if r.shape != g.shape:
                raise ValueError(f"feature_loss: a pair of shapes {tuple(r.shape)} and {tuple(g.shape)}")
            if not (KG.dense_like(r) and KG.same_layout(r, g)):
                r, g = r.contiguous(), g.contiguous()
            pairs.append((r, g))
        out = KG.feature_loss_fwd(pairs)
        ctx.pairs = pairs
        ctx.save_for_backward(*tensors)          # the version check of the inputs
        means = out[:n]
        ctx.mark_non_differentiable(means)
        return out[n], means

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_means):
        ctx.saved_tensors
        n = len(ctx.pairs)
        need = ctx.needs_input_grad[1:]
        ga, gb = KG.feature_loss_bwd(ctx.pairs, g_loss.detach().float().reshape(1), need[:n], need[n:])
        return (None,) + tuple(ga) + tuple(gb)


def feature_loss(features_real, features_generated):
    """The reference's feature_loss (urhythmic/vocoder.py:428-436): the sum over all feature pairs of mean(|real - generated|), one
    autograd node, 2 launches forward and 1 backward for all (54) pairs.  The pairs are walked in their physical storage: the
    discriminators' features are permuted views of dense channel-last buffers, both tensors of a pair equally strided, and the gradient
    comes back in the same layout, which the discriminators' backward reads in place.  A pair that is not dense and equally strided
    gets one contiguous copy of each tensor first.  The gradient is fl(upstream / numel) * sgn(real - generated) for `real` and its
    negation for `generated` (stock torch's fp32 values, signed zeros included), each computed only when that side requires grad."""
    real = [t for fl in features_real for t in fl]
    gen = [t for fl in features_generated for t in fl]
    if len(real) != len(gen):
        raise ValueError(f"feature_loss: {len(real)} real features, {len(gen)} generated ones")
    _loss_inputs("feature_loss", real + gen)
    return _FeatureLossFunction.apply(len(real), *real, *gen)[0]


class _ScoreLossFunction(torch.autograd.Function):
    """The least-squares losses over a list of score tensors as ONE autograd node.  launch plan: forward 2 library launches, backward 1."""

    @staticmethod
    def forward(ctx, kinds, *tensors):
        entries = []
        for x, kind in zip(tensors, kinds):
            x = x.detach()
            entries.append((x if KG.dense_like(x) else x.contiguous(), kind))
        out = KG.score_loss_fwd(entries)
        ctx.entries = entries
        ctx.save_for_backward(*tensors)
        means = out[:len(entries)]
        ctx.mark_non_differentiable(means)
        return out[len(entries)], means

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_means):
        ctx.saved_tensors
        return (None,) + tuple(KG.score_loss_bwd(ctx.entries, g_loss.detach().float().reshape(1), ctx.needs_input_grad[1:]))


def discriminator_loss(real, generated, detail=True):
    """The reference's discriminator_loss (urhythmic/vocoder.py:439-452): sum over the pairs of mean((1 - r)^2) + mean(g^2) ->
    (loss, real_losses, generated_losses).  One autograd node, 2 launches forward, 1 backward.  The two lists are Python floats as in
    the reference, read with ONE device-to-host copy (the reference reads 16 times); detail=False returns empty lists and never
    touches the host."""
    real, generated = list(real), list(generated)
    if len(real) != len(generated):
        raise ValueError(f"discriminator_loss: {len(real)} real scores, {len(generated)} generated ones")
    _loss_inputs("discriminator_loss", real + generated)
    n = len(real)
    loss, means = _ScoreLossFunction.apply((KG.KIND_ONE_MINUS_SQ,) * n + (KG.KIND_SQ,) * n, *real, *generated)
    if not detail:
        return loss, [], []
    host = means.tolist()
    return loss, host[:n], host[n:]


def generator_loss(discriminator_outputs):
    """The reference's generator_loss (urhythmic/vocoder.py:455-465): sum of mean((1 - x)^2) -> (loss, [the per-score losses]).  One
    autograd node; the per-score losses are 0-dim views of one device vector and, unlike the reference's, carry no gradient (the loop
    logs them)."""
    outputs = list(discriminator_outputs)
    _loss_inputs("generator_loss", outputs)
    loss, means = _ScoreLossFunction.apply((KG.KIND_ONE_MINUS_SQ,) * len(outputs), *outputs)
    return loss, list(means.unbind(0))
