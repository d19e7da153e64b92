"""What the three vocoder nets (HifiganGenerator, PeriodDiscriminator, ScaleDiscriminator) share on the host: the weight-norm leaf,
the per-call record of a layer and the plan executor.

A net lists the launches of one call as dicts (`launch_plan()`, `backward_plan()`, the generator's `train_plan()`) and walks such a
list through its own table from `kind` to handler.  A handler is a method `f(self, c, e)` (c = the state of the call, e = the entry)
marked with `@handles(kind, *calls)`: `calls` are the names `_lib.check` reports for the library calls the handler makes, so the one
place that makes a call is the one place that names it, and `calls(plan, stage)` expands any plan into one dict per library call.
A class's table is its parents' plus the handlers it defines, so "wgrad" may be hifigan_wgrad in one net and hifigan_disc_wgrad in
another.  The lists depend on constructor arguments and the train() / eval() mode only: `_plan` builds each once per module."""
import math

import torch
from torch import nn

from ..ops import kernels_vocoder as KV


class WNConv(nn.Module):
    """Parameters of one weight-normed convolution, torch's default initialisation, in either checkpoint form: (bias, weight_g,
    weight_v) or, folded, (bias, weight).  `shape` is the weight's: (O, C, k) for Conv1d, (O, C / groups, k) with groups, (O, C, k, 1)
    for Conv2d(C, O, (k, 1)), (C, O, k) for ConvTranspose1d, whose bias has nbias = shape[1] values."""

    def __init__(self, shape, nbias=None):
        super().__init__()
        self.wshape = tuple(shape)
        bound = 1.0 / math.sqrt(shape[1] * shape[2])
        v = torch.empty(*shape).uniform_(-bound, bound)
        self.bias = nn.Parameter(torch.empty(shape[0] if nbias is None else nbias).uniform_(-bound, bound))
        self._set_normed(v)

    def _set_normed(self, v):
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(-1, *[1] * (len(self.wshape) - 1)))
        self.weight_v = nn.Parameter(v)

    @property
    def normed(self):
        return "weight_v" in self._parameters

    def set_form(self, normed, weight=None):
        if normed == self.normed and weight is None:
            return
        for name in ("weight_g", "weight_v", "weight"):
            self._parameters.pop(name, None)
        if weight is None:
            weight = torch.zeros(self.wshape, dtype=self.bias.dtype, device=self.bias.device)
        if normed:
            self._set_normed(weight)
        else:
            self.weight = nn.Parameter(weight)

    def vg(self):
        """(v (D0, D1, k), g with D0 values) fp32 contiguous views of the live parameters; g is None in the folded form"""
        v, g = (self.weight_v, self.weight_g) if self.normed else (self.weight, None)
        v = v.detach().float().contiguous()
        return v if v.dim() == 3 else v.flatten(2), None if g is None else g.detach().float().contiguous()


class Layer:
    """What one call holds of a layer: v, g = the parameters' views (v = weight_orig and g = None under spectral norm), bias, w32 =
    the folded weight, op = the GEMM operand, opT = the data gradient's, and under spectral norm sigma and uv = copies of the u, v the
    call used."""
    __slots__ = ("v", "g", "bias", "w32", "op", "opT", "sigma", "uv")

    def __init__(self, v, g, bias, w32=None, op=None, opT=None, sigma=None, uv=None):
        self.v, self.g, self.bias, self.w32, self.op, self.opT, self.sigma, self.uv = v, g, bias, w32, op, opT, sigma, uv


def handles(kind, *calls):
    """Mark a method as the handler of plan entries of `kind`.  calls: the library calls it makes, in order, or one function of the
    entry that returns them."""
    def mark(f):
        f.kind, f.calls = kind, calls[0] if callable(calls[0]) else calls
        return f
    return mark


def fold_calls(e):
    """hifigan_fold zero-fills the operand buffer it lays out with one more library call; the folded weight alone needs none"""
    return ("fill_zero", "hifigan_fold") if e["op"] else ("hifigan_fold",)


class PlanExecutor(nn.Module):
    """A module whose calls walk stored plans (module docstring)."""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls._HANDLERS = {f.kind: f for k in reversed(cls.__mro__) for f in vars(k).values() if hasattr(f, "kind")}

    def _plan(self, name, *args):
        """the list that the method `name` builds for `args`: built once per train() / eval() mode and arguments"""
        key = (name, self.training) + args
        plans = self.__dict__.setdefault("_plans", {})
        if key not in plans:
            plans[key] = getattr(self, name)(*args)
        return plans[key]

    def _walk(self, plan, c):
        with torch.no_grad():
            for e in plan:
                self._HANDLERS[e["kind"]](self, c, e)

    @classmethod
    def calls(cls, plan, stage=None):
        """Plan entries -> one dict per library call: the entry's fields, `stage` and `call`, the name the launcher reports."""
        out = []
        for e in plan:
            names = cls._HANDLERS[e["kind"]].calls
            out += [dict(e, stage=stage, call=name) for name in (names(e) if callable(names) else names)]
        return out

    def _param_grads(self, out):
        """per-layer (grad_weight, grad_g, grad_bias) -> the gradients in named_parameters() order"""
        grads = []
        for name, p in self.named_parameters():
            layer, leaf = name.rsplit(".", 1)
            gw, gg, gb = out[layer]
            t = (gb if leaf == "bias" else (gg if leaf == "weight_g" else gw)).view_as(p)
            grads.append(t if t.dtype == p.dtype else t.to(p.dtype))
        return grads

    @handles("finish", "hifigan_wgrad_finish")
    def _do_finish(self, c, e):
        o = c.ops[e["layer"]]
        c.out[e["layer"]] = KV.hifigan_wgrad_finish(e["mode"], c.parts[0], c.parts[1], o.v, o.g, u=e.get("u", 1))
        c.parts = None
