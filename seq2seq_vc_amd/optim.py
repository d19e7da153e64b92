"""Flat-buffer Adam with gradient clipping and WarmupLR, one fused HIP launch sequence per step.

Replaces the reference's `clip_grad_norm_` -> `torch.optim.Adam.step()` -> `WarmupLR.step()` sequence
(trainers/ar_vc.py:99-107, trainers/aas_vc.py:151-158, schedulers/warmup_lr.py:54-61).

All trainable parameters of the model are re-pointed into ONE contiguous fp32 buffer (`flat_p`); their
gradients live in a parallel buffer (`flat_g`, exposed as `p.grad` views and as `p._s2s_grad` so the
wgrad kernels accumulate straight into it); Adam moments and the bf16 shadow used by bf16 GEMMs are
flat as well, and the matrix-shaped weights additionally keep a TRANSPOSED bf16 copy (refreshed by one batched tile-
transpose launch per step) so that data-gradient GEMMs read K-contiguous operands.  The step counter, learning rate, gradient norm and clip coefficient live in a 4-float
device tensor, so the optimiser step is hipGraph-capturable and needs no host synchronisation.  The
flat gradient buffer is also what data-parallel training all-reduces (distributed.py): a handful of
large RCCL collectives instead of one per tensor.

MultiAdamW (end of this file) is the other kind: torch.optim.AdamW over the caller's own tensors, as a torch.optim.Optimizer with
torch's state-dict layout, stepped by a few table-driven launches (csrc/adamw_multi.hip) -- the vocoder fine-tuning loop's optimiser.
"""
import collections

import torch

from .ops import kernels as K


# What plan_layout returns.  params / offsets: the trainable parameters in flat order and where each starts; numel: the flat element
# count; groups / stacks: the Q|K|V groups and decoder K|V stacks that turned out contiguous (dicts of _attention_groups /
# _source_attention_stacks plus "ow", "ob": offsets of their first weight and bias); t_table: the transposed-shadow table, one
# (source offset, destination offset, rows, cols, owner) per matrix, owner = the parameter, or (object, attribute, key) of a
# fused view that FlatAdam attaches (module._fused["w_qkv"], decoder._src_kv_all["w"]); t_numel: elements of the transposed buffer.
Layout = collections.namedtuple("Layout", "params offsets numel groups stacks t_table t_numel")


def _round_up(n, align):
    return (n + align - 1) // align * align


def _source_attention_stacks(model):
    """Per modules.Decoder: the K / V weights and biases of the source-attention blocks of all its layers, in layer order
    (k_1, v_1, k_2, v_2, ...)."""
    from .modules import Decoder, MultiHeadedAttention
    stacks = []
    for dec in model.modules():
        if not isinstance(dec, Decoder):
            continue
        mods = [layer.src_attn for layer in dec.decoders]
        if not mods or not all(type(m) is MultiHeadedAttention for m in mods):
            continue
        ws = [w for m in mods for w in (m.linear_k.weight, m.linear_v.weight)]
        bs = [b for m in mods for b in (m.linear_k.bias, m.linear_v.bias)]
        qs = [p for m in mods for p in (m.linear_q.weight, m.linear_q.bias)]
        if all(p is not None and p.requires_grad for p in ws + bs + qs) and len({w.shape for w in ws}) == 1:
            stacks.append({"decoder": dec, "mods": mods, "w": ws, "b": bs})
    return stacks


def _attention_groups(model, skip=()):
    from .modules import MultiHeadedAttention
    groups = []
    for m in model.modules():
        if id(m) in skip:
            continue
        if isinstance(m, MultiHeadedAttention):
            ws = [m.linear_q.weight, m.linear_k.weight, m.linear_v.weight]
            bs = [m.linear_q.bias, m.linear_k.bias, m.linear_v.bias]
            if all(p is not None and p.requires_grad for p in ws + bs):
                groups.append({"module": m, "w": ws, "b": bs})
    return groups


def _flat_order(params, runs):
    """The parameters in flat order: every run (group or stack) moves, weights then biases, to where its first weight stood.
    Also the ids of the `tight` members, which start right where their predecessor ends (no alignment gap)."""
    first = {id(r["w"][0]): r for r in runs}
    in_run = {id(p) for r in runs for p in r["w"] + r["b"]}
    ordered, tight = [], set()
    for p in params:
        if id(p) in first:
            r = first[id(p)]
            ordered += r["w"] + r["b"]
            if all(q.numel() % 8 == 0 for q in r["w"] + r["b"]):
                tight.update(id(q) for q in r["w"][1:] + r["b"][1:])
        elif id(p) not in in_run:
            ordered.append(p)
    return ordered, tight


def _contiguous(run, off_of):
    """Do the weights of a run lie back to back as ONE (len * D, D) matrix, and its biases as one vector?  Records "ow" / "ob"."""
    D = run["w"][0].shape[0]
    run["ow"], run["ob"] = ow, ob = off_of[id(run["w"][0])], off_of[id(run["b"][0])]
    return all(off_of[id(w)] == ow + i * D * D for i, w in enumerate(run["w"])) and \
        all(off_of[id(b)] == ob + i * D for i, b in enumerate(run["b"]))


def _transposed_table(params, offsets, numel, groups, stacks, align):
    """Matrices (Linear, 1x1 Conv1d) keep their offset in the transposed buffer; the fused views get extra room behind `numel`."""
    table = [(o, o, p.shape[0], p.shape[1], p) for p, o in zip(params, offsets)
             if p.dim() == 2 or (p.dim() == 3 and p.shape[-1] == 1)]
    extras = []
    for g in groups:
        D = g["w"][0].shape[0]
        extras += [(g["ow"], 3 * D, D, (g["module"], "_fused", "w_qkv")), (g["ow"] + D * D, 2 * D, D, (g["module"], "_fused", "w_kv"))]
    for st in stacks:
        D = st["w"][0].shape[0]
        extras.append((st["ow"], len(st["w"]) * D, D, (st["decoder"], "_src_kv_all", "w")))
    end = numel
    for off, rows, cols, owner in extras:
        table.append((off, end, rows, cols, owner))
        end += _round_up(rows * cols, align)
    return table, end


def plan_layout(model, align=64, fuse_qkv=True, transposed=True):
    """The flat layout of the trainable parameters of `model` (a Layout): pure host arithmetic, allocates nothing, works on a CPU
    model.  Offsets are multiples of `align` except inside a run.  The Q / K / V weights (and biases) of every attention module lie
    back to back, so that [Wq;Wk;Wv] is ONE (3D, D) matrix (fused projection GEMMs, modules.py); so do the source-attention K / V
    weights of all layers of a decoder, [Wk_1; Wv_1; ...; Wk_L; Wv_L] (the memory is projected for all layers by a single GEMM,
    modules.Decoder.forward).  Packed projections, the flat gradient slots, the data-parallel buckets (param_ranges) and the flat
    checkpoint format all hang on these offsets."""
    params = [p for p in model.parameters() if p.requires_grad]
    if not params:
        raise ValueError("no trainable parameters")
    stacks = _source_attention_stacks(model) if fuse_qkv else []
    groups = _attention_groups(model, skip={id(m) for st in stacks for m in st["mods"]}) if fuse_qkv else []
    ordered, tight = _flat_order(params, groups + stacks)
    offsets, n = [], 0
    for p in ordered:
        if id(p) not in tight:
            n = _round_up(n, align)
        offsets.append(n)
        n += p.numel()
    n = _round_up(n, align)
    off_of = {id(p): o for p, o in zip(ordered, offsets)}
    groups = [g for g in groups if _contiguous(g, off_of)]
    stacks = [st for st in stacks if _contiguous(st, off_of)]
    table, t_numel = _transposed_table(ordered, offsets, n, groups, stacks, align) if transposed else ([], n)
    return Layout(ordered, offsets, n, groups, stacks, table, t_numel)


class FlatAdam:
    def __init__(self, model, lr=8e-5, betas=(0.9, 0.999), eps=1e-8, grad_norm=1.0, warmup_steps=4000, bf16_shadow=False,
                 align=64, fuse_qkv=True, transposed_shadow=True):
        # torch.optim.Adam(model.parameters()) -- what the reference builds (bin/vc_train.py:405-416) -- numbers its state by
        # position in model.parameters(), frozen parameters included; kept for checkpoint interchange (state_dict below)
        self.all_params = list(model.parameters())
        self._model = model
        plan = plan_layout(model, align, fuse_qkv, transposed=bf16_shadow and transposed_shadow)
        self.params, self.offsets, self.numel = plan.params, plan.offsets, plan.numel
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FlatAdam needs the model on the GPU (there is no CPU path)")
        self.lr, self.betas, self.eps = float(lr), betas, float(eps)
        self.grad_norm, self.warmup_steps = float(grad_norm), float(warmup_steps or 0)
        n = self.numel
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev) if bf16_shadow else None
        self.state = torch.zeros(4, dtype=torch.float32, device=dev)  # step, lr, grad_norm, clip_coef
        self.partial = torch.empty(1024, dtype=torch.float64, device=dev)
        self._perm_jobs = K.PermRegistry()   # (parameter, permutation, persistent buffer): filled by ops.kernels.gather3_cached
        self._adopt_parameters()
        self._attach_fused_views(plan)
        self.shadow_t = self.t_tiles = None
        if plan.t_table:
            self._attach_transposed(plan)
        if self.shadow is not None:
            self.refresh_shadow()

    def _adopt_parameters(self):
        """Move the parameters into flat_p and point their gradient (and bf16 shadow) at the parallel buffers."""
        for p, o in zip(self.params, self.offsets):
            k = p.numel()
            self.flat_p[o:o + k].copy_(p.data.reshape(-1))
            p.data = self.flat_p[o:o + k].view(p.shape)
            p._s2s_grad = self.flat_g[o:o + k].view(p.shape)
            p.grad = p._s2s_grad
            p._s2s_perm_registry, p._s2s_perms = self._perm_jobs, {}
            if self.shadow is not None:
                p._s2s_bf16 = self.shadow[o:o + k].view(p.shape)

    def _attach_fused_views(self, plan):
        """module._fused of every contiguous Q|K|V group and source-attention block, decoder._src_kv_all of every stack."""
        for g in plan.groups:
            D, ow, ob = g["w"][0].shape[0], g["ow"], g["ob"]
            g["module"]._fused = {
                "w_qkv": self._view(ow, (3 * D, D)), "b_qkv": self._view(ob, (3 * D,)),
                "w_q": self._view(ow, (D, D)), "b_q": self._view(ob, (D,)),
                "w_kv": self._view(ow + D * D, (2 * D, D)), "b_kv": self._view(ob + D, (2 * D,))}
        for st in plan.stacks:                  # each block keeps its own (2D, D) view of the stack
            D, ow, ob = st["w"][0].shape[0], st["ow"], st["ob"]
            for li, m in enumerate(st["mods"]):
                m._fused = {"w_q": m.linear_q.weight, "b_q": m.linear_q.bias,
                            "w_kv": self._view(ow + li * 2 * D * D, (2 * D, D)), "b_kv": self._view(ob + li * 2 * D, (2 * D,))}
            st["decoder"]._src_kv_all = {"w": self._view(ow, (len(st["w"]) * D, D)), "b": self._view(ob, (len(st["b"]) * D,))}

    def _attach_transposed(self, plan):
        """The transposed bf16 shadow of the matrix-shaped weights: dX = dY.W then reads a K-contiguous operand and runs on the
        all-DMA GEMM kernel.  `_s2s_bf16_t` on every owner of plan.t_table, and the tile list of the batched transpose."""
        dev = self.flat_p.device
        self.shadow_t = torch.zeros(plan.t_numel, dtype=torch.bfloat16, device=dev)
        tiles = []
        for so, do, rows, cols, owner in plan.t_table:
            t = owner if isinstance(owner, torch.Tensor) else getattr(owner[0], owner[1])[owner[2]]
            t._s2s_bf16_t = self.shadow_t[do:do + rows * cols].view(cols, rows)
            nt = ((rows + 63) // 64) * ((cols + 63) // 64)
            tiles += [(so, do, (rows << 32) | cols, i) for i in range(nt)]
        self.t_tiles = torch.tensor(tiles, dtype=torch.int64, device=dev)
        for g in plan.groups:                   # w_q view: the transposed copy of linear_q.weight
            g["module"]._fused["w_q"]._s2s_bf16_t = g["w"][0]._s2s_bf16_t

    def _view(self, off, shape):
        """A trainable-looking view of the flat buffers (fp32 master, flat-gradient slot, bf16 shadow)."""
        n = 1
        for d in shape:
            n *= d
        t = self.flat_p[off:off + n].view(shape)
        t.requires_grad_(True)
        t._s2s_grad = self.flat_g[off:off + n].view(shape)
        t._s2s_perm_registry = self._perm_jobs
        if self.shadow is not None:
            t._s2s_bf16 = self.shadow[off:off + n].view(shape)
        return t

    def _touch(self):
        """The parameters changed through raw pointers (no tensor version bump): advance the model's weight generation so
        that cached derived state (decode sessions with packed / bf16 weight copies, decode.py) is rebuilt."""
        self._model.__dict__["_s2s_weight_gen"] = self._model.__dict__.get("_s2s_weight_gen", 0) + 1

    def refresh_shadow(self):
        """bf16 copy of the fp32 master weights (after loading a checkpoint / at start)."""
        self._touch()
        if self.shadow is not None:
            self.shadow.copy_(K.cast(self.flat_p, torch.bfloat16))
        self.refresh_derived()

    def refresh_derived(self):
        """Every derived copy of the weights, in line on the current stream -- called from exactly step() and refresh_shadow(), so
        nothing that reads a copy can see a stale one: the permuted convolution weights that the forward / backward passes
        registered (ops.kernels.gather3_cached) and the class matrices of the front-end's transposed convolution
        (tconv2d_weights_cached) in ONE launch, then the transposed bf16 shadow (one tile-transpose launch).
        Copies that a captured refresh cannot know (`covered`, `tconv_covered`) are computed again on use."""
        reg = self._perm_jobs
        K.derived_refresh(reg, reg.tconv)
        if self.flat_p.is_cuda and torch.cuda.is_current_stream_capturing():
            # a captured refresh updates exactly the copies registered NOW on every replay; copies that register later (first
            # evaluation in another dtype, a convolution first used later) are not in it
            reg.covered = len(reg) if reg.covered is None else min(reg.covered, len(reg))
            reg.tconv_covered = len(reg.tconv) if reg.tconv_covered is None else min(reg.tconv_covered, len(reg.tconv))
        if self.shadow_t is not None:
            K.transpose_tiles(self.t_tiles, self.shadow, self.shadow_t)

    # After an optimiser step three memory-bound passes stand between it and the next backward pass: the permuted convolution
    # weights with the class matrices of the front-end's transposed convolution (needed by the forward / backward pass; ONE
    # launch, ops.kernels.derived_refresh), the transposed bf16 shadow (data-gradient GEMMs) and the zero-fill of the flat
    # gradient buffer (weight-gradient kernels accumulate): 82 + 145 + 80 us of a 10.9 ms AAS-VC step, 24 + 31 + 17 us of a
    # 3.6 ms VTN step.  They run IN LINE: the refresh at the end of step(), the zero-fill in begin_step() / zero_grad().
    # (Running them on a stream of their own beside the forward pass lost: 13.0 vs 12.74 ms per AAS-VC step, VTN equal; as capped
    # grids of 16 ... 2048 workgroups 11.52-11.59 vs 11.40 ms -- what runs beside the forward chain is not free even when it is
    # HBM-bound.  profiles/AB_LOG.md.)

    def begin_step(self, zero=True):
        """First call of a training step (before the forward pass): clear the gradients unless the caller keeps them (gradient
        accumulation, or a trainer that clears them after its optimiser step)."""
        if zero:
            self._zero_gradients()

    def join_prologue(self):
        """Empty on purpose: bench.py calls it before the backward pass and is not ours to change; there is nothing to join."""

    def _zero_gradients(self):
        if self.flat_g.is_cuda:
            K.zero_(self.flat_g)                 # (a launch of this library: no ATen kernel inside a captured step)
        else:
            self.flat_g.zero_()

    def param_ranges(self, modules):
        """Maximal contiguous [lo, hi) ranges of the flat buffers that hold exactly the trainable parameters of `modules`
        (alignment gaps between neighbours are absorbed): the buckets of the data-parallel gradient exchange.  Returns []
        if the modules have no trainable parameters."""
        mine = set()
        for m in modules:
            mine.update(id(p) for p in (m.parameters() if isinstance(m, torch.nn.Module) else [m]))
        order = sorted(zip(self.offsets, self.params), key=lambda t: t[0])
        ranges, cur = [], None
        for i, (o, p) in enumerate(order):
            end = order[i + 1][0] if i + 1 < len(order) else self.numel      # up to the next parameter (absorbs the padding)
            if id(p) in mine:
                if cur is not None and cur[1] == o:
                    cur[1] = end
                else:
                    cur = [o, end]
                    ranges.append(cur)
            else:
                cur = None
        return [tuple(r) for r in ranges]

    def zero_grad(self, set_to_none=False):
        """The zero-fill of the flat gradient buffer, in line (the gradients are views of it: never set to None)."""
        self._zero_gradients()

    def step(self):
        K.adam_step(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.shadow, self.state, self.partial, self.lr,
                    self.betas, self.eps, self.grad_norm, self.warmup_steps)
        self.refresh_derived()               # in line: a captured step leaves the derived copies fresh for its next replay
        self._touch()

    # -- introspection (host sync; for logging / tests only) -------------------------------------
    def last_stats(self):
        s = self.state.tolist()
        return {"step": int(s[0]), "lr": s[1], "grad_norm": s[2], "clip_coef": s[3]}

    # -- checkpoints: the reference saves `optimizer.state_dict()` of torch.optim.Adam (trainers/base.py:85-105) --------------
    def state_dict(self):
        """torch.optim.Adam's format -- {"state": {i: {step, exp_avg, exp_avg_sq}}, "param_groups": [...]} with i = position
        in model.parameters() -- so that the reference (or a stock torch Adam over the same model) resumes from a checkpoint
        written here and vice versa.  Deviation (documented): ONE step counter for all parameters, so every entry carries the
        same `step`; torch keeps one per parameter, which only differs for parameters that joined training late."""
        step = self.state[0].detach().cpu().clone()
        off_of = {id(p): o for p, o in zip(self.params, self.offsets)}
        state = {}
        if float(step) > 0:
            for i, p in enumerate(self.all_params):
                o = off_of.get(id(p))
                if o is None:
                    continue
                k = p.numel()
                state[i] = {"step": step.clone(), "exp_avg": self.exp_avg[o:o + k].view(p.shape).detach().cpu().clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + k].view(p.shape).detach().cpu().clone()}
        k = int(float(step))
        # torch's group["lr"] after k optimiser + k scheduler steps is the value the NEXT step will use (WarmupLR at k + 1)
        w = self.warmup_steps
        next_lr = self.lr * w ** 0.5 * min((k + 1) ** -0.5, (k + 1) * w ** -1.5) if w > 0 else self.lr
        group = {"lr": next_lr, "betas": tuple(self.betas), "eps": self.eps,
                 "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                 "differentiable": False, "fused": None, "initial_lr": self.lr, "params": list(range(len(self.all_params)))}
        return {"state": state, "param_groups": [group],
                "s2svc": {"grad_norm": self.grad_norm, "warmup_steps": self.warmup_steps, "layout": "torch.optim.Adam"}}

    def load_state_dict(self, sd):
        """Accepts torch.optim.Adam state dicts (reference checkpoints) and the flat format of round 1."""
        if "state" in sd and "param_groups" in sd:
            ids = sd["param_groups"][0]["params"]
            if len(ids) != len(self.all_params):
                raise ValueError(f"optimizer state is for {len(ids)} parameters, the model has {len(self.all_params)}")
            pos = {pid: i for i, pid in enumerate(ids)}
            off_of = {id(p): o for p, o in zip(self.params, self.offsets)}
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            steps = set()
            for pid, st in sd["state"].items():
                i = pos[pid]
                p = self.all_params[i]
                o = off_of.get(id(p))
                if o is None:
                    continue            # state of a parameter that is frozen here
                if tuple(st["exp_avg"].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state {pid}: shape {tuple(st['exp_avg'].shape)} vs parameter {tuple(p.shape)}")
                k = p.numel()
                self.exp_avg[o:o + k].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
                steps.add(int(float(st["step"])))
            if len(steps) > 1:
                import logging
                logging.warning(f"per-parameter Adam steps {sorted(steps)} differ; FlatAdam keeps one counter and resumes at {max(steps)}")
            g = sd["param_groups"][0]
            self.lr = float(g.get("initial_lr", self.lr))
            self.betas, self.eps = tuple(g.get("betas", self.betas)), float(g.get("eps", self.eps))
            extra = sd.get("s2svc", {})
            self.grad_norm = float(extra.get("grad_norm", self.grad_norm))
            self.warmup_steps = float(extra.get("warmup_steps", self.warmup_steps))
            self.state.zero_()
            self.state[0] = float(max(steps)) if steps else 0.0
        else:
            if list(sd.get("offsets", [])) != list(self.offsets) or sd["exp_avg"].numel() != self.numel:
                raise ValueError("flat optimizer state was written for a different parameter layout (frozen modules, fused "
                                 "projections or alignment differ); re-save it in the torch.optim.Adam format")
            self.state.copy_(sd["step"])
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.refresh_shadow()


# ---------------------------------------------------------------------------------------------------------------------------
# MultiAdamW: torch.optim.AdamW over the caller's own tensors, a few table-driven launches per step (csrc/adamw_multi.hip)
# ---------------------------------------------------------------------------------------------------------------------------
ADAMW_GROUP = 80        # tensors per launch; the library states the same number (adamw_multi_group)
ADAMW_CHUNK = 4096      # elements per workgroup (adamw_multi_chunk)
MOMENT_ALIGN = 4        # elements: every tensor's chunk of the flat moment buffers starts 16-byte aligned


def plan_moments(numels, align=MOMENT_ALIGN):
    """(offsets, total): tensor i owns [offsets[i], offsets[i] + numels[i]) of the two flat moment buffers, offsets multiples of
    `align`; the gap up to the next offset belongs to nobody.  Pure host arithmetic."""
    offsets, n = [], 0
    for k in numels:
        if k < 1:
            raise ValueError("plan_moments: every tensor has at least one element")
        offsets.append(n)
        n = _round_up(n + int(k), align)
    return offsets, n


def adamw_table(numels, offsets, chunk=ADAMW_CHUNK):
    """The index model of one launch over these tensors: the workgroup prefix table and, per workgroup, what it touches --
    (tensor, [lo, hi) inside the tensor, vector elements, tail elements).  A workgroup walks whole groups of four from `lo` and then
    the tensor's OWN tail: it never reaches past offsets[i] + numels[i], so it never touches the neighbour's chunk or the gap."""
    prefix, work = [0], []
    for i, k in enumerate(numels):
        nch = -(-int(k) // chunk)
        prefix.append(prefix[-1] + nch)
        for c in range(nch):
            lo, hi = c * chunk, min(int(k), (c + 1) * chunk)
            work.append((i, lo, hi, (hi - lo) // 4 * 4, (hi - lo) % 4))
    return prefix, work


class MultiAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay, torch's formula, eps added after the sqrt(v) / sqrt(1 - beta2^t) division) with
    every tensor of a step updated by a few table-driven HIP launches: the addresses of the parameters and of their -- every step
    fresh -- gradients travel as kernel arguments in groups of 80, so a step is ceil(tensors with a gradient / 80) launches and
    nothing else: 3 for the HiFi-GAN generator (234 tensors), 2 for the discriminator (154), no device table, no copy, no stream
    stop, no per-tensor launch.  `exp_avg` / `exp_avg_sq` live in two flat buffers (`self.exp_avg`, `self.exp_avg_sq`), each
    tensor's chunk 16-byte aligned; the state entries are views of them.

    A torch.optim.Optimizer: lr schedulers accept it, `param_groups[i]["lr"]` is the live rate, read on the host at each step().
    Parameters whose .grad is None are skipped and their step count does not advance, as in torch.  state_dict() /
    load_state_dict() use torch.optim.AdamW's own layout (state[i] = {step, exp_avg, exp_avg_sq}, the same param_groups keys), so an
    optimiser block of a reference checkpoint loads and ours loads into torch.optim.AdamW; state_dict() holds copies, and
    load_state_dict() copies into the flat buffers without rebinding them.  fp32 parameters on the GPU only (construction and the
    state-dict layout work on CPU tensors; step() there raises)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("MultiAdamW: lr, eps, weight_decay >= 0 and 0 <= beta < 1")
        params = list(params)
        # torch's own defaults dict for these arguments: the param_groups keys of whatever torch release is installed
        defaults = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        super().__init__(params, defaults)
        flat = [p for g in self.param_groups for p in g["params"]]
        for p in flat:
            if p.dtype != torch.float32:
                raise TypeError("MultiAdamW: float32 parameters")
            if not p.is_contiguous():
                raise ValueError("MultiAdamW: contiguous parameters")
        if len({p.device for p in flat}) != 1:
            raise ValueError("MultiAdamW: all parameters on one device")
        self._flat = flat
        self.offsets, self.numel = plan_moments([p.numel() for p in flat])
        dev = flat[0].device
        self.exp_avg = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self._offset_of = {id(p): o for p, o in zip(flat, self.offsets)}
        # the step counts of all tensors in ONE host tensor, state[p]["step"] a 0-dim view of it: one vector increment and one
        # tolist() per step (a `+= 1` and a float() per tensor were 70 % of step()'s host time over 154 tensors)
        self._steps = torch.zeros(len(flat), dtype=torch.float32)
        self._index_of = {id(p): i for i, p in enumerate(flat)}

    def launches_per_step(self, tensors=None):
        """Library launches of one step() over `tensors` tensors with a gradient (default: all)."""
        return -(-(len(self._flat) if tensors is None else tensors) // ADAMW_GROUP)

    def _views(self, p):
        o, k = self._offset_of[id(p)], p.numel()
        return self.exp_avg[o:o + k].view(p.shape), self.exp_avg_sq[o:o + k].view(p.shape)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("MultiAdamW: amsgrad / maximize are not implemented")
            lr, (beta1, beta2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
            live = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("MultiAdamW needs GPU parameters (there is no CPU path)")
                g = p.grad
                if g.is_sparse or g.dtype != torch.float32:
                    raise TypeError("MultiAdamW: dense float32 gradients")
                if not g.is_contiguous():
                    g = g.contiguous()
                st = self.state[p]
                if not st:
                    st["step"] = self._steps[self._index_of[id(p)]]
                    st["exp_avg"], st["exp_avg_sq"] = self._views(p)
                live.append((p, g, self._index_of[id(p)]))
            if len(live) == len(self._flat):
                self._steps += 1
            elif live:
                self._steps[[i for _, _, i in live]] += 1
            counts, corr, rows = self._steps.tolist(), {}, []
            for p, g, i in live:
                t = counts[i]
                if t not in corr:
                    corr[t] = (lr / (1.0 - beta1 ** t), (1.0 - beta2 ** t) ** 0.5)
                rows.append((p, g) + corr[t])
            for i in range(0, len(rows), ADAMW_GROUP):
                K.adamw_multi([(p, g, self._offset_of[id(p)], ss, bs) for p, g, ss, bs in rows[i:i + ADAMW_GROUP]], self.exp_avg,
                              self.exp_avg_sq, 1.0 - lr * wd, beta1, beta2, eps)
        return loss

    def state_dict(self):
        """torch.optim.AdamW's layout; the moments and step counts are copies (a checkpoint does not move with later steps)."""
        sd = super().state_dict()
        sd["state"] = {i: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()} for i, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts torch.optim.AdamW state dicts (and this class's own): the moments are copied INTO the flat buffers, which stay
        where they are; parameters without an entry go back to zero moments and no state."""
        super().load_state_dict(state_dict)
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self._steps.zero_()
        for p in self._flat:
            st = self.state.get(p)
            if not st:
                continue
            m, v = self._views(p)
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            st["exp_avg"], st["exp_avg_sq"] = m, v
            i = self._index_of[id(p)]
            self._steps[i] = float(st["step"])
            st["step"] = self._steps[i]
