"""Where and when the parameter-gradient work of a training step is launched: gradient cuts, the side-stream pool and its
batches, the auxiliary-stream branch, and the roots of a backward pass.  The autograd ops (ops.functional*) hand their
weight / bias / norm gradient closures to `_side_run`; trainers call `side_join()` between backward and the optimiser step.
What a batch queues and how it is launched is ops.kernels.GradBatch."""
import os

import torch

from . import kernels as K

# ------------------------------------------------------------------------------------------------
# Gradient cuts (data-parallel overlap).  A model's forward marks a few tensors with cut_point(x, name).  Normally that is
# the identity.  Inside `with grad_cuts(GradCuts([...]))` the autograd graph is cut there: the consumer sees a detached leaf,
# so loss.backward() stops at it, and `cuts.resume(name)` later continues the backward pass below the cut.  Everything
# above a cut has then finished its parameter gradients and their all-reduce can travel while the rest of the backward
# pass runs (distributed.OverlappedBackward); each piece can also be captured as its own hipGraph with the collectives
# issued between the replays.  Values and gradients are exactly those of the uncut graph.
# ------------------------------------------------------------------------------------------------


class GradCuts:
    def __init__(self, names):
        self.names = set(names)
        self.points = {}          # name -> (tensor above the cut [graph side of the producer], detached leaf the consumers see)

    def cut(self, x, name):
        """x: a tensor, or a tuple of tensors crossing the cut together (e.g. the residual stream of a pre-norm layer stack
        and the feed-forward output still to be added to it); None members pass through."""
        if name not in self.names or not torch.is_grad_enabled():
            return x
        xs = x if isinstance(x, tuple) else (x,)
        if not any(t is not None and t.requires_grad for t in xs):
            return x
        if name in self.points:
            raise RuntimeError(f"gradient cut '{name}' was reached twice in one forward pass")
        inner = tuple(t.detach().requires_grad_(True) if (t is not None and t.requires_grad) else t for t in xs)
        self.points[name] = (xs, inner)
        return inner if isinstance(x, tuple) else inner[0]

    def resume(self, name):
        """Continue the backward pass below the cut (no-op if the forward pass never reached it or nothing above it
        needed the gradient)."""
        outer, inner = self.points.get(name, (None, None))
        if outer is None:
            return
        pairs = [(o, i.grad) for o, i in zip(outer, inner) if o is not None and o.requires_grad and i is not o and i.grad is not None]
        if pairs:
            torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs], retain_graph=False)

    def clear(self):
        self.points.clear()


_CUTS = {"active": None}


class grad_cuts:
    def __init__(self, cuts):
        self.cuts = cuts

    def __enter__(self):
        self.prev, _CUTS["active"] = _CUTS["active"], self.cuts
        if self.cuts is not None:
            self.cuts.clear()
        return self.cuts

    def __exit__(self, *exc):
        _CUTS["active"] = self.prev
        return False


def cut_point(x, name):
    c = _CUTS["active"]
    return x if c is None else c.cut(x, name)


# ------------------------------------------------------------------------------------------------
# Side streams for parameter-gradient work.  Weight / bias / LayerNorm gradients are only consumed by
# the optimiser at the end of the step, so (when they land in flat-gradient slots) their kernels are
# issued on a small pool of side HIP streams and overlap with the data-gradient chain on the main
# stream; `side_join()` must be called after backward() and before the optimiser step.  Under hipGraph
# capture the cross-stream waits become graph edges, i.e. parallel branches of the captured step.
# ------------------------------------------------------------------------------------------------
class _Side:
    enabled = False
    streams = []
    idx = 0
    pending = []     # tensors that must stay alive until the join (their memory is in use on a side stream)
    queue = []       # closures waiting for the next fork point
    origins = []     # the stream each queued closure was issued from
    inline = False   # no side streams, but batched (see enable_side_streams)
    inline_q = {}    # stream handle -> (stream, [closures])
    batch = 16
    on_flush = None  # callable(): called on the flushing stream behind every flushed batch (distributed.FlushExchange)


# Workgroups of the grouped weight-gradient launches (GEMMs and Conv1d) of a FORKED batch (VTN / TTS; K.GradBatch.cap): such a
# launch runs beside the latency-bound data-gradient chain, and a 144 KB-LDS workgroup on every CU makes each small kernel of the
# chain wait for one -- measured 3.789 -> 3.773 ms per VTN step (five interleaved repeats; 48 / 96 / 128 workgroups: 3.778 /
# 3.774 / 3.780).  Units are walked in order: bit-identical results.  Inline batches, immediate mode and the batch side_join
# flushes are not capped (0 = one workgroup per unit).
_FORK_CAP = 64


def set_on_flush(callback=None):
    """callback(): called on the flushing stream behind every flushed batch; None takes it out."""
    _Side.on_flush = callback


def gradient_streams():
    """The streams that gradient work may be on beside the current one: the auxiliary stream (if a branch has run) and the side streams."""
    return ([] if _Branch.stream is None else [_Branch.stream]) + list(_Side.streams)


def taken_streams():
    """Handles of the streams that are spoken for: gradient_streams() and the current stream."""
    h = {st.cuda_stream for st in gradient_streams()}
    if torch.cuda.is_available():
        h.add(torch.cuda.current_stream().cuda_stream)
    return h


def distinct_stream(taken=None):
    """A torch.cuda.Stream whose underlying stream is none of `taken` (default: the side streams, the auxiliary stream and the
    current stream).  torch hands out Stream objects round-robin from a pool of 32 per device: a process that has created many
    (every trainer / test / decode session creates a few) gets ALIASES of earlier ones, and two roles that the scheduling here
    keeps apart -- e.g. the auxiliary stream of a branch and a side stream of the gradient work -- end up on one stream, which a
    capture with forks and joins between them does not survive (seen as a segmentation fault in hipStreamEndCapture)."""
    taken = taken_streams() if taken is None else set(taken)
    for _ in range(96):
        st = torch.cuda.Stream()
        if st.cuda_stream not in taken:
            return st
    raise RuntimeError("no distinct stream left in torch's stream pool")


def enable_side_streams(n=4, inline_batches=False, batch=None):
    """batch: closures per gradient batch (default: 16 forked / 64 inline).  Round 4 re-measured both with
    the 8-wave weight-gradient kernel that takes 40 problems per launch: VTN 12 -> 16: 3.95 -> 3.86 ms, AAS-VC 12 -> 48 ... 160:
    11.85 -> 11.6-11.7 ms (larger grids, fewer ragged last rounds; the operands stay alive a little longer).
    n > 0: parameter-gradient work is forked to n side streams (small, latency-bound models: VTN).
    n == 0 and inline_batches: the work stays on the stream that issued it but is still queued and run in batches, so
    that the dense weight-gradient GEMMs of a batch become one grouped launch -- for models whose kernels fill the chip
    anyway (AAS-VC: d = 1536) the forks cost more than the overlap gives (19.3 vs 20.9 ms/step).  Both need side_join()
    between backward and the optimiser step; n == 0 without inline_batches runs everything immediately."""
    _Side.enabled = n > 0
    _Side.inline = (n == 0) and inline_batches
    _Side.batch = int(batch) if batch else (64 if _Side.inline else 16)
    old, others = _Side.streams, taken_streams() - {st.cuda_stream for st in _Side.streams}
    if n > 0 and len(old) == n and len({st.cuda_stream for st in old}) == n and not ({st.cuda_stream for st in old} & others):
        pass                                     # keep the ones we have: every new Stream object eats a slot of torch's pool
    else:
        _Side.streams = []
        for _ in range(n):
            _Side.streams.append(distinct_stream())
    _Side.idx = 0


def _side_run(fn, keep=(), solo=False):
    """Parameter-gradient work off the data-gradient chain: `fn` is queued and runs on a side stream in batches of
    `_Side.batch` closures -- one fork point (cross-stream edge of the captured graph) per batch instead of one per call.
    The stream the caller runs on is remembered: backward nodes of a branch (branch_run) execute on the branch's stream.
    solo=True: `fn` is forked NOW as a batch of its own (long kernels at the end of the backward pass: whatever shares their
    batch runs behind them on the same stream)."""
    if _Side.inline:
        cur = torch.cuda.current_stream()
        q = _Side.inline_q.setdefault(cur.cuda_stream, (cur, []))[1]
        q.append(fn)
        _Side.pending.append(keep)
        if len(q) >= _Side.batch:
            _inline_flush(cur.cuda_stream)
        return
    if not _Side.enabled:
        fn()
        return
    _Side.pending.append(keep)
    if solo:
        _fork([fn], [torch.cuda.current_stream()], _FORK_CAP)
        return
    _Side.queue.append(fn)
    _Side.origins.append(torch.cuda.current_stream())
    if len(_Side.queue) >= _Side.batch:
        _side_flush()


def _run_batch(closures, batch):
    """Run a batch of gradient closures on the current stream: their dense weight-gradient GEMMs become ONE grouped launch
    (no split-K, no reduction passes), their column reductions into gradient slots (LayerNorm / BatchNorm / bias vectors)
    two grouped launches, the eligible Conv1d weight gradients of a FORKED batch (the Postnet's) one launch capped like the grouped
    GEMMs (csrc/conv1d_wgrad.hip); everything else they launch (other conv weight gradients, ...) runs as issued."""
    with K.recording(batch):
        for fn in closures:
            fn()
    batch.flush()
    if _Side.on_flush is not None:
        _Side.on_flush()


def _inline_flush(key):
    """Run the closures queued from one stream ON that stream (no fork), the dense weight gradients as a grouped launch."""
    st, q = _Side.inline_q.pop(key)
    with torch.cuda.stream(st):
        _run_batch(q, K.GradBatch())
    return st


def _fork(closures, origins, cap):
    """Fork `closures` (issued from the streams `origins`) as one batch, now, to the next side stream of the pool."""
    k = _Side.idx % len(_Side.streams)
    st = _Side.streams[k]
    cur = torch.cuda.current_stream().cuda_stream
    if st.cuda_stream == cur or (_Branch.stream is not None and st.cuda_stream == _Branch.stream.cuda_stream):
        st = _Side.streams[k] = distinct_stream()        # an alias (see distinct_stream): e.g. the capture stream of a later graph
    _Side.idx += 1
    seen = set()
    for origin in origins + [torch.cuda.current_stream()]:     # every stream that produced an input of the batch
        if origin.cuda_stream not in seen:
            seen.add(origin.cuda_stream)
            st.wait_stream(origin)
    with torch.cuda.stream(st):
        _run_batch(closures, K.GradBatch(cap))


def _side_flush(cap=_FORK_CAP):
    """Fork what is queued (forked mode; nothing otherwise)."""
    if _Side.inline or not _Side.queue:
        return
    closures, origins = _Side.queue, _Side.origins
    _Side.queue, _Side.origins = [], []
    _fork(closures, origins, cap)


# ------------------------------------------------------------------------------------------------
# Independent sub-networks (e.g. the duration predictor next to the length regulator + decoder of AAS-VC) can run on
# an auxiliary stream: hundreds of small dependent kernels then fill the gaps of the other branch instead of extending
# the chain.  torch's autograd engine runs every backward node on the stream of its forward op, so the backward pass of
# the branch overlaps as well; under hipGraph capture fork and join are two graph edges.
# ------------------------------------------------------------------------------------------------
_NO_BRANCH = os.environ.get("S2SVC_NO_BRANCH", "0") == "1"      # diagnostic: branches run in line on the issuing stream


class _Branch:
    stream = None
    active = False
    dirty = False        # work was put on the auxiliary stream since the last join of a backward pass (side_join)


def branch_run(fn, uses=()):
    """Run fn() on the auxiliary stream, after everything queued on the current stream.  Call branch_join() on the
    current stream before anything there consumes the results.
    `uses`: the tensors of the CURRENT stream that fn reads (or saves for its backward pass).  They are recorded on the auxiliary
    stream: the caching allocator hands a block back to the stream that allocated it the moment the last reference goes, and
    the last reference to these is dropped by the branch (autograd releasing what its nodes saved) while the kernel that
    reads them may not have run yet -- a kernel of the allocating stream queued after that point could then overwrite the block
    under the reader.  Eager launches hide this (the reader was launched first and the GPU keeps up); in a captured graph
    only dependencies order the two streams (seen as wrong duration-predictor gradients in the AAS-VC stage graphs: the
    alignment search's durations `ds`, saved by the flow's backward pass, held another tensor by the time it read them)."""
    if not torch.cuda.is_available() or _NO_BRANCH:
        return fn()
    main = torch.cuda.current_stream()
    if _Branch.stream is None or _Branch.stream.cuda_stream == main.cuda_stream:
        _Branch.stream = distinct_stream()
    _Branch.stream.wait_stream(main)
    for t in uses:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            t.record_stream(_Branch.stream)
    with torch.cuda.stream(_Branch.stream):
        out = fn()
    _Branch.active = True
    _Branch.dirty = True
    return out


def branch_join(*results):
    """Make the current stream wait for the auxiliary stream; `results` are tensors produced there that the current
    stream goes on to use (their memory must not return to the auxiliary stream's pool while that use is pending)."""
    if _Branch.active:
        main = torch.cuda.current_stream()
        main.wait_stream(_Branch.stream)
        for t in results:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(main)
        _Branch.active = False


def branch_backward(loss, fork_event, retain_graph=False, scale=1.0):
    """loss.backward() rooted on the auxiliary stream, which starts from `fork_event` (recorded on the calling stream at the
    start of a backward stage).  Call it BEFORE the stage's other roots and branch_wait() after them: the nodes of a
    sub-network that ran under branch_run() go to the auxiliary stream, the loss arithmetic and whatever else of this root ran on
    the calling stream goes there while it is still empty, and the other roots then queue beside the branch.  (A root processed
    on the calling stream after other work puts its first nodes -- and with them the whole branch -- behind that work; one
    processed there before it stalls the caller at the first node that consumes a result of the branch.)"""
    if _Branch.stream is None or _NO_BRANCH:
        root_backward(loss, scale, retain_graph)
        return
    _Branch.stream.wait_event(fork_event)
    _Branch.dirty = True
    with torch.cuda.stream(_Branch.stream):
        root_backward(loss, scale, retain_graph)


def branch_resume(cuts, name, fork_event):
    """cuts.resume(name) rooted on the auxiliary stream (see branch_backward): the part of a branch below a gradient cut, run one
    stage after the part above it."""
    if _Branch.stream is None or _NO_BRANCH:
        cuts.resume(name)
        return
    _Branch.stream.wait_event(fork_event)
    _Branch.dirty = True
    with torch.cuda.stream(_Branch.stream):
        cuts.resume(name)


def branch_wait():
    """The current stream waits for what has been queued on the auxiliary stream (end of a stage that used branch_backward)."""
    if _Branch.stream is not None and not _NO_BRANCH:
        torch.cuda.current_stream().wait_stream(_Branch.stream)


def side_join():
    """Run what is still queued and make the current stream wait for all side-stream gradient work (call between
    backward and optimiser)."""
    if _Side.inline:
        main = torch.cuda.current_stream()
        for key in list(_Side.inline_q):
            st = _inline_flush(key)
            if st.cuda_stream != main.cuda_stream:
                main.wait_stream(st)
    if _Side.enabled:
        # the batch flushed HERE runs behind the end of the data-gradient chain: there is nothing left to protect from a
        # chip-filling weight-gradient grid, so its launches are not capped
        _side_flush(cap=0)
        main = torch.cuda.current_stream()
        for st in _Side.streams:
            main.wait_stream(st)
    _join_branch_stream()
    K.audit_reset()                  # (writer audit, ops.kernels._Audit: a join -- every slot may change hands)
    _Side.pending.clear()
    _Side.idx = 0


def _join_branch_stream():
    """Backward nodes of a sub-network that ran under branch_run() execute on the auxiliary stream; nothing guarantees that the
    last of them is followed by work another stream waits for (autograd only joins streams that ran gradient-accumulation
    nodes; the parameter gradients here go straight to their slots).  So the join after a backward pass (side_join) also joins
    the auxiliary stream -- if a branch was started since the last join (a later stage graph of a staged backward pass has no
    part of the branch in it, and must not wait for an event of another capture)."""
    if _Branch.stream is not None and _Branch.dirty:
        torch.cuda.current_stream().wait_stream(_Branch.stream)
    _Branch.dirty = False


# ------------------------------------------------------------------------------------------------
# Roots of a backward pass
# ------------------------------------------------------------------------------------------------
_CONST_SCALAR = {}


def const_scalar(device, value=0.0):
    """A constant 0-dim fp32 tensor per (device, value): made once, outside any capture (the first step of a shape runs eagerly),
    so that roots of backward passes and absent loss terms cost no fill launch inside a captured step."""
    device = torch.device(device)
    key = (device.type, device.index, float(value))
    if key not in _CONST_SCALAR:
        _CONST_SCALAR[key] = torch.full((), float(value), dtype=torch.float32, device=device)
    return _CONST_SCALAR[key]


def _zero_scalar(device):
    return const_scalar(device, 0.0)


def root_backward(loss, scale=1.0, retain_graph=False):
    """(scale * loss).backward() with the root gradient handed in as a cached constant: autograd's implicit ones_like and a
    `loss * scale` would each be an ATen launch inside a captured step."""
    if loss.dim() == 0 and loss.dtype == torch.float32:
        loss.backward(gradient=const_scalar(loss.device, scale), retain_graph=retain_graph)
    else:
        (loss * scale if scale != 1.0 else loss).backward(retain_graph=retain_graph)
