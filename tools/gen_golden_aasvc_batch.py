"""Generate the fixtures of AASVC.inference_batch by IMPORTING the reference (see tools/gen_golden.py; runs only where it exists).

    python tools/gen_golden_aasvc_batch.py      # writes tests/golden/aasvc_tiny_inference_batch.npz, aasvc_det_tiny_inference_batch.npz

The reference cannot run a padded batch in inference, so the fixture IS the contract of inference_batch: B = 4 utterances
run ONE AT A TIME through the reference's AASVC.inference(x_b, dp_input=x_b) in eval(), their inputs and outputs stored padded.
The lengths are the test (asserted below and again by tests/test_aasvc_batch_host.py): a row that fills the batch, one with T % 4 != 0
(post-encoder reduction, AAS_TINY only), one with at most 3 encoder frames (shorter than the half width of the ks = 7 depthwise
convolution), one whose output crosses a 64-frame time tile of the kernels, every other output length different from that one.

Durations are compared exactly, so no pre-rounding duration may sit near a rounding boundary: every one of them is recomputed in float64
with the oracle's functions (oracle/models.py) and must stay a relative 1e-3 away from the boundaries of ceil / round (the margin of
gen_golden.py's stop threshold); pick another seed if one does not.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402

MARGIN = 1e-3
MAX_DP_OUTPUT = 10


def _pre_rounding(OM, sd, cfg, x, noise):
    """The value the duration predictor rounds (stochastic: exp(z0) before ceil; deterministic: exp(.) - 1 before round) of one utterance,
    in float64, from the oracle's own forward pass (its torch.ceil / torch.round call is observed), and the oracle's durations."""
    seen = []
    real = {"ceil": torch.ceil, "round": torch.round}

    def spy(name):
        def f(t, *a, **k):
            seen.append((name, t.detach().clone().reshape(-1)))
            return real[name](t, *a, **k)
        return f

    torch.ceil, torch.round = spy("ceil"), spy("round")
    try:
        with torch.no_grad():
            o = OM.aasvc_forward({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}, cfg, x[None].double(),
                                 torch.tensor([x.shape[0]]), None, None, dp_inputs=x[None].double(),
                                 noise=None if noise is None else noise.double(), training=False, inference=True)
    finally:
        torch.ceil, torch.round = real["ceil"], real["round"]
    assert len(seen) == 1, [s[0] for s in seen]
    return seen[0][0], seen[0][1], o["d_outs"][0]


def _boundary_margin(kind, v):
    """Smallest relative distance of the pre-rounding values to a boundary that changes the clamped duration: ceil(v) then min(., 10)
    changes at 1 .. 9 (v > 9 gives 10 either way, v > 0 always); max(round(v), 0) then min(., 10) changes at 0.5 .. 9.5."""
    bounds = torch.arange(1, MAX_DP_OUTPUT, dtype=torch.float64) if kind == "ceil" else torch.arange(0, MAX_DP_OUTPUT, dtype=torch.float64) + 0.5
    return float(((v.double()[:, None] - bounds[None, :]).abs() / bounds[None, :]).min())


def gen(M, name, cfg, Ts, seed, sd_from, sd_seed):
    """sd_from / sd_seed: the single-utterance fixture of tools/gen_golden.py (gen_aasvc_inference) whose state dict this one shares, and
    the seed that fixture's model was built with.  The weights are rebuilt here the same way and must equal the stored ones bit for
    bit; the new file then holds inputs and outputs only (the state dict is nine tenths of a tiny fixture's size)."""
    from oracle import models as OM
    torch.manual_seed(sd_seed)
    model = M.AASVC(**cfg)
    with torch.no_grad():                    # as gen_golden.gen_aasvc_inference: durations spread over 0 .. MAX_DP_OUTPUT
        for k, p in model.named_parameters():
            if k.startswith("duration_predictor") and p.dim() > 1:
                p.mul_(3.0)
    G.kill_dropout(model)
    model.eval()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    z = np.load(os.path.join(G.ROOT, "tests", "golden", sd_from + ".npz"))
    stored = {k[3:] for k in z.files if k.startswith("sd.")}
    assert stored == set(sd0) and all(np.array_equal(z["sd." + k], G.to_np(v)) for k, v in sd0.items()), f"{sd_from}: another state dict"
    g = torch.Generator().manual_seed(seed + 1)
    xs = [torch.randn(T, cfg["idim"], generator=g) for T in Ts]
    pr = cfg.get("post_encoder_reduction_factor", 1)
    stochastic = cfg["duration_predictor_type"] == "stochastic"
    outs, d_outs, noises, margins = [], [], [], []
    real_randn = torch.randn
    for b, x in enumerate(xs):
        drawn = []

        def spy(*a, **k):
            t = real_randn(*a, **k)
            drawn.append(t.clone())
            return t

        torch.randn = spy
        try:
            torch.manual_seed(seed + 5 + b)
            with torch.no_grad():
                out = model.inference(x, dp_input=x)
        finally:
            torch.randn = real_randn
        assert len(out) == 2 and len(drawn) == (1 if stochastic else 0)
        noise = drawn[0] if drawn else None
        kind, pre, d64 = _pre_rounding(OM, sd0, cfg, x, noise)
        assert kind == ("ceil" if stochastic else "round")
        assert torch.equal(d64.double().reshape(-1), out[1].double().reshape(-1)), f"{name} row {b}: float64 oracle durations differ from the reference's"
        margins.append(_boundary_margin(kind, pre))
        outs.append(out[0])
        d_outs.append(out[1].reshape(-1))
        noises.append(noise)
    B, Tmax = len(Ts), max(Ts)
    txs = [int(d.numel()) for d in d_outs]
    olens = [int(o.shape[0]) for o in outs]
    Txmax, Lmax = max(txs), max(olens)
    print(f"  {name}: T {list(Ts)}  Tx {txs}  olens {olens}  boundary margins {['%.2e' % m for m in margins]}")
    print(f"  {name}: durations {[d.tolist() for d in d_outs]}")
    # the lengths are the test
    assert Ts.count(Tmax) == 1 and txs == [T // pr for T in Ts]
    assert pr == 1 or any(T % pr != 0 for T in Ts)
    assert any(t <= 3 for t in txs)
    cross = [L for L in olens if L > 64 and L % 64 != 0]
    assert cross, olens
    assert any(all(o != L for i, o in enumerate(olens) if i != olens.index(L)) for L in cross), olens
    assert all(L == int(d.clamp(max=MAX_DP_OUTPUT).sum()) * cfg.get("decoder_reduction_factor", 1) for L, d in zip(olens, d_outs))
    assert min(margins) >= MARGIN, f"{name}: a pre-rounding duration lies within {MARGIN:g} of a rounding boundary: pick another seed"
    arr = {}
    px = torch.zeros(B, Tmax, cfg["idim"])
    po = torch.zeros(B, Lmax, cfg["odim"])
    pd = torch.zeros(B, Txmax, dtype=d_outs[0].dtype)
    for b in range(B):
        px[b, : Ts[b]] = xs[b]
        po[b, : olens[b]] = outs[b]
        pd[b, : txs[b]] = d_outs[b]
    arr.update({"in.xs": G.to_np(px), "in.ilens": np.asarray(Ts, np.int64), "out.outs": G.to_np(po), "out.olens": np.asarray(olens, np.int64),
                "out.d_outs": G.to_np(pd)})
    if stochastic:
        pn = torch.zeros(B, 2, Txmax)
        for b in range(B):
            pn[b, :, : txs[b]] = noises[b][0]
        arr["in.sdp_noise"] = G.to_np(pn)
    G.save(name, dict(cfg, __model__="AASVC", __train__=False, __sd_from__=sd_from), arr)


def main():
    M, _, _ = G.import_reference()
    torch.set_num_threads(4)
    # (lengths: from T = [52, 37, 24, 9]; the stochastic predictor's durations average 2 per encoder frame, so the row that has to cross
    # a 64-frame tile of the output needs ~ 40 encoder frames input frames at the post-encoder reduction of 4; 166 % 4 != 0, so the BATCH drops trailing frames too)
    gen(M, "aasvc_tiny_inference_batch", G.AAS_TINY, [166, 37, 24, 9], seed=120, sd_from="aasvc_tiny_inference", sd_seed=109)
    gen(M, "aasvc_det_tiny_inference_batch", G.AAS_DET_TINY, [52, 37, 24, 3], seed=122, sd_from="aasvc_det_tiny_inference", sd_seed=111)


if __name__ == "__main__":
    main()
