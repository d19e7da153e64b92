"""Generate tests/golden/hifigan_msd.npz by IMPORTING the reference's MultiScaleDiscriminator (seq2seq_vc/urhythmic/vocoder.py) and its
three loss functions.

Runs only where the reference tree exists (never on the GPU box).  The weights come from the seeded numpy rule of tests/msd_ref.py
(30 M values are NOT stored); the fixture holds the key list and shapes of the reference's state_dict, the two inputs, the reference's
scores in train() mode from the seeded buffers (D(xr), then D(xg): two power iterations) and in eval() mode, for each feature its
mean |.| and a fixed sample of elements, dx plus a sample of every parameter gradient of the fixed scalar loss (feature_loss +
discriminator_loss + generator_loss), and samples of the updated u and v.

    python tools/gen_golden_msd.py
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("S2SVC_REFERENCE", "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import msd_ref as MR  # noqa: E402

T_GOLDEN = 331


def main():
    sys.path.insert(0, REF)
    from seq2seq_vc.urhythmic import vocoder as RV
    torch.manual_seed(0)
    msd = RV.MultiScaleDiscriminator()
    ref_sd = msd.state_dict()
    keys = list(ref_sd.keys())
    shapes = [tuple(v.shape) for v in ref_sd.values()]
    assert [(k, s) for k, s in zip(keys, shapes)] == MR.state_dict_shapes(), "the restatement's key list differs from the reference's"
    params = {k for k, _ in msd.named_parameters()}
    assert all((k not in params) == MR.is_buffer(k) for k in keys), "the parameter / buffer split differs from the reference's"
    assert len(keys) == 80 and sum(int(np.prod(s)) for s in shapes) == 29637357 and len(params) == 64
    sd = MR.seeded_state_dict(MR.SEED)
    xr, xg = MR.inputs(T_GOLDEN)
    msd.load_state_dict(sd)
    msd.eval()
    with torch.no_grad():
        eval_scores, _ = msd(xg)
    same = all(torch.equal(msd.state_dict()[k], sd[k]) for k in keys if MR.is_buffer(k))
    assert same, "eval() moved the buffers"
    msd.train()
    xr, xg = xr.requires_grad_(True), xg.requires_grad_(True)
    sr, fr = msd(xr)
    sg, fg = msd(xg)
    ok, msg = MR.alive(xg, fg)
    print("reference features:", msg)
    assert ok, "the seeded network is dead or exploding: " + msg
    loss = RV.feature_loss(fr, fg) + RV.discriminator_loss(sr, sg)[0] + RV.generator_loss(sg)[0]
    loss.backward()
    arrays = dict(keys=np.array(keys), shapes=np.array([",".join(map(str, s)) for s in shapes]), buffer=np.array([MR.is_buffer(k) for k in keys]),
                  T=np.int64(T_GOLDEN), seed=np.int64(MR.SEED), xr=xr.detach().numpy(), xg=xg.detach().numpy(), loss=loss.detach().numpy(),
                  dxr=xr.grad.numpy(), dxg=xg.grad.numpy())
    for i, (s, fl) in enumerate(zip(sg, fg)):
        arrays[f"score/{i}"] = s.detach().numpy()
        arrays[f"eval_score/{i}"] = eval_scores[i].numpy()
        for j, f in enumerate(fl):
            flat = f.detach().reshape(-1).numpy()
            arrays[f"feat_mean/{i}.{j}"] = np.float64(np.abs(flat.astype(np.float64)).mean())
            arrays[f"feat_shape/{i}.{j}"] = np.array(f.shape, dtype=np.int64)
            arrays[f"feat_sample/{i}.{j}"] = flat[MR.sample_positions(flat.size)]
    for k, prm in msd.named_parameters():
        flat = prm.grad.reshape(-1).numpy()
        arrays["grad_sample/" + k] = flat[MR.sample_positions(flat.size)]
        arrays["grad_absmax/" + k] = np.float64(np.abs(flat).max())
    after = msd.state_dict()
    for k in keys:
        if MR.is_buffer(k):
            flat = after[k].reshape(-1).numpy()
            arrays["buffer_sample/" + k] = flat[MR.sample_positions(flat.size)]
    out = MR.GOLDEN
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print(f"wrote {out} ({size / 1024:.0f} KiB, {len(arrays)} arrays); loss {float(loss):.6f}")
    assert size < 1024 * 1024, "fixture above the committed-file limit"
    # the restatement against what was just recorded
    r = MR.run(sd, xr.detach(), xg.detach(), torch.float64)
    worst = max(float((r["grads"][k] - p.grad.double()).abs().max()) / float(p.grad.abs().max()) for k, p in msd.named_parameters())
    print(f"restatement float64 vs reference fp32: loss {abs(float(r['loss']) - float(loss)):.2e}, "
          f"dxg {float((r['dxg'] - xg.grad.double()).abs().max()):.2e} of {float(xg.grad.abs().max()):.2e}, "
          f"worst parameter gradient {worst:.2e} of its largest magnitude")


if __name__ == "__main__":
    main()
