"""Generate tests/golden/hifigan_mpd.npz by IMPORTING the reference's MultiPeriodDiscriminator (seq2seq_vc/urhythmic/vocoder.py) and its
three loss functions.

Runs only where the reference tree exists (never on the GPU box).  The weights come from the seeded numpy rule of tests/disc_ref.py
(41 M values are NOT stored); the fixture holds the key list and shapes of the reference's state_dict, the two inputs, the reference's
scores, for each feature its mean |.| and a fixed sample of elements, and dx plus a sample of every parameter gradient of the fixed
scalar loss (feature_loss + discriminator_loss + generator_loss).

    python tools/gen_golden_disc.py
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

import disc_ref as DR  # noqa: E402

T_GOLDEN = 331


def main():
    sys.path.insert(0, REF)
    from seq2seq_vc.urhythmic import vocoder as RV
    torch.manual_seed(0)
    mpd = RV.MultiPeriodDiscriminator()
    ref_sd = mpd.state_dict()
    keys = list(ref_sd.keys())
    shapes = [tuple(v.shape) for v in ref_sd.values()]
    assert [(k, s) for k, s in zip(keys, shapes)] == DR.state_dict_shapes(), "the restatement's key list differs from the reference's"
    sd = DR.seeded_state_dict(DR.SEED)
    mpd.load_state_dict(sd)
    xr, xg = DR.inputs(T_GOLDEN)
    xr, xg = xr.requires_grad_(True), xg.requires_grad_(True)
    sr, fr = mpd(xr)
    sg, fg = mpd(xg)
    ok, msg = DR.alive(xg, fg)
    print("reference features:", msg)
    assert ok, "the seeded network is dead or exploding: " + msg
    loss = RV.feature_loss(fr, fg) + RV.discriminator_loss(sr, sg)[0] + RV.generator_loss(sg)[0]
    loss.backward()
    arrays = dict(keys=np.array(keys), shapes=np.array([",".join(map(str, s)) for s in shapes]), T=np.int64(T_GOLDEN), seed=np.int64(DR.SEED),
                  xr=xr.detach().numpy(), xg=xg.detach().numpy(), loss=loss.detach().numpy(), dxr=xr.grad.numpy(), dxg=xg.grad.numpy())
    for i, (s, fl) in enumerate(zip(sg, fg)):
        arrays[f"score/{i}"] = s.detach().numpy()
        for j, f in enumerate(fl):
            flat = f.detach().reshape(-1).numpy()
            arrays[f"feat_mean/{i}.{j}"] = np.float64(np.abs(flat.astype(np.float64)).mean())
            arrays[f"feat_shape/{i}.{j}"] = np.array(f.shape, dtype=np.int64)
            arrays[f"feat_sample/{i}.{j}"] = flat[DR.sample_positions(flat.size)]
    for k, prm in mpd.named_parameters():
        flat = prm.grad.reshape(-1).numpy()
        arrays["grad_sample/" + k] = flat[DR.sample_positions(flat.size)]
        arrays["grad_absmax/" + k] = np.float64(np.abs(flat).max())
    out = DR.GOLDEN
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print(f"wrote {out} ({size / 1024:.0f} KiB, {len(arrays)} arrays); loss {float(loss):.6f}")
    assert size < 1024 * 1024, "fixture above the committed-file limit"
    # the restatement against what was just recorded
    r = DR.run(sd, xr.detach(), xg.detach(), torch.float64)
    print(f"restatement float64 vs reference fp32: loss {abs(float(r['loss']) - float(loss)):.2e}, "
          f"dxg {float((r['dxg'] - xg.grad.double()).abs().max()):.2e} of {float(xg.grad.abs().max()):.2e}")


if __name__ == "__main__":
    main()
