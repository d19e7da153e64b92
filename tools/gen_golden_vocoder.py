"""Generate tests/golden/hifigan_tiny.npz and hifigan_tiny_taps.npz by IMPORTING the reference's HiFi-GAN generator (seq2seq_vc/urhythmic/vocoder.py).

Runs only where the reference tree exists (never on the GPU box).  The fixture holds the tiny configuration, the full weight-normed
state_dict (seeded: tests/vocoder_ref.seed_state_dict), the input, the reference's waveform and -- through forward hooks -- the
outputs of conv_pre, of every ups[i], of every stage (after the MRF average) and of conv_post before tanh.

    python tools/gen_golden_vocoder.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("S2SVC_REFERENCE", "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vocoder_ref as VR  # noqa: E402


def reference_generator(cfg):
    sys.path.insert(0, REF)
    from seq2seq_vc.urhythmic.vocoder import HifiganGenerator
    return HifiganGenerator(**cfg)


def run_with_taps(gen, x):
    """Reference forward with hooks: the stage outputs are the inputs of the next ups[i] (before its leaky_relu) / of the last
    leaky_relu, i.e. the output of the last ResBlock sum divided by num_kernels -- recomputed here from the ResBlock outputs."""
    taps, blocks, hooks = {}, {}, []
    hooks.append(gen.conv_pre.register_forward_hook(lambda m, i, o: taps.__setitem__("conv_pre", o.detach().clone())))
    hooks.append(gen.conv_post.register_forward_hook(lambda m, i, o: taps.__setitem__("conv_post", o.detach().clone())))
    for i, up in enumerate(gen.ups):
        hooks.append(up.register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(f"ups.{i}", o.detach().clone())))
    for n, rb in enumerate(gen.resblocks):
        hooks.append(rb.register_forward_hook(lambda m, a, o, n=n: blocks.__setitem__(n, o.detach().clone())))
    with torch.no_grad():
        y = gen(x)
    for h in hooks:
        h.remove()
    nk = gen.num_kernels
    for i in range(gen.num_upsamples):
        # the hooks see each block's own output; z_sum accumulates IN PLACE into block 0's tensor, which is why they were cloned
        z = blocks[i * nk]
        for j in range(1, nk):
            z = z + blocks[i * nk + j]
        taps[f"stage.{i}"] = z / nk
    return y, taps


def main():
    cfg = dict(VR.TINY_CFG)
    torch.manual_seed(0)
    gen = reference_generator(cfg).eval()
    sd = VR.seed_state_dict(gen.state_dict(), seed=5)
    gen.load_state_dict(sd)
    x = torch.randn(2, 80, 37, generator=torch.Generator().manual_seed(1))
    y, taps = run_with_taps(gen, x)
    ok, msg = VR.alive(y, taps, cfg)
    print("reference output:", msg)
    assert ok, "the seeded generator is dead or saturated: " + msg
    nparam = sum(p.numel() for p in gen.parameters())
    y64 = VR.generator_forward({k: v.double() for k, v in sd.items()}, cfg, x.double())
    print(f"{nparam} parameters; reference fp32 vs restatement float64: {float((y.double() - y64).abs().max()):.2e}")
    # two files: the weights are random numbers and do not compress, so one file would pass the 1 MiB limit of a committed file
    cfg_arr = np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)
    main_arrays = {"sd/" + k: v.numpy() for k, v in gen.state_dict().items()}
    main_arrays.update(keys=np.array(list(gen.state_dict().keys())), x=x.numpy(), y=y.numpy(), __cfg__=cfg_arr)
    tap_arrays = {"tap/" + k: v.numpy() for k, v in taps.items()}
    for name, arrays in (("hifigan_tiny", main_arrays), ("hifigan_tiny_taps", tap_arrays)):
        out = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(out, **arrays)
        size = os.path.getsize(out)
        print(f"wrote {out} ({size / 1024:.0f} KiB, {len(arrays)} arrays)")
        assert size < 1024 * 1024, "fixture above the committed-file limit"

if __name__ == "__main__":
    main()
