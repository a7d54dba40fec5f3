#!/usr/bin/env python
"""Mint tests/golden/cogvideox_vae_encode_small.pt: the reference's OWN AutoencoderKLCogVideoX (autoencoder_kl_cogvideox.py) run on the
CPU in float64 in its published configuration, ENCODE side.  Runs only where the reference tree is present
(oracle.ref_loader.build_reference_cogvideox_vae).

    python tools/mint_cogvideox_vae_encode.py            write the fixture
    python tools/mint_cogvideox_vae_encode.py --check    rebuild in memory and compare with the committed file (exit 1 on any difference)

The fixture holds data only: the seed of the weights (``synth_state_dict(seed, encoder=True)`` reproduces them bit for bit; the
encoder's tensors would be far more than a committed file may hold), the encode-side state-dict names and shapes of the reference
model, and three inputs of 16 x 16 pixels with the float64 moments of their posteriors — the body of ``encode`` (:1086-1088: ``encoder`` and
the optional ``quant_conv``) split into mean | logvar and the logvar clamped to [-30, 20], which is all the third-party
``DiagonalGaussianDistribution`` that ``encode`` wraps them in does to them (it is not part of the reference tree):
  x9  [1, 3, 9, 16, 16] -> [1, 16, 3, 2, 2]   (odd frame counts at both pooling layers: 9 -> 5 -> 3, a lone first frame each time)
  x8  [1, 3, 8, 16, 16] -> [1, 16, 2, 2, 2]   (even: 8 -> 4 -> 2)
  x1  [1, 3, 1, 16, 16] -> [1, 16, 1, 2, 2]   (an image: nothing to pool)
Every input runs on a FRESHLY built model: the reference's encode leaves its conv_cache behind, and a second call would read it.
Asserted here for every input: the bf16 floor (the restatement of tests/test_cogvideox_vae_encode_cpu.py run in bf16) lies below
0.05 x the rms of the reference, so the GPU test's bound of 1.5 floors means something."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
PATH = os.path.join(ROOT, "tests", "golden", "cogvideox_vae_encode_small.pt")

SEED = 2411
FRAMES = dict(x9=9, x8=8, x1=1)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def mint():
    import test_cogvideox_vae_encode_cpu as E
    from oracle import ref_loader
    from videosys_amd.vae_cogvideox import synth_state_dict

    sd = synth_state_dict(SEED, encoder=True)
    g = torch.Generator().manual_seed(SEED + 1)
    fx = dict(seed=SEED)
    for name, T in FRAMES.items():
        x = torch.randn(1, 3, T, 16, 16, generator=g).clamp(-1, 1).to(torch.bfloat16).float()      # pixels in [-1, 1], bf16-representable
        model = ref_loader.build_reference_cogvideox_vae(sd, dtype=torch.float64)                    # fresh: no conv_cache from another input
        fx.setdefault("state_dict_shapes", [(k, tuple(v.shape)) for k, v in model.state_dict().items() if k.startswith(("encoder.", "quant_conv."))])
        with torch.no_grad():                                                                        # encode :1086-1088
            h = model.encoder(x.double())
            h = h if model.quant_conv is None else model.quant_conv(h)
        mean, logvar = torch.chunk(h, 2, dim=1)                                                      # DiagonalGaussianDistribution
        fx[name], fx[name + "_mean"], fx[name + "_logvar"] = x, mean.clone(), logvar.clamp(-30.0, 20.0).clone()
        low = E.moments(x, sd, dtype=torch.bfloat16)
        for part, lo in zip(("mean", "logvar"), low):
            ref = fx[f"{name}_{part}"]
            floor = rms(lo - ref)
            print(f"{name} {part}: {tuple(ref.shape)} rms {rms(ref):.4f}, bf16 floor {floor:.4e} ({floor / rms(ref):.4f} of it)")
            assert floor < 0.05 * rms(ref), "the bf16 floor is no small fraction of the reference: choose another seed or input scale"
    return fx


def main():
    from mint_osp_vae import same

    fx = mint()
    if "--check" in sys.argv:
        if not same(fx, torch.load(PATH, weights_only=True)):
            print("stale:", os.path.relpath(PATH, ROOT))
            sys.exit(1)
        print("fixture matches")
        return
    torch.save(fx, PATH)
    print("wrote", os.path.relpath(PATH, ROOT), os.path.getsize(PATH), "bytes")
    assert os.path.getsize(PATH) <= 100 << 10, "the fixture is meant to stay well under 100 KB"


if __name__ == "__main__":
    main()
