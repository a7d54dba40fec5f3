#!/usr/bin/env python
"""Mint tests/golden/osp_vae_encode_small.pt: the reference's OWN CausalVAEModel (autoencoder_kl_open_sora_plan_v120.py) run on the CPU
in float64 at hidden_size 32, ENCODE side.  Runs only where the reference tree is present (tools/mint_osp_vae.py ``reference_module``).

    python tools/mint_osp_vae_encode.py            write the fixture
    python tools/mint_osp_vae_encode.py --check    rebuild in memory and compare with the committed file (exit 1 on any difference)

The fixture holds data only: the seed of the weights (``synth_state_dict(seed, 32, encoder=True)``: the 6.3 M encoder parameters are
12 MB in bf16, more than a committed file may hold, and the seed reproduces them bit for bit, as in osp_vae_small.pt), the
construction kwargs, the encode-side state-dict names and shapes of the reference model, and two inputs with the float64 moments of
their posteriors (``CausalVAEModel.encode(x).mean`` / ``.logvar``):
  x5  [1, 3, 5, 32, 32] -> [1, 4, 2, 4, 4]   (frames 0 and 1..4: the replicated front of both causal downsamplers)
  x1  [1, 3, 1, 32, 32] -> [1, 4, 1, 4, 4]   (an image: every temporal tap reads the one frame)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PATH = os.path.join(ROOT, "tests", "golden", "osp_vae_encode_small.pt")

SEED = 1207


def mint():
    import mint_osp_vae as base
    from videosys_amd.vae_open_sora_plan import synth_state_dict

    m = base.reference_module()
    sd = synth_state_dict(SEED, hidden_size=base.HIDDEN, encoder=True)
    model = m.CausalVAEModel(**base.KWARGS)
    model.load_state_dict(sd, strict=True)
    model = model.to(torch.float64).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x5 = torch.randn(1, 3, 5, 32, 32, generator=g).clamp(-1, 1).to(torch.bfloat16).float()      # pixels in [-1, 1], bf16-representable
    x1 = torch.randn(1, 3, 1, 32, 32, generator=g).clamp(-1, 1).to(torch.bfloat16).float()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if k.startswith(("encoder.", "quant_conv."))]
    fx = dict(seed=SEED, hidden_size=base.HIDDEN, kwargs=dict(base.KWARGS), state_dict_shapes=shapes, x5=x5, x1=x1)
    with torch.no_grad():
        for name, x in (("x5", x5), ("x1", x1)):
            post = model.encode(x.double())
            fx[name + "_mean"], fx[name + "_logvar"] = post.mean.clone(), post.logvar.clone()
    assert tuple(fx["x5_mean"].shape) == (1, 4, 2, 4, 4) and tuple(fx["x1_logvar"].shape) == (1, 4, 1, 4, 4)
    return fx


def main():
    import mint_osp_vae as base

    fx = mint()
    if "--check" in sys.argv:
        if not base.same(fx, torch.load(PATH, weights_only=True)):
            print("stale:", os.path.relpath(PATH, ROOT))
            sys.exit(1)
        print("fixture matches")
        return
    torch.save(fx, PATH)
    print("wrote", os.path.relpath(PATH, ROOT), os.path.getsize(PATH), "bytes")
    assert os.path.getsize(PATH) <= 1 << 20, "a committed file may hold at most 1 MiB"


if __name__ == "__main__":
    main()
