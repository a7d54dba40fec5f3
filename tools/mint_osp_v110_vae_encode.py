#!/usr/bin/env python
"""Mint tests/golden/osp_v110_vae_encode_small.pt: the reference's OWN v1.1 CausalVAEModel (autoencoder_kl_open_sora_plan_v110.py) run on
the CPU in float64 at hidden_size 32, ENCODE side.  Runs only where the reference tree is present (tools/mint_osp_v110_vae.py
``reference_module``).

    python tools/mint_osp_v110_vae_encode.py            write the fixture
    python tools/mint_osp_v110_vae_encode.py --check    rebuild in memory and compare with the committed file (exit 1 on any difference)

The fixture holds data only: the seed of the weights (``synth_state_dict(seed, 32, encoder=<temporal downsamplers>)`` reproduces them bit
for bit), the construction kwargs, the encode-side state-dict names and shapes of the reference model, three 32 x 32 inputs and the
float64 moments of their posteriors (``CausalVAEModel.encode(x).mean`` / ``.logvar``) for two configurations of the temporal
downsamplers of levels 1 and 2, ``res`` = (TimeDownsampleRes2x, TimeDownsampleRes2x) and ``mix`` = (TimeDownsampleRes2x, TimeDownsample2x):
  x9  [1, 3, 9, 32, 32] -> [1, 4, 3, 4, 4]   (odd T: 9 -> 5 -> 3 frames)
  x8  [1, 3, 8, 32, 32] -> [1, 4, 2, 4, 4]   (even T twice: 8 -> 4 -> 2, the last frame of each level unread)
  x1  [1, 3, 1, 32, 32] -> [1, 4, 1, 4, 4]   (an image: every temporal tap reads the one frame)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PATH = os.path.join(ROOT, "tests", "golden", "osp_v110_vae_encode_small.pt")

SEED = 1109
CONFIGS = {"res": ("", "TimeDownsampleRes2x", "TimeDownsampleRes2x", ""), "mix": ("", "TimeDownsampleRes2x", "TimeDownsample2x", "")}
INPUTS = {"x9": 9, "x8": 8, "x1": 1}


def mint():
    import mint_osp_v110_vae as base
    from videosys_amd.vae_open_sora_plan_v110 import synth_state_dict

    m = base.reference_module()
    kwargs = dict(base.KWARGS, encoder_conv_in="CausalConv3d", encoder_conv_out="CausalConv3d", encoder_attention="AttnBlock3DFix",
                  encoder_resnet_blocks=("ResnetBlock3D",) * 4, encoder_spatial_downsample=("SpatialDownsample2x",) * 3 + ("",),
                  encoder_mid_resnet="ResnetBlock3D")
    g = torch.Generator().manual_seed(SEED + 1)
    fx = dict(seed=SEED, hidden_size=base.HIDDEN, kwargs=kwargs, configs=dict(CONFIGS))
    for name, T in INPUTS.items():                              # pixels in [-1, 1], bf16-representable
        fx[name] = torch.randn(1, 3, T, 32, 32, generator=g).clamp(-1, 1).to(torch.bfloat16).float()
    for cfg, temporal in CONFIGS.items():
        model = m.CausalVAEModel(**dict(kwargs, encoder_temporal_downsample=temporal))
        model.load_state_dict(synth_state_dict(SEED, base.HIDDEN, encoder=temporal), strict=True)
        model = model.to(torch.float64).eval()
        fx[f"state_dict_shapes_{cfg}"] = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if k.startswith(("encoder.", "quant_conv."))]
        with torch.no_grad():
            for name in INPUTS:
                post = model.encode(fx[name].double())
                fx[f"{name}_{cfg}_mean"], fx[f"{name}_{cfg}_logvar"] = post.mean.clone(), post.logvar.clone()
    assert tuple(fx["x9_res_mean"].shape) == (1, 4, 3, 4, 4) and tuple(fx["x8_mix_logvar"].shape) == (1, 4, 2, 4, 4)
    assert tuple(fx["x1_res_mean"].shape) == (1, 4, 1, 4, 4) and not torch.equal(fx["x9_res_mean"], fx["x9_mix_mean"])
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
