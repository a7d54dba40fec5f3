#!/usr/bin/env python
"""Mint tests/golden/osp_v110_vae_small*.pt: the reference's OWN v1.1 CausalVAEModel (autoencoder_kl_open_sora_plan_v110.py) run on the CPU
in float64 at hidden_size 32, decode side.  Runs only where the reference tree is present (oracle.ref_loader.REFERENCE_ROOT); the
fixture holds data only — the seed and the construction kwargs, not the weights — and tests/test_osp_v110_vae_cpu.py pins
tests/osp_v110_vae_ref.py and the HIP decoder's state-dict names to it without the reference tree.

    python tools/mint_osp_v110_vae.py            write the fixture
    python tools/mint_osp_v110_vae.py --check    rebuild in memory and compare with the committed files (exit 1 on any difference)

Five cases of ``CausalVAEModelWrapper.decode`` ([B, T_out, 3, 8H, 8W], float64).  With TimeUpsampleRes2x at levels 2 and 3:
  a  latent [1, 4, 3, 6, 8], untiled -> [1, 9, 3, 48, 64]
  b  the same latent, tiled (TILING below, the v1.2 fixture's): two temporal chunks, 2 x 3 spatial tiles with smaller edge tiles
  c  the first latent frame alone (T = 1) -> one frame
  d  the first two latent frames (T = 2) -> five frames
With TimeUpsample2x at levels 2 and 3 (its own seeded weights, no mix_factor / conv):
  e  latent [1, 4, 2, 4, 4], untiled -> [1, 5, 3, 32, 32]
Three files, each below the 1 MiB a committed file may hold: osp_v110_vae_small.pt (seed, kwargs, latents, state-dict names and shapes,
the two alphas, cases c, d and e), osp_v110_vae_small_a.pt and osp_v110_vae_small_b.pt.

The reference class needs, beyond oracle/diffusers_stub.py and what tools/mint_osp_vae.py adds, ``diffusers.utils.logging`` with
``set_verbosity_error`` (the file calls it at import); it is added here, in this process only."""
import importlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = {"": "osp_v110_vae_small.pt", "a": "osp_v110_vae_small_a.pt", "b": "osp_v110_vae_small_b.pt"}

SEED = 1105        # (its two mix_factors give alphas 0.94 and 0.58: far apart, neither term of the mix vanishes)
HIDDEN = 32
RES = ("", "", "TimeUpsampleRes2x", "TimeUpsampleRes2x")
PLAIN = ("", "", "TimeUpsample2x", "TimeUpsample2x")
# the decoder side is the configuration this build supports; the encoder side is the reference's default and is never run
KWARGS = dict(hidden_size=HIDDEN, z_channels=4, hidden_size_mult=(1, 2, 4, 4), attn_resolutions=(), dropout=0.0, resolution=256,
              double_z=True, embed_dim=4, num_res_blocks=2, q_conv="CausalConv3d",
              decoder_conv_in="CausalConv3d", decoder_conv_out="CausalConv3d", decoder_attention="AttnBlock3DFix",
              decoder_resnet_blocks=("ResnetBlock3D",) * 4,
              decoder_spatial_upsample=("", "SpatialUpsample2x", "SpatialUpsample2x", "SpatialUpsample2x"),
              decoder_temporal_upsample=RES, decoder_mid_resnet="ResnetBlock3D")
from mint_osp_vae import TILING, same  # noqa: E402  (the v1.2 fixture's tiling; the fixture comparison)


def reference_module():
    import mint_osp_vae

    mint_osp_vae.reference_module()             # the stubs the v1.2 file needs; the v1.1 file needs one more name
    utils = sys.modules["diffusers.utils"]
    if not hasattr(utils, "logging"):
        utils.logging = types.SimpleNamespace(set_verbosity_error=lambda: None, get_logger=lambda *a, **k: None)
    from oracle import ref_loader

    m = importlib.import_module("videosys.models.autoencoders.autoencoder_kl_open_sora_plan_v110")
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_loader.REFERENCE_ROOT) + os.sep), m.__file__
    return m


def build(m, temporal, seed):
    from videosys_amd.vae_open_sora_plan_v110 import synth_state_dict

    sd = synth_state_dict(seed, hidden_size=HIDDEN, temporal=temporal)
    model = m.CausalVAEModel(**dict(KWARGS, decoder_temporal_upsample=temporal))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in missing), missing
    model = model.to(torch.float64).eval()
    wrap = m.CausalVAEModelWrapper.__new__(m.CausalVAEModelWrapper)      # (its __init__ only loads a checkpoint from disk)
    torch.nn.Module.__init__(wrap)
    wrap.vae = model
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if k.startswith(("decoder.", "post_quant_conv."))]
    return sd, model, wrap, shapes


def mint():
    m = reference_module()
    sd, model, wrap, shapes = build(m, RES, SEED)
    g = torch.Generator().manual_seed(SEED + 1)
    # latents at the scale the sampler hands over: N(0, 1) * 0.18215, bf16-representable
    z = (torch.randn(1, 4, 3, 6, 8, generator=g) * 0.18215).to(torch.bfloat16).float()
    ze = (torch.randn(1, 4, 2, 4, 4, generator=g) * 0.18215).to(torch.bfloat16).float()
    alphas = [float(torch.sigmoid(sd[f"decoder.up.{lvl}.time_upsample.mix_factor"].double())) for lvl in (2, 3)]
    main = dict(seed=SEED, hidden_size=HIDDEN, kwargs=dict(KWARGS), tiling=dict(TILING), z=z, ze=ze, state_dict_shapes=shapes, alphas=alphas)
    with torch.no_grad():
        a = wrap.decode(z.double()).clone()
        main["c"] = wrap.decode(z[:, :, :1].double()).clone()
        main["d"] = wrap.decode(z[:, :, :2].double()).clone()
        for k, v in TILING.items():
            setattr(model, k, v)
        model.enable_tiling()
        b = wrap.decode(z.double()).clone()
        _, _, wrap_e, shapes_e = build(m, PLAIN, SEED + 2)
        main["e"] = wrap_e.decode(ze.double()).clone()
    main["seed_e"], main["state_dict_shapes_e"] = SEED + 2, shapes_e
    assert tuple(a.shape) == (1, 9, 3, 48, 64) == tuple(b.shape) and main["c"].shape[1] == 1 and main["d"].shape[1] == 5
    assert tuple(main["e"].shape) == (1, 5, 3, 32, 32) and abs(alphas[0] - alphas[1]) > 0.01
    assert not torch.equal(a, b), "tiling changed nothing"
    return {"": main, "a": dict(a=a), "b": dict(b=b)}


def main():
    fx = mint()
    if "--check" in sys.argv:
        stale = [f for k, f in FILES.items() if not same(fx[k], torch.load(os.path.join(GOLDEN, f), weights_only=True))]
        if stale:
            print("stale:", stale)
            sys.exit(1)
        print("fixture matches")
        return
    for k, f in FILES.items():
        p = os.path.join(GOLDEN, f)
        torch.save(fx[k], p)
        print("wrote", os.path.relpath(p, ROOT), os.path.getsize(p), "bytes")
        assert os.path.getsize(p) <= 1 << 20, "a committed file may hold at most 1 MiB"


if __name__ == "__main__":
    main()
