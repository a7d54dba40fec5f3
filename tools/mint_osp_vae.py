#!/usr/bin/env python
"""Mint tests/golden/osp_vae_small*.pt: the reference's OWN CausalVAEModel (autoencoder_kl_open_sora_plan_v120.py) run on the CPU in
float64 at hidden_size 32, decode side, untiled and tiled.  Runs only where the reference tree is present
(oracle.ref_loader.REFERENCE_ROOT); the fixture holds data only — the seed and the construction kwargs, not the weights — and
tests/test_osp_pipeline_cpu.py pins tests/osp_vae_ref.py and the HIP decoder's state-dict names to it without the reference tree.

    python tools/mint_osp_vae.py            write the fixture
    python tools/mint_osp_vae.py --check    rebuild in memory and compare with the committed files (exit 1 on any difference)

Four cases of ``CausalVAEModelWrapper.decode`` ([B, T_out, 3, 8H, 8W], float64):
  a  latent [1, 4, 3, 6, 8], untiled -> [1, 9, 3, 48, 64]
  b  the same latent, tiled (TILING below): two temporal chunks, 2 x 3 spatial tiles with smaller edge tiles
  c  the first latent frame alone (T = 1) -> one frame
  d  the first two latent frames (T = 2) -> five frames
The outputs are 1.8 MB of float64, more than one committed file may hold, so the fixture is three files: osp_vae_small.pt (seed,
kwargs, latent, state-dict names and shapes, cases c and d), osp_vae_small_a.pt and osp_vae_small_b.pt.

The reference class needs three names beyond oracle/diffusers_stub.py; they are added here, in this process only:
diffusers.ConfigMixin / diffusers.ModelMixin at the top level of the stub package, and torchvision.transforms.Lambda as a
pass-through callable (the file builds its ``ae_norm`` table at import)."""
import importlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = {"": "osp_vae_small.pt", "a": "osp_vae_small_a.pt", "b": "osp_vae_small_b.pt"}

SEED = 1203
HIDDEN = 32
# the decoder side is the one configuration this build supports; the encoder side only has to be constructible from the classes the
# reference file still contains (its defaults name classes that are gone) — it is never run
KWARGS = dict(hidden_size=HIDDEN, z_channels=4, hidden_size_mult=(1, 2, 4, 4), attn_resolutions=(), dropout=0.0, resolution=256,
              double_z=True, embed_dim=4, num_res_blocks=2, q_conv="CausalConv3d",
              encoder_conv_in="CausalConv3d", encoder_conv_out="CausalConv3d", encoder_attention="AttnBlock3DFix",
              encoder_resnet_blocks=("ResnetBlock3D",) * 4,
              encoder_spatial_downsample=("Downsample", "Spatial2xTime2x3DDownsample", "Spatial2xTime2x3DDownsample", ""),
              encoder_temporal_downsample=("", "", "", ""), encoder_mid_resnet="ResnetBlock3D",
              decoder_conv_in="CausalConv3d", decoder_conv_out="CausalConv3d", decoder_attention="AttnBlock3DFix",
              decoder_resnet_blocks=("ResnetBlock3D",) * 4,
              decoder_spatial_upsample=("", "SpatialUpsample2x", "Spatial2xTime2x3DUpsample", "Spatial2xTime2x3DUpsample"),
              decoder_temporal_upsample=("", "", "", ""), decoder_mid_resnet="ResnetBlock3D", use_quant_layer=True)
TILING = dict(tile_latent_min_size=4, tile_sample_min_size=32, tile_latent_min_size_t=2, tile_sample_min_size_t=5,
              tile_overlap_factor=0.25)


def reference_module():
    from oracle import diffusers_stub as ds
    from oracle import ref_loader

    ref_loader.install_stubs()
    for k in [k for k in sys.modules if k == "diffusers" or k.startswith("diffusers.")]:
        del sys.modules[k]
    ds.install()
    sys.modules["diffusers"].__dict__.update(ConfigMixin=ds.ConfigMixin, ModelMixin=ds.ModelMixin)
    try:
        importlib.import_module("torchvision.transforms")
    except Exception:
        tv = types.ModuleType("torchvision")
        tv.__path__ = []
        sys.modules["torchvision"] = tv
        tv.transforms = sys.modules["torchvision.transforms"] = types.ModuleType("torchvision.transforms")
        tv.transforms.Lambda = lambda fn: fn
    try:
        importlib.import_module("huggingface_hub")
    except Exception:
        sys.modules["huggingface_hub"] = types.ModuleType("huggingface_hub")
        sys.modules["huggingface_hub"].hf_hub_download = None
    m = importlib.import_module("videosys.models.autoencoders.autoencoder_kl_open_sora_plan_v120")
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_loader.REFERENCE_ROOT) + os.sep), m.__file__
    return m


def mint():
    from videosys_amd.vae_open_sora_plan import synth_state_dict

    m = reference_module()
    sd = synth_state_dict(SEED, hidden_size=HIDDEN)
    model = m.CausalVAEModel(**KWARGS)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in missing), missing
    model = model.to(torch.float64).eval()
    wrap = m.CausalVAEModelWrapper.__new__(m.CausalVAEModelWrapper)      # (its __init__ only loads a checkpoint from disk)
    torch.nn.Module.__init__(wrap)
    wrap.vae = model
    g = torch.Generator().manual_seed(SEED + 1)
    # latents at the scale the sampler hands over: N(0, 1) * 0.18215, bf16-representable
    z = (torch.randn(1, 4, 3, 6, 8, generator=g) * 0.18215).to(torch.bfloat16).float()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if k.startswith(("decoder.", "post_quant_conv."))]
    main = dict(seed=SEED, hidden_size=HIDDEN, kwargs=dict(KWARGS), tiling=dict(TILING), z=z, state_dict_shapes=shapes)
    with torch.no_grad():
        a = wrap.decode(z.double()).clone()
        main["c"] = wrap.decode(z[:, :, :1].double()).clone()
        main["d"] = wrap.decode(z[:, :, :2].double()).clone()
        for k, v in TILING.items():
            setattr(model, k, v)
        model.enable_tiling()
        b = wrap.decode(z.double()).clone()
    assert tuple(a.shape) == (1, 9, 3, 48, 64) == tuple(b.shape) and main["c"].shape[1] == 1 and main["d"].shape[1] == 5
    assert not torch.equal(a, b), "tiling changed nothing"
    return {"": main, "a": dict(a=a), "b": dict(b=b)}


def same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    return a == b


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
