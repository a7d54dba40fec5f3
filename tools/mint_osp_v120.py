#!/usr/bin/env python
"""Mint tests/golden/osp_v120_fwd_small.pt: the reference's OWN OpenSoraT2V class (open_sora_plan_v120_transformer_3d.py) run on the
CPU at a small geometry, in float64, float32 and bfloat16, without and with PAB.  Runs only where the reference tree is present
(oracle.ref_loader.REFERENCE_ROOT); the fixture it writes holds data only, and tests/test_osp_cpu.py pins tests/osp_ref.py and the
HIP model's state-dict names to it without the reference tree.

    python tools/mint_osp_v120.py            write the fixture
    python tools/mint_osp_v120.py --check    rebuild in memory and compare with the committed file (exit 1 on any difference)

The reference class needs a few third-party names beyond oracle/diffusers_stub.py; they are added here, in this process only:
  * a subclass of the stub Attention with the attributes AttnProcessor2_0 reads (spatial_norm = group_norm = norm_cross = None,
    residual_connection = False, rescale_output_factor = 1.0);
  * AdaLayerNormSingle: the reference's own class from latte_transformer_3d.py;
  * GatedSelfAttentionDense / SinusoidalPositionalEmbedding: placeholders that raise when constructed (never used here);
  * diffusers.utils.is_torch_version, diffusers.pipelines.pipeline_utils.DiffusionPipeline (an empty class);
  * a ``dtype`` property on OpenSoraT2V (diffusers' ModelMixin provides it)."""
import importlib
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "osp_v120_fwd_small.pt")

SEED = 1202
KWARGS = dict(num_attention_heads=2, attention_head_dim=96, in_channels=4, out_channels=4, num_layers=2, cross_attention_dim=192,
              attention_bias=True, sample_size=(8, 12), sample_size_t=3, patch_size=2, patch_size_t=1,
              activation_fn="gelu-approximate", norm_type="ada_norm_single", norm_elementwise_affine=False, norm_eps=1e-6,
              caption_channels=32, use_rope=True, interpolation_scale_h=1.0, interpolation_scale_w=1.0, interpolation_scale_t=1.0)
PAB = dict(spatial_broadcast=True, spatial_threshold=[100, 900], spatial_range=2, cross_broadcast=True, cross_threshold=[100, 900],
           cross_range=2)
# a second geometry with non-unit scales and two axes of EQUAL length (T = H/p = 4): the reference's table cache has no scale in its
# key, so the rows take the frames' table — the case pins the scales and that property of the class
SCALED = dict(sample_size_t=4, interpolation_scale_t=2.0, interpolation_scale_h=1.5, interpolation_scale_w=2.0)
T1, T2 = 500, 480          # the PAB pair: computed at T1 (counter 0), broadcast at T2 (counter 1, inside both windows)


def reference_class():
    from oracle import diffusers_stub as ds
    from oracle import ref_loader

    ref_loader.install_stubs()
    for k in [k for k in sys.modules if k == "diffusers" or k.startswith("diffusers.")]:
        del sys.modules[k]
    ds.install()
    latte = importlib.import_module("videosys.models.transformers.latte_transformer_3d")

    class Attn(ds.Attention):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.spatial_norm = self.group_norm = self.norm_cross = None
            self.residual_connection, self.rescale_output_factor = False, 1.0

    class Unused(nn.Module):
        def __init__(self, *a, **k):
            raise RuntimeError("placeholder: not used by the minted configuration")

    sys.modules["diffusers.models.attention"].__dict__.update(GatedSelfAttentionDense=Unused)
    sys.modules["diffusers.models.attention_processor"].__dict__.update(Attention=Attn)
    sys.modules["diffusers.models.embeddings"].__dict__.update(SinusoidalPositionalEmbedding=Unused)
    sys.modules["diffusers.models.normalization"].__dict__.update(AdaLayerNormSingle=latte.AdaLayerNormSingle)
    sys.modules["diffusers.utils"].__dict__.update(is_torch_version=lambda *a: True)
    ds._mod("diffusers.pipelines")
    ds._mod("diffusers.pipelines.pipeline_utils", DiffusionPipeline=type("DiffusionPipeline", (), {}))
    m = importlib.import_module("videosys.models.transformers.open_sora_plan_v120_transformer_3d")
    m.OpenSoraT2V.dtype = property(lambda s: next(s.parameters()).dtype)
    return m.OpenSoraT2V, importlib.import_module("videosys.core.pab.pab_mgr")


def build(cls, sd, dtype, **over):
    class SP:
        sp_size, cp_size, sp_group = 1, 1, None

    model = cls(attention_mode="math", **{**KWARGS, **over})
    model.load_state_dict(sd, strict=True)
    model.parallel_manager = SP()
    for _, mod in model.named_modules():
        if hasattr(mod, "parallel_manager"):
            mod.parallel_manager = SP()
    return model.eval().to(dtype)


def mint():
    from videosys_amd.open_sora_plan import synth_state_dict

    cls, pab_mgr = reference_class()
    sd = synth_state_dict(num_layers=KWARGS["num_layers"], num_heads=KWARGS["num_attention_heads"], caption_channels=KWARGS["caption_channels"],
                          in_channels=KWARGS["in_channels"], out_channels=KWARGS["out_channels"], patch_size=KWARGS["patch_size"], seed=SEED)
    g = torch.Generator().manual_seed(SEED + 1)
    bf = lambda t: t.to(torch.bfloat16).float()
    B, L = 2, 8
    x = bf(torch.randn(B, 4, 3, 8, 12, generator=g))
    x2 = bf(torch.randn(B, 4, 3, 8, 12, generator=g))
    enc = bf(torch.randn(B, 1, L, KWARGS["caption_channels"], generator=g))
    mask = torch.ones(B, 1, L)
    mask[1, 0, 5:] = 0
    video_mask = torch.ones(B, 3, 8, 12)
    x3 = bf(torch.randn(B, 4, 4, 8, 12, generator=g))
    out = dict(kwargs=dict(KWARGS), seed=SEED, pab=dict(PAB), pab_timesteps=(T1, T2), x=x, x2=x2, encoder_hidden_states=enc,
               encoder_attention_mask=mask, attention_mask=video_mask, scaled_kwargs={**KWARGS, **SCALED}, scaled_x=x3)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32"), (torch.bfloat16, "bf16")):
        model = build(cls, sd, dtype)
        if tag == "f64":
            out["state_dict_shapes"] = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        run = lambda lat, t: model(lat.to(dtype), timestep=torch.tensor([t, t]), encoder_hidden_states=enc.to(dtype),
                                   attention_mask=video_mask, encoder_attention_mask=mask, return_dict=False)[0]
        with torch.no_grad():
            pab_mgr.PAB_MANAGER = None
            out["ref_" + tag] = run(x, T1).clone()
            pab_mgr.set_pab_manager(pab_mgr.PABConfig(**PAB))
            pab_mgr.update_steps(2)
            first = run(x, T1)
            assert torch.equal(first, out["ref_" + tag]), "the computing PAB step differs from the PAB-free forward"
            out["pab_" + tag] = run(x2, T2).clone()
            pab_mgr.PAB_MANAGER = None
            if tag != "f32":
                scaled = build(cls, sd, dtype, **SCALED)       # a fresh model: empty table caches
                out["scaled_ref_" + tag] = scaled(x3.to(dtype), timestep=torch.tensor([T1, T1]), encoder_hidden_states=enc.to(dtype),
                                                  encoder_attention_mask=mask, return_dict=False)[0].clone()
    return out


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
        old = torch.load(FIXTURE, weights_only=True)
        if not same(fx, old):
            print("stale:", FIXTURE)
            sys.exit(1)
        print("fixture matches")
        return
    torch.save(fx, FIXTURE)
    print("wrote", os.path.relpath(FIXTURE, ROOT), os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
