#!/usr/bin/env python
"""Mint tests/golden/osp_v110_fwd_small.pt: the reference's OWN v1.1 LatteT2V class (open_sora_plan_v110_transformer_3d.py) run on the
CPU at a small geometry, in float64 and bfloat16.  Runs only where the reference tree is present (oracle.ref_loader.REFERENCE_ROOT);
the fixture it writes holds data only, and tests/test_osp_v110_cpu.py pins tests/osp_v110_ref.py and the HIP model's state-dict names to
it without the reference tree.

    python tools/mint_osp_v110.py            write the fixture
    python tools/mint_osp_v110.py --check    rebuild in memory and compare with the committed file (exit 1 on any difference)

The reference class needs a few third-party names beyond oracle/diffusers_stub.py; they are added here, in this process only:
  * placeholder classes for the processors open_sora_plan_v110_transformer_3d.py:24-40 imports from
    diffusers.models.attention_processor (they raise when constructed; the minted configuration uses the file's own AttnProcessor2_0);
  * diffusers.models.embeddings.SinusoidalPositionalEmbedding, diffusers.models.normalization.AdaLayerNorm / AdaLayerNormZero: the same;
  * diffusers.utils.is_xformers_available = lambda: False;
  * a ``dtype`` property on the class (diffusers' ModelMixin provides it);
  * a stand-in parallel_manager with sp_size = cp_size = 1 on the model and its blocks.

Cases (each in float64 and bfloat16; 2 heads x 72, 2 + 2 layers, sample_size (8, 8), patch 2, video_length 5, 32 caption channels, 6
text tokens with a mask that hides the tail of sample 1): use_rope on; use_rope off; a non-square INPUT of 8 x 12 on the (8, 8) model
(the recomputed position table, row and column positions of different ranges); a SCALED model, sample_size (128, 128) with a 128 x 8
input and interpolation_scale_1d = 2.0 (both scales 2, so the truncation of the scaled positions shows); encoder_attention_mask = None;
a three-step PAB sequence with spatial, temporal and cross broadcast and one MLP window.  sample_size stays square in every case: the
reference's construction-time table is a sqrt(n) x sqrt(n) grid (:397-399).  Beside the model cases: the reference's own
LinearScalingRoPE2D / 1D modules applied in bf16 (``rope_module``).  The bf16 outputs are what the restatement's bf16 run is held to,
bit for bit (same operations in the same order on the CPU).

The attn1.to_q / to_k weights of the synthetic state dict are scaled by QK_GAIN: at default-sized projections the logits are so flat
that the rotation moves the output by about one bf16 floor, and no model-level test could see a missing or wrongly paired rotation
(tests/test_osp_v110_cpu.py asserts the sensitivity at this gain)."""
import importlib
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "osp_v110_fwd_small.pt")

SEED = 1101
QK_GAIN = 3.0
KWARGS = dict(num_attention_heads=2, patch_size_t=1, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=2,
              cross_attention_dim=144, attention_bias=True, sample_size=(8, 8), patch_size=2, activation_fn="gelu-approximate",
              norm_type="ada_norm_single", norm_elementwise_affine=False, norm_eps=1e-6, caption_channels=32, video_length=5,
              use_rope=True, model_max_length=6, rope_scaling_type="linear", compress_kv_factor=1)
SCALED = dict(sample_size=(128, 128), interpolation_scale_1d=2.0, video_length=3)   # (three frames keep the file small: positions 0, 1, 2 -> 0, 0, 1)
PAB = dict(spatial_broadcast=True, spatial_threshold=[100, 900], spatial_range=2, temporal_broadcast=True, temporal_threshold=[100, 900],
           temporal_range=3, cross_broadcast=True, cross_threshold=[100, 900], cross_range=2, mlp_broadcast=True,
           mlp_spatial_broadcast_config={500: {"block": [0, 1], "skip_count": 2}}, mlp_temporal_broadcast_config={})
PAB_TIMESTEPS = (500, 480, 460)
T0 = 500
# The HIP model's GEMMs need hidden sizes that are multiples of 192 (N) and 64 (K): with 72-wide heads the smallest such model has 8
# heads (576).  The GPU tests therefore run the same cases, inputs and weights recipe at 8 heads against tests/osp_v110_ref.py; one
# case of the class at 8 heads pins the restatement there as well.
WIDE_HEADS = dict(num_attention_heads=8, cross_attention_dim=576)


def reference_class():
    from oracle import diffusers_stub as ds
    from oracle import ref_loader

    ref_loader.install_stubs()
    for k in [k for k in sys.modules if k == "diffusers" or k.startswith("diffusers.")]:
        del sys.modules[k]
    ds.install()

    class Unused(nn.Module):
        def __init__(self, *a, **k):
            raise RuntimeError("placeholder: not used by the minted configuration")

    ap = sys.modules["diffusers.models.attention_processor"].__dict__
    for name in ("AttnAddedKVProcessor", "AttnAddedKVProcessor2_0", "AttnProcessor", "CustomDiffusionAttnProcessor",
                 "CustomDiffusionAttnProcessor2_0", "CustomDiffusionXFormersAttnProcessor", "LoRAAttnAddedKVProcessor", "LoRAAttnProcessor",
                 "LoRAAttnProcessor2_0", "LoRAXFormersAttnProcessor", "SlicedAttnAddedKVProcessor", "SlicedAttnProcessor", "SpatialNorm",
                 "XFormersAttnAddedKVProcessor", "XFormersAttnProcessor"):
        ap.setdefault(name, type(name, (Unused,), {}))
    sys.modules["diffusers.models.embeddings"].__dict__.setdefault("SinusoidalPositionalEmbedding", Unused)
    for name in ("AdaLayerNorm", "AdaLayerNormZero"):
        sys.modules["diffusers.models.normalization"].__dict__.setdefault(name, type(name, (Unused,), {}))
    sys.modules["diffusers.utils"].__dict__.update(is_xformers_available=lambda: False)
    m = importlib.import_module("videosys.models.transformers.open_sora_plan_v110_transformer_3d")
    m.LatteT2V.dtype = property(lambda s: next(s.parameters()).dtype)
    return m.LatteT2V, importlib.import_module("videosys.core.pab.pab_mgr")


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
    from videosys_amd.open_sora_plan_v110 import synth_state_dict

    cls, pab_mgr = reference_class()
    sd = synth_state_dict(num_layers=KWARGS["num_layers"], num_heads=KWARGS["num_attention_heads"], caption_channels=KWARGS["caption_channels"],
                          in_channels=KWARGS["in_channels"], out_channels=KWARGS["out_channels"], patch_size=KWARGS["patch_size"], seed=SEED,
                          qk_gain=QK_GAIN)
    g = torch.Generator().manual_seed(SEED + 1)
    bf = lambda t: t.to(torch.bfloat16).float()
    B, L, T = 2, 6, KWARGS["video_length"]
    x = bf(torch.randn(B, 4, T, 8, 8, generator=g))
    xs = [bf(torch.randn(B, 4, T, 8, 8, generator=g)) for _ in PAB_TIMESTEPS]
    x_wide = bf(torch.randn(B, 4, T, 8, 12, generator=g))
    x_scaled = bf(torch.randn(B, 4, 3, 128, 8, generator=g))
    enc = bf(torch.randn(B, 1, L, KWARGS["caption_channels"], generator=g))
    mask = torch.ones(B, L)
    mask[1, 4:] = 0
    sd8 = synth_state_dict(num_layers=KWARGS["num_layers"], num_heads=WIDE_HEADS["num_attention_heads"], caption_channels=KWARGS["caption_channels"],
                           in_channels=KWARGS["in_channels"], out_channels=KWARGS["out_channels"], patch_size=KWARGS["patch_size"], seed=SEED,
                           qk_gain=QK_GAIN)
    out = dict(kwargs=dict(KWARGS), wide_heads=dict(WIDE_HEADS), scaled_kwargs={**KWARGS, **SCALED}, seed=SEED, qk_gain=QK_GAIN, pab=dict(PAB), pab_timesteps=PAB_TIMESTEPS,
               timestep=T0, x=x.bfloat16(), pab_x=[v.bfloat16() for v in xs], x_wide=x_wide.bfloat16(), x_scaled=x_scaled.bfloat16(),
               encoder_hidden_states=enc.bfloat16(), encoder_attention_mask=mask)          # (inputs are bf16 values: stored as such)
    for dtype, tag in ((torch.float64, "f64"), (torch.bfloat16, "bf16")):
        def run(model, lat, t, m=mask, **kw):
            return model(lat.to(dtype), timestep=torch.tensor([t, t]), encoder_hidden_states=enc.to(dtype), encoder_attention_mask=m,
                         return_dict=False, **kw)[0].clone()

        with torch.no_grad():
            pab_mgr.PAB_MANAGER = None
            model = build(cls, sd, dtype)
            if tag == "f64":
                out["state_dict_shapes"] = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
            out["rope_" + tag] = run(model, x, T0)
            out["wide_" + tag] = run(model, x_wide, T0)
            out["nomask_" + tag] = run(model, x, T0, m=None)
            out["norope_" + tag] = run(build(cls, sd, dtype, use_rope=False), x, T0)
            if tag == "f64":
                out["rope_heads8_f64"] = run(build(cls, sd8, dtype, **WIDE_HEADS), x, T0)
            out["scaled_" + tag] = run(build(cls, sd, dtype, **SCALED), x_scaled, T0)
            pab_mgr.set_pab_manager(pab_mgr.PABConfig(**PAB))
            pab_mgr.update_steps(len(PAB_TIMESTEPS))
            model = build(cls, sd, dtype)           # fresh counters
            ats = torch.tensor(PAB_TIMESTEPS)
            out["pab_" + tag] = [run(model, xs[i], t, all_timesteps=ats) for i, t in enumerate(PAB_TIMESTEPS)]
            pab_mgr.PAB_MANAGER = None
    # the reference's own rotation modules in bf16 on a 5 x 7 grid / 35 frames at scale 2: pins the cast of the angles to the compute dtype
    # BEFORE cos / sin and the truncation of the scaled positions, which no float64 run exercises
    mod = sys.modules[cls.__module__]
    tok = torch.randn(1, 1, 35, 72, generator=g).to(torch.bfloat16)
    pos2 = torch.cartesian_prod(torch.arange(5), torch.arange(7)).view(1, 35, 2)
    out["rope_module"] = dict(tokens=tok, grid=(5, 7), scale=2.0,
                              out_2d=mod.LinearScalingRoPE2D(scaling_factor=2.0)(tok, pos2).clone(),
                              out_1d=mod.LinearScalingRoPE1D(scaling_factor=2.0)(tok, torch.arange(35).view(1, 35)).clone())
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
