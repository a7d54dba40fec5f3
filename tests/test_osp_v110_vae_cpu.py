"""CPU tests of the Open-Sora-Plan v1.1 CausalVAE decode (no GPU):

  * tests/osp_v110_vae_ref.py (the torch restatement of the v1.1 decoder, tiling included) against the float64 outputs of the reference's
    own CausalVAEModel (tests/golden/osp_v110_vae_small*.pt, tools/mint_osp_v110_vae.py) to 1e-9 — the bound tests/test_osp_pipeline_cpu.py
    holds the v1.2 restatement to — on all five cases: untiled, tiled, T = 1, T = 2 with TimeUpsampleRes2x, and TimeUpsample2x;
  * state-dict names and shapes against the fixture's for both temporal upsamplers, and the two different alphas of the synthetic weights;
  * every unsupported configuration raises; the v1.2 decoder's inventory and weights are what they were."""
import functools
import os

import pytest
import torch

import osp_v110_vae_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PLAIN = ("", "", "TimeUpsample2x", "TimeUpsample2x")


@functools.lru_cache(maxsize=None)
def fixture():
    fx = dict(torch.load(os.path.join(GOLDEN, "osp_v110_vae_small.pt"), weights_only=True))
    fx["a"] = torch.load(os.path.join(GOLDEN, "osp_v110_vae_small_a.pt"), weights_only=True)["a"]
    fx["b"] = torch.load(os.path.join(GOLDEN, "osp_v110_vae_small_b.pt"), weights_only=True)["b"]
    return fx


@functools.lru_cache(maxsize=None)
def weights(plain=False):
    from videosys_amd.vae_open_sora_plan_v110 import synth_state_dict

    fx = fixture()
    return synth_state_dict(fx["seed_e"], fx["hidden_size"], PLAIN) if plain else synth_state_dict(fx["seed"], fx["hidden_size"])


def case(name):
    """(latent, tiling or None, the TimeUpsample2x weights?) of a fixture case."""
    fx = fixture()
    z = fx["z"]
    return {"a": (z, None, False), "b": (z, fx["tiling"], False), "c": (z[:, :, :1], None, False), "d": (z[:, :, :2], None, False),
            "e": (fx["ze"], None, True)}[name]


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_restatement_equals_the_reference_class(name):
    fx = fixture()
    zz, tiling, plain = case(name)
    out = R.wrapper_decode(zz, weights(plain), tiling)
    ref = fx[name]
    assert out.dtype == torch.float64 and tuple(out.shape) == tuple(ref.shape) == (1, 4 * (zz.shape[2] - 1) + 1, 3, 8 * zz.shape[3], 8 * zz.shape[4])
    err = float((out - ref).abs().max())
    print(f"case {name}: max |restatement - reference class| = {err:.3e}")
    assert err <= 1e-9
    if name == "b":      # two temporal chunks, 2 x 3 spatial tiles, edge tiles smaller than the interior ones
        t = fx["tiling"]
        assert R.t_chunks(3, t["tile_latent_min_size_t"]) == [[0, 2], [1, 3]]
        step = int(t["tile_latent_min_size"] * (1 - t["tile_overlap_factor"]))
        assert (len(range(0, 6, step)), len(range(0, 8, step))) == (2, 3) and 6 - step < t["tile_latent_min_size"]
        assert float((fx["a"] - fx["b"]).abs().max()) > 1e-3        # tiling changes the result


def test_state_dict_names_and_shapes():
    from videosys_amd import vae_open_sora_plan as V120
    from videosys_amd.vae_open_sora_plan_v110 import decoder_param_shapes

    fx = fixture()
    want = decoder_param_shapes(32)
    assert dict(fx["state_dict_shapes"]) == want and set(weights()) == set(want)
    assert dict(fx["state_dict_shapes_e"]) == decoder_param_shapes(32, PLAIN) and set(weights(True)) == set(decoder_param_shapes(32, PLAIN))
    for lvl, c in ((1, 64), (2, 128), (3, 128)):
        assert want[f"decoder.up.{lvl}.upsample.conv.conv.weight"] == (c, c, 1, 3, 3)
    for lvl in (2, 3):
        assert want[f"decoder.up.{lvl}.time_upsample.mix_factor"] == (1,)
        assert want[f"decoder.up.{lvl}.time_upsample.conv.conv.weight"] == (128, 128, 3, 3, 3)
        assert want[f"decoder.up.{lvl}.time_upsample.conv.conv.bias"] == (128,)
    assert not any("time_upsample" in k for k in decoder_param_shapes(32, PLAIN)) and "decoder.up.1.time_upsample.mix_factor" not in want
    sd = weights()
    alphas = [float(torch.sigmoid(sd[f"decoder.up.{lvl}.time_upsample.mix_factor"].double())) for lvl in (2, 3)]
    assert alphas == pytest.approx(fx["alphas"], rel=1e-12) and abs(alphas[0] - alphas[1]) > 0.1 and all(0.25 < a < 0.96 for a in alphas)
    assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())
    # the v1.2 inventory (and with it the draw order of its synthetic weights) is what it was
    v120 = V120.decoder_param_shapes(32)
    assert not any("time_upsample" in k for k in v120) and v120["decoder.up.3.upsample.conv.conv.weight"] == (128, 128, 3, 3, 3)
    old = dict(torch.load(os.path.join(GOLDEN, "osp_vae_small.pt"), weights_only=True))
    assert dict(old["state_dict_shapes"]) == v120


def test_unsupported_configurations_raise():
    from videosys_amd import vae_open_sora_plan_v110 as V

    for kw in (dict(decoder_attention="AttnBlock3D"), dict(decoder_temporal_upsample=("", "", "", "")),
               dict(decoder_temporal_upsample=("", "", "", "TimeUpsampleRes2x")), dict(decoder_temporal_upsample=("", "TimeUpsample2x") * 2),
               dict(decoder_temporal_upsample=("", "", "TimeUpsampleResAdv2x", "TimeUpsampleResAdv2x")),
               dict(hidden_size_mult=(1, 2, 4)), dict(z_channels=8), dict(attn_resolutions=[16]), dict(bogus=1),
               dict(decoder_conv_in="Conv2d"), dict(decoder_resnet_blocks=("ResnetBlock2D",) * 4), dict(num_res_blocks=3),
               dict(decoder_spatial_upsample=("", "SpatialUpsample2x", "Spatial2xTime2x3DUpsample", "Spatial2xTime2x3DUpsample"))):
        with pytest.raises(NotImplementedError):
            V._check_config(kw)
    V._check_config(dict(hidden_size=32, decoder_attention="AttnBlock3DFix", attn_resolutions=[], encoder_attention="whatever",
                         decoder_temporal_upsample=["", "", "TimeUpsample2x", "TimeUpsampleRes2x"]))
    with pytest.raises(RuntimeError, match="HIP device"):
        V.CausalVAEDecoder(weights(), device="cpu")
    with pytest.raises(NotImplementedError, match="use_ema"):
        V.CausalVAEModelWrapper("synthetic:1", use_ema=True)
    assert V.CausalVAEDecoder.TILE_DEFAULTS == dict(tile_sample_min_size=256, tile_sample_min_size_t=65, tile_latent_min_size_t=17,
                                                    tile_overlap_factor=0.25)                       # :420-426
