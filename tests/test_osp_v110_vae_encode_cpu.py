"""CPU: the encode side of the Open-Sora-Plan v1.1 CausalVAE — the fixture of the reference's own v1.1 CausalVAEModel
(tests/golden/osp_v110_vae_encode_small.pt, tools/mint_osp_v110_vae_encode.py) against the parameter inventory and a torch restatement
(``moments``: Encoder :134-249, SpatialDownsample2x :1487-1507, TimeDownsample2x :1533-1542, TimeDownsampleRes2x :1557-1575, encode :470-480
of autoencoder_kl_open_sora_plan_v110.py on the blocks of tests/osp_vae_ref.py; run in bf16 it is the floor
tests/test_gpu_osp_v110_vae_encode.py measures against); the configurations that are not built; the new entry point and its refusals."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import osp_vae_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = {"x9": (1, 4, 3, 4, 4), "x8": (1, 4, 2, 4, 4), "x1": (1, 4, 1, 4, 4)}


@functools.lru_cache(maxsize=None)
def fixture():
    return torch.load(os.path.join(ROOT, "tests", "golden", "osp_v110_vae_encode_small.pt"), weights_only=True)


@functools.lru_cache(maxsize=None)
def weights(cfg):
    from videosys_amd.vae_open_sora_plan_v110 import synth_state_dict

    return synth_state_dict(fixture()["seed"], fixture()["hidden_size"], encoder=fixture()["configs"][cfg])


def time_down(h, sd, name, kind):
    h = torch.cat([h[:, :, :1], h[:, :, :1], h], dim=2)                   # two copies of the first frame
    To, up = (h.shape[2] - 3) // 2 + 1, (h.dtype if h.dtype == torch.float64 else torch.float32)
    # AvgPool3d((3, 1, 1), stride (2, 1, 1)) written out (torch has no bf16 avg_pool3d on the CPU): the sum in the accumulation type, one rounding
    pool = ((h[:, :, 0:2 * To - 1:2].to(up) + h[:, :, 1:2 * To:2].to(up) + h[:, :, 2:2 * To + 1:2].to(up)) / 3).to(h.dtype)
    if kind == "TimeDownsample2x":
        return pool
    alpha = torch.sigmoid(sd[name + ".mix_factor"])
    return alpha * pool + (1 - alpha) * F.conv3d(h, sd[name + ".conv.weight"], sd[name + ".conv.bias"], stride=(2, 1, 1), padding=(0, 1, 1))


def moments(x, sd, temporal, dtype=torch.float64):
    """x [B, 3, T, H, W] -> (mean, logvar) [B, 4, t, h, w] as float64, every layer computed in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    e = "encoder."
    h = R.causal_conv(x.to(dtype), sd, e + "conv_in", 1)
    for lvl in range(4):
        for j in range(2):
            h = R.resnet(h, sd, f"{e}down.{lvl}.block.{j}")
        if lvl < 3:                                             # per frame: pad right and bottom, 3 x 3, stride 2
            h = F.conv3d(F.pad(h, (0, 1, 0, 1)), sd[f"{e}down.{lvl}.downsample.conv.conv.weight"], sd[f"{e}down.{lvl}.downsample.conv.conv.bias"],
                         stride=(1, 2, 2))
        if temporal[lvl]:
            h = time_down(h, sd, f"{e}down.{lvl}.time_downsample", temporal[lvl])
    h = R.resnet(h, sd, e + "mid.block_1")
    h = R.attn(h, sd, e + "mid.attn_1")
    h = R.resnet(h, sd, e + "mid.block_2")
    h = R.causal_conv(R.silu(R.norm(h, sd, e + "norm_out")), sd, e + "conv_out", 1)
    mean, logvar = torch.chunk(R.causal_conv(h, sd, "quant_conv", 0).double(), 2, dim=1)
    return mean, logvar.clamp(-30.0, 20.0)


@pytest.mark.parametrize("cfg", ["res", "mix"])
def test_fixture_inventory_and_restatement(cfg):
    from videosys_amd.vae_open_sora_plan_v110 import encoder_param_shapes, synth_state_dict

    fx, temporal = fixture(), fixture()["configs"][cfg]
    want = encoder_param_shapes(32, temporal)
    shapes = fx[f"state_dict_shapes_{cfg}"]
    assert dict(shapes) == want and [k for k, _ in shapes] == list(want)
    assert want["encoder.down.0.downsample.conv.conv.weight"] == (32, 32, 1, 3, 3) and want["encoder.down.1.time_downsample.conv.weight"] == (64, 64, 3, 3, 3)
    assert want["encoder.down.1.time_downsample.mix_factor"] == (1,) and "encoder.down.0.time_downsample.mix_factor" not in want
    assert ("encoder.down.2.time_downsample.conv.bias" in want) == (cfg == "res") and want["quant_conv.conv.weight"] == (8, 8, 1, 1, 1)
    sd = weights(cfg)
    assert {k: tuple(v.shape) for k, v in sd.items() if k.startswith(("encoder.", "quant_conv."))} == want
    assert all(torch.equal(sd[k], v) for k, v in synth_state_dict(fx["seed"], 32).items()), "the decoder weights of a seed moved"
    for name, shape in INPUTS.items():
        mean, logvar = moments(fx[name], sd, temporal)
        assert tuple(mean.shape) == shape == tuple(fx[f"{name}_{cfg}_mean"].shape)
        assert float((mean - fx[f"{name}_{cfg}_mean"]).abs().max()) < 1e-9 and float((logvar - fx[f"{name}_{cfg}_logvar"]).abs().max()) < 1e-9


def test_unbuilt_encoder_configurations_raise_at_construction():
    from videosys_amd import vae_open_sora_plan_v110 as V

    for kw in (dict(encoder_temporal_downsample=("", "TimeDownsampleResAdv2x", "TimeDownsampleResAdv2x", "")),
               dict(encoder_temporal_downsample=("", "", "TimeDownsampleRes2x", "")), dict(encoder_spatial_downsample=("Downsample",) * 3 + ("",)),
               dict(attn_resolutions=[16]), dict(encoder_conv_in="Conv2d"), dict(encoder_attention="AttnBlock3D"), dict(double_z=False)):
        with pytest.raises(NotImplementedError):
            V.CausalVAEEncoder({}, device="cpu", **kw)
    V._check_config(dict(encoder_attention="whatever", encoder_temporal_downsample=("bogus",)))     # decode only: any encoder_* passes
    with pytest.raises(RuntimeError, match="HIP device"):      # the built configurations get as far as the device check
        V.CausalVAEEncoder({}, device="cpu", **dict(fixture()["kwargs"], encoder_temporal_downsample=fixture()["configs"]["mix"]))
    assert V.CausalVAEDecoder.ENCODER is V.CausalVAEEncoder


def test_entry_point_in_header_and_binding_and_its_refusals():
    from videosys_amd import _lib
    from videosys_amd._opcodes import ENTRY_POINTS, OPCODES

    header = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    assert "int vsys_conv_time_down2_bf16(void* stream, const void* x," in header and "autoencoder_kl_open_sora_plan_v110.py:1557-1575" in header
    assert ENTRY_POINTS["vsys_conv_time_down2_bf16"] == ("pplplplppllf", "i") and "vsys_conv_time_down2_bf16" in _lib.SIGNATURES
    assert "vsys_conv_time_down2_bf16" not in OPCODES
    lib, P = _lib.load(), 0x10000       # an aligned address that is never dereferenced: every call below is refused before any launch
    grid = (ctypes.c_int64 * 6)(3, 8, 8, 0, 0, 192)
    third = 1.0 / 3.0

    def call(x=P, ldx=128, n=1, w=P, ldw=27 * 128, C=128, a3=0.25, g=grid, ldo=128):
        return lib.vsys_conv_time_down2_bf16(None, x, ldx, g, n, w, ldw, None, P, ldo, C, a3)

    assert call(C=64, ldx=64) == -1 and call(C=12, w=None) == -1 and call(ldx=64) == -1 and call(n=70000) == -1 and call(ldw=128) == -1
    assert call(g=(ctypes.c_int64 * 6)(3, 1, 8, 0, 0, 24)) == -1 and call(g=(ctypes.c_int64 * 6)(0, 8, 8, 0, 0, 192)) == -1
    assert call(g=(ctypes.c_int64 * 6)(3, 8, 8, 0, 0, 100)) == -1
    assert call(ldx=1 << 22, g=(ctypes.c_int64 * 6)(1, 64, 64, 0, 0, 4096)) == -1            # a tile's source span reaches 2 GiB
    assert call(x=P + 2) == -2 and call(ldx=132) == -2 and call(ldo=132) == -2 and call(w=P + 8) == -2
    assert call(a3=-0.01) == -3 and call(a3=0.34) == -3 and call(a3=float("nan")) == -3 and call(x=None) == -3
    assert call(n=0, a3=third) == 0 and call(n=0, w=None, C=8, ldx=8, ldo=8) == 0       # accepted: nothing to launch
