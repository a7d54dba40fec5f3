"""CPU: the encode side of the Open-Sora-Plan v1.2 CausalVAE — the fixture of the reference's own CausalVAEModel against the parameter
inventory and a torch restatement (``moments``: Encoder :509-626, Downsample :430-464, Spatial2xTime2x3DDownsample :418-427, encode
:859-870 of autoencoder_kl_open_sora_plan_v120.py on the blocks of tests/osp_vae_ref.py; run in bf16 it is the floor
tests/test_gpu_osp_vae_encode.py measures against); the configurations that are not built; the new entry point and its refusals."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import osp_vae_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOWN = ("Downsample", "Spatial2xTime2x3DDownsample", "Spatial2xTime2x3DDownsample", "")


def fixture():
    return torch.load(os.path.join(ROOT, "tests", "golden", "osp_vae_encode_small.pt"), weights_only=True)


def moments(x, sd, dtype=torch.float64):
    """x [B, 3, T, H, W] -> (mean, logvar) [B, 4, t, h, w] as float64, every layer computed in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    e = "encoder."
    h = R.causal_conv(x.to(dtype), sd, e + "conv_in", 1)
    for lvl, kind in enumerate(DOWN):
        for j in range(2):
            h = R.resnet(h, sd, f"{e}down.{lvl}.block.{j}")
        if kind == "Downsample":                                # per frame: pad right and bottom, 3 x 3, stride 2
            w, b = sd[f"{e}down.{lvl}.downsample.conv.weight"], sd[f"{e}down.{lvl}.downsample.conv.bias"]
            h = F.conv3d(F.pad(h, (0, 1, 0, 1)), w.unsqueeze(2), b, stride=(1, 2, 2))
        elif kind:                                              # the same padding, two copies of the first frame, stride 2 everywhere
            h = F.pad(h, (0, 1, 0, 1))
            h = torch.cat([h[:, :, :1], h[:, :, :1], h], dim=2)
            h = F.conv3d(h, sd[f"{e}down.{lvl}.downsample.conv.conv.weight"], sd[f"{e}down.{lvl}.downsample.conv.conv.bias"], stride=2)
    h = R.resnet(h, sd, e + "mid.block_1")
    h = R.attn(h, sd, e + "mid.attn_1")
    h = R.resnet(h, sd, e + "mid.block_2")
    h = R.causal_conv(R.silu(R.norm(h, sd, e + "norm_out")), sd, e + "conv_out", 1)
    mean, logvar = torch.chunk(R.causal_conv(h, sd, "quant_conv", 0).double(), 2, dim=1)
    return mean, logvar.clamp(-30.0, 20.0)


def test_fixture_inventory_and_restatement():
    from videosys_amd.vae_open_sora_plan import encoder_param_shapes, synth_state_dict

    fx = fixture()
    want = encoder_param_shapes(fx["hidden_size"])
    assert dict(fx["state_dict_shapes"]) == want and [k for k, _ in fx["state_dict_shapes"]] == list(want)
    assert want["encoder.down.0.downsample.conv.weight"] == (32, 32, 3, 3) and want["encoder.down.2.downsample.conv.conv.weight"] == (128, 128, 3, 3, 3)
    assert "encoder.down.3.downsample.conv.weight" not in want and want["quant_conv.conv.weight"] == (8, 8, 1, 1, 1)
    sd = synth_state_dict(fx["seed"], fx["hidden_size"], encoder=True)
    assert {k: tuple(v.shape) for k, v in sd.items() if k.startswith(("encoder.", "quant_conv."))} == want
    assert all(torch.equal(sd[k], v) for k, v in synth_state_dict(fx["seed"], fx["hidden_size"]).items()), "the decoder weights of a seed moved"
    for name, shape in (("x5", (1, 4, 2, 4, 4)), ("x1", (1, 4, 1, 4, 4))):
        mean, logvar = moments(fx[name], sd)
        assert tuple(mean.shape) == shape == tuple(fx[name + "_mean"].shape)
        assert float((mean - fx[name + "_mean"]).abs().max()) < 1e-9 and float((logvar - fx[name + "_logvar"]).abs().max()) < 1e-9


def test_unbuilt_encoder_configurations_raise_at_construction():
    from videosys_amd import vae_open_sora_plan as V

    for kw in (dict(encoder_spatial_downsample=("Downsample", "Downsample", "Downsample", "")), dict(double_z=False), dict(z_channels=8),
               dict(encoder_temporal_downsample=("", "", "TimeDownsampleRes2x", "")), dict(encoder_conv_in="Conv2d"),
               dict(encoder_resnet_blocks=("ResnetBlock2D", "ResnetBlock2D", "ResnetBlock3D", "ResnetBlock3D")), dict(encoder_attention="AttnBlock3D")):
        with pytest.raises(NotImplementedError):
            V.CausalVAEEncoder({}, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="HIP device"):      # the built configuration gets as far as the device check
        V.CausalVAEEncoder({}, device="cpu", **fixture()["kwargs"])


def test_entry_point_in_header_and_binding_and_its_refusals():
    from videosys_amd import _lib
    from videosys_amd._opcodes import ENTRY_POINTS

    assert "int vsys_conv_down2_bf16(" in open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    assert ENTRY_POINTS["vsys_conv_down2_bf16"][1] == "i" and "vsys_conv_down2_bf16" in _lib.SIGNATURES
    lib, P = _lib.load(), 0x10000       # an aligned address that is never dereferenced: every call below is refused before any launch
    grid = (ctypes.c_int64 * 6)(3, 8, 8, 0, 0, 192)
    call = lambda x=P, ldx=32, n=1, ldw=288, cin=32, cout=128, kt=1, g=grid: lib.vsys_conv_down2_bf16(None, x, ldx, g, n, P, ldw, None, P, 128, cin, cout, kt)
    assert call(kt=2) == -1 and call(cout=64) == -1 and call(cin=48, ldx=48) == -1 and call(ldx=16) == -1 and call(n=70000) == -1
    assert call(g=(ctypes.c_int64 * 6)(3, 1, 8, 0, 0, 24)) == -1 and call(g=(ctypes.c_int64 * 6)(3, 8, 8, 0, 0, 100)) == -1
    assert call(ldx=1 << 22, g=(ctypes.c_int64 * 6)(1, 64, 64, 0, 0, 4096)) == -1            # a tile's source span reaches 2 GiB
    assert call(x=P + 2) == -2 and call(ldx=36) == -2 and call(x=None) == -3
