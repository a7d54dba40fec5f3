"""CPU: the encode side of the CogVideoX VAE — the fixture of the reference's own AutoencoderKLCogVideoX in float64
(tests/golden/cogvideox_vae_encode_small.pt, tools/mint_cogvideox_vae_encode.py) against the parameter inventory and a plain-torch
restatement (``moments``: CogVideoXEncoder3D :597-728, CogVideoXResnetBlock3D :267-299 with zq None, CogVideoXDownsample3D
modules/downsampling.py:40-71, every causal convolution from a fresh state).  Run in bf16 the restatement is the floor
tests/test_gpu_cogvideox_vae_encode.py measures against."""
import os

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ("x9", "x8", "x1")


def fixture():
    return torch.load(os.path.join(ROOT, "tests", "golden", "cogvideox_vae_encode_small.pt"), weights_only=True)


def moments(x, sd, dtype=torch.float64):
    """x [B, 3, T, H, W] -> (mean, logvar) [B, 16, t, h, w] as float64, every layer computed in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith(("encoder.", "quant_conv."))}

    def cconv(h, key):                                           # causal 3 x 3 x 3: the first frame twice in front, zeros around
        h = F.pad(torch.cat([h[:, :, :1], h[:, :, :1], h], dim=2), (1, 1, 1, 1))
        return F.conv3d(h, sd[key + ".conv.weight"], sd[key + ".conv.bias"])

    def act(h, key):
        return F.silu(F.group_norm(h, 32, sd[key + ".weight"], sd[key + ".bias"], 1e-6))

    def resnet(h, p):
        y = cconv(act(h, p + ".norm1"), p + ".conv1")
        y = cconv(act(y, p + ".norm2"), p + ".conv2")
        if p + ".conv_shortcut.weight" in sd:
            h = F.conv3d(h, sd[p + ".conv_shortcut.weight"], sd[p + ".conv_shortcut.bias"])
        return y + h

    e = "encoder."
    h = cconv(x.to(dtype), e + "conv_in")
    for i in range(4):
        for j in range(3):
            h = resnet(h, f"{e}down_blocks.{i}.resnets.{j}")
        if i < 3:
            if i < 2:                                            # compress_time: pairwise mean, a lone first frame when T is odd
                odd = h.shape[2] % 2
                h = torch.cat([h[:, :, :odd], (h[:, :, odd::2] + h[:, :, odd + 1::2]) / 2], dim=2)
            k = f"{e}down_blocks.{i}.downsamplers.0.conv"
            h = F.conv3d(F.pad(h, (0, 1, 0, 1)), sd[k + ".weight"].unsqueeze(2), sd[k + ".bias"], stride=(1, 2, 2))
    for i in range(2):
        h = resnet(h, f"{e}mid_block.resnets.{i}")
    h = cconv(act(h, e + "norm_out"), e + "conv_out")
    if "quant_conv.weight" in sd:
        h = F.conv3d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])
    mean, logvar = torch.chunk(h.double(), 2, dim=1)
    return mean, logvar.clamp(-30.0, 20.0)


def test_fixture_inventory_and_restatement():
    from videosys_amd.vae_cogvideox import encoder_param_shapes, synth_state_dict

    fx = fixture()
    want = encoder_param_shapes()
    assert dict(fx["state_dict_shapes"]) == want and [k for k, _ in fx["state_dict_shapes"]] == list(want)
    assert want["encoder.down_blocks.1.downsamplers.0.conv.weight"] == (256, 256, 3, 3) and want["encoder.conv_out.conv.bias"] == (32,)
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in want
    sd = synth_state_dict(fx["seed"], encoder=True)
    assert {k: tuple(v.shape) for k, v in sd.items() if k.startswith("encoder.")} == want
    for name, frames in zip(INPUTS, (3, 2, 1)):
        mean, logvar = moments(fx[name], sd)
        assert tuple(mean.shape) == (1, 16, frames, 2, 2) == tuple(fx[name + "_mean"].shape)
        assert float((mean - fx[name + "_mean"]).abs().max()) < 1e-9 and float((logvar - fx[name + "_logvar"]).abs().max()) < 1e-9


def test_encoder_weights_leave_the_decoder_weights_of_a_seed_alone():
    from videosys_amd.vae_cogvideox import synth_state_dict

    both, dec = synth_state_dict(fixture()["seed"], encoder=True), synth_state_dict(fixture()["seed"])
    assert dec and all(k.startswith("decoder.") for k in dec) and all(torch.equal(both[k], v) for k, v in dec.items())
    assert [k for k in both if k.startswith("decoder.")] == list(dec)
