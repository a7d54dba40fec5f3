"""SD3 VAE decode for the Vchitect-2.0 pipeline (reference videosys/pipelines/vchitect/pipeline_vchitect.py:980-985): diffusers'
``AutoencoderKL`` at the Stable Diffusion 3 config — 16 latent channels, block_out_channels (128, 256, 512, 512), layers_per_block 2,
scaling_factor 1.5305, shift_factor 0.0609, NO quant convs — decode side only.

The decoder between its two ends is the 2-D decoder of vae_open_sora.py, reused unchanged (mid block with the 512-wide attention,
four up blocks, GroupNorm + SiLU, conv_out on the implicit-GEMM convolution).  The two ends are their own kernels (csrc/vae_sd3.hip):

  * ``vsys_vae_first_im2col_nc``: fp32 latents [F, 16, h, w] -> ``latents / scaling_factor + shift_factor`` with the reference's bf16
    roundings (:980 runs on bf16 latents) -> im2col rows of conv_in (16 -> 512, 3 x 3), which then is a plain GEMM over 160 columns;
  * ``vsys_pixels_to_u8``: conv_out rows -> uint8 [F, 8h, 8w, 3], what ``VaeImageProcessor.postprocess(image, "pil")`` (:984) computes:
    ``(x / 2 + 0.5).clamp(0, 1)`` on the bf16 tensor, then ``(float32 * 255).round()`` as uint8.

The reference decodes one frame per ``vae.decode`` call (:982-985); GroupNorm and the attention are per frame, so ``frames_per_launch``
frames in one pass give the same values.  There is no CPU path."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch

from . import ops, vchitect_ops as vops
from .ops import VaeGrid
from .vae_open_sora import OpenSoraVAE, _Conv, _Norm, _Res, _conv_w, _synth, _vec

LATENT_CHANNELS = 16
BLOCK_OUT_CHANNELS = (128, 256, 512, 512)
SCALING_FACTOR, SHIFT_FACTOR = 1.5305, 0.0609
_KCOLS = 160          # 9 taps x 16 channels = 144 -> the next multiple of the GEMM's 32-column K step


class AutoencoderKLSD3Decoder(OpenSoraVAE):
    """Decode side of diffusers ``AutoencoderKL`` at the SD3 config, state-dict keys ``decoder.*`` (diffusers' names)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", scaling_factor: float = SCALING_FACTOR,
                 shift_factor: float = SHIFT_FACTOR, frames_per_launch: int = 8):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("videosys_amd.AutoencoderKLSD3Decoder needs a HIP device (no CPU path)")
        quant = sorted(k for k in state_dict if k.startswith(("post_quant_conv.", "quant_conv.")))
        if quant:
            raise ValueError(f"the SD3 VAE has no quant convs (use_quant_conv / use_post_quant_conv are False), but the state dict holds "
                             f"{quant}: this is not an SD3 AutoencoderKL checkpoint (vae_open_sora.AutoencoderKLDecoder reads the SD / SDXL one)")
        w_in = state_dict["decoder.conv_in.weight"]
        if tuple(w_in.shape[1:]) != (LATENT_CHANNELS, 3, 3) or w_in.shape[0] != BLOCK_OUT_CHANNELS[-1]:
            raise ValueError(f"decoder.conv_in.weight {tuple(w_in.shape)}: expected ({BLOCK_OUT_CHANNELS[-1]}, {LATENT_CHANNELS}, 3, 3)")
        self.device = dev
        self.frames_per_launch = frames_per_launch
        self.config = SimpleNamespace(latent_channels=LATENT_CHANNELS, block_out_channels=BLOCK_OUT_CHANNELS, layers_per_block=2,
                                      scaling_factor=scaling_factor, shift_factor=shift_factor, use_quant_conv=False,
                                      use_post_quant_conv=False)
        self._padded = {}
        self._init_decoder(state_dict, dev)

    def _init_decoder(self, sd, dev):
        """OpenSoraVAE._init_spatial without the post_quant_conv and with the 16-channel conv_in (K = 144 -> 160)."""
        d = "decoder."
        self.s_conv_in_w = _conv_w(sd[d + "conv_in.weight"].to(dev), None, _KCOLS)
        self.s_conv_in_b = _vec(sd[d + "conv_in.bias"].to(dev))
        self.s_mid = [_Res(sd, f"{d}mid_block.resnets.{i}", dev, False) for i in range(2)]
        a = self._attn_weights(sd, d + "mid_block.attentions.0.", dev)
        self.a_norm, self.a_wq, self.a_bq, self.a_wk, self.a_bk = a.a_norm, a.a_wq, a.a_bq, a.a_wk, a.a_bk
        self.a_wv, self.a_wo, self.a_bo = a.a_wv, a.a_wo, a.a_bo
        self.s_up = []
        for i in range(4):
            res = [_Res(sd, f"{d}up_blocks.{i}.resnets.{j}", dev, False) for j in range(3)]
            upk = f"{d}up_blocks.{i}.upsamplers.0.conv"
            self.s_up.append((res, _Conv(sd, upk, dev) if (upk + ".weight") in sd else None))
        self.s_norm = _Norm(sd, d + "conv_norm_out", dev, 1e-6)
        self.s_out = _Conv(sd, d + "conv_out", dev, n_pad=128)

    def _decode_rows(self, z: torch.Tensor, scaling: float, shift: float):
        """z fp32 [m, 16, h, w] -> (conv_out rows [rows, 128] whose first 3 columns are the pixel, their grid).  ``scaling`` / ``shift``:
        the pipeline's `latents / scaling_factor + shift_factor` (:980), or 1 / 0 when the caller hands over decoder inputs."""
        m, _, H, W = z.shape
        a = vops.vae_first_im2col_nc(z, _KCOLS, scaling, shift)
        g = VaeGrid(m, 1, H, W, 0, 0)
        x = ops.gemm128(a, self.s_conv_in_w, self.s_conv_in_b)
        x, g = self._resblock(x, g, self.s_mid[0])
        x, g = self._attention(x, g)
        x, g = self._resblock(x, g, self.s_mid[1])
        for res, up in self.s_up:
            for r in res:
                x, g = self._resblock(x, g, r)
            if up is not None:
                gp = VaeGrid(m, 1, 2 * g.H, 2 * g.W, 1, 0)
                xp = self._padded_buf(gp, up.cin)
                ops.regrid(x, g, xp, gp, up.cin, up=1)
                x = ops.conv(xp, gp, up.w, up.b, up.cin, 1, 3)
                g = gp.conv_out()
        h, gh = self._norm_act(x, g, self.s_norm, 128, 0)
        return ops.conv(h, gh, self.s_out.w, self.s_out.b, 128, 1, 3), gh.conv_out()

    def _check(self, z):
        if not z.is_cuda:
            raise RuntimeError("AutoencoderKLSD3Decoder needs a HIP device tensor (no CPU path)")
        if z.dim() != 4 or z.shape[1] != LATENT_CHANNELS:
            raise ValueError(f"expected latents [F, {LATENT_CHANNELS}, h, w], got {tuple(z.shape)}")

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = False):
        """AutoencoderKL.decode: z [F, 16, h, w] (what the pipeline hands over at :983: already `/ scaling_factor + shift_factor`) ->
        (sample [F, 3, 8h, 8w] bf16,); the input is rounded to bf16 as the reference's bf16 VAE sees it."""
        self._check(z)
        Fr, _, H, W = z.shape
        zf = z.to(torch.float32).contiguous()
        vid = torch.empty(3, Fr, 8 * H, 8 * W, dtype=torch.bfloat16, device=self.device)
        for f in range(0, Fr, self.frames_per_launch):
            y, g = self._decode_rows(zf[f:f + self.frames_per_launch], 1.0, 0.0)
            ops.extract_planar(y, g, 3, 0, vid, f)
        sample = vid.permute(1, 0, 2, 3)
        return SimpleNamespace(sample=sample) if return_dict else (sample,)

    @torch.no_grad()
    def decode_u8(self, latents: torch.Tensor) -> torch.Tensor:
        """pipeline_vchitect.py:980-985 for output_type "pil": the sampler's latents [1, F, 16, h, w] -> uint8 frames [F, 8h, 8w, 3] on
        the device (one PIL image per frame is ``Image.fromarray`` of a row of it)."""
        if latents.dim() != 5 or latents.shape[0] != 1:
            raise ValueError(f"expected latents [1, F, {LATENT_CHANNELS}, h, w], got {tuple(latents.shape)}")
        z = latents[0]
        self._check(z)
        Fr, _, H, W = z.shape
        zf = z.to(torch.float32).contiguous()
        out = torch.empty(Fr, 8 * H, 8 * W, 3, dtype=torch.uint8, device=self.device)
        c = self.config
        for f in range(0, Fr, self.frames_per_launch):
            y, g = self._decode_rows(zf[f:f + self.frames_per_launch], c.scaling_factor, c.shift_factor)
            vops.pixels_to_u8(y, g, out, f)
        return out

    __call__ = decode_u8


def decoder_param_shapes() -> Dict[str, tuple]:
    """Names and shapes of the decode-side parameters of diffusers' AutoencoderKL at the SD3 config."""
    p: Dict[str, tuple] = {}

    def norm(name, c):
        p[name + ".weight"] = (c,)
        p[name + ".bias"] = (c,)

    def conv2(name, ci, co, k):
        p[name + ".weight"] = (co, ci, k, k)
        p[name + ".bias"] = (co,)

    def res2(name, ci, co):
        norm(name + ".norm1", ci); conv2(name + ".conv1", ci, co, 3)
        norm(name + ".norm2", co); conv2(name + ".conv2", co, co, 3)
        if ci != co:
            conv2(name + ".conv_shortcut", ci, co, 1)

    d = "decoder."
    conv2(d + "conv_in", LATENT_CHANNELS, 512, 3)
    res2(d + "mid_block.resnets.0", 512, 512)
    a = d + "mid_block.attentions.0."
    norm(a + "group_norm", 512)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        p[a + n + ".weight"] = (512, 512)
        p[a + n + ".bias"] = (512,)
    res2(d + "mid_block.resnets.1", 512, 512)
    prev = 512
    for i, co in enumerate(reversed(BLOCK_OUT_CHANNELS)):
        for j in range(3):
            res2(f"{d}up_blocks.{i}.resnets.{j}", prev, co)
            prev = co
        if i < 3:
            conv2(f"{d}up_blocks.{i}.upsamplers.0.conv", co, co, 3)
    norm(d + "conv_norm_out", 128)
    conv2(d + "conv_out", 128, 3, 3)
    return p


def synth_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic random decoder weights with diffusers' names (bf16-representable fp32, the distributions of
    vae_open_sora.synth_state_dict): no pretrained SD3 VAE is available offline."""
    return _synth(decoder_param_shapes(), torch.Generator().manual_seed(seed))
