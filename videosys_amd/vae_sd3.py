"""SD3 VAE decode for the Vchitect-2.0 pipeline (reference videosys/pipelines/vchitect/pipeline_vchitect.py:980-985): diffusers'
``AutoencoderKL`` at the Stable Diffusion 3 config — 16 latent channels, block_out_channels (128, 256, 512, 512), layers_per_block 2,
scaling_factor 1.5305, shift_factor 0.0609, NO quant convs — decode side only.

The decoder between its two ends is the shared diffusers 2-D decoder body of vae_blocks.py (``Decoder2DWeights`` / ``_decoder2d``: mid
block with the 512-wide attention, four up blocks, GroupNorm + SiLU, conv_out on the implicit-GEMM convolution), the one the Open-Sora
and SVD decoders run as well.  The two ends are their own kernels (csrc/vae_sd3.hip):

  * ``vsys_vae_first_im2col_nc``: fp32 latents [F, 16, h, w] -> ``latents / scaling_factor + shift_factor`` with the reference's bf16
    roundings (:980 runs on bf16 latents) -> im2col rows of conv_in (16 -> 512, 3 x 3), which then is a plain GEMM over 160 columns;
  * ``vsys_pixels_to_u8``: conv_out rows -> uint8 [F, 8h, 8w, 3], what ``VaeImageProcessor.postprocess(image, "pil")`` (:984) computes:
    ``(x / 2 + 0.5).clamp(0, 1)`` on the bf16 tensor, then ``(float32 * 255).round()`` as uint8.

The reference decodes one frame per ``vae.decode`` call (:982-985); GroupNorm and the attention are per frame, so ``frames_per_launch``
frames in one pass give the same values — and, under a group of ranks (``decode_u8(latents, group=)`` / ``decode(z, group=)``), a
contiguous block of frames per rank and one all-gather do.  There is no CPU path."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch

from . import ops, vchitect_ops as vops
from .ops import VaeGrid
from .vae_blocks import Decoder2DWeights, VaeBlocks, _conv_w, _vec, diffusers_decoder_shapes, frame_shards, synth_weights

LATENT_CHANNELS = 16
BLOCK_OUT_CHANNELS = (128, 256, 512, 512)
SCALING_FACTOR, SHIFT_FACTOR = 1.5305, 0.0609
_KCOLS = 160          # 9 taps x 16 channels = 144 -> the next multiple of the GEMM's 32-column K step


class AutoencoderKLSD3Decoder(VaeBlocks):
    """Decode side of diffusers ``AutoencoderKL`` at the SD3 config, state-dict keys ``decoder.*`` (diffusers' names)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", scaling_factor: float = SCALING_FACTOR,
                 shift_factor: float = SHIFT_FACTOR, frames_per_launch: int = 8):
        super().__init__(device)
        quant = sorted(k for k in state_dict if k.startswith(("post_quant_conv.", "quant_conv.")))
        if quant:
            raise ValueError(f"the SD3 VAE has no quant convs (use_quant_conv / use_post_quant_conv are False), but the state dict holds "
                             f"{quant}: this is not an SD3 AutoencoderKL checkpoint (vae_open_sora.AutoencoderKLDecoder reads the SD / SDXL one)")
        w_in = state_dict["decoder.conv_in.weight"]
        if tuple(w_in.shape[1:]) != (LATENT_CHANNELS, 3, 3) or w_in.shape[0] != BLOCK_OUT_CHANNELS[-1]:
            raise ValueError(f"decoder.conv_in.weight {tuple(w_in.shape)}: expected ({BLOCK_OUT_CHANNELS[-1]}, {LATENT_CHANNELS}, 3, 3)")
        self.frames_per_launch = frames_per_launch
        self.config = SimpleNamespace(latent_channels=LATENT_CHANNELS, block_out_channels=BLOCK_OUT_CHANNELS, layers_per_block=2,
                                      scaling_factor=scaling_factor, shift_factor=shift_factor, use_quant_conv=False,
                                      use_post_quant_conv=False)
        self.conv_in_w = _conv_w(w_in.to(self.device), None, _KCOLS)       # 16-channel conv_in: K = 144 -> 160
        self.conv_in_b = _vec(state_dict["decoder.conv_in.bias"].to(self.device))
        self.dec = Decoder2DWeights(state_dict, "decoder.", self.device)

    def _decode_rows(self, z: torch.Tensor, scaling: float, shift: float):
        """z fp32 [m, 16, h, w] -> (conv_out rows [rows, 128] whose first 3 columns are the pixel, their grid).  ``scaling`` / ``shift``:
        the pipeline's `latents / scaling_factor + shift_factor` (:980), or 1 / 0 when the caller hands over decoder inputs."""
        m, _, H, W = z.shape
        a = vops.vae_first_im2col_nc(z, _KCOLS, scaling, shift)
        x = ops.gemm128(a, self.conv_in_w, self.conv_in_b)
        return self._decoder2d(x, VaeGrid(m, 1, H, W, 0, 0), self.dec)

    def _check(self, z):
        if not z.is_cuda:
            raise RuntimeError("AutoencoderKLSD3Decoder needs a HIP device tensor (no CPU path)")
        if z.dim() != 4 or z.shape[1] != LATENT_CHANNELS:
            raise ValueError(f"expected latents [F, {LATENT_CHANNELS}, h, w], got {tuple(z.shape)}")

    def _my_frames(self, Fr: int, group):
        """(f0, f1, frames per rank, ranks): this rank's contiguous frame range of ``frame_shards`` and the size of every rank's
        piece of the gather; the whole range, alone, without a group (or in a group of one)."""
        if group is None:
            return 0, Fr, Fr, 1
        from . import dsp

        P = dsp.group_size(group)
        if P == 1:
            return 0, Fr, Fr, 1
        f0, f1 = frame_shards(Fr, P)[dsp.group_rank(group)]
        return f0, f1, -(-Fr // P), P

    def _gather_frames(self, mine: torch.Tensor, P: int, group) -> torch.Tensor:
        """mine [per, ...] (this rank's piece, zero behind its frames) -> [P, per, ...] after ONE all-gather: the ranks' pieces
        in rank order, which is frame order."""
        from . import dsp

        flat = torch.empty((P * mine.shape[0],) + tuple(mine.shape[1:]), dtype=mine.dtype, device=self.device)
        dsp.all_gather_into_tensor(flat, mine, group)
        return flat.view((P,) + tuple(mine.shape))

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = False, group=None):
        """AutoencoderKL.decode: z [F, 16, h, w] (what the pipeline hands over at :983: already `/ scaling_factor + shift_factor`) ->
        (sample [F, 3, 8h, 8w] bf16,); the input is rounded to bf16 as the reference's bf16 VAE sees it.  ``group``: see decode_u8
        (the gathered pieces are planar bf16)."""
        self._check(z)
        Fr, _, H, W = z.shape
        zf = z.to(torch.float32).contiguous()
        f0, f1, per, P = self._my_frames(Fr, group)
        alloc = torch.zeros if P > 1 else torch.empty
        vid = alloc(3, per, 8 * H, 8 * W, dtype=torch.bfloat16, device=self.device)
        for f in range(f0, f1, self.frames_per_launch):
            y, g = self._decode_rows(zf[f:min(f + self.frames_per_launch, f1)], 1.0, 0.0)
            ops.extract_planar(y, g, 3, 0, vid, f - f0)
        if P > 1:                                    # [P, 3, per, 8h, 8w] -> [3, F, 8h, 8w]
            vid = self._gather_frames(vid, P, group).permute(1, 0, 2, 3, 4).reshape(3, P * per, 8 * H, 8 * W)[:, :Fr]
        sample = vid.permute(1, 0, 2, 3)
        return SimpleNamespace(sample=sample) if return_dict else (sample,)

    @torch.no_grad()
    def decode_u8(self, latents: torch.Tensor, group=None) -> torch.Tensor:
        """pipeline_vchitect.py:980-985 for output_type "pil": the sampler's latents [1, F, 16, h, w] -> uint8 frames [F, 8h, 8w, 3] on
        the device (one PIL image per frame is ``Image.fromarray`` of a row of it).  ``group`` (dsp.py group protocol; every rank
        holds the same latents): rank r decodes the frames of ``frame_shards(F, P)[r]`` into its ceil(F / P)-frame piece and ONE
        all-gather of the uint8 pieces gives every rank every frame — the reference decodes all of them on every rank; the 2-D decoder
        is per frame, so the bits are the ungrouped call's.  A rank without frames launches nothing and still takes part."""
        if latents.dim() != 5 or latents.shape[0] != 1:
            raise ValueError(f"expected latents [1, F, {LATENT_CHANNELS}, h, w], got {tuple(latents.shape)}")
        z = latents[0]
        self._check(z)
        Fr, _, H, W = z.shape
        zf = z.to(torch.float32).contiguous()
        f0, f1, per, P = self._my_frames(Fr, group)
        alloc = torch.zeros if P > 1 else torch.empty
        out = alloc(per, 8 * H, 8 * W, 3, dtype=torch.uint8, device=self.device)
        c = self.config
        for f in range(f0, f1, self.frames_per_launch):
            y, g = self._decode_rows(zf[f:min(f + self.frames_per_launch, f1)], c.scaling_factor, c.shift_factor)
            vops.pixels_to_u8(y, g, out, f - f0)
        if P > 1:
            out = self._gather_frames(out, P, group).view(P * per, 8 * H, 8 * W, 3)[:Fr]
        return out

    __call__ = decode_u8


def decoder_param_shapes() -> Dict[str, tuple]:
    """Names and shapes of the decode-side parameters of diffusers' AutoencoderKL at the SD3 config."""
    return diffusers_decoder_shapes("decoder.", LATENT_CHANNELS, BLOCK_OUT_CHANNELS)


def synth_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic random decoder weights with diffusers' names (vae_blocks.synth_weights: bf16-representable fp32, the distributions
    of vae_open_sora.synth_state_dict): no pretrained SD3 VAE is available offline."""
    return synth_weights(decoder_param_shapes(), torch.Generator().manual_seed(seed))
