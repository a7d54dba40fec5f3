"""Open-Sora-Plan v1.1 CausalVAE decode on MI355X: the decoder half of the v1.1 ``CausalVAEModel`` and ``CausalVAEModelWrapper.decode``
(reference videosys/models/autoencoders/autoencoder_kl_open_sora_plan_v110.py: Decoder :251-354, CausalVAEModel.decode / tiled_decode /
tiled_decode2d :482-491, :672-693, :735-771, the wrapper :800-826), under the reference's state-dict names.

It is the v1.2 decoder of vae_open_sora_plan.py — same residual blocks, mid-block attention, whole-sample GroupNorm, channel map for
hidden sizes 32 / 64, causal front frames, tiling and sharing of a tiled decode over ranks, all inherited — with other upsamplers:

  * every spatial upsampler is ``SpatialUpsample2x`` (:1510-1530): vsys_regrid(up=1) into the padded grid of its (1, 3, 3) conv;
  * levels 3 and 2 then run a temporal upsampler (:346-349), ``TimeUpsampleRes2x`` (:1578-1596) or ``TimeUpsample2x`` (:1545-1554):
    vsys_upsample_time2x copies frame 0 and interpolates frames 1.. by (2, 1, 1) among themselves.  For ``TimeUpsample2x`` that is all.
    For ``TimeUpsampleRes2x``, ``alpha x + (1 - alpha) conv(x)`` with alpha = sigmoid(mix_factor): the kernel writes x into the padded
    input grid of the causal 3 x 3 x 3 conv and bf16(alpha x) — from the same fp32 value — into a second buffer that the conv takes as its
    residual operand; the conv's weights and bias are scaled by (1 - alpha) in fp32 at load, before their one rounding to bf16.  (Folding
    alpha into the identity tap of the bf16 weights instead would swallow the low bits of the diagonal.)

The one configuration the reference file's decoder is asked for here is supported (``_check_config``): CausalConv3d in and out,
AttnBlock3DFix in the mid block, ResnetBlock3D everywhere, spatial upsamplers ("", S, S, S), temporal upsamplers ("", "", X, X) with X one
of the two classes above, no attention at the resolutions, multipliers (1, 2, 4, 4), 4 latent channels.  The tile attributes start at
the reference's (:420-426: 256 / 65 / 17 frames, overlap 0.25).  There is no CPU path."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import open_sora_plan_v110_ops as vops
from . import vae_open_sora_plan as v120
from .ops import VaeGrid
from .vae_blocks import synth_weights
from .vae_open_sora_plan import HIDDEN_SIZE_MULT, SCALE, Z_CHANNELS, _CConv, check_attention_keys  # noqa: F401

SPATIAL_UPSAMPLE = ("", "SpatialUpsample2x", "SpatialUpsample2x", "SpatialUpsample2x")
TIME_UPSAMPLERS = ("TimeUpsampleRes2x", "TimeUpsample2x")
TEMPORAL_UPSAMPLE = ("", "", "TimeUpsampleRes2x", "TimeUpsampleRes2x")      # what "synthetic:<seed>" builds


def _temporal(kw: dict) -> tuple:
    return tuple(kw.get("decoder_temporal_upsample", TEMPORAL_UPSAMPLE))


def _check_config(kw: dict) -> None:
    want = dict(z_channels=Z_CHANNELS, hidden_size_mult=HIDDEN_SIZE_MULT, attn_resolutions=(), decoder_conv_in="CausalConv3d",
                decoder_conv_out="CausalConv3d", decoder_attention="AttnBlock3DFix", decoder_resnet_blocks=("ResnetBlock3D",) * 4,
                decoder_spatial_upsample=SPATIAL_UPSAMPLE, decoder_mid_resnet="ResnetBlock3D", num_res_blocks=2, embed_dim=4,
                q_conv="CausalConv3d", dropout=0.0)
    for k, v in kw.items():
        got = tuple(v) if isinstance(v, (list, tuple)) else v
        if k == "decoder_temporal_upsample":
            if len(got) != 4 or got[:2] != ("", "") or got[2] not in TIME_UPSAMPLERS or got[3] not in TIME_UPSAMPLERS:
                raise NotImplementedError(f"CausalVAEModel({k}={v!r}): this build decodes ('', '', X, X) with X one of {TIME_UPSAMPLERS}")
        elif k in want:
            if got != want[k]:
                raise NotImplementedError(f"CausalVAEModel({k}={v!r}): this build decodes the Open-Sora-Plan v1.1 configuration only "
                                          f"({k}={want[k]!r})")
        elif not (k.startswith("encoder_") or k in ("hidden_size", "resolution", "double_z", "lr", "loss_type", "loss_params")):
            raise NotImplementedError(f"CausalVAEModel: unknown argument {k!r}")


class _TimeUp:
    """One temporal upsampler: ``conv`` (scaled by 1 - alpha) and ``alpha`` for TimeUpsampleRes2x, ``conv`` None for TimeUpsample2x."""

    def __init__(self, sd, key, dev, cm, kind):
        self.kind, self.conv, self.alpha = kind, None, 0.0
        if kind == "TimeUpsampleRes2x":
            self.alpha = 1.0 / (1.0 + math.exp(-float(sd[key + ".mix_factor"].reshape(-1)[0])))      # sigmoid on the host
            keep = torch.tensor(1.0 - self.alpha, dtype=torch.float32)
            scaled = {key + ".conv.conv." + n: sd[key + ".conv.conv." + n].float() * keep for n in ("weight", "bias")}   # fp32, then ONE rounding
            self.conv = _CConv(scaled, key + ".conv", dev, cm, cm)


class CausalVAEDecoder(v120.CausalVAEDecoder):
    """Decode side of the reference's v1.1 ``CausalVAEModel``: ``decode(z)``, z [B, 4, T, H, W] -> [B, 3, 4(T-1)+1, 8H, 8W] bf16, with the
    reference's tiling attributes.  ``decoder_temporal_upsample`` chooses the temporal upsamplers (default: TimeUpsampleRes2x twice)."""

    SPATIAL = SPATIAL_UPSAMPLE
    TILE_DEFAULTS = dict(tile_sample_min_size=256, tile_sample_min_size_t=65, tile_latent_min_size_t=17, tile_overlap_factor=0.25)
    _check = staticmethod(_check_config)

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", hidden_size: Optional[int] = None, **config):
        _check_config(config)
        self.temporal = _temporal(config)
        self.time_ups: Dict[int, _TimeUp] = {}
        super().__init__(state_dict, device=device, hidden_size=hidden_size, **config)

    def _param_shapes(self, hidden_size: int) -> Dict[str, tuple]:
        return decoder_param_shapes(hidden_size, self.temporal)

    def _level_extra(self, sd, lvl, cm, dev) -> None:
        if self.temporal[lvl]:
            self.time_ups[lvl] = _TimeUp(sd, f"decoder.up.{lvl}.time_upsample", dev, cm, self.temporal[lvl])

    def _after_level(self, x, g: VaeGrid, lvl: int):
        """``up[lvl].time_upsample`` (:348-349) on the rows of the spatial upsampler's conv (pad 1, no front frames)."""
        tu = self.time_ups.get(lvl)
        if tu is None:
            return x, g
        C = x.shape[1]
        T2 = 1 if g.T == 1 else 2 * g.T - 1
        if tu.conv is None:                                                          # TimeUpsample2x :1549-1554: no conv follows
            gd = VaeGrid(1, T2, g.H, g.W, 1, 0)
            y = torch.empty(gd.rows, C, dtype=torch.bfloat16, device=self.device)
            vops.upsample_time2x(x, g, y, gd, C)
            return y, gd
        gu = VaeGrid(1, T2, g.H, g.W, 1, 2)                                          # TimeUpsampleRes2x :1590-1596
        xu = self._padded_buf(gu, C)
        gr = gu.conv_out()
        ax = torch.empty(gr.rows, C, dtype=torch.bfloat16, device=self.device)       # alpha x, the conv's residual operand
        vops.upsample_time2x(x, g, xu, gu, C, ax, gr, tu.alpha)
        self._front(xu, gu)
        return self._conv(xu, gu, tu.conv, res=ax), gr


CausalVAEModel = CausalVAEDecoder        # the reference's class name; decode side only


class CausalVAEModelWrapper(v120.CausalVAEModelWrapper):
    """``CausalVAEModelWrapper`` :800-826, decode side; as vae_open_sora_plan.CausalVAEModelWrapper with the v1.1 decoder.
    ``model_path``: a state dict, ``"synthetic:<seed>"`` or a LOCAL directory with the checkpoint (utils.read_component)."""

    def __init__(self, model_path, subfolder=None, cache_dir=None, use_ema=False, device="cuda", hidden_size: Optional[int] = None, **kwargs):
        if use_ema:
            raise NotImplementedError("CausalVAEModelWrapper(use_ema=True): the EMA copy is a training artefact; load its weights as the state dict")
        if isinstance(model_path, dict):
            sd = model_path
        elif isinstance(model_path, str) and model_path.startswith("synthetic:"):
            _check_config(kwargs)
            sd = synth_state_dict(int(model_path.split(":", 1)[1]), hidden_size or 128, _temporal(kwargs))
        else:
            from .utils import read_component

            sd = read_component(model_path if subfolder is None else f"{model_path}/{subfolder}")[1]
            if sd is None:
                raise FileNotFoundError(f"CausalVAEModelWrapper({model_path!r}): not a local checkpoint directory, a state dict or 'synthetic:<seed>'")
        self.vae = CausalVAEDecoder(sd, device=device, hidden_size=hidden_size, **kwargs)


# ---------------------------------------------------------------------------------------------------- synthetic weights
def decoder_param_shapes(hidden_size: int = 128, temporal=TEMPORAL_UPSAMPLE) -> Dict[str, tuple]:
    """Names and shapes of the decode-side parameters of the reference's v1.1 CausalVAEModel (checked against its own state_dict through
    tests/golden/osp_v110_vae_small.pt)."""
    return v120.decoder_param_shapes(hidden_size, SPATIAL_UPSAMPLE, tuple(temporal))


def _mix_factor(draw, fan_in):
    """A normal draw -> uniform in [-1, 3] (alpha between 0.27 and 0.95): the two upsamplers of a decoder get different alphas, and none
    of them makes either term of alpha x + (1 - alpha) conv(x) vanish.  (The reference initialises mix_factor to 2.0.)"""
    return -1.0 + 4.0 * 0.5 * (1.0 + torch.erf(draw / math.sqrt(2.0)))


def synth_state_dict(seed: int = 0, hidden_size: int = 128, temporal=TEMPORAL_UPSAMPLE) -> Dict[str, torch.Tensor]:
    """Deterministic random decoder weights with the reference's names (vae_blocks.synth_weights; ``mix_factor`` uniform in [-1, 3]):
    no checkpoint can be fetched here."""
    return synth_weights(decoder_param_shapes(hidden_size, temporal), torch.Generator().manual_seed(seed), rules=(("mix_factor", _mix_factor),))
