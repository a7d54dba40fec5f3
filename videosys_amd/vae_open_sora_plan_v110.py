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
the reference's (:420-426: 256 / 65 / 17 frames, overlap 0.25).  There is no CPU path.

Encode side (``CausalVAEEncoder``, ``CausalVAEModel.encode``, ``CausalVAEModelWrapper.encode``; Encoder :134-249, encode :470-480, the
wrapper :802-806): the v1.2 encoder of vae_open_sora_plan.py with other downsamplers, built when the state dict holds ``encoder.*``:

  * every spatial downsampler is ``SpatialDownsample2x`` (:1487-1507): vsys_conv_down2_bf16 with kt = 1;
  * levels 1 and 2 then run a temporal downsampler (:235-239), ``TimeDownsampleRes2x`` (:1557-1575) or ``TimeDownsample2x`` (:1533-1542),
    ONE launch of vsys_conv_time_down2_bf16 (csrc/conv_time_down_bf16.hip) on the dense rows the spatial downsampler wrote.  For
    ``TimeDownsampleRes2x``, ``alpha pool(x') + (1 - alpha) conv(x')``: the conv's weights and bias are scaled by (1 - alpha) in fp32 at
    load, before their one rounding to bf16 (as ``_TimeUp`` does), and the kernel adds alpha / 3 times the three pooled frames to the
    fp32 accumulator in its epilogue.  The layer's input and output share one channel map, so at hidden sizes 32 / 64 the pooled column
    of an output column is the column itself.

``_check_encoder_config`` names what is built (CausalConv3d in and out, AttnBlock3DFix, ResnetBlock3D, spatial (S, S, S, ""), temporal
("", X, X, "")); it runs only when there is an encoder to build, and ``_check_config`` keeps accepting any ``encoder_*`` argument."""
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
SPATIAL_DOWNSAMPLE = ("SpatialDownsample2x",) * 3 + ("",)
TIME_DOWNSAMPLERS = ("TimeDownsampleRes2x", "TimeDownsample2x")
TEMPORAL_DOWNSAMPLE = ("", "TimeDownsampleRes2x", "TimeDownsampleRes2x", "")  # what synth_state_dict(encoder=True) builds
ENCODER_CONFIG = dict(v120.ENCODER_CONFIG, encoder_spatial_downsample=SPATIAL_DOWNSAMPLE)
del ENCODER_CONFIG["encoder_temporal_downsample"]


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


def _temporal_down(kw: dict) -> tuple:
    return tuple(kw.get("encoder_temporal_downsample", TEMPORAL_DOWNSAMPLE))


def _check_encoder_config(kw: dict) -> None:
    """The encode side of the configuration (its own check: ``_check_config`` lets every ``encoder_*`` argument pass, since a
    decode-only state dict never builds an encoder)."""
    _check_config({k: v for k, v in kw.items() if not k.startswith("encoder_")})
    for k, want in ENCODER_CONFIG.items():
        if k in kw:
            got = tuple(kw[k]) if isinstance(kw[k], (list, tuple)) else kw[k]
            if got != want:
                raise NotImplementedError(f"CausalVAEModel({k}={kw[k]!r}): this build encodes the Open-Sora-Plan v1.1 configuration only "
                                          f"({k}={want!r})")
    got = _temporal_down(kw)
    if len(got) != 4 or (got[0], got[3]) != ("", "") or got[1] not in TIME_DOWNSAMPLERS or got[2] not in TIME_DOWNSAMPLERS:
        raise NotImplementedError(f"CausalVAEModel(encoder_temporal_downsample={got!r}): this build encodes ('', X, X, '') with X one of "
                                  f"{TIME_DOWNSAMPLERS}")


class _TimeDown:
    """One temporal downsampler: ``conv`` (scaled by 1 - alpha) and ``a3`` = alpha / 3 for TimeDownsampleRes2x, ``conv`` None for
    TimeDownsample2x."""

    def __init__(self, sd, key, dev, cm, kind):
        self.kind, self.conv, self.a3 = kind, None, 1.0 / 3.0
        if kind == "TimeDownsampleRes2x":
            alpha = 1.0 / (1.0 + math.exp(-float(sd[key + ".mix_factor"].reshape(-1)[0])))           # sigmoid on the host, in double
            keep = torch.tensor(1.0 - alpha, dtype=torch.float32)
            scaled = {key + ".conv." + n: sd[key + ".conv." + n].float() * keep for n in ("weight", "bias")}     # fp32, then ONE rounding
            self.conv, self.a3 = _CConv(scaled, key, dev, cm, cm), alpha / 3.0       # (a plain nn.Conv3d: no ``.conv.conv``)


class CausalVAEEncoder(v120.CausalVAEEncoder):
    """Encode side of the reference's v1.1 ``CausalVAEModel`` (Encoder :134-249 + quant_conv): ``moments(x)``, x [B, 3, T, H, W] in
    [-1, 1] -> bf16 [B, 8, ((T - 1) // 2) // 2 + 1, H / 8, W / 8].  ``encoder_temporal_downsample`` chooses the temporal downsamplers
    of levels 1 and 2 (default: TimeDownsampleRes2x twice)."""

    SPATIAL = SPATIAL_DOWNSAMPLE
    _check = staticmethod(_check_encoder_config)

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", hidden_size: Optional[int] = None, **config):
        _check_encoder_config(config)
        self.temporal = _temporal_down(config)
        self.time_downs: Dict[int, _TimeDown] = {}
        super().__init__(state_dict, device=device, hidden_size=hidden_size, **config)

    def _param_shapes(self, hidden_size: int) -> Dict[str, tuple]:
        return encoder_param_shapes(hidden_size, self.temporal)

    def _level_extra(self, sd, lvl, cm, dev) -> None:
        if self.temporal[lvl]:
            self.time_downs[lvl] = _TimeDown(sd, f"encoder.down.{lvl}.time_downsample", dev, cm, self.temporal[lvl])

    def _after_level(self, x, g: VaeGrid, lvl: int):
        """``down[lvl].time_downsample`` (:237-239) on the dense rows of the spatial downsampler: one launch either way."""
        td = self.time_downs.get(lvl)
        if td is None:
            return x, g
        cv = td.conv
        y = vops.conv_time_down2(x, g, None if cv is None else cv.w, None if cv is None else cv.b, x.shape[1], td.a3)
        return y, vops.time_down2_grid(g)


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
    ENCODER = CausalVAEEncoder           # built when the state dict holds encoder.*; a decode-only state dict's encode() raises

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


CausalVAEModel = CausalVAEDecoder        # the reference's class name: both sides (the encode side when the state dict holds it)


class CausalVAEModelWrapper(v120.CausalVAEModelWrapper):
    """``CausalVAEModelWrapper`` :800-826; as vae_open_sora_plan.CausalVAEModelWrapper (``encode`` / ``decode``) with the v1.1 model.
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


def encoder_param_shapes(hidden_size: int = 128, temporal=TEMPORAL_DOWNSAMPLE) -> Dict[str, tuple]:
    """Names and shapes of the encode-side parameters of the reference's v1.1 CausalVAEModel, ``encoder.*`` and ``quant_conv.*`` (checked
    against its own state_dict through tests/golden/osp_v110_vae_encode_small.pt)."""
    return v120.encoder_param_shapes(hidden_size, SPATIAL_DOWNSAMPLE, tuple(temporal))


def _mix_factor(draw, fan_in):
    """A normal draw -> uniform in [-1, 3] (alpha between 0.27 and 0.95): the two upsamplers of a decoder get different alphas, and none
    of them makes either term of alpha x + (1 - alpha) conv(x) vanish.  (The reference initialises mix_factor to 2.0.)"""
    return -1.0 + 4.0 * 0.5 * (1.0 + torch.erf(draw / math.sqrt(2.0)))


def synth_state_dict(seed: int = 0, hidden_size: int = 128, temporal=TEMPORAL_UPSAMPLE, encoder=False) -> Dict[str, torch.Tensor]:
    """Deterministic random decoder weights with the reference's names (vae_blocks.synth_weights; ``mix_factor`` uniform in [-1, 3]):
    no checkpoint can be fetched here.  ``encoder``: the encode side as well — True for ``TEMPORAL_DOWNSAMPLE``, or the temporal
    downsampler per level — drawn AFTER the decoder's (the decoder weights of a seed are the same either way)."""
    shapes = decoder_param_shapes(hidden_size, temporal)
    if encoder:
        shapes.update(encoder_param_shapes(hidden_size, TEMPORAL_DOWNSAMPLE if encoder is True else encoder))
    return synth_weights(shapes, torch.Generator().manual_seed(seed), rules=(("mix_factor", _mix_factor),))
