"""Torch restatement of the decode side of the Open-Sora-Plan v1.1 CausalVAE (reference videosys/models/autoencoders/
autoencoder_kl_open_sora_plan_v110.py: CausalVAEModel.decode / tiled_decode / tiled_decode2d :482-491, :672-693, :735-771, Decoder
:251-354, SpatialUpsample2x :1510-1530, TimeUpsample2x :1545-1554, TimeUpsampleRes2x :1578-1596, CausalVAEModelWrapper.decode :812-816) as
plain functions over a state dict — test scaffolding, as tests/osp_vae_ref.py is for v1.2 and built from its pieces (the residual
block, the attention, the causal conv and the tiling are the same code in both reference files): the float64 run is held to the
reference class's own outputs (tests/golden/osp_v110_vae_small*.pt, tests/test_osp_v110_vae_cpu.py), the bf16 run on the CPU is the
rounding floor the HIP decoder is measured against (tests/test_gpu_osp_v110_vae.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import osp_vae_ref as R

SCALE = R.SCALE
t_chunks = R.t_chunks


def time_upsample(x, sd, name, kind):
    if x.size(2) > 1:
        x = torch.cat([x[:, :, :1], F.interpolate(x[:, :, 1:], scale_factor=(2, 1, 1), mode="trilinear")], dim=2)
    if kind == "TimeUpsample2x":
        return x
    alpha = torch.sigmoid(sd[name + ".mix_factor"].to(x.dtype))
    return alpha * x + (1 - alpha) * R.causal_conv(x, sd, name + ".conv", 1)


def temporal_of(sd):
    """The temporal upsampler per level, read off the state dict (TimeUpsample2x has no parameters)."""
    return tuple("TimeUpsampleRes2x" if f"decoder.up.{lvl}.time_upsample.mix_factor" in sd else ("TimeUpsample2x" if lvl >= 2 else "")
                 for lvl in range(4))


def decoder(z, sd, temporal=None):
    temporal = temporal_of(sd) if temporal is None else temporal
    d = "decoder."
    h = R.causal_conv(z, sd, d + "conv_in", 1)
    h = R.resnet(h, sd, d + "mid.block_1")
    h = R.attn(h, sd, d + "mid.attn_1")
    h = R.resnet(h, sd, d + "mid.block_2")
    for lvl in (3, 2, 1, 0):
        for j in range(3):
            h = R.resnet(h, sd, f"{d}up.{lvl}.block.{j}")
        if lvl:
            h = R.upsample(h, sd, f"{d}up.{lvl}.upsample", "SpatialUpsample2x")
        if temporal[lvl]:
            h = time_upsample(h, sd, f"{d}up.{lvl}.time_upsample", temporal[lvl])
    return R.causal_conv(R.silu(R.norm(h, sd, d + "norm_out")), sd, d + "conv_out", 1)


def decode_tile(z, sd):
    return decoder(R.causal_conv(z, sd, "post_quant_conv", 0), sd)


def tiled_decode2d(z, sd, tiling):
    lat, smp, ov = tiling["tile_latent_min_size"], tiling["tile_sample_min_size"], tiling["tile_overlap_factor"]
    step, ext = int(lat * (1 - ov)), int(smp * ov)
    lim = smp - ext
    rows = [[decode_tile(z[:, :, :, i:i + lat, j:j + lat], sd) for j in range(0, z.shape[4], step)] for i in range(0, z.shape[3], step)]
    out_rows = []
    for i, row in enumerate(rows):
        res = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = R.blend(rows[i - 1][j], tile, ext, 3)
            if j > 0:
                tile = R.blend(row[j - 1], tile, ext, 4)
            res.append(tile[:, :, :, :lim, :lim])
        out_rows.append(torch.cat(res, dim=4))
    return torch.cat(out_rows, dim=3)


def vae_decode(z, sd, tiling=None):
    t = tiling
    if t is None or not (z.shape[-1] > t["tile_latent_min_size"] or z.shape[-2] > t["tile_latent_min_size"]
                         or z.shape[-3] > t["tile_latent_min_size_t"]):
        return decode_tile(z, sd)
    out = []
    for i, (a, b) in enumerate(t_chunks(z.shape[2], t["tile_latent_min_size_t"])):
        dec = tiled_decode2d(z[:, :, a:b], sd, t)
        out.append(dec if i == 0 else dec[:, :, 1:])
    return torch.cat(out, dim=2)


def wrapper_decode(x, sd, tiling=None, dtype=torch.float64):
    """CausalVAEModelWrapper.decode :812-816 in ``dtype``: x [B, 4, T, H, W] -> [B, T_out, 3, 8H, 8W]."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    return vae_decode(x.to(dtype) / SCALE, sd, tiling).permute(0, 2, 1, 3, 4).contiguous()
