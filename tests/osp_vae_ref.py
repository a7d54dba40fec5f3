"""Torch restatement of the decode side of the Open-Sora-Plan v1.2 CausalVAE (reference videosys/models/autoencoders/
autoencoder_kl_open_sora_plan_v120.py: CausalVAEModel.decode / tiled_decode / tiled_decode2d :872-882, :942-963, :1006-1043, Decoder
:629-738, CausalVAEModelWrapper.decode :1129-1133) as plain functions over a state dict — test scaffolding: the float64 run is
held to the reference class's own outputs (tests/golden/osp_vae_small.pt, tests/test_osp_pipeline_cpu.py), the bf16 run on the CPU is
the rounding floor the HIP decoder is measured against (tests/test_gpu_osp_vae.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

SCALE = 0.18215


def causal_conv(x, sd, name, pad):
    """CausalConv3d.forward :94-97: kt - 1 copies of the first frame in front, zero padding in space."""
    w, b = sd[name + ".conv.weight"].to(x.dtype), sd[name + ".conv.bias"].to(x.dtype)
    kt = w.shape[2]
    if kt > 1:
        x = torch.cat([x[:, :, :1].repeat(1, 1, kt - 1, 1, 1), x], dim=2)
    return F.conv3d(x, w, b, padding=(0, pad, pad))


def norm(x, sd, name):
    return F.group_norm(x, 32, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype), eps=1e-6)


def silu(x):
    return x * torch.sigmoid(x)


def resnet(x, sd, name):
    h = causal_conv(silu(norm(x, sd, name + ".norm1")), sd, name + ".conv1", 1)
    h = causal_conv(silu(norm(h, sd, name + ".norm2")), sd, name + ".conv2", 1)
    if (name + ".nin_shortcut.conv.weight") in sd:
        x = causal_conv(x, sd, name + ".nin_shortcut", 0)
    return x + h


def attn(x, sd, name):
    """AttnBlock3DFix :375-415: one head of width C over the h * w positions of every frame."""
    h = norm(x, sd, name + ".norm")
    q, k, v = (causal_conv(h, sd, f"{name}.{n}", 0) for n in "qkv")
    b, c, t, hh, ww = q.shape
    flat = lambda a: a.permute(0, 2, 1, 3, 4).reshape(b * t, c, hh * ww)
    q, k, v = flat(q).permute(0, 2, 1), flat(k), flat(v)
    p = torch.softmax(torch.bmm(q, k) * (int(c) ** (-0.5)), dim=2)
    o = torch.bmm(v, p.permute(0, 2, 1)).reshape(b, t, c, hh, ww).permute(0, 2, 1, 3, 4)
    return x + causal_conv(o, sd, name + ".proj_out", 0)


def upsample(x, sd, name, kind):
    if kind == "SpatialUpsample2x":                       # :334-341
        b, c, t, h, w = x.shape
        x = F.interpolate(x.reshape(b, c * t, h, w), scale_factor=(2, 2), mode="nearest").reshape(b, c, t, 2 * h, 2 * w)
        w_, b_ = sd[name + ".conv.conv.weight"].to(x.dtype), sd[name + ".conv.conv.bias"].to(x.dtype)
        return F.conv3d(x, w_, b_, padding=(0, 1, 1))
    if x.size(2) > 1:                                     # Spatial2xTime2x3DUpsample :349-357
        a, r = x[:, :, :1], x[:, :, 1:]
        r = F.interpolate(r, scale_factor=(2, 2, 2), mode="trilinear")
        a = F.interpolate(a, scale_factor=(1, 2, 2), mode="trilinear")
        x = torch.cat([a, r], dim=2)
    else:
        x = F.interpolate(x, scale_factor=(1, 2, 2), mode="trilinear")
    return causal_conv(x, sd, name + ".conv", 1)


UPSAMPLE = ("", "SpatialUpsample2x", "Spatial2xTime2x3DUpsample", "Spatial2xTime2x3DUpsample")


def decoder(z, sd):
    d = "decoder."
    h = causal_conv(z, sd, d + "conv_in", 1)
    h = resnet(h, sd, d + "mid.block_1")
    h = attn(h, sd, d + "mid.attn_1")
    h = resnet(h, sd, d + "mid.block_2")
    for lvl in (3, 2, 1, 0):
        for j in range(3):
            h = resnet(h, sd, f"{d}up.{lvl}.block.{j}")
        if UPSAMPLE[lvl]:
            h = upsample(h, sd, f"{d}up.{lvl}.upsample", UPSAMPLE[lvl])
    return causal_conv(silu(norm(h, sd, d + "norm_out")), sd, d + "conv_out", 1)


def decode_tile(z, sd):
    return decoder(causal_conv(z, sd, "post_quant_conv", 0), sd)


def t_chunks(t, lat_t):
    """tiled_decode :943-953."""
    idx = list(range(0, t, lat_t - 1))
    if len(idx) == 1:
        return [[0, t]]
    se = [[idx[i], idx[i + 1] + 1] for i in range(len(idx) - 1)]
    if se[-1][-1] > t:
        se[-1][-1] = t
    elif se[-1][-1] < t:
        se.append([idx[-1], t])
    return se


def blend(a, b, ext, dim):
    ext = min(a.shape[dim], b.shape[dim], ext)
    for y in range(ext):
        ia = [slice(None)] * 5
        ib = [slice(None)] * 5
        ia[dim], ib[dim] = a.shape[dim] - ext + y, y
        b[tuple(ib)] = a[tuple(ia)] * (1 - y / ext) + b[tuple(ib)] * (y / ext)
    return b


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
                tile = blend(rows[i - 1][j], tile, ext, 3)
            if j > 0:
                tile = blend(row[j - 1], tile, ext, 4)
            res.append(tile[:, :, :, :lim, :lim])
        out_rows.append(torch.cat(res, dim=4))
    return torch.cat(out_rows, dim=3)


def vae_decode(z, sd, tiling=None):
    """CausalVAEModel.decode on z [B, 4, T, H, W] -> [B, 3, T_out, 8H, 8W]; ``tiling``: None (use_tiling False) or the dict of the
    tile attributes."""
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
    """CausalVAEModelWrapper.decode :1129-1133 in ``dtype``: x [B, 4, T, H, W] -> [B, T_out, 3, 8H, 8W]."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    return vae_decode(x.to(dtype) / SCALE, sd, tiling).permute(0, 2, 1, 3, 4).contiguous()
