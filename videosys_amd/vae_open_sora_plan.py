"""Open-Sora-Plan v1.2 CausalVAE decode on MI355X: the decoder half of ``CausalVAEModel`` and ``CausalVAEModelWrapper.decode``
(reference videosys/models/autoencoders/autoencoder_kl_open_sora_plan_v120.py: Decoder :629-738, CausalVAEModel.decode / tiled_decode /
tiled_decode2d :872-882, :942-963, :1006-1043, the wrapper :1112-1139), under the reference's state-dict names (``decoder.conv_in.conv.
weight``, ``decoder.mid.block_1.norm1.weight``, ..., ``post_quant_conv.conv.*``).

The one configuration the reference file can still construct is supported (``_check_config``): CausalConv3d in and out,
AttnBlock3DFix in the mid block, ResnetBlock3D everywhere, spatial upsamplers ("", SpatialUpsample2x, Spatial2xTime2x3DUpsample,
Spatial2xTime2x3DUpsample), no temporal upsamplers, no attention at the resolutions, multipliers (1, 2, 4, 4), 4 latent channels.

Layout and kernels (DESIGN.md "Open-Sora-Plan CausalVAE decode"):
  * activations are bf16 channels-last rows over a ``VaeGrid``; every convolution is the tap-shifted implicit GEMM (vsys_conv_bf16).
    A causal conv replicates the first frame of its own input (CausalConv3d.forward :94-97): the two front frames of the padded
    conv-input grid are copies of its first frame (``_front``), as vae_cogvideox.py does for a fresh cache;
  * x / 0.18215 and post_quant_conv live in the parameters of the first-layer im2col (vsys_vae_first_im2col), conv_in is a GEMM over
    its rows.  The kernel pads time with zeros, so the latent is handed over with two copies of its first frame in front and the
    two leading output frames are dropped;
  * GroupNorm (+ SiLU) is vsys_gn_stats / vsys_gn_apply over all frames of the sample, eps 1e-6;
  * AttnBlock3DFix is GEMMs + vsys_softmax_rows per frame (one head of width C, scale C^-0.5): at most 8192 keys per frame;
  * SpatialUpsample2x is vsys_regrid(up=1), Spatial2xTime2x3DUpsample is vsys_upsample_trilinear2x, each straight into the padded
    input grid of its conv;
  * tiles are blended by vsys_blend_edge on planar [3, T, H, W] tiles.

Channel counts below 128 (``hidden_size`` 32 or 64 — the test geometry; the published model has 128) run in a 128-column physical
layout in which every GroupNorm group's channels are repeated to fill four columns (``_ChanMap``): the GEMM tile is 128 columns wide
anyway, a group of repeated channels has the mean and variance of the group itself, and a consumer's weights are zero on the copies.
No kernel changes, no extra launches; at ``hidden_size`` 128 the map is the identity.

The residual block, the staging cache, the attention core (with the mask for key counts that are no multiple of four) and the tile
stitching are the shared ones of vae_blocks.py; this module adds the channel map, the causal front frames (``_norm_act``), the
whole-sample GroupNorm around the attention core and the tiling geometry.  Under a group of ranks (``decode(z, group=)``) the
(sample, temporal chunk, spatial tile) units of a tiled decode are dealt over the ranks and gathered once.  There is no CPU path."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import ops
from . import open_sora_plan_ops as oops
from .ops import VaeGrid
from .vae_blocks import (AttnWeights, VaeBlocks, _vec, attention_core, conv3, deal_units, gather_units, norm, stitch_tiles,
                         synth_weights)

SCALE = 0.18215                      # CausalVAEModelWrapper.decode :1131
Z_CHANNELS = 4
HIDDEN_SIZE_MULT = (1, 2, 4, 4)
SPATIAL_UPSAMPLE = ("", "SpatialUpsample2x", "Spatial2xTime2x3DUpsample", "Spatial2xTime2x3DUpsample")
MAX_KEYS = 8192                      # vsys_softmax_rows: ld <= 8192
_KCOLS = 128                         # 27 taps x 4 channels = 108 -> the GEMM's 32-column K step


def check_attention_keys(h: int, w: int) -> int:
    """The per-frame key count of the mid-block attention rounded up to the 128-column GEMM tile; more than the row softmax takes
    raises (host side, before any launch)."""
    Lp = (h * w + 127) // 128 * 128
    if Lp > MAX_KEYS:
        raise ValueError(f"CausalVAE mid-block attention over {h} x {w} = {h * w} keys per frame: the row softmax takes at most "
                         f"{MAX_KEYS}; enable tiling (vae.enable_tiling(): tiles of tile_latent_min_size <= 90)")
    return Lp


def _check_config(kw: dict) -> None:
    want = dict(z_channels=Z_CHANNELS, hidden_size_mult=HIDDEN_SIZE_MULT, attn_resolutions=(), decoder_conv_in="CausalConv3d",
                decoder_conv_out="CausalConv3d", decoder_attention="AttnBlock3DFix", decoder_resnet_blocks=("ResnetBlock3D",) * 4,
                decoder_spatial_upsample=SPATIAL_UPSAMPLE, decoder_temporal_upsample=("",) * 4, decoder_mid_resnet="ResnetBlock3D",
                num_res_blocks=2, embed_dim=4, q_conv="CausalConv3d", use_quant_layer=True, dropout=0.0)
    for k, v in kw.items():
        if k in want:
            got = tuple(v) if isinstance(v, (list, tuple)) else v
            if got != want[k]:
                raise NotImplementedError(f"CausalVAEModel({k}={v!r}): this build decodes the Open-Sora-Plan v1.2 configuration only "
                                          f"({k}={want[k]!r})")
        elif not (k.startswith("encoder_") or k in ("hidden_size", "resolution", "double_z")):
            raise NotImplementedError(f"CausalVAEModel: unknown argument {k!r}")


class _ChanMap:
    """Physical column layout of a C-channel activation.  C >= 128: the channels as they are.  C = 32 / 64 (1 / 2 channels per
    GroupNorm group): 128 columns, group g in columns 4g .. 4g + 3 as its channels repeated.  ``src[p]`` = the channel in column p;
    ``first`` = the columns that hold the first copy (a consumer's weights are non-zero there only)."""

    def __init__(self, C: int):
        cg = C // 32
        if C % 32 or not (cg in (1, 2) or (C % 128 == 0 and (C // 128) & (C // 128 - 1) == 0)):
            raise NotImplementedError(f"CausalVAE decoder: {C} channels (hidden_size must be 32, 64 or a power-of-two multiple of 128)")
        self.C = C
        if cg >= 4:
            self.P, self.src, self.first = C, torch.arange(C), torch.ones(C, dtype=torch.bool)
        else:
            self.P = 128
            self.src = torch.arange(C).view(32, cg).repeat(1, 4 // cg).flatten()
            self.first = (torch.arange(128) % 4) < cg

    def out_rows(self, w: torch.Tensor) -> torch.Tensor:
        """A producer's [C, ...] (weight rows, bias, norm scale) -> [P, ...]."""
        return w[self.src.to(w.device)]

    def in_cols(self, w: torch.Tensor) -> torch.Tensor:
        """A consumer's weight [Cout, C, ...] -> [Cout, P, ...], zero on the copies."""
        out = torch.zeros(w.shape[0], self.P, *w.shape[2:], dtype=w.dtype, device=w.device)
        out[:, self.first.to(w.device)] = w
        return out


class _CConv:
    """One CausalConv3d between two layouts: bf16 weight matrix [N, taps * P_in] (k = tap * P_in + column), bias [N]."""

    def __init__(self, sd, key, dev, cin: _ChanMap, cout: Optional[_ChanMap], n_pad: Optional[int] = None):
        w = sd[key + ".conv.weight"].to(dev).float()
        b = sd[key + ".conv.bias"].to(dev).float()
        self.key, self.kt, self.ks = key, w.shape[2], w.shape[-1]
        w = cin.in_cols(w)
        if cout is not None:
            w, b = cout.out_rows(w), cout.out_rows(b)
        n = n_pad or w.shape[0]
        self.cin = cin.P
        m = w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)
        self.w = torch.zeros(n, m.shape[1], dtype=torch.bfloat16, device=dev)
        self.w[:m.shape[0]] = m.to(torch.bfloat16)
        self.b = _vec(b, n)


class _CNorm:
    def __init__(self, sd, key, dev, cm: _ChanMap):
        self.g = cm.out_rows(sd[key + ".weight"]).to(dev).to(torch.bfloat16).contiguous()
        self.b = cm.out_rows(sd[key + ".bias"]).to(dev).to(torch.bfloat16).contiguous()
        self.C, self.eps = cm.P, 1e-6


class _CRes:
    def __init__(self, sd, p, dev, ci: _ChanMap, co: _ChanMap):
        self.n1, self.c1 = _CNorm(sd, p + ".norm1", dev, ci), _CConv(sd, p + ".conv1", dev, ci, co)
        self.n2, self.c2 = _CNorm(sd, p + ".norm2", dev, co), _CConv(sd, p + ".conv2", dev, co, co)
        self.sc = _CConv(sd, p + ".nin_shortcut", dev, ci, co) if (p + ".nin_shortcut.conv.weight") in sd else None


class CausalVAEDecoder(VaeBlocks):
    """Decode side of the reference ``CausalVAEModel``: ``decode(z)``, z [B, 4, T, H, W] (already divided by 0.18215 unless
    ``in_scale`` says otherwise) -> [B, 3, 4(T-1)+1, 8H, 8W] bf16, with the reference's tiling attributes."""

    # what a decoder of the same family with other upsamplers overrides (vae_open_sora_plan_v110.py)
    SPATIAL = SPATIAL_UPSAMPLE
    TILE_DEFAULTS = dict(tile_sample_min_size=256, tile_sample_min_size_t=33, tile_latent_min_size_t=16, tile_overlap_factor=0.125)
    _check = staticmethod(_check_config)

    @staticmethod
    def _param_shapes(hidden_size: int) -> Dict[str, tuple]:
        return decoder_param_shapes(hidden_size)

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", hidden_size: Optional[int] = None, **config):
        self._check(config)
        super().__init__(device)
        dev = self.device
        sd = state_dict
        hs = sd["decoder.conv_out.conv.weight"].shape[1]
        if hidden_size is not None and hidden_size != hs:
            raise ValueError(f"hidden_size {hidden_size}, but decoder.conv_out.conv.weight has {hs} input channels")
        missing = sorted(set(self._param_shapes(hs)) - set(sd))
        if missing:
            raise KeyError(f"CausalVAE decoder: the state dict lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        self.hidden_size = hs
        self.config = SimpleNamespace(hidden_size=hs, z_channels=Z_CHANNELS, hidden_size_mult=HIDDEN_SIZE_MULT)
        self.dtype = torch.bfloat16
        # CausalVAEModel.__init__ :798-806
        self.tile_sample_min_size = self.TILE_DEFAULTS["tile_sample_min_size"]
        self.tile_sample_min_size_t = self.TILE_DEFAULTS["tile_sample_min_size_t"]
        self.tile_latent_min_size = int(self.tile_sample_min_size / (2 ** (len(HIDDEN_SIZE_MULT) - 1)))
        self.tile_latent_min_size_t = self.TILE_DEFAULTS["tile_latent_min_size_t"]
        self.tile_overlap_factor = self.TILE_DEFAULTS["tile_overlap_factor"]
        self.use_tiling = False
        self.pq = (sd["post_quant_conv.conv.weight"].float().reshape(4, 4).cpu(), sd["post_quant_conv.conv.bias"].float().cpu())
        d = "decoder."
        cm = {c: _ChanMap(c) for c in {hs * m for m in HIDDEN_SIZE_MULT}}
        top = cm[hs * 4]
        w_in = sd[d + "conv_in.conv.weight"].to(dev).float()                       # [4h, 4, 3, 3, 3]: column = tap * 4 + channel
        w_in = top.out_rows(w_in).permute(0, 2, 3, 4, 1).reshape(top.P, -1)
        self.conv_in_w = torch.zeros(top.P, _KCOLS, dtype=torch.bfloat16, device=dev)
        self.conv_in_w[:, :w_in.shape[1]] = w_in.to(torch.bfloat16)
        self.conv_in_b = top.out_rows(sd[d + "conv_in.conv.bias"]).to(dev).to(torch.bfloat16).contiguous()
        self.mid = [_CRes(sd, f"{d}mid.block_{i}", dev, top, top) for i in (1, 2)]
        a = d + "mid.attn_1."
        lin = lambda n: _CConv(sd, a + n, dev, top, top)
        self.attn = AttnWeights.from_convs(_CNorm(sd, a + "norm", dev, top), lin("q"), lin("k"), lin("v"), lin("proj_out"))
        self.ups = []
        prev = top
        for lvl in (3, 2, 1, 0):
            co = cm[hs * HIDDEN_SIZE_MULT[lvl]]
            res = []
            for j in range(3):
                res.append(_CRes(sd, f"{d}up.{lvl}.block.{j}", dev, prev, co))
                prev = co
            up = _CConv(sd, f"{d}up.{lvl}.upsample.conv", dev, co, co) if self.SPATIAL[lvl] else None
            self.ups.append((res, up, self.SPATIAL[lvl]))
            self._level_extra(sd, lvl, co, dev)
        self.norm_out = _CNorm(sd, d + "norm_out", dev, prev)
        self.conv_out = _CConv(sd, d + "conv_out", dev, prev, None, n_pad=128)

    def _level_extra(self, sd, lvl: int, cm: _ChanMap, dev) -> None:
        """Weights a level holds beside its residual blocks and its spatial upsampler (none in v1.2)."""

    def _after_level(self, x, g: VaeGrid, lvl: int):
        """What a level runs after its spatial upsampler (nothing in v1.2)."""
        return x, g

    # ------------------------------------------------------------------------------------------------ reference surface
    def enable_tiling(self, use_tiling: bool = True):
        self.use_tiling = use_tiling

    def disable_tiling(self):
        self.enable_tiling(False)

    # ------------------------------------------------------------------------------------------------ building blocks
    @staticmethod
    def _front(rows, g: VaeGrid):
        """CausalConv3d.forward :94-97: the g.tf frames in front of the conv's input are copies of its first frame."""
        if g.tf:
            v = rows.view(g.T + g.tf, g.Hp, g.Wp, rows.shape[1])
            v[:g.tf].copy_(v[g.tf:g.tf + 1].expand(g.tf, -1, -1, -1))

    def _norm_act(self, x, gx: VaeGrid, norm, C: int, tf: int, silu=True, dense=False):
        """GroupNorm over all frames of the sample (+ SiLU) into the padded conv-input grid, then the causal front frames.
        With it the shared ``_resblock`` is ResnetBlock3D.forward :295-315."""
        y, gd = super()._norm_act(x, gx, norm, C, tf, silu, dense)
        self._front(y, gd)
        return y, gd

    def _conv(self, h, gh: VaeGrid, cv: _CConv, res=None):
        return ops.conv(h, gh, cv.w, cv.b, cv.cin, cv.kt, cv.ks, res=res)

    def _attention(self, x, g: VaeGrid, aw: AttnWeights):
        """AttnBlock3DFix.forward :375-415 with its residual: one head of width C per frame.  x rows over g (pad 1, no front frames)
        -> dense rows.  Inside, a frame takes the key count rounded up to the 128-column GEMM tile (pad rows zero on input)."""
        C, L, n = aw.C, g.H * g.W, g.T
        Lp = check_attention_keys(g.H, g.W)
        gf = VaeGrid(n, 1, g.H, g.W, g.pad, 0, sample_rows=g.plane)                 # the same rows, one sample per frame
        gdn = VaeGrid(n, 1, g.H, g.W, 0, 0, sample_rows=Lp)
        hn, xd = self._attn_bufs(n, g.H, g.W, C, Lp)
        gn1 = VaeGrid(1, n, g.H, g.W, 0, 0)
        stage = torch.empty(gn1.rows, C, dtype=torch.bfloat16, device=self.device)
        ops.group_norm(x, g, stage, gn1, C, aw.norm.g, aw.norm.b, aw.norm.eps, False)      # statistics over all frames of the sample
        ops.regrid(stage, VaeGrid(n, 1, g.H, g.W, 0, 0), hn, gdn, C)                       # ... then one frame per Lp rows
        ops.regrid(x, gf, xd, gdn, C)
        y = attention_core(hn, xd, n, L, Lp, C, aw)
        # (a per-frame stride of Lp rows is no grid of ONE sample, and the next GroupNorm runs over the whole sample: frame-dense rows)
        out = torch.empty(gn1.rows, C, dtype=torch.bfloat16, device=self.device)
        ops.regrid(y, gdn, out, VaeGrid(n, 1, g.H, g.W, 0, 0), C)
        return out, gn1

    def _decode_tile(self, zt: torch.Tensor, in_scale: float) -> torch.Tensor:
        """zt planar bf16 [4, T, h, w] -> planar bf16 [3, 4(T-1)+1, 8h, 8w]: post_quant_conv + Decoder.forward :713-738."""
        _, T, h, w = zt.shape
        check_attention_keys(h, w)
        zz = torch.cat([zt[:, :1], zt[:, :1], zt], dim=1).contiguous()              # conv_in's two copies of the first frame
        params = [in_scale] * 4 + [0.0] * 4 + self.pq[0].flatten().tolist() + self.pq[1].tolist()
        a = ops.vae_first_im2col(zz, 3, _KCOLS, params)
        x = ops.gemm128(a, self.conv_in_w, self.conv_in_b)[2 * h * w:]
        g = VaeGrid(1, T, h, w, 0, 0)
        x, g = self._resblock(x, g, self.mid[0])
        x, g = self._attention(x, g, self.attn)
        x, g = self._resblock(x, g, self.mid[1])
        for lvl, (res, up, kind) in zip((3, 2, 1, 0), self.ups):
            for r in res:
                x, g = self._resblock(x, g, r)
            if kind == "SpatialUpsample2x":                                          # :334-341 (a (1, 3, 3) conv: no front frames)
                gu = VaeGrid(1, g.T, 2 * g.H, 2 * g.W, 1, 0)
                xu = self._padded_buf(gu, up.cin)
                ops.regrid(x, g, xu, gu, up.cin, up=1)
                x, g = self._conv(xu, gu, up), gu.conv_out()
            elif kind:                                                               # Spatial2xTime2x3DUpsample :349-357
                gu = VaeGrid(1, 1 if g.T == 1 else 2 * g.T - 1, 2 * g.H, 2 * g.W, 1, 2)
                xu = self._padded_buf(gu, up.cin)
                oops.upsample_trilinear2x(x, g, xu, gu, up.cin)
                self._front(xu, gu)
                x, g = self._conv(xu, gu, up), gu.conv_out()
            x, g = self._after_level(x, g, lvl)
        hN, gN = self._norm_act(x, g, self.norm_out, self.norm_out.C, 2)
        y = self._conv(hN, gN, self.conv_out)
        out = torch.empty(3, g.T, g.H, g.W, dtype=torch.bfloat16, device=self.device)
        ops.extract_planar(y, gN.conv_out(), 3, 0, out, 0)
        return out

    # ------------------------------------------------------------------------------------------------ tiling
    def _t_chunks(self, t: int):
        """tiled_decode :943-953: chunks of tile_latent_min_size_t frames that overlap by one."""
        idx = list(range(0, t, self.tile_latent_min_size_t - 1))
        if len(idx) == 1:
            return [[0, t]]
        se = [[idx[i], idx[i + 1] + 1] for i in range(len(idx) - 1)]
        if se[-1][-1] > t:
            se[-1][-1] = t
        elif se[-1][-1] < t:
            se.append([idx[-1], t])
        return se

    def _tile_geometry(self):
        """(latent tile, latent step, blend extent in pixels, row / column limit in pixels) of tiled_decode2d :1006-1012."""
        lat, smp = self.tile_latent_min_size, self.tile_sample_min_size
        step, ext = int(lat * (1 - self.tile_overlap_factor)), int(smp * self.tile_overlap_factor)
        return lat, step, ext, smp - ext

    def _tiled2d(self, zb: torch.Tensor, in_scale: float) -> torch.Tensor:
        """tiled_decode2d :1006-1043 on planar [4, T, H, W]."""
        lat, step, ext, lim = self._tile_geometry()
        H, W = zb.shape[-2:]
        rows = [[self._decode_tile(zb[:, :, i:i + lat, j:j + lat].contiguous(), in_scale) for j in range(0, W, step)]
                for i in range(0, H, step)]
        return stitch_tiles(rows, ext, ext, lim, lim)

    def tile_units(self, B: int, T: int, H: int, W: int):
        """The independent pieces of a tiled decode of latents [B, 4, T, H, W], in decode order: [(sample, (t0, t1), i, j)], one per
        temporal chunk and spatial tile, and their costs (chunk latent frames x tile latent rows x tile latent columns)."""
        lat, step, _, _ = self._tile_geometry()
        units = [(b, (t0, t1), i, j) for b in range(B) for t0, t1 in self._t_chunks(T) for i in range(0, H, step)
                 for j in range(0, W, step)]
        costs = [(t1 - t0) * min(lat, H - i) * min(lat, W - j) for _, (t0, t1), i, j in units]
        return units, costs

    def _decode_over_ranks(self, z: torch.Tensor, in_scale: float, group) -> torch.Tensor:
        """The tiled decode with its (sample, chunk, tile) units dealt over the ranks of ``group`` (vae_blocks.deal_units) and ONE
        all-gather of the decoded units, each padded to a full chunk of a full tile; then the tail of the unsharded decode on every
        rank: stitch per chunk, drop the first frame of the later chunks, concatenate.  A unit is decoded by ``_decode_tile`` exactly
        as the unsharded decode does it (its GroupNorm runs over the unit alone), so the bits are the unsharded decode's."""
        from . import dsp

        B, _, T, H, W = z.shape
        lat, step, ext, lim = self._tile_geometry()
        smp, ft = self.tile_sample_min_size, 4 * (self.tile_latent_min_size_t - 1) + 1
        if 8 * lat > smp:
            raise ValueError(f"tile_latent_min_size {lat} decodes to {8 * lat} pixels, more than tile_sample_min_size {smp}")
        units, costs = self.tile_units(B, T, H, W)
        owner, slot, per = deal_units(costs, dsp.group_size(group))
        r = dsp.group_rank(group)
        shapes = [(3, 4 * (t1 - t0 - 1) + 1, 8 * min(lat, H - i), 8 * min(lat, W - j)) for _, (t0, t1), i, j in units]
        zs = [z[b].to(torch.bfloat16) for b in range(B)]
        mine = {}
        for u in sorted((u for u in range(len(units)) if owner[u] == r), key=lambda u: slot[u]):
            b, (t0, t1), i, j = units[u]
            mine[u] = self._decode_tile(zs[b][:, t0:t1, i:i + lat, j:j + lat].contiguous(), in_scale)
        tiles = gather_units(mine, owner, slot, per, (3, ft, smp, smp), group, self.device, shapes)
        nrow, ncol, nchunk = len(range(0, H, step)), len(range(0, W, step)), len(self._t_chunks(T))
        outs, u = [], 0
        for b in range(B):
            parts = []
            for c in range(nchunk):
                rows = [tiles[u + k * ncol:u + (k + 1) * ncol] for k in range(nrow)]
                u += nrow * ncol
                dec = stitch_tiles(rows, ext, ext, lim, lim)
                parts.append(dec if c == 0 else dec[:, 1:])
            outs.append(torch.cat(parts, dim=1))
        return torch.stack(outs, 0)

    @torch.no_grad()
    def decode(self, z: torch.Tensor, in_scale: float = 1.0, group=None) -> torch.Tensor:
        """CausalVAEModel.decode :872-882: z [B, 4, T, H, W] -> [B, 3, 4(T-1)+1, 8H, 8W] bf16.  ``in_scale`` multiplies z inside the
        first-layer kernel (the wrapper's 1 / 0.18215).  ``group`` (dsp.py group protocol; every rank holds the same latents): the
        units of a TILED decode are decoded by the ranks in turn and gathered once (``_decode_over_ranks``) — the reference decodes
        all of them on every rank; every rank returns the whole video.  An untiled decode is not sharded and issues no collective."""
        if not z.is_cuda:
            raise RuntimeError("CausalVAEDecoder.decode needs a HIP device tensor (no CPU path)")
        if z.dim() != 5 or z.shape[1] != Z_CHANNELS:
            raise ValueError(f"expected latents [B, {Z_CHANNELS}, T, H, W], got {tuple(z.shape)}")
        tiled = self.use_tiling and (z.shape[-1] > self.tile_latent_min_size or z.shape[-2] > self.tile_latent_min_size
                                     or z.shape[-3] > self.tile_latent_min_size_t)
        if tiled and group is not None:
            from . import dsp

            if dsp.group_size(group) > 1:
                return self._decode_over_ranks(z, in_scale, group)
        outs = []
        for b in range(z.shape[0]):
            zb = z[b].to(torch.bfloat16).contiguous()
            if not tiled:
                outs.append(self._decode_tile(zb, in_scale))
                continue
            parts = []
            for i, (t0, t1) in enumerate(self._t_chunks(zb.shape[1])):
                dec = self._tiled2d(zb[:, t0:t1], in_scale)
                parts.append(dec if i == 0 else dec[:, 1:])
            outs.append(torch.cat(parts, dim=1))
        return torch.stack(outs, 0)

    __call__ = decode


CausalVAEModel = CausalVAEDecoder        # the reference's class name; decode side only


class CausalVAEModelWrapper:
    """``CausalVAEModelWrapper`` :1112-1139, decode side: ``vae`` is the decoder (the pipeline sets ``wrapper.vae.tile_*`` and calls
    ``wrapper.vae.enable_tiling()``, pipeline_open_sora_plan.py:309-321); ``decode(x)`` = vae.decode(x / 0.18215) as [B, T, 3, H, W].
    ``model_path``: a state dict, ``"synthetic:<seed>"`` or a LOCAL directory with the checkpoint (utils.read_component)."""

    def __init__(self, model_path, subfolder=None, cache_dir=None, use_ema=False, device="cuda", hidden_size: Optional[int] = None, **kwargs):
        if use_ema:
            raise NotImplementedError("CausalVAEModelWrapper(use_ema=True): the EMA copy is a training artefact; load its weights as the state dict")
        if isinstance(model_path, dict):
            sd = model_path
        elif isinstance(model_path, str) and model_path.startswith("synthetic:"):
            sd = synth_state_dict(int(model_path.split(":", 1)[1]), hidden_size or 128)
        else:
            from .utils import read_component

            sd = read_component(model_path if subfolder is None else f"{model_path}/{subfolder}")[1]
            if sd is None:
                raise FileNotFoundError(f"CausalVAEModelWrapper({model_path!r}): not a local checkpoint directory, a state dict or 'synthetic:<seed>'")
        self.vae = CausalVAEDecoder(sd, device=device, hidden_size=hidden_size, **kwargs)

    def encode(self, x):
        raise NotImplementedError("the CausalVAE encoder is not part of this build (decode only)")

    @torch.no_grad()
    def decode(self, x: torch.Tensor, group=None) -> torch.Tensor:
        """``group``: the ranks that share this decode (CausalVAEDecoder.decode)."""
        return self.vae.decode(x, in_scale=1.0 / SCALE, group=group).permute(0, 2, 1, 3, 4).contiguous()

    forward = __call__ = decode

    def dtype(self):
        return self.vae.dtype


# ---------------------------------------------------------------------------------------------------- synthetic weights
def decoder_param_shapes(hidden_size: int = 128, spatial=SPATIAL_UPSAMPLE, temporal=("",) * 4) -> Dict[str, tuple]:
    """Names and shapes of the decode-side parameters of the reference CausalVAEModel (checked against its own state_dict through
    tests/golden/osp_vae_small.pt).  ``spatial`` / ``temporal``: the upsampler class per level (the v1.2 ones by default; the v1.1
    decoder of vae_open_sora_plan_v110.py passes its own: a ``TimeUpsampleRes2x`` holds ``mix_factor`` and a causal 3 x 3 x 3 conv)."""
    p: Dict[str, tuple] = {}
    hs = hidden_size

    def cconv(name, ci, co, k):
        conv3(p, name, ci, co, k)

    def res(name, ci, co):
        norm(p, name + ".norm1", ci); cconv(name + ".conv1", ci, co, 3)
        norm(p, name + ".norm2", co); cconv(name + ".conv2", co, co, 3)
        if ci != co:
            cconv(name + ".nin_shortcut", ci, co, 1)

    d = "decoder."
    top = hs * HIDDEN_SIZE_MULT[-1]
    cconv(d + "conv_in", Z_CHANNELS, top, 3)
    res(d + "mid.block_1", top, top)
    norm(p, d + "mid.attn_1.norm", top)
    for n in ("q", "k", "v", "proj_out"):
        cconv(f"{d}mid.attn_1.{n}", top, top, 1)
    res(d + "mid.block_2", top, top)
    prev = top
    for lvl in (3, 2, 1, 0):
        co = hs * HIDDEN_SIZE_MULT[lvl]
        for j in range(3):
            res(f"{d}up.{lvl}.block.{j}", prev, co)
            prev = co
        if spatial[lvl]:
            cconv(f"{d}up.{lvl}.upsample.conv", co, co, (1, 3, 3) if spatial[lvl] == "SpatialUpsample2x" else 3)
        if temporal[lvl] == "TimeUpsampleRes2x":
            p[f"{d}up.{lvl}.time_upsample.mix_factor"] = (1,)
            cconv(f"{d}up.{lvl}.time_upsample.conv", co, co, 3)
    norm(p, d + "norm_out", prev)
    cconv(d + "conv_out", prev, 3, 3)
    cconv("post_quant_conv", Z_CHANNELS, Z_CHANNELS, 1)
    return p


def synth_state_dict(seed: int = 0, hidden_size: int = 128) -> Dict[str, torch.Tensor]:
    """Deterministic random decoder weights with the reference's names (vae_blocks.synth_weights: bf16-representable fp32, norm
    scales 1 + N(0, 0.1), norm shifts N(0, 0.1)): no checkpoint can be fetched here."""
    return synth_weights(decoder_param_shapes(hidden_size), torch.Generator().manual_seed(seed))
