"""Host-side building blocks shared by the five VAE decoders (vae_open_sora.py, vae_svd_temporal.py, vae_sd3.py, vae_cogvideox.py,
vae_open_sora_plan.py): the model modules describe their networks on top of these and own nothing of the list below.

  * weight holders: ``_Conv`` / ``_Norm`` / ``_Res`` (weight matrices in the layout of the implicit-GEMM convolution), ``AttnWeights``
    (single-head mid-block attention with the value bias folded into the output bias), ``Decoder2DWeights`` (the diffusers 2-D decoder);
  * ``StagingCache``: the zero-bordered conv-input buffers kept per geometry; ``VaeBlocks`` on top of it: GroupNorm + SiLU into such a
    buffer, the residual block, the per-frame attention and the body of the diffusers 2-D decoder;
  * ``attention_core``: q / k GEMMs, batched V^T, chunked fp32 scores, row softmax, P V^T and the out-projection with the residual;
  * ``stitch_tiles``: the in-place cross-fade and crop of a grid of decoded tiles;
  * ``deal_units`` / ``gather_units`` / ``frame_shards``: who decodes what when the ranks of a group share one decode, and the one
    all-gather that hands every rank every unit;
  * ``synth_weights`` and the parameter-inventory helpers behind every module's ``synth_state_dict`` / ``*_param_shapes``.

Kernels are the ones of csrc/conv_bf16.hip and csrc/vae_ops.hip through ops.py; there is no CPU path."""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .ops import VaeGrid


# ---------------------------------------------------------------------------------------------------- weight holders
def _conv_w(w: torch.Tensor, n_pad: Optional[int] = None, k_pad: Optional[int] = None) -> torch.Tensor:
    """[Cout, Cin, (kt,) kh, kw] -> bf16 [Cout(+pad), taps*Cin(+pad)] with k = tap*Cin + c."""
    co = w.shape[0]
    if w.dim() == 5:
        m = w.permute(0, 2, 3, 4, 1).reshape(co, -1)
    else:
        m = w.permute(0, 2, 3, 1).reshape(co, -1)
    n_pad = n_pad or co
    k_pad = k_pad or m.shape[1]
    out = torch.zeros(n_pad, k_pad, dtype=torch.bfloat16, device=w.device)
    out[:co, :m.shape[1]] = m.to(torch.bfloat16)
    return out.contiguous()


def _vec(v: Optional[torch.Tensor], n_pad: Optional[int] = None) -> Optional[torch.Tensor]:
    if v is None:
        return None
    n_pad = n_pad or v.numel()
    out = torch.zeros(n_pad, dtype=torch.bfloat16, device=v.device)
    out[:v.numel()] = v.to(torch.bfloat16)
    return out


class _Conv:
    """One convolution under state-dict key ``key``: weight matrix, bias, geometry (cin, temporal taps, spatial kernel).  ``cin_pad``:
    zero input channels up to that count (an activation held in a wider row), ``n_pad``: zero output rows up to the GEMM tile."""

    def __init__(self, sd, key, dev, n_pad=None, cin_pad=None):
        w = sd[key + ".weight"].to(dev)
        if cin_pad is not None and w.shape[1] < cin_pad:
            w = torch.cat([w, torch.zeros(w.shape[0], cin_pad - w.shape[1], *w.shape[2:], dtype=w.dtype, device=dev)], 1)
        self.key = key
        self.kt = w.shape[2] if w.dim() == 5 else 1
        self.ks = w.shape[-1]
        self.cin, self.cout = w.shape[1], w.shape[0]
        self.w = _conv_w(w, n_pad)
        b = sd.get(key + ".bias")
        self.b = _vec(b.to(dev), n_pad) if b is not None else None


class _Norm:
    def __init__(self, sd, prefix, dev, eps):
        self.g = sd[prefix + ".weight"].to(dev).to(torch.bfloat16).contiguous()
        self.b = sd[prefix + ".bias"].to(dev).to(torch.bfloat16).contiguous()
        self.eps = eps


class _Res:
    """norm1 -> SiLU -> conv1 -> norm2 -> SiLU -> conv2 (+ shortcut): ResBlock (autoencoder_kl_open_sora.py:127-164, GroupNorm
    eps 1e-5, bias-free causal 3x3x3 convs, ``conv3``) and diffusers ResnetBlock2D (eps 1e-6, ``conv_shortcut``)."""

    def __init__(self, sd, prefix, dev, three_d):
        sub = ".conv" if three_d else ""
        eps = 1e-5 if three_d else 1e-6
        self.n1 = _Norm(sd, prefix + ".norm1", dev, eps)
        self.c1 = _Conv(sd, prefix + ".conv1" + sub, dev)
        self.n2 = _Norm(sd, prefix + ".norm2", dev, eps)
        self.c2 = _Conv(sd, prefix + ".conv2" + sub, dev)
        sk = prefix + (".conv3.conv" if three_d else ".conv_shortcut")
        self.sc = _Conv(sd, sk, dev) if (sk + ".weight") in sd else None


class AttnWeights:
    """The single-head mid-block attention: norm, wq / bq, wk / bk, wv, wo and the folded bo.  Softmax rows sum to 1, so the value bias
    passes through the attention: P (V + 1 b_v^T) = P V + b_v; it is folded into the output projection's bias (the transposed
    V^T = W_v X^T product has no per-column bias slot).  ``wo`` / ``bv`` are bf16 as the kernels see them, ``bo`` as the caller holds it."""

    def __init__(self, norm, wq, bq, wk, bk, wv, bv, wo, bo):
        self.norm, self.wq, self.bq, self.wk, self.bk, self.wv, self.wo = norm, wq, bq, wk, bk, wv, wo
        self.bo = (bo.float() + wo.float() @ bv.float()).to(torch.bfloat16)
        self.C = wq.shape[1]

    @classmethod
    def from_linear(cls, sd, a, dev):
        """diffusers ``Attention`` under key prefix ``a`` (``group_norm``, ``to_q``, ``to_k``, ``to_v``, ``to_out.0``)."""
        bf = lambda k: sd[k].to(dev).to(torch.bfloat16).contiguous()
        return cls(_Norm(sd, a + "group_norm", dev, 1e-6), bf(a + "to_q.weight"), bf(a + "to_q.bias"), bf(a + "to_k.weight"),
                   bf(a + "to_k.bias"), bf(a + "to_v.weight"), bf(a + "to_v.bias"), bf(a + "to_out.0.weight"),
                   sd[a + "to_out.0.bias"].to(dev))

    @classmethod
    def from_convs(cls, norm, q, k, v, o):
        """1x1x1 convolutions held as ``w`` / ``b`` pairs (AttnBlock3DFix)."""
        return cls(norm, q.w, q.b, k.w, k.b, v.w, v.b, o.w, o.b)


class Decoder2DWeights:
    """diffusers ``Decoder`` under key prefix ``prefix`` (``...decoder.``) between conv_in and the pixels: ``mid`` (two blocks), ``attn``,
    ``up`` = [(res blocks, upsampler conv or None)], ``norm_out``, ``conv_out`` padded to the 128-column tile.  ``res(key)`` builds one
    block's weights (default: ResnetBlock2D)."""

    def __init__(self, sd, prefix, dev, res: Optional[Callable] = None):
        d = prefix
        res = res or (lambda key: _Res(sd, key, dev, False))
        self.mid = [res(f"{d}mid_block.resnets.{i}") for i in range(2)]
        self.attn = AttnWeights.from_linear(sd, d + "mid_block.attentions.0.", dev)
        self.up = []
        for i in range(4):
            blocks = [res(f"{d}up_blocks.{i}.resnets.{j}") for j in range(3)]
            upk = f"{d}up_blocks.{i}.upsamplers.0.conv"
            self.up.append((blocks, _Conv(sd, upk, dev) if (upk + ".weight") in sd else None))
        self.norm_out = _Norm(sd, d + "conv_norm_out", dev, 1e-6)
        self.conv_out = _Conv(sd, d + "conv_out", dev, n_pad=128)


# ---------------------------------------------------------------------------------------------------- launches
def attention_core(hn, xd, n: int, L: int, Lp: int, C: int, w: AttnWeights):
    """Single-head attention of width C over n frames of L tokens, each frame in Lp rows (Lp = L rounded up to the 128-column GEMM
    tile; the pad rows of ``hn`` and ``xd`` are zero).  hn: the normed rows, xd: the residual rows -> rows [n * Lp, C]
    (pad rows: finite junk)."""
    dev = hn.device
    q = ops.gemm128(hn, w.wq, w.bq)
    k = ops.gemm128(hn, w.wk, w.bk)
    vt = torch.empty(n, C, Lp, dtype=torch.bfloat16, device=dev)       # V^T per frame = W_v X^T (pad columns = 0)
    ops.gemm128(w.wv, hn.view(n, Lp, C), out=vt, batch=n, batch_a=0, batch_w=Lp * C, batch_o=C * Lp, M=C)
    o = torch.empty(n * Lp, C, dtype=torch.bfloat16, device=dev)
    L4 = (L + 3) // 4 * 4
    step = max(1, min(n, (1 << 28) // (Lp * Lp)))                       # <= 1 GiB of fp32 scores at a time
    for f in range(0, n, step):
        m = min(step, n - f)
        s = torch.empty(m, Lp, Lp, dtype=torch.float32, device=dev)
        ops.gemm128(q[f * Lp:(f + m) * Lp].view(m, Lp, C), k[f * Lp:(f + m) * Lp].view(m, Lp, C), out_f32=s,
                    out_scale=1.0 / math.sqrt(C), batch=m, batch_a=Lp * C, batch_w=Lp * C, batch_o=Lp * Lp, M=Lp)
        if L4 != L:    # the softmax kernel counts keys in fours: a key count like 3 x 2 (an edge tile) masks its last columns
            s[:, :, L:L4] = -3.0e38
        p = ops.softmax_rows(s, n=L4)
        ops.gemm128(p, vt[f:f + m], out=o[f * Lp:(f + m) * Lp].view(m, Lp, C), batch=m, batch_a=Lp * Lp, batch_w=C * Lp,
                    batch_o=Lp * C, M=Lp)
    return ops.gemm128(o, w.wo, w.bo, res=xd)


def stitch_tiles(rows, ext_h: int, ext_w: int, lim_h: int, lim_w: int) -> torch.Tensor:
    """``rows[i][j]``: decoded planar tiles [C, T, h, w] of overlapping latent tiles -> the stitched frames.  Every tile is cross-faded
    over ``ext_h`` rows with the tile above, then over ``ext_w`` columns with the tile to its left, IN PLACE — so later tiles see the
    blended neighbours, as blend_v / blend_h do in the references' tiled decodes — and cropped to (lim_h, lim_w)."""
    out_rows = []
    for i, row in enumerate(rows):
        res = []
        for j, tile in enumerate(row):
            if i > 0:
                a = rows[i - 1][j]
                ops.blend_edge(a, tile, min(a.shape[-2], tile.shape[-2], ext_h), 0)
            if j > 0:
                a = row[j - 1]
                ops.blend_edge(a, tile, min(a.shape[-1], tile.shape[-1], ext_w), 1)
            res.append(tile[:, :, :lim_h, :lim_w])
        out_rows.append(torch.cat(res, dim=3))
    return torch.cat(out_rows, dim=2)


# ---------------------------------------------------------------------------------------------------- decode shared by a group
def deal_units(costs, P):
    """Which rank decodes which unit (a tile, a chunk of a tile): largest cost first, each to the rank with the least cost so far, ties
    to the lower index (the ragged last row and column of tiles are a fraction of a full tile: dealt r, r + P, ... the 3 x 3 tiles of
    CogVideoX config 5 give one of four ranks 2 880 of 7 560 latent pixels; this way the busiest has 1 980).  Deterministic: every
    rank computes the same table.  Returns (owner[u], slot[u], units per rank)."""
    load, count = [0] * P, [0] * P
    owner, slot = [0] * len(costs), [0] * len(costs)
    for u in sorted(range(len(costs)), key=lambda k: (-costs[k], k)):
        r = min(range(P), key=lambda q: (load[q], q))
        owner[u], slot[u] = r, count[r]
        load[r] += costs[u]
        count[r] += 1
    return owner, slot, max(count) if count else 0


def gather_units(mine, owner, slot, per, pad_shape, group, device, shapes):
    """``mine[u]``: the decoded tensor of every unit this rank owns (``deal_units``) -> the list of ALL units on every rank, after ONE
    all-gather of a zeroed bf16 [per, *pad_shape] buffer per rank that holds unit u in the leading corner of slot ``slot[u]``.
    ``shapes[u]``: unit u's own shape (every rank derives it from the geometry without decoding; no header gather), to which it is
    cropped back; the returned tensors are contiguous copies, so they can be blended in place."""
    from . import dsp

    P = dsp.group_size(group)
    buf = torch.zeros((per,) + tuple(pad_shape), dtype=torch.bfloat16, device=device)
    for u, t in mine.items():
        assert tuple(t.shape) == tuple(shapes[u]) and all(a <= b for a, b in zip(t.shape, pad_shape)), (u, tuple(t.shape), pad_shape)
        buf[slot[u]][tuple(slice(0, s) for s in t.shape)] = t
    allb = torch.empty((P * per,) + tuple(pad_shape), dtype=torch.bfloat16, device=device)
    dsp.all_gather_into_tensor(allb, buf, group)
    return [allb[owner[u] * per + slot[u]][tuple(slice(0, s) for s in shp)].contiguous() for u, shp in enumerate(shapes)]


def frame_shards(F: int, P: int):
    """Contiguous frame ranges [(f0, f1)] of ceil(F / P) frames, one per rank; empty (F, F) for the ranks past the end."""
    per = -(-F // P)
    return [(min(r * per, F), min((r + 1) * per, F)) for r in range(P)]


class StagingCache:
    """``device`` and the zero-bordered staging buffers, kept per geometry.  The constructor refuses anything but a HIP device."""

    def __init__(self, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"videosys_amd.{type(self).__name__} needs a HIP device (no CPU path)")
        self.device = dev
        self._padded: Dict[tuple, tuple] = {}

    def clear_cache(self):
        """Drop the zero-bordered staging buffers (they are kept per geometry; call after changing resolution to free HBM)."""
        self._padded.clear()

    def _padded_buf(self, g: VaeGrid, C: int):
        """Zero-bordered conv-input buffer for grid g, allocated once per geometry (kernels only ever write its interior)."""
        key = (g.n, g.T, g.H, g.W, g.tf, C)
        hit = self._padded.get(key)
        if hit is None:
            hit = g.alloc(C, self.device, zero=True)
            self._padded[key] = hit
        return hit[1]


class VaeBlocks(StagingCache):
    """The blocks a GroupNorm / conv / single-head-attention decoder is made of, over channels-last rows on a ``VaeGrid``."""

    def _attn_bufs(self, n, H, W, C, Lp):
        """The normed-rows and residual-rows buffers of the attention, [n * Lp, C] each: the pad rows must be zero (and stay zero:
        kernels write the L interior rows only)."""
        key = ("attn", n, H, W)
        bufs = self._padded.get(key)
        if bufs is None:
            bufs = (torch.zeros(n * Lp, C, dtype=torch.bfloat16, device=self.device),
                    torch.zeros(n * Lp, C, dtype=torch.bfloat16, device=self.device))
            self._padded[key] = bufs
        return bufs

    def _norm_act(self, x, gx: VaeGrid, norm, C: int, tf: int, silu=True, dense=False):
        gd = VaeGrid(gx.n, gx.T, gx.H, gx.W, 0 if dense else 1, 0 if dense else tf)
        y = torch.empty(gd.rows, C, dtype=torch.bfloat16, device=self.device) if dense else self._padded_buf(gd, C)
        ops.group_norm(x, gx, y, gd, C, norm.g, norm.b, norm.eps, silu)
        return y, gd

    def _resblock(self, x, gx: VaeGrid, r):
        """x rows over gx (any layout) -> rows over the conv-output grid (pad 1, tf 0).  ``r``: n1 / c1 / n2 / c2 / sc holders."""
        tf = r.c1.kt - 1
        h, gh = self._norm_act(x, gx, r.n1, r.c1.cin, tf)
        y = ops.conv(h, gh, r.c1.w, r.c1.b, r.c1.cin, r.c1.kt, r.c1.ks)
        go = gh.conv_out()
        h2, gh2 = self._norm_act(y, go, r.n2, r.c2.cin, tf)
        if gx.pad != 1 or gx.tf != 0:   # the residual is added row-for-row in the conv-output layout
            xr = torch.empty(go.rows, x.shape[1], dtype=torch.bfloat16, device=self.device)
            ops.regrid(x, gx, xr, go, x.shape[1])
            x = xr
        res = x
        if r.sc is not None:
            res = ops.gemm128(x, r.sc.w, r.sc.b)
        out = ops.conv(h2, gh2, r.c2.w, r.c2.b, r.c2.cin, r.c2.kt, r.c2.ks, res=res)
        return out, go

    def _attention(self, x, g: VaeGrid, aw: AttnWeights):
        """diffusers Attention (1 head, d = C) with residual, GroupNorm per frame; x rows over g -> dense rows whose per-frame stride
        is the token count rounded up to the 128-column GEMM tile (pad rows are zero on input, finite junk on output)."""
        C, L, n = aw.C, g.H * g.W, g.n
        Lp = (L + 127) // 128 * 128
        gdn = VaeGrid(n, 1, g.H, g.W, 0, 0, sample_rows=Lp)
        hn, xd = self._attn_bufs(n, g.H, g.W, C, Lp)
        ops.group_norm(x, g, hn, gdn, C, aw.norm.g, aw.norm.b, aw.norm.eps, False)
        ops.regrid(x, g, xd, gdn, C)
        return attention_core(hn, xd, n, L, Lp, C, aw), gdn

    def _decoder2d(self, x, g: VaeGrid, w: Decoder2DWeights, res_fn: Optional[Callable] = None):
        """The diffusers 2-D decoder from the rows after conv_in to (conv_out rows [rows, 128], their grid): mid block with attention,
        four up blocks (nearest 2x regrid + 3x3 conv between them), GroupNorm + SiLU, conv_out.  ``res_fn(x, g, block)``: the
        residual block (default ``_resblock``)."""
        res_fn = res_fn or self._resblock
        x, g = res_fn(x, g, w.mid[0])
        x, g = self._attention(x, g, w.attn)
        x, g = res_fn(x, g, w.mid[1])
        for blocks, up in w.up:
            for r in blocks:
                x, g = res_fn(x, g, r)
            if up is not None:
                gp = VaeGrid(g.n, 1, 2 * g.H, 2 * g.W, 1, 0)
                xp = self._padded_buf(gp, up.cin)
                ops.regrid(x, g, xp, gp, up.cin, up=1)
                x = ops.conv(xp, gp, up.w, up.b, up.cin, 1, 3)
                g = gp.conv_out()
        h, gh = self._norm_act(x, g, w.norm_out, 128, 0)
        return ops.conv(h, gh, w.conv_out.w, w.conv_out.b, 128, 1, 3), gh.conv_out()


# ---------------------------------------------------------------------------------------------------- synthetic weights, inventories
def synth_weights(shapes: Dict[str, tuple], g: torch.Generator, rules: Sequence[Tuple[str, Callable]] = ()) -> Dict[str, torch.Tensor]:
    """Deterministic random weights (bf16-representable fp32), ONE ``randn`` draw per key in the inventory's order: conv / linear
    weights N(0, 1/fan_in), norm scales 1 + N(0, 0.1), norm shifts N(0, 0.1), other biases N(0, 0.02).  ``rules``: a model's own
    (substring of the key, fn(draw, fan_in)) pairs, looked at first."""
    sd = {}
    for k, shp in shapes.items():
        r = torch.randn(shp, generator=g)
        fan_in = 1
        for s in shp[1:]:
            fan_in *= s
        is_norm = ".norm" in k or "group_norm" in k or "conv_norm_out" in k
        own = next((fn for needle, fn in rules if needle in k), None)
        if own is not None:
            v = own(r, fan_in)
        elif k.endswith(".weight") and len(shp) >= 2:
            v = r / math.sqrt(fan_in)
        elif k.endswith(".weight") and is_norm:
            v = 1.0 + 0.1 * r
        elif is_norm:
            v = 0.1 * r
        else:
            v = 0.02 * r
        sd[k] = v.to(torch.bfloat16).float()
    return sd


def norm(p, name, c):
    p[name + ".weight"] = (c,)
    p[name + ".bias"] = (c,)


def conv2(p, name, ci, co, k):
    p[name + ".weight"] = (co, ci, k, k)
    p[name + ".bias"] = (co,)


def res2(p, name, ci, co):
    norm(p, name + ".norm1", ci); conv2(p, name + ".conv1", ci, co, 3)
    norm(p, name + ".norm2", co); conv2(p, name + ".conv2", co, co, 3)
    if ci != co:
        conv2(p, name + ".conv_shortcut", ci, co, 1)


def conv3(p, name, ci, co, k, bias=True):
    """``name.conv.*`` of a causal 3-D convolution; k: one size or (kt, kh, kw)."""
    p[name + ".conv.weight"] = (co, ci) + (k if isinstance(k, tuple) else (k, k, k))
    if bias:
        p[name + ".conv.bias"] = (co,)


def res3(p, name, ci, co):
    norm(p, name + ".norm1", ci); conv3(p, name + ".conv1", ci, co, 3, False)
    norm(p, name + ".norm2", co); conv3(p, name + ".conv2", co, co, 3, False)
    if ci != co:
        conv3(p, name + ".conv3", ci, co, 1, False)


def diffusers_decoder_shapes(prefix: str, latent_channels: int, block_out_channels=(128, 256, 512, 512), res: Callable = res2) -> Dict[str, tuple]:
    """Names and shapes of diffusers' ``Decoder`` (layers_per_block 2) under ``prefix``, in state-dict order; ``res(p, name, ci, co)``
    lists one residual block (default ResnetBlock2D)."""
    p: Dict[str, tuple] = {}
    d, top = prefix, block_out_channels[-1]
    conv2(p, d + "conv_in", latent_channels, top, 3)
    res(p, d + "mid_block.resnets.0", top, top)
    a = d + "mid_block.attentions.0."
    norm(p, a + "group_norm", top)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        p[a + n + ".weight"] = (top, top)
        p[a + n + ".bias"] = (top,)
    res(p, d + "mid_block.resnets.1", top, top)
    prev = top
    for i, co in enumerate(reversed(block_out_channels)):
        for j in range(3):
            res(p, f"{d}up_blocks.{i}.resnets.{j}", prev, co)
            prev = co
        if i < 3:
            conv2(p, f"{d}up_blocks.{i}.upsamplers.0.conv", co, co, 3)
    norm(p, d + "conv_norm_out", block_out_channels[0])
    conv2(p, d + "conv_out", block_out_channels[0], 3, 3)
    return p
