"""Plain-torch restatement of the Open-Sora-Plan v1.2 transformer forward (reference
videosys/models/transformers/open_sora_plan_v120_transformer_3d.py: OpenSoraT2V.forward :1734-2016, BasicTransformerBlock.forward
:1322-1455, AttnProcessor2_0.__call__ :837-961, RoPE3D :63-118, PatchEmbed2D :245-369) on the CPU, in a dtype the caller chooses —
TEST INFRASTRUCTURE, imported the way tests/numerics.py and tests/vchitect_ref.py are.  PINNED: tests/test_osp_cpu.py holds its
float64 run against the float64 output of the reference's own class (tests/golden/osp_v120_fwd_small.pt, written by
tools/mint_osp_v120.py) to 1e-9 of the output's magnitude, with and without PAB.

Only the configuration the HIP model builds is restated: ada_norm_single, use_rope, gelu-approximate, no downsampler, patch_size_t 1,
no norm affine, biased projections, no image joint training.  The RoPE tables are INPUTS (per-token [tokens, head_dim], as the
kernels take them); ``rope_tables`` restates how the reference makes them."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def cos_sin_1d(D: int, seq_len: int, dtype, interpolation_scale=1.0):
    """RoPE3D.get_cos_sin (:73-82): the angles are made in fp32, cast to ``dtype`` BEFORE cos / sin (so a bf16 run takes the cosine of
    bf16-rounded angles), the position divided by the interpolation scale."""
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    t = torch.arange(seq_len, dtype=inv_freq.dtype) / interpolation_scale
    freqs = torch.einsum("i,j->ij", t, inv_freq).to(dtype)
    freqs = torch.cat((freqs, freqs), dim=-1)
    return freqs.cos(), freqs.sin()


def rope_tables(T: int, H: int, W: int, head_dim: int, dtype, interpolation_scale_thw=(1.0, 1.0, 1.0)):
    """(cos, sin) [T*H*W, head_dim] in ``dtype``: PositionGetter3D (:39-60, tokens ordered (t, h, w)) + the three embedding lookups
    of RoPE3D.forward (:109-117) concatenated along the head columns (frame | row | column chunk).  The reference caches a table
    under its LENGTH, not its scale (:74), and asks for frame, row, column in that order: an axis as long as an earlier one gets the
    earlier one's table.  Restated as such (a fresh module's first forward); pinned by the fixture's ``scaled`` case."""
    D = head_dim // 3
    pos = torch.cartesian_prod(torch.arange(T), torch.arange(H), torch.arange(W)).reshape(T * H * W, 3)
    cs, sn, cache = [], [], {}
    for axis, n in enumerate((T, H, W)):
        if n not in cache:          # RoPE3D.cache is keyed (D, seq_len, device, dtype): no scale in the key (:74)
            cache[n] = cos_sin_1d(D, n, dtype, interpolation_scale_thw[axis])
        c, s = cache[n]
        cs.append(F.embedding(pos[:, axis], c))
        sn.append(F.embedding(pos[:, axis], s))
    return torch.cat(cs, dim=-1), torch.cat(sn, dim=-1)


def rotate_half_chunks(x, nchunk=3):
    """RoPE3D.rotate_half (:85-87) inside each of the three chunks of the last dimension."""
    out = []
    for c in x.chunk(nchunk, dim=-1):
        x1, x2 = c[..., : c.shape[-1] // 2], c[..., c.shape[-1] // 2:]
        out.append(torch.cat((-x2, x1), dim=-1))
    return torch.cat(out, dim=-1)


def apply_rope(x, cos, sin):
    """RoPE3D.forward on x [B, H, N, D] with per-token tables [N, D]: (tokens * cos) + (rotate_half(tokens) * sin), every operation
    in x's dtype (:95)."""
    c, s = cos.to(x.dtype)[None, None], sin.to(x.dtype)[None, None]
    return (x * c) + (rotate_half_chunks(x) * s)


def timestep_proj(timestep, dim=256):
    """diffusers Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0): fp32 [cos | sin]."""
    half = dim // 2
    exponent = -math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half
    emb = timestep[:, None].float() * torch.exp(exponent)[None, :]
    return torch.cat([torch.cos(emb), torch.sin(emb)], dim=-1)


def _heads(x, H):
    B, N, C = x.shape
    return x.view(B, N, H, C // H).transpose(1, 2)


def attention(q, k, v, H, bias=None, cos=None, sin=None):
    """AttnProcessor2_0 from the projected tensors on: heads split, RoPE3D on q and k, F.scaled_dot_product_attention with the
    additive bias [B, 1, 1, Lk] (or none), heads merged."""
    B, N, C = q.shape
    q, k, v = _heads(q, H), _heads(k, H), _heads(v, H)
    if cos is not None:
        q, k = apply_rope(q, cos, sin), apply_rope(k, cos, sin)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias, dropout_p=0.0, is_causal=False)
    return o.transpose(1, 2).reshape(B, N, C).to(q.dtype)


def forward(sd, cfg, x, timestep, enc, enc_mask, cos, sin, dtype, cache=None, broadcast=(False, False)):
    """OpenSoraT2V.forward in ``dtype``.  sd: the reference's state dict (any float dtype); cfg: the constructor kwargs; x
    [B, Cin, T, H, W]; timestep [B]; enc [B, 1, L, caption_channels]; enc_mask [B, 1, L] (1 = visible) or None; cos / sin the
    per-token tables.  ``cache`` (a dict) receives every block's un-gated attn1 output and attn2 output, as the reference keeps them
    under PAB (:1372-1373,1418-1419); ``broadcast`` = (spatial, cross): take them from ``cache`` instead of computing (:1353-1355,
    :1390-1392).  Returns [B, out_channels, T, H, W] in ``dtype``."""
    w = {k: v.to(dtype) for k, v in sd.items()}
    lin = lambda t, name: F.linear(t, w[name + ".weight"], w[name + ".bias"])
    Hn, hd, p = cfg["num_attention_heads"], cfg["attention_head_dim"], cfg["patch_size"]
    C = Hn * hd
    eps = cfg.get("norm_eps", 1e-5)
    cout = cfg.get("out_channels") or cfg["in_channels"]
    B, cin, T, Hh, Ww = x.shape
    gh, gw = Hh // p, Ww // p
    # PatchEmbed2D (use_abs_pos = False under RoPE): Conv2d(k = s = p) per frame, tokens ordered (t, h, w)
    lat = x.to(dtype).permute(0, 2, 1, 3, 4).reshape(B * T, cin, Hh, Ww)
    lat = F.conv2d(lat, w["pos_embed.proj.weight"], w["pos_embed.proj.bias"], stride=p)
    h = lat.flatten(2).transpose(1, 2).reshape(B, T * gh * gw, C)
    # AdaLayerNormSingle
    proj = timestep_proj(timestep).to(dtype)
    emb = lin(F.silu(lin(proj, "adaln_single.emb.timestep_embedder.linear_1")), "adaln_single.emb.timestep_embedder.linear_2")
    t6 = lin(F.silu(emb), "adaln_single.linear")
    # PixArtAlphaTextProjection
    y = lin(F.gelu(lin(enc.to(dtype), "caption_projection.linear_1"), approximate="tanh"), "caption_projection.linear_2")[:, 0]
    bias = None
    if enc_mask is not None:
        bias = ((1 - enc_mask.to(dtype)) * -10000.0)[:, None]          # [B, 1, 1, L]
        if not torch.any(bias.bool()):
            bias = None
    for i in range(cfg["num_layers"]):
        pre = f"transformer_blocks.{i}"
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = (w[pre + ".scale_shift_table"][None] + t6.reshape(B, 6, -1)).chunk(6, dim=1)
        if broadcast[0]:
            a = cache[(i, "spatial")]
        else:
            n = F.layer_norm(h, (C,), eps=eps) * (1 + sc_a) + sh_a
            a = attention(lin(n, pre + ".attn1.to_q"), lin(n, pre + ".attn1.to_k"), lin(n, pre + ".attn1.to_v"), Hn, None, cos, sin)
            a = lin(a, pre + ".attn1.to_out.0")
            if cache is not None:
                cache[(i, "spatial")] = a
        h = g_a * a + h
        if broadcast[1]:
            a = cache[(i, "cross")]
        else:
            a = attention(lin(h, pre + ".attn2.to_q"), lin(y, pre + ".attn2.to_k"), lin(y, pre + ".attn2.to_v"), Hn, bias)
            a = lin(a, pre + ".attn2.to_out.0")
            if cache is not None:
                cache[(i, "cross")] = a
        h = a + h
        n = F.layer_norm(h, (C,), eps=eps) * (1 + sc_m) + sh_m
        f = lin(F.gelu(lin(n, pre + ".ff.net.0.proj"), approximate="tanh"), pre + ".ff.net.2")
        h = g_m * f + h
    shift, scale = (w["scale_shift_table"][None] + emb[:, None]).chunk(2, dim=1)
    h = F.layer_norm(h, (C,), eps=1e-6) * (1 + scale) + shift
    h = lin(h, "proj_out")
    h = h.reshape(B, T, gh, gw, 1, p, p, cout)
    h = torch.einsum("nthwopqc->nctohpwq", h)
    return h.reshape(B, cout, T, gh * p, gw * p)
