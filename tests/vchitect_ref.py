"""float64 restatement of VchitectAttnProcessor (reference videosys/models/modules/attentions.py:641-949) in plain torch on the CPU —
TEST INFRASTRUCTURE for tests/test_gpu_vchitect_attention.py, imported the way tests/numerics.py is.  It follows the reference line
by line from the PROJECTED tensors on (the q / k / v the Linear layers produced; the projections themselves are the GEMM family's
tests), on bf16-exact inputs widened to float64.  PINNED: tests/test_vchitect_pinned_cpu.py holds attention_layer, block_forward and
model_forward — in the pipeline's call form (B = 1, one text row), at one frame, on a rectangular latent, at B = 2 with one frame, and
over eight calls under PAB (PabState) — to float64 runs of the reference's own JointTransformerBlock and VchitectXLTransformerModel
(tests/golden/vchitect_{fwd,pab,layer}_small.pt, tools/mint_vchitect.py), within the class's own fp32-to-float64 distance.  What
stays a reading of the class: B > 1 with more than one frame, which the class cannot execute (its norm_out does not broadcast);
model_forward's norm_out at that shape is this project's extension.

Shapes.  B samples, T frames, S video tokens and L text tokens per frame, H heads of 64.  Video tensors [B*T, S, H*64] and text
tensors [B*T, L, H*64], rows ordered (b, t) as the reference's `(B T)` batch."""
from __future__ import annotations

import torch

HD = 64
THETA = 1e6


def rope_tables(T: int, theta: float = THETA, scaling: float = 1.0):
    """cos / sin fp32 [T, 32] of precompute_freqs_cis (vchitect_transformer_3d.py:341-347): freqs_cis = polar(1, t theta^(-2i/64)),
    every step in fp32 as there."""
    freqs = 1.0 / (theta ** (torch.arange(0, HD, 2)[: HD // 2].float() / HD))
    t = torch.arange(T, dtype=torch.float) / scaling
    ang = torch.outer(t, freqs).float()
    cis = torch.polar(torch.ones_like(ang), ang)
    return cis.real.contiguous(), cis.imag.contiguous()


def apply_rotary(x, cos, sin):
    """apply_rotary_emb (:654-665) on x [..., T, H, 64] with cos / sin [T, 32]: view_as_complex(x) * freqs_cis, unrounded."""
    a, b = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    c, s = cos[:, None, :].to(x), sin[:, None, :].to(x)
    return torch.stack((a * c - b * s, a * s + b * c), dim=-1).flatten(-2)


def rotary_error(x, cos, sin):
    """Worst-case error of the bf16 result of apply_rotary computed in fp32 (two products and one sum per value, one bf16 rounding),
    as tests/test_gpu_numerics_attention.py::q_chain64 writes it: acc(2, |a c| + |b s|) + rnd(result)."""
    import numerics as nm

    a, b = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    c, s = cos[:, None, :].to(x).abs(), sin[:, None, :].to(x).abs()
    mag = torch.stack((a.abs() * c + b.abs() * s, a.abs() * s + b.abs() * c), dim=-1).flatten(-2)
    return nm.acc(2, mag) + nm.rnd(apply_rotary(x, cos, sin))


def sdpa(q, k, v):
    """F.scaled_dot_product_attention on [..., heads, L, 64] in the dtype given (float64 here)."""
    w = torch.softmax((q @ k.transpose(-1, -2)) * HD**-0.5, dim=-1)
    return w @ v


def temporal_tokens(x_vid, x_txt, B, T, H):
    """`cat([x, encoder_x], dim=1)` then `(B T) S H C -> (B S) T H C` (:723-737): [B * (S + L), T, H, 64]."""
    x = torch.cat([x_vid, x_txt], dim=1)
    SL = x.shape[1]
    return x.view(B, T, SL, H, HD).permute(0, 2, 1, 3, 4).reshape(B * SL, T, H, HD)


def temporal_attention(q_vid, k_vid, v_vid, q_txt, k_txt, v_txt, cos, sin, B, T, H, round_rope=True):
    """temporal_attention (:705-764) without to_*_temp / to_out_temporal: returns (video [B*T, S, C], text [B*T, L, C]).
    round_rope: the rotated q / k are cast back to bf16 (`type_as`, :665) as in the reference's bf16 run."""
    S = q_vid.shape[1]
    q, k, v = (temporal_tokens(a, b, B, T, H) for a, b in ((q_vid, q_txt), (k_vid, k_txt), (v_vid, v_txt)))
    if cos is not None:
        q, k = apply_rotary(q, cos, sin), apply_rotary(k, cos, sin)
        if round_rope:
            q, k = q.to(torch.bfloat16).to(v.dtype), k.to(torch.bfloat16).to(v.dtype)
    o = sdpa(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)          # [(B S'), T, H, 64]
    SL = o.shape[0] // B
    o = o.reshape(B, SL, T, H * HD).permute(0, 2, 1, 3).reshape(B * T, SL, H * HD)             # `(B S) T C -> (B T) S C`
    return o[:, :S], o[:, S:]


def spatial_attention(q_vid, k_vid, v_vid, q_txt, k_txt, v_txt, H):
    """spatial_attn (:667-703) without to_q / to_k / to_v: joint attention of the S + L tokens of every frame -> [B*T, S + L, C]."""
    q, k, v = (torch.cat([a, b], dim=1) for a, b in ((q_vid, q_txt), (k_vid, k_txt), (v_vid, v_txt)))
    n, SL = q.shape[:2]
    heads = lambda x: x.view(n, SL, H, HD).transpose(1, 2)
    return sdpa(heads(q), heads(k), heads(v)).transpose(1, 2).reshape(n, SL, H * HD)


def cross_keys(k_txt, v_txt, B, H):
    """The keys of cross_attention (:781-786): frame 0 of SAMPLE 0, `[0].unsqueeze(0)`, viewed as (batchsize, -1, heads, 64) — with
    B > 1 the L text keys are dealt out in B runs of L / B (the reference's view; it needs L % B == 0).  [B, L / B, H, 64] each."""
    return k_txt[0].reshape(B, -1, H, HD), v_txt[0].reshape(B, -1, H, HD)


def cross_attention(q_vid, q_txt, k_txt, v_txt, B, T, H):
    """cross_attention (:766-800) without to_q_cross / to_out_context: every query of sample b attends cross_keys()[b]; the `(S T)`
    query order is undone by the final rearrange, so the result is [B*T, S + L, C] in the order of the queries."""
    q = torch.cat([q_vid, q_txt], dim=1)
    n, SL = q.shape[:2]
    ky, vy = cross_keys(k_txt, v_txt, B, H)
    qy = q.view(B, T, SL, H, HD).permute(0, 2, 1, 3, 4).reshape(B, SL * T, H, HD)              # `(B T) S H C -> B (S T) H C`
    o = sdpa(qy.transpose(1, 2), ky.transpose(1, 2), vy.transpose(1, 2)).transpose(1, 2).reshape(B, SL, T, H * HD)
    return o.permute(0, 2, 1, 3).reshape(n, SL, H * HD)                                        # `B (S T) C -> (B T) S C`


def combine_bf16(spatial, cross):
    """`hidden_states * 1.1 + cross_output` (:899) as the reference's bf16 run computes it: two bf16 tensor ops."""
    return spatial.to(torch.bfloat16) * 1.1 + cross.to(torch.bfloat16)


class PabState:
    """What VchitectAttention keeps between calls under PAB (attentions.py:528-534), one entry per block: the three counters and
    last_temporal = (video AFTER to_out_temporal, text raw), last_cross (after to_out_context), last_spatial (before `* 1.1`)."""

    def __init__(self, depth):
        from types import SimpleNamespace

        self.blocks = [SimpleNamespace(temporal_count=0, cross_count=0, spatial_count=0, last_temporal=None, last_cross=None, last_spatial=None,
                                       last_decisions=None) for _ in range(depth)]


def attention_layer(sd, hidden_states, encoder_hidden_states, B, T, H, context_pre_only=False, dtype=torch.float64, state=None, timestep=None):
    """VchitectAttnProcessor.__call__ (:802-926) on weights ``sd`` (VchitectAttention's names) and inputs [B*T, S, C] /
    [B*T, L, C], all computed in ``dtype``: float64 = the reference for the numerics; bfloat16 = the reference's own bf16 run on the
    CPU (nn.Linear, F.scaled_dot_product_attention and the fp32 rotation cast back, as there): its distance to the float64 run is the
    bf16 floor the HIP layer is held to.  Returns (hidden_states [B*T, S, C], encoder_hidden_states [B*T, L, C]).
    ``state`` (one entry of PabState.blocks) with ``timestep`` (`int(timestep[0])`): PAB as :839-896 — a branch whose decision
    (videosys_amd.pab, the manager set by the caller) is to broadcast takes the cached tensor, one that computes caches its result."""
    import torch.nn.functional as F

    lin = lambda x, n: F.linear(x, sd[n + ".weight"].to(dtype), sd[n + ".bias"].to(dtype))
    hs, enc = hidden_states.to(dtype), encoder_hidden_states.to(dtype)
    S = hs.shape[1]
    heads = lambda x: x.reshape(x.shape[0], -1, H, HD).transpose(1, 2)
    att = lambda q, k, v: F.scaled_dot_product_attention(q, k, v)
    eq, ek, ev = lin(enc, "add_q_proj"), lin(enc, "add_k_proj"), lin(enc, "add_v_proj")
    SL = S + enc.shape[1]
    bt = bc = bs = False
    if state is not None:
        from videosys_amd import pab

        bt, state.temporal_count = pab.if_broadcast_temporal(timestep, state.temporal_count)
    # temporal (:705-764)
    if bt:
        temp_v, temp_t = state.last_temporal
    else:
        q, k, v = (temporal_tokens(lin(hs, n), e, B, T, H) for n, e in (("to_q_temp", eq), ("to_k_temp", ek), ("to_v_temp", ev)))
        cos, sin = rope_tables(T)
        rot = lambda x: apply_rotary(x.float() if dtype != torch.float64 else x, cos, sin).to(dtype)       # xq.float() ... type_as(xq)
        o = att(rot(q).transpose(1, 2), rot(k).transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
        o = o.reshape(B, SL, T, H * HD).permute(0, 2, 1, 3).reshape(B * T, SL, H * HD)
        temp_v, temp_t = lin(o[:, :S], "to_out_temporal"), o[:, S:]
        if state is not None:
            state.last_temporal = (temp_v, temp_t)
    # cross (:766-800)
    if state is not None:
        bc, state.cross_count = pab.if_broadcast_cross(timestep, state.cross_count)
    if bc:
        cross = state.last_cross
    else:
        qc = torch.cat([lin(hs, "to_q_cross"), eq], dim=1)
        ky, vy = ek[0].unsqueeze(0).reshape(B, -1, H, HD), ev[0].unsqueeze(0).reshape(B, -1, H, HD)
        qy = qc.reshape(B, T, SL, H, HD).permute(0, 2, 1, 3, 4).reshape(B, SL * T, H, HD)
        c = att(qy.transpose(1, 2), ky.transpose(1, 2), vy.transpose(1, 2)).transpose(1, 2).reshape(B, SL, T, H * HD)
        cross = lin(c.permute(0, 2, 1, 3).reshape(B * T, SL, H * HD), "to_out_context")
        if state is not None:
            state.last_cross = cross
    # spatial (:667-703)
    if state is not None:
        bs, state.spatial_count = pab.if_broadcast_spatial(timestep, state.spatial_count)
        state.last_decisions = (bt, bc, bs)
    if bs:
        sp = state.last_spatial
    else:
        q, k, v = (torch.cat([lin(hs, n), e], dim=1) for n, e in (("to_q", eq), ("to_k", ek), ("to_v", ev)))
        sp = att(heads(q), heads(k), heads(v)).transpose(1, 2).reshape(B * T, SL, H * HD)
        if state is not None:
            state.last_spatial = sp
    h = sp * 1.1 + cross
    hv, ht = h[:, :S], h[:, S:]
    hv = lin(hv, "to_out.0")
    if T == 1:
        temp_v = temp_v * 0
    hv = hv + temp_v
    if not context_pre_only:
        ht = lin(ht, "to_add_out")
    tt = lin(temp_t, "to_add_out_temporal")
    if T == 1:
        tt = tt * 0
    return hv, ht + tt


# ------------------------------------------------------------------------------------------------ block and model
def layer_inputs(seed):
    """The bf16-exact inputs of tests/golden/vchitect_layer_small.pt (B = 1, F = 3, S = 16, L = 4, dim 192), regenerated from the seed
    the fixture records: hidden_states [3, 16, 192], encoder_hidden_states [3, 4, 192], temb [3, 192] (float32 holding bf16 values)."""
    g = torch.Generator().manual_seed(seed + 2)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    return bf(3, 16, 192), bf(3, 4, 192), bf(3, 192)


def sincos_2d(embed_dim, grid, base_size):
    """diffusers get_2d_sincos_pos_embed(embed_dim, grid, base_size=base_size): float64 [grid * grid, embed_dim] (w goes first)."""
    import numpy as np

    def one(dim, pos):
        omega = 1.0 / 10000 ** (np.arange(dim // 2, dtype=np.float64) / (dim / 2.0))
        out = np.einsum("m,d->md", pos.reshape(-1), omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)
    g = np.arange(grid, dtype=np.float32) / (grid / base_size)
    gw, gh = np.meshgrid(g, g)
    return torch.from_numpy(np.concatenate([one(embed_dim // 2, gw), one(embed_dim // 2, gh)], axis=1))


def timestep_proj(t, dim=256):
    """Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin], fp32 as diffusers computes it."""
    import math

    half = dim // 2
    e = t[:, None].float() * torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)[None]
    return torch.cat([torch.cos(e), torch.sin(e)], dim=-1)


def block_forward(sd, pre, x, y, temb, B, F, H, last, dtype=torch.float64, state=None, timestep=None):
    """JointTransformerBlock.forward (vchitect_transformer_3d.py:114-175) on the weights under prefix ``pre``: x [B*F, S, C], y [B*F, L, C],
    temb [B*F, C] -> (x, y, attention outputs); y comes back unchanged from a context_pre_only block (the reference returns None)."""
    import torch.nn.functional as Fn

    lin = lambda x, n: Fn.linear(x, sd[n + ".weight"].to(dtype), sd[n + ".bias"].to(dtype))
    ln = lambda x: Fn.layer_norm(x, x.shape[-1:], eps=1e-6)
    cur = temb
    asd = {k[len(pre) + 5:]: v for k, v in sd.items() if k.startswith(pre + "attn.")}
    sh, sc, g, sh2, sc2, g2 = lin(Fn.silu(cur), pre + "norm1.linear").chunk(6, dim=1)
    xn = ln(x) * (1 + sc[:, None]) + sh[:, None]
    if last:
        csc, csh = lin(Fn.silu(cur), pre + "norm1_context.linear").chunk(2, dim=1)
        yn = ln(y) * (1 + csc)[:, None] + csh[:, None]
    else:
        csh, csc, cg, csh2, csc2, cg2 = lin(Fn.silu(cur), pre + "norm1_context.linear").chunk(6, dim=1)
        yn = ln(y) * (1 + csc[:, None]) + csh[:, None]
    av, at = attention_layer(asd, xn, yn, B, F, H, last, dtype, state, timestep)
    x = x + g.unsqueeze(1) * av
    xn = ln(x) * (1 + sc2[:, None]) + sh2[:, None]
    ff = lin(Fn.gelu(lin(xn, pre + "ff.net.0.proj"), approximate="tanh"), pre + "ff.net.2")
    x = x + g2.unsqueeze(1) * ff
    if not last:
        y = y + cg.unsqueeze(1) * at
        yn = ln(y) * (1 + csc2[:, None]) + csh2[:, None]
        y = y + cg2.unsqueeze(1) * lin(Fn.gelu(lin(yn, pre + "ff_context.net.0.proj"), approximate="tanh"), pre + "ff_context.net.2")
    return x, y, (av, at)


def model_forward(sd, cfg, hidden_states, encoder_hidden_states, pooled, timestep, dtype=torch.float64, pab_state=None):
    """VchitectXLTransformerModel.forward (vchitect_transformer_3d.py:489-590) with JointTransformerBlock.forward (block_forward), the diffusers
    leaves restated (PatchEmbed with cropped_pos_embed, CombinedTimestepTextProjEmbeddings, AdaLayerNormZero, AdaLayerNormContinuous,
    FeedForward gelu-approximate), all in ``dtype``.  cfg: dict(num_layers, heads, patch, out_channels, sample_size, pos_embed_max_size).
    encoder_hidden_states [B*F, L, D], or [B, L, D] — the pipeline's form: every frame of a sample reads its row, which is what the
    broadcast of norm1_context over the F rows of temb does in the class at B = 1.  `cur_temb = temb.repeat(F, 1)` literally (:548);
    norm_out with the temb of each row's own sample (the reference's line broadcasts only at B = 1, where the two agree).
    ``pab_state``: a PabState kept across calls (PAB decisions of `int(timestep[0])`); None: no PAB."""
    import torch.nn.functional as Fn

    lin = lambda x, n: Fn.linear(x, sd[n + ".weight"].to(dtype), sd[n + ".bias"].to(dtype))
    ln = lambda x: Fn.layer_norm(x, x.shape[-1:], eps=1e-6)
    B, F, cin, Hh, Ww = hidden_states.shape
    p, H, depth = cfg["patch"], cfg["heads"], cfg["num_layers"]
    C = H * HD
    Hp, Wp = Hh // p, Ww // p
    if encoder_hidden_states.shape[0] == B and F > 1:
        encoder_hidden_states = encoder_hidden_states.repeat_interleave(F, dim=0)
    x = Fn.conv2d(hidden_states.reshape(B * F, cin, Hh, Ww).to(dtype), sd["pos_embed.proj.weight"].to(dtype), sd["pos_embed.proj.bias"].to(dtype),
                  stride=p).flatten(2).transpose(1, 2)
    m = cfg["pos_embed_max_size"]
    pos = sincos_2d(C, m, cfg["sample_size"] // p).float().reshape(m, m, C)
    top, left = (m - Hp) // 2, (m - Wp) // 2
    pos = pos[top:top + Hp, left:left + Wp].reshape(1, Hp * Wp, C)
    x = (x + (pos.double() if dtype == torch.float64 else pos)).to(dtype)
    te = "time_text_embed.timestep_embedder."
    tx = "time_text_embed.text_embedder."
    t_emb = lin(Fn.silu(lin(timestep_proj(timestep).to(dtype), te + "linear_1")), te + "linear_2")
    temb = t_emb + lin(Fn.silu(lin(pooled.to(dtype), tx + "linear_1")), tx + "linear_2")
    y = lin(encoder_hidden_states.to(dtype), "context_embedder")
    cur = temb.repeat(F, 1)
    for i in range(depth):
        st = None if pab_state is None else pab_state.blocks[i]
        x, y, _ = block_forward(sd, f"transformer_blocks.{i}.", x, y, cur, B, F, H, i == depth - 1, dtype, st, int(timestep[0]))
    scale, shift = lin(Fn.silu(temb), "norm_out.linear").repeat_interleave(F, dim=0).chunk(2, dim=1)
    x = lin(ln(x) * (1 + scale)[:, None] + shift[:, None], "proj_out")
    co = cfg["out_channels"]
    x = x.reshape(B * F, Hp, Wp, p, p, co)
    return torch.einsum("nhwpqc->nchpwq", x).reshape(B * F, co, Hp * p, Wp * p)
