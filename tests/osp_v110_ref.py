"""TEST INFRASTRUCTURE ONLY — plain-torch restatement of the reference's Open-Sora-Plan v1.1 LatteT2V
(videosys/models/transformers/open_sora_plan_v110_transformer_3d.py: LatteT2V.forward :2406-2765, BasicTransformerBlock.forward
:1910-2071, BasicTransformerBlock_.forward :1537-1711, AttnProcessor2_0 :1156-1267, RoPE2D / RoPE1D with linear scaling :136-253,
PatchEmbed :361-424) in a dtype the caller chooses.  It takes the reference's UN-PERMUTED weights and rotates rotate-half, exactly as
the reference does: tables from fp32 inv_freq with the angles cast to the compute dtype before cos / sin, positions divided by the
scale and truncated to integers.  tests/test_osp_v110_cpu.py holds it to the class's own float64 outputs
(tests/golden/osp_v110_fwd_small.pt, tools/mint_osp_v110.py) to 1e-9 of the output's magnitude; the GPU tests take their bf16 floor
from its float64 and bf16 runs.  The leaves (linear, layer norm, GELU-tanh feed-forward, sincos tables, timestep embedding) are those
of oracle/latte_oracle.py; PAB decisions come from videosys_amd.pab (host logic, pinned by its own tests)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.latte_oracle import feed_forward, layer_norm, linear, sincos_1d, sincos_2d, timestep_embedding


# ------------------------------------------------------------------------------------------------ RoPE
def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def cos_sin(D, positions, scale, dtype):
    """get_cos_sin (:144-153) gathered at LinearScalingRoPE*'s positions (:190-196): (cos, sin) [len, D] in ``dtype``."""
    pos = (positions.float() / scale).to(positions.dtype)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    t = torch.arange(int(pos.max()) + 1, dtype=inv_freq.dtype)
    freqs = torch.einsum("i,j->ij", t, inv_freq).to(dtype)
    freqs = torch.cat((freqs, freqs), dim=-1)
    return freqs.cos()[pos], freqs.sin()[pos]


def rope_1d(x, cos_half, sin_half):
    """x [..., L, D] rotated rotate-half with per-token angles given as their first halves [L, D / 2] (tests: any dtype)."""
    c, s = torch.cat([cos_half, cos_half], -1), torch.cat([sin_half, sin_half], -1)
    return x * c + rotate_half(x) * s


def rope_tokens_1d(x, T, scale):
    """RoPE1D.forward on x [N, H, T, 72] at positions 0 .. T - 1."""
    c, s = cos_sin(x.shape[-1], torch.arange(T), scale, x.dtype)
    return x * c + rotate_half(x) * s


def rope_tokens_2d(x, gh, gw, scale):
    """RoPE2D.forward on x [N, H, gh * gw, 72]: row half with y, column half with x; token = y * gw + x."""
    D = x.shape[-1] // 2
    y, xx = torch.arange(gh).repeat_interleave(gw), torch.arange(gw).repeat(gh)
    # ONE table for both axes in the reference: its length comes from the largest position of either axis, the entries do not
    cy, sy = cos_sin(D, y, scale, x.dtype)
    cx, sx = cos_sin(D, xx, scale, x.dtype)
    a, b = x[..., :D], x[..., D:]
    return torch.cat([a * cy + rotate_half(a) * sy, b * cx + rotate_half(b) * sx], dim=-1)


def tables_2d(gh, gw, scale, dtype=torch.bfloat16):
    """The (cos, sin) [S, 36] fp32 tables of the HIP kernels, restated from the rotate-half ones: pair p < 18 = row angle p, else column."""
    y, xx = torch.arange(gh).repeat_interleave(gw), torch.arange(gw).repeat(gh)
    cy, sy = cos_sin(36, y, scale, dtype)
    cx, sx = cos_sin(36, xx, scale, dtype)
    return torch.cat([cy[:, :18], cx[:, :18]], 1).float(), torch.cat([sy[:, :18], sx[:, :18]], 1).float()


def tables_1d(T, scale, dtype=torch.bfloat16):
    c, s = cos_sin(72, torch.arange(T), scale, dtype)
    return c[:, :36].float().repeat_interleave(2, dim=1), s[:, :36].float().repeat_interleave(2, dim=1)


# ------------------------------------------------------------------------------------------------ model
def attention(x, ctx, sd, prefix, heads, bias_mask=None, rope=None):
    """AttnProcessor2_0.__call__ (:1156-1267): projections, optional rotation of q and k, F.scaled_dot_product_attention, to_out."""
    B, Lq, C = x.shape
    Lk, D = ctx.shape[1], C // heads
    q = linear(x, sd, prefix + ".to_q").view(B, Lq, heads, D).transpose(1, 2)
    k = linear(ctx, sd, prefix + ".to_k").view(B, Lk, heads, D).transpose(1, 2)
    v = linear(ctx, sd, prefix + ".to_v").view(B, Lk, heads, D).transpose(1, 2)
    if rope is not None:
        q, k = rope(q), rope(k)
    am = None if bias_mask is None else bias_mask[:, None].to(q.dtype).expand(B, heads, Lq, Lk)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=am).transpose(1, 2).reshape(B, Lq, C)
    return linear(o, sd, prefix + ".to_out.0")


class RefState:
    def __init__(self, block_idx):
        self.block_idx = block_idx
        self.attn_count = self.cross_count = self.mlp_count = 0
        self.last_attn = self.last_cross = None


class LatteT2VRef:
    def __init__(self, sd, num_layers, num_heads, head_dim=72, patch_size=2, sample_size=(8, 8), out_channels=8, video_length=5,
                 use_rope=True, interpolation_scale_1d=None, norm_eps=1e-6, dtype=torch.float64):
        self.sd = {k: v.to(dtype) for k, v in sd.items()}
        self.L, self.H, self.C, self.p = num_layers, num_heads, num_heads * head_dim, patch_size
        self.sample_size, self.out_channels, self.video_length, self.eps, self.dtype = sample_size, out_channels, video_length, norm_eps, dtype
        self.use_rope = use_rope
        self.scale_2d = max(sample_size[0] // 64, 1)
        if interpolation_scale_1d is None:
            interpolation_scale_1d = (video_length - 1) // 16 if video_length % 2 == 1 else video_length // 16
        self.scale_1d = max(interpolation_scale_1d, 1)
        self.reset_pab_state()

    def reset_pab_state(self):
        self.sp_states = [RefState(i) for i in range(self.L)]
        self.tp_states = [RefState(i) for i in range(self.L)]

    def _chunks6(self, prefix, t6):
        return (self.sd[prefix + ".scale_shift_table"][None] + t6.reshape(t6.shape[0], 6, -1)).chunk(6, dim=1)

    def _ff(self, x, prefix, st, shift, scale, gate, ts, ats, temporal):
        from videosys_amd import pab

        bc, nxt, rng = False, False, None
        if pab.enable_pab():
            bc, st.mlp_count, nxt, rng = pab.if_broadcast_mlp(ts, st.mlp_count, st.block_idx, ats, is_temporal=temporal)
        if bc:
            return pab.get_mlp_output(rng, timestep=ts, block_idx=st.block_idx, is_temporal=temporal) + x
        h = layer_norm(x, self.eps) * (1 + scale) + shift
        ff = gate * feed_forward(h, self.sd, prefix + ".ff")
        if nxt:
            pab.save_mlp_output(timestep=ts, block_idx=st.block_idx, ff_output=ff, is_temporal=temporal)
        return ff + x

    def forward(self, hidden_states, timestep, encoder_hidden_states, encoder_attention_mask=None, all_timesteps=None):
        from videosys_amd import pab

        sd, C, p, dt, H = self.sd, self.C, self.p, self.dtype, self.H
        B, cin, Fr, Hh, Ww = hidden_states.shape
        gh, gw = Hh // p, Ww // p
        S = gh * gw
        ts = int(timestep.reshape(-1)[0])
        ats = None if all_timesteps is None else [int(v) for v in torch.as_tensor(all_timesteps).tolist()]
        x = hidden_states.to(dt).permute(0, 2, 1, 3, 4).reshape(B * Fr, cin, Hh, Ww)
        bias = None
        if encoder_attention_mask is not None:                                        # :2507-2511
            m = encoder_attention_mask.reshape(B, -1)
            bias = ((1 - m.to(dt)) * -10000.0).unsqueeze(1).repeat_interleave(Fr, dim=0)
        x = F.conv2d(x, sd["pos_embed.proj.weight"], sd["pos_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
        # PatchEmbed (:393-424): the construction-time buffer follows the module's dtype (nn.Module.to casts buffers); the table
        # recomputed for another input size is float32 and the sum is rounded
        tab = sincos_2d(C, gh, gw, self.sample_size[0] // p, self.scale_2d)[None]
        own = (gh, gw) == (self.sample_size[0] // p, self.sample_size[1] // p)
        x = x + tab.to(dt) if own else (x + tab).to(dt)
        emb = linear(F.silu(linear(timestep_embedding(timestep.float()).to(dt), sd, "adaln_single.emb.timestep_embedder.linear_1")),
                     sd, "adaln_single.emb.timestep_embedder.linear_2")
        t6 = linear(F.silu(emb), sd, "adaln_single.linear")
        y = encoder_hidden_states.reshape(B, -1, encoder_hidden_states.shape[-1]).to(dt)
        y = linear(F.gelu(linear(y, sd, "caption_projection.linear_1"), approximate="tanh"), sd, "caption_projection.linear_2")
        y_sp, t_sp, t_tp = y.repeat_interleave(Fr, dim=0), t6.repeat_interleave(Fr, dim=0), t6.repeat_interleave(S, dim=0)
        pos = (torch.arange(0, self.video_length).unsqueeze(1) / self.scale_1d).numpy()
        tpe = torch.from_numpy(sincos_1d(C, pos)).float()[None].to(dt)                 # float32 buffer (:2251-2254), cast with the module
        rope2 = (lambda t: rope_tokens_2d(t, gh, gw, float(self.scale_2d))) if self.use_rope else None
        rope1 = (lambda t: rope_tokens_1d(t, Fr, float(self.scale_1d))) if self.use_rope else None
        use_pab = pab.enable_pab()
        for i in range(self.L):
            pre, st = f"transformer_blocks.{i}", self.sp_states[i]
            sh1, sc1, g1, sh2, sc2, g2 = self._chunks6(pre, t_sp)
            bc = False
            if use_pab:
                bc, st.attn_count = pab.if_broadcast_spatial(ts, st.attn_count)
            if bc:
                a = st.last_attn
            else:
                a = g1 * attention(*(2 * [layer_norm(x, self.eps) * (1 + sc1) + sh1]), sd, pre + ".attn1", H, rope=rope2)
                if use_pab:
                    st.last_attn = a
            x = a + x
            bc = False
            if use_pab:
                bc, st.cross_count = pab.if_broadcast_cross(ts, st.cross_count)
            if bc:
                x = x + st.last_cross
            else:
                a = attention(x, y_sp, sd, pre + ".attn2", H, bias)
                x = a + x
                if use_pab:
                    st.last_cross = a
            x = self._ff(x, pre, st, sh2, sc2, g2, ts, ats, False)
            # temporal block on "(b t) f d"
            x = x.view(B, Fr, S, C).permute(0, 2, 1, 3).reshape(B * S, Fr, C)
            if i == 0:
                x = x + tpe[:, :Fr]
            pre, st = f"temporal_transformer_blocks.{i}", self.tp_states[i]
            sh1, sc1, g1, sh2, sc2, g2 = self._chunks6(pre, t_tp)
            bc = False
            if use_pab:
                bc, st.attn_count = pab.if_broadcast_temporal(ts, st.attn_count)
            if bc:
                a = st.last_attn
            else:
                a = g1 * attention(*(2 * [layer_norm(x, self.eps) * (1 + sc1) + sh1]), sd, pre + ".attn1", H, rope=rope1)
                if use_pab:
                    st.last_attn = a
            x = a + x
            x = self._ff(x, pre, st, sh2, sc2, g2, ts, ats, True)
            x = x.view(B, S, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr, S, C)
        e = emb.repeat_interleave(Fr, dim=0)
        shift, scale = (sd["scale_shift_table"][None] + e[:, None]).chunk(2, dim=1)
        x = linear(layer_norm(x, 1e-6) * (1 + scale) + shift, sd, "proj_out")
        co = self.out_channels
        x = torch.einsum("nhwpqc->nchpwq", x.reshape(-1, gh, gw, p, p, co)).reshape(-1, co, gh * p, gw * p)
        return x.view(B, Fr, co, gh * p, gw * p).permute(0, 2, 1, 3, 4).contiguous()

    __call__ = forward
