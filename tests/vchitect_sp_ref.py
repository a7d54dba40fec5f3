"""The SHARDED forward of VchitectXLTransformerModel restated in plain torch on the CPU — TEST INFRASTRUCTURE for
tests/test_vchitect_sp_cpu.py and tests/test_gpu_vchitect_sp.py, built from the pieces of tests/vchitect_ref.py (imported, not edited).

All P ranks run in lockstep in one process; a "rank" is an entry of a list.  What the reference does with sp_size = P
(vchitect_transformer_3d.py:543-562, attentions.py:733-757,928-949, core/distributed/comm.py:282-318), written out as it writes it:

  * frames at rest: after patch embed + position table, F is zero-padded to Fp = ceil(F / P) P and rank r keeps frames
    [r Fl, (r + 1) Fl) (set_pad("temporal", F) + split_from_second_dim); `cur_temb = temb.repeat(Fl, 1)`: local row i, sample i % B.
    The text rows are split by frame the same way ([B*F, L, D] input); a padded frame's text rows are ZERO here (the reference hands
    it its sample's prompt; no real row can see the difference, which test_vchitect_sp_cpu checks by poisoning them).
  * the temporal switch is all_to_all_with_pad on the JOINT [video | text] tokens of q, k and v: zero pad, tensor_split, concatenate,
    narrow — S + L tokens scattered (padded to a multiple of P), Fp frames gathered and the padding dropped; back the other way.  The
    product shards video and text tokens separately and moves the normed activations instead: temporal attention is row-wise in the
    token, so every real row must come out the same.
  * cross attention keys: row 0 OF THE LOCAL SHARD (attentions.py:781-786); the `cur_frame == 1` rule with the LOCAL frame count.

PINNED at P = 2: tests/test_vchitect_pinned_cpu.py holds model_forward(P = 2) to a float64 run of the reference's own class with
sp_size = 2 in two gloo processes (tests/golden/vchitect_sp_small.pt, tools/mint_vchitect.py: F = 3 with one padded frame, S + L = 71
with one padded token), within the class's own fp32-to-float64 distance.  Other P, B > 1 and per-frame text stay readings of the class."""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

import vchitect_ref as vr

HD = vr.HD


def pad_to(n: int, P: int) -> int:
    """set_pad (comm.py:271-275)."""
    return (P - n % P) % P


def all_to_all_with_pad(xs, scatter_dim, gather_dim, scatter_pad=0, gather_pad=0):
    """comm.py:282-304 + _all_to_all_func :104-108 for all ranks at once: xs[r] is rank r's input, the result rank r's output."""
    P = len(xs)
    if scatter_pad > 0:
        padded = []
        for x in xs:
            shape = list(x.shape)
            shape[scatter_dim] = scatter_pad
            padded.append(torch.cat([x, torch.zeros(shape, dtype=x.dtype)], dim=scatter_dim))
        xs = padded
    assert xs[0].shape[scatter_dim] % P == 0
    lists = [[t.contiguous() for t in torch.tensor_split(x, P, scatter_dim)] for x in xs]       # lists[src][dst]
    outs = [torch.cat([lists[src][dst] for src in range(P)], dim=gather_dim).contiguous() for dst in range(P)]
    if gather_pad > 0:
        outs = [o.narrow(gather_dim, 0, o.size(gather_dim) - gather_pad) for o in outs]
    return outs


def dynamic_switch(xs, B, to_spatial_shard, temporal_pad, spatial_pad):
    """attentions.py:928-949 on [(B T), S, ...] per rank."""
    xs = [x.reshape(B, -1, *x.shape[1:]) for x in xs]
    if to_spatial_shard:
        xs = all_to_all_with_pad(xs, 2, 1, scatter_pad=spatial_pad, gather_pad=temporal_pad)
    else:
        xs = all_to_all_with_pad(xs, 1, 2, scatter_pad=temporal_pad, gather_pad=spatial_pad)
    return [x.reshape(-1, *x.shape[2:]) for x in xs]


def split_frames(x, B, P):
    """split_from_second_dim (comm.py:307-311) with the zero padding of split_sequence: [(B F), ...] -> P x [(B Fl), ...]."""
    x = x.reshape(B, -1, *x.shape[1:])
    F = x.shape[1]
    pad = pad_to(F, P)
    if pad:
        x = torch.cat([x, torch.zeros(B, pad, *x.shape[2:], dtype=x.dtype)], dim=1)
    return [c.reshape(-1, *c.shape[2:]) for c in torch.tensor_split(x, P, dim=1)]


def gather_frames(xs, B, F):
    """gather_from_second_dim (comm.py:314-318): P x [(B Fl), ...] -> [(B F), ...], padding dropped."""
    x = torch.cat([x.reshape(B, -1, *x.shape[1:]) for x in xs], dim=1)[:, :F]
    return x.reshape(-1, *x.shape[2:])


def attention_layers(sd, hs, enc, B, F, H, context_pre_only=False, dtype=torch.float64):
    """VchitectAttnProcessor.__call__ on every rank: hs[r] [B*Fl, S, C], enc[r] [B*Fl, L, C] -> per rank (hidden, encoder)."""
    P = len(hs)
    Fl = hs[0].shape[0] // B
    S, L = hs[0].shape[1], enc[0].shape[1]
    SL = S + L
    lin = lambda x, n: Fn.linear(x, sd[n + ".weight"].to(dtype), sd[n + ".bias"].to(dtype))
    heads = lambda x: x.reshape(x.shape[0], -1, H, HD).transpose(1, 2)
    att = lambda q, k, v: Fn.scaled_dot_product_attention(q, k, v)
    hs, enc = [h.to(dtype) for h in hs], [e.to(dtype) for e in enc]
    eq, ek, ev = ([lin(e, n) for e in enc] for n in ("add_q_proj", "add_k_proj", "add_v_proj"))
    # ---- temporal (:705-764): joint tokens, switch, attention over the GLOBAL frames, switch back
    tpad, spad = pad_to(F, P), pad_to(SL, P)
    qkv = []
    for n, e in (("to_q_temp", eq), ("to_k_temp", ek), ("to_v_temp", ev)):
        joint = [torch.cat([lin(h, n), e[r]], dim=1).reshape(B * Fl, SL, H, HD) for r, h in enumerate(hs)]
        qkv.append(dynamic_switch(joint, B, True, tpad, spad))            # per rank [(B F), SLl, H, HD]
    cos, sin = vr.rope_tables(F)
    rot = lambda x: vr.apply_rotary(x.float() if dtype != torch.float64 else x, cos, sin).to(dtype)
    outs = []
    for r in range(P):
        SLl = qkv[0][r].shape[1]
        to_t = lambda x: x.reshape(B, F, SLl, H, HD).permute(0, 2, 1, 3, 4).reshape(B * SLl, F, H, HD)       # (B T) S H C -> (B S) T H C
        q, k, v = (to_t(qkv[i][r]) for i in range(3))
        o = att(rot(q).transpose(1, 2), rot(k).transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
        outs.append(o.reshape(B, SLl, F, H * HD).permute(0, 2, 1, 3).reshape(B * F, SLl, H * HD))           # (B S) T C -> (B T) S C
    temp = dynamic_switch(outs, B, False, tpad, spad)                                                        # per rank [(B Fl), SL, C]
    res = []
    for r in range(P):
        temp_v, temp_t = lin(temp[r][:, :S], "to_out_temporal"), temp[r][:, S:]
        # ---- cross (:766-800): keys = row 0 of the LOCAL shard
        qc = torch.cat([lin(hs[r], "to_q_cross"), eq[r]], dim=1)
        ky, vy = ek[r][0].unsqueeze(0).reshape(B, -1, H, HD), ev[r][0].unsqueeze(0).reshape(B, -1, H, HD)
        qy = qc.reshape(B, Fl, SL, H, HD).permute(0, 2, 1, 3, 4).reshape(B, SL * Fl, H, HD)
        c = att(qy.transpose(1, 2), ky.transpose(1, 2), vy.transpose(1, 2)).transpose(1, 2).reshape(B, SL, Fl, H * HD)
        cross = lin(c.permute(0, 2, 1, 3).reshape(B * Fl, SL, H * HD), "to_out_context")
        # ---- spatial (:667-703)
        q, k, v = (torch.cat([lin(hs[r], n), e[r]], dim=1) for n, e in (("to_q", eq), ("to_k", ek), ("to_v", ev)))
        sp = att(heads(q), heads(k), heads(v)).transpose(1, 2).reshape(B * Fl, SL, H * HD)
        h = sp * 1.1 + cross
        hv, ht = lin(h[:, :S], "to_out.0"), h[:, S:]
        if Fl == 1:                          # cur_frame == 1 (:836,909-919): the LOCAL frame count
            temp_v = temp_v * 0
        hv = hv + temp_v
        if not context_pre_only:
            ht = lin(ht, "to_add_out")
        tt = lin(temp_t, "to_add_out_temporal")
        if Fl == 1:
            tt = tt * 0
        res.append((hv, ht + tt))
    return res


def model_forward(sd, cfg, hidden_states, encoder_hidden_states, pooled, timestep, P, dtype=torch.float64, pad_text=0.0):
    """vr.model_forward with sp_size = P: returns the gathered prediction [(B F), co, H, W] (the same on every rank).
    ``pad_text``: what the text rows of a padded frame hold (zero; the sanity test poisons it with another value)."""
    lin = lambda x, n: Fn.linear(x, sd[n + ".weight"].to(dtype), sd[n + ".bias"].to(dtype))
    ln = lambda x: Fn.layer_norm(x, x.shape[-1:], eps=1e-6)
    B, F, cin, Hh, Ww = hidden_states.shape
    p, H, depth = cfg["patch"], cfg["heads"], cfg["num_layers"]
    C = H * HD
    Hp, Wp = Hh // p, Ww // p
    x = Fn.conv2d(hidden_states.reshape(B * F, cin, Hh, Ww).to(dtype), sd["pos_embed.proj.weight"].to(dtype), sd["pos_embed.proj.bias"].to(dtype),
                  stride=p).flatten(2).transpose(1, 2)
    m = cfg["pos_embed_max_size"]
    pos = vr.sincos_2d(C, m, cfg["sample_size"] // p).float().reshape(m, m, C)
    top, left = (m - Hp) // 2, (m - Wp) // 2
    pos = pos[top:top + Hp, left:left + Wp].reshape(1, Hp * Wp, C)
    x = (x + (pos.double() if dtype == torch.float64 else pos)).to(dtype)
    te = "time_text_embed.timestep_embedder."
    tx = "time_text_embed.text_embedder."
    t_emb = lin(Fn.silu(lin(vr.timestep_proj(timestep).to(dtype), te + "linear_1")), te + "linear_2")
    temb = t_emb + lin(Fn.silu(lin(pooled.to(dtype), tx + "linear_1")), tx + "linear_2")
    y = lin(encoder_hidden_states.to(dtype), "context_embedder")
    xs, ys = split_frames(x, B, P), split_frames(y, B, P)
    Fl = xs[0].shape[0] // B
    if pad_text:
        for r in range(P):
            nreal = max(0, min(Fl, F - r * Fl))
            ys[r] = ys[r].clone()
            ys[r].reshape(B, Fl, *ys[r].shape[1:])[:, nreal:] = pad_text
    # cur_temb = temb.repeat(Fl, 1): the first B Fl rows of temb.repeat(F, 1), whose linears are evaluated on all B F rows so that the
    # host BLAS rounds them as in vchitect_ref (it picks another kernel for a handful of rows)
    cur, nloc = temb.repeat(F, 1), B * Fl
    for i in range(depth):
        pre, last = f"transformer_blocks.{i}.", i == depth - 1
        asd = {k[len(pre) + 5:]: v for k, v in sd.items() if k.startswith(pre + "attn.")}
        first = lambda t: t[:nloc] if nloc <= t.shape[0] else t.repeat(-(-nloc // t.shape[0]), 1)[:nloc]
        sh, sc, g, sh2, sc2, g2 = (first(t) for t in lin(Fn.silu(cur), pre + "norm1.linear").chunk(6, dim=1))
        if last:
            csc, csh = (first(t) for t in lin(Fn.silu(cur), pre + "norm1_context.linear").chunk(2, dim=1))
        else:
            csh, csc, cg, csh2, csc2, cg2 = (first(t) for t in lin(Fn.silu(cur), pre + "norm1_context.linear").chunk(6, dim=1))
        xn = [ln(x) * (1 + sc[:, None]) + sh[:, None] for x in xs]
        yn = [ln(y) * (1 + csc)[:, None] + csh[:, None] if last else ln(y) * (1 + csc[:, None]) + csh[:, None] for y in ys]
        att = attention_layers(asd, xn, yn, B, F, H, last, dtype)
        for r in range(P):
            av, at = att[r]
            x = xs[r] + g.unsqueeze(1) * av
            xn_ = ln(x) * (1 + sc2[:, None]) + sh2[:, None]
            xs[r] = x + g2.unsqueeze(1) * lin(Fn.gelu(lin(xn_, pre + "ff.net.0.proj"), approximate="tanh"), pre + "ff.net.2")
            if not last:
                y = ys[r] + cg.unsqueeze(1) * at
                yn_ = ln(y) * (1 + csc2[:, None]) + csh2[:, None]
                ys[r] = y + cg2.unsqueeze(1) * lin(Fn.gelu(lin(yn_, pre + "ff_context.net.0.proj"), approximate="tanh"), pre + "ff_context.net.2")
    x = gather_frames(xs, B, F)
    scale, shift = lin(Fn.silu(temb), "norm_out.linear").repeat_interleave(F, dim=0).chunk(2, dim=1)
    x = lin(ln(x) * (1 + scale)[:, None] + shift[:, None], "proj_out")
    co = cfg["out_channels"]
    x = x.reshape(B * F, Hp, Wp, p, p, co)
    return torch.einsum("nhwpqc->nchpwq", x).reshape(B * F, co, Hp * p, Wp * p)
