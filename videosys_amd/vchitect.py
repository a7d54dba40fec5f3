"""Vchitect-2.0 on the MI355X kernels: the attention layer of a JointTransformerBlock (reference videosys/models/modules/attentions.py,
VchitectAttention :321-534 + VchitectAttnProcessor :641-949) with the reference's state-dict names and its three PAB counters.

What is here is the LAYER: the projections (GEMM family), the three attentions (vsys_attn_temporal_d64; vsys_attn_prep_kv64 +
vsys_flash_attn_d64 without norm / RoPE for the joint spatial and the cross attention), `spatial * 1.1 + to_out_context(cross)`
(vsys_scale_add_rows), the output projections, the `cur_frame == 1` rule and the PAB caches.  The transformer around it
(VchitectXLTransformerModel, JointTransformerBlock below) adds patch embed with the cropped 2-D sincos table, AdaLayerNormZero /
AdaLayerNormContinuous (vsys_ln_modulate), FeedForward (bias + GELU and gate + residual GEMM epilogues), the time-text embedding
(vsys_timestep_embedding, vsys_linear_small), proj_out and unpatchify, with the reference's constructor config and state-dict names.
The pipeline around it (flow-match sampler, T5, SD3 VAE decode) is pipeline_vchitect.py.  Not built: the two CLIP text encoders (they
are injected objects there).

Sequence parallelism (vchitect_transformer_3d.py:326-338,543-562; attentions.py:733-757,928-949).  Frames are sharded at rest: rank r of
P keeps frames [r Fl, (r + 1) Fl), Fl = ceil(F / P), frames past F being zero rows written after the embedding; the text rows of a frame
travel with it.  Spatial and cross attention run on the local frames.  Around the temporal attention the NORMED activations (C wide,
a third of q | k | v) switch to a token shard — video and text tokens separately, Sl = ceil(S / P) and Ll = ceil(L / P), zero rows
past S and L — so every rank attends over the global F frames of its tokens with RoPE positions 0 .. F - 1; `_qkv_temp` and `_add_qkv`
run on the token shard, and the result switches back (dsp.SequenceParallel, both its exchange routes).  Over all_to_all_single the
attention runs on the receive image as it lies and writes the send image of the way back (``attn_route = "image"``, the measured
default: vsys_attn_temporal_d64_img, four copy launches a block instead of eight); ``"rows"`` unpacks and packs around the old kernel
and is the route the peer-to-peer exchange uses.  The fp32 prediction of the local frames is all-gathered into the caller's ``out``.

Every launch goes through ops._call and every buffer is resident, so a step can be recorded once (program.Recorder) and replayed.

Two readings of the reference that matter:
  * cross attention keys are `encoder_hidden_states_key_proj[0]` viewed as (batchsize, -1, heads, 64) (:781-786): frame 0 of SAMPLE 0,
    dealt out over the B samples in runs of L / B keys.  That is what runs here (B == 1, the only batch the reference pipeline uses,
    gives all L keys); L % B != 0 raises, as the reference's view does.  Under sequence parallelism row 0 is row 0 OF THE LOCAL SHARD:
    sample 0's frame r Fl.  After the first block the text rows differ per frame, so a sharded run equals the reference's sharded
    run and not the single-process one; it is kept literally.
  * the `cur_frame == 1` rule (:836,909-919) reads the LOCAL frame count: with one frame per rank the temporal contributions are
    multiplied by zero.  Kept literally, as the F == 1 path: the exchange and the attention still run (the caches are filled), nothing
    is added.
  * the `(S T)` query order of cross attention (:788) is undone by :798 and attention is row-wise in the queries, so the video rows
    (batch B, q_len F S) and the text rows (batch B, q_len F L) are two launches over the same keys; nothing is transposed."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import dsp, ops, pab, program, vchitect_ops
from .modules import sincos_1d
from .workspace import Workspace

HEAD_DIM = 64
ROPE_THETA = 1e6


def rope_tables(frames: int, device, theta: float = ROPE_THETA, rope_scaling_factor: float = 1.0):
    """cos / sin fp32 [frames, 32] of precompute_freqs_cis (vchitect_transformer_3d.py:341-347), every step in fp32 as there."""
    freqs = 1.0 / (theta ** (torch.arange(0, HEAD_DIM, 2)[: HEAD_DIM // 2].float() / HEAD_DIM))
    ang = torch.outer(torch.arange(frames, dtype=torch.float) / rope_scaling_factor, freqs).float()
    cis = torch.polar(torch.ones_like(ang), ang)
    return cis.real.contiguous().to(device), cis.imag.contiguous().to(device)


class _NoGroupOfThatSize(NotImplementedError, AssertionError):
    """enable_parallel without an injected manager asked for a dp x cp x sp mesh that is not the size of the process group initialised
    in this process (none = 1).  A NotImplementedError for callers written when sequence parallelism was not built; also the
    AssertionError dsp.ParallelManager raises for the same mismatch."""


def _resolve_parallel(dp_size, sp_size, enable_cp, parallel_mgr):
    """vchitect_transformer_3d.py:326-338: `enable_cp` with an even sp_size halves it and builds a dp x cp x sp mesh.  Returns the
    manager to use, or None for a single rank.  The CFG split (cp > 1) is not built, as for Latte and CogVideoX."""
    import torch.distributed as dist

    if parallel_mgr is not None:
        if enable_cp and parallel_mgr.sp_size * getattr(parallel_mgr, "cp_size", 1) > 1:
            raise NotImplementedError("Vchitect: the CFG split (enable_cp) is not built; shard with enable_cp=False")
        if getattr(parallel_mgr, "cp_size", 1) > 1:
            raise NotImplementedError("Vchitect: the CFG split (cp_size > 1) is not built")
        return parallel_mgr if parallel_mgr.sp_size > 1 else None
    dp, sp, cp = dp_size or 1, sp_size or 1, 1
    if enable_cp and sp % 2 == 0:
        sp, cp = sp // 2, 2
    world = dist.get_world_size() if dist.is_initialized() else 1
    if dp * cp * sp != world:
        raise _NoGroupOfThatSize(f"Vchitect sequence parallelism: there is no process group of {dp} x {cp} x {sp} = {dp * cp * sp} ranks in "
                                 f"this process (the initialised world has {world}); initialise torch.distributed with that many ranks, "
                                 f"or hand in a manager (parallel_mgr=)")
    if cp > 1:
        raise NotImplementedError("Vchitect: the CFG split (enable_cp) is not built; shard with enable_cp=False")
    return dsp.ParallelManager(dp, cp, sp) if sp > 1 else None


class VchitectAttention:
    """attn of JointTransformerBlock: query_dim = added_kv_proj_dim = out_dim = dim, heads x 64, bias everywhere."""

    LINEARS = ("to_q", "to_k", "to_v", "to_q_cross", "to_q_temp", "to_k_temp", "to_v_temp", "add_q_proj", "add_k_proj", "add_v_proj",
               "to_out.0", "to_out_temporal", "to_add_out", "to_add_out_temporal", "to_out_context")

    def __init__(self, dim: int, heads: int, context_pre_only: bool = False, rope_scaling_factor: float = 1.0, device="cuda"):
        from . import _lib

        _lib.load()  # fail loudly if the HIP library is missing
        if dim != heads * HEAD_DIM:
            raise ValueError("the Vchitect attention kernels are built for head_dim 64")
        if dim % 192:
            raise ValueError("hidden size must be a multiple of 192 (GEMM tile); 1536 is")
        self.C, self.H, self.context_pre_only = dim, heads, context_pre_only
        self.rope_scaling_factor = rope_scaling_factor
        self.device = torch.device(device)
        self.w: Dict[str, torch.Tensor] = {}
        self.parallel_manager = None
        self._ws, self._rope = Workspace(self.device), {}
        self._buf = self._ws.buf   # bound to this Workspace: _ws is cleared, never replaced (rebind _buf with it otherwise)
        self.spatial_count = self.cross_count = self.temporal_count = 0
        self.last_spatial = self.last_cross = self.last_temporal = None
        self.last_decisions = (False, False, False)
        self._geometry = None
        self._sp, self._sp_tag = None, ""
        self.attn_route = None      # None: the measured default (_route); "rows" | "image" force one (as STDiT3's _switch)

    # Which temporal-attention route runs over all_to_all_single when nothing is forced: the image kernel, whose per-rank step (wire
    # stubbed, 2B geometry) was 25.4 ms against 26.0 ms at 8 ranks and 40.0 against 40.7 ms at 4 (profiles/vchitect_sp_timing.json,
    # DESIGN.md 3.3).  "rows" stays reachable through ``attn_route`` and is what the peer-to-peer exchange runs.
    DEFAULT_A2A_ROUTE = "image"

    def enable_parallel(self, dp_size=1, sp_size=1, enable_cp=False, parallel_mgr=None, copy_executor=None, sp=None, tag=""):
        """The layer's side of VchitectXLTransformerModel.enable_parallel: ``sp`` is the model's dsp.SequenceParallel (one for all
        blocks: they run one after the other and share its staging buffers), ``tag`` names this block's exchange sites.  Called on
        its own it builds a SequenceParallel from the manager (or raises as the model does)."""
        if sp is None:
            mgr = _resolve_parallel(dp_size, sp_size, enable_cp, parallel_mgr)
            if mgr is not None:
                kw = {} if copy_executor is None else {"copy_executor": copy_executor}
                sp = dsp.SequenceParallel(mgr.sp_group, **kw)
            self.parallel_manager = mgr
        self._sp, self._sp_tag = sp, tag
        self._geometry = None

    def _route(self):
        """"rows" or "image" for this call.  The one-kernel peer-to-peer exchange writes straight into the peers' (b, t, s) tensors:
        there is no receive image, so it always takes "rows"."""
        if self._sp.p2p is not None:
            return "rows"
        r = self.attn_route or self.DEFAULT_A2A_ROUTE
        if r not in ("rows", "image"):
            raise ValueError(f"attn_route {r!r}: expected 'rows' or 'image'")
        return r

    def _zeroed(self, name, shape, F):
        """A resident buffer of the SequenceParallel object that is zero when it is made (the send image of the way back: the image
        kernel never writes the frames past F, which the peers receive as their padded frames).  One per F: another frame count
        with the same image shape would leave its rows where this one's padding is."""
        sp = self._sp
        key = (name, tuple(shape), F)
        if key not in sp._bufs:
            sp._bufs[key] = torch.zeros(shape, dtype=torch.bfloat16, device=self.device)
        return sp._bufs[key]

    def _temporal_sharded(self, hs, enc, B, Fl, F, S, L, cos, sin):
        """Temporal attention of a frame-sharded step: hs [B*Fl*S, C], enc [B*Fl*L, C] (normed, local frames) -> (tv [B*Fl*S, C],
        tt [B*Fl*L, C]) rows of the local frames (zero rows for frames past F).  Two exchanges there, two back."""
        sp, C, H = self._sp, self.C, self.H
        P = sp.P
        tag = self._sp_tag if sp.p2p is not None else ""   # a peer-to-peer site is one destination tensor: one site per block
        Sl, Ll = -(-S // P), -(-L // P)
        tv, tt = self._buf("temp_v", (B, Fl, S, C)), self._buf("temp_t", (B, Fl, L, C))
        if self._route() == "rows":
            xv = sp.to_spatial_shard(hs.view(B, Fl, S, C), F, Sl, out=self._buf("sp_xv", (B, F, Sl, C)), tag="v" + tag)
            xt = sp.to_spatial_shard(enc.view(B, Fl, L, C), F, Ll, out=self._buf("sp_xt", (B, F, Ll, C)), tag="t" + tag)
            nv, nt = B * F * Sl, B * F * Ll
            qt = self._lin(xv.view(nv, C), "_qkv_temp", self._buf("qkv_temp", (nv, 3 * C)))
            tq = self._lin(xt.view(nt, C), "_add_qkv", self._buf("tq_temp", (nt, 3 * C)))
            ov, ot = self._buf("sp_ov", (nv, C)), self._buf("sp_ot", (nt, C))
            vchitect_ops.attn_temporal64(qt[:, :C], qt[:, C:2 * C], qt[:, 2 * C:], tq[:, :C], tq[:, C:2 * C], tq[:, 2 * C:], cos, sin,
                                         ov, ot, B, F, Sl, Ll, H)
            sp.to_temporal_shard(ov.view(B, F, Sl, C), S, out=tv, tag="v" + tag)
            sp.to_temporal_shard(ot.view(B, F, Ll, C), L, out=tt, tag="t" + tag)
            return tv.view(B * Fl * S, C), tt.view(B * Fl * L, C)
        # ---- "image": the GEMMs and the attention run on the receive image [P (source)][B][Fl][n][C] as it lies, the attention writes
        # the send image of the way back; per tensor one pack there and one unpack back, nothing around the attention
        pv, _, shape_v, _ = dsp.plan_switch_to_spatial_shard(B, Fl, F, S, Sl, C, P)
        pt, _, shape_t, _ = dsp.plan_switch_to_spatial_shard(B, Fl, F, L, Ll, C, P)
        _, uv, _, _ = dsp.plan_switch_to_temporal_shard(B, F, Sl, S, C, P)
        _, ut, _, _ = dsp.plan_switch_to_temporal_shard(B, F, Ll, L, C, P)
        send_v, recv_v = sp._buf("img_send_v", shape_v, hs), sp._buf("img_recv_v", shape_v, hs)
        send_t, recv_t = sp._buf("img_send_t", shape_t, hs), sp._buf("img_recv_t", shape_t, hs)
        sp.exec(hs, send_v, pv)
        dsp.all_to_all_single(recv_v, send_v, sp.group)
        sp.exec(enc, send_t, pt)
        dsp.all_to_all_single(recv_t, send_t, sp.group)
        nv, nt = P * B * Fl * Sl, P * B * Fl * Ll
        qt = self._lin(recv_v.view(nv, C), "_qkv_temp", self._buf("qkv_temp", (nv, 3 * C)))
        tq = self._lin(recv_t.view(nt, C), "_add_qkv", self._buf("tq_temp", (nt, 3 * C)))
        back_v, back_t = self._zeroed("img_back_v", shape_v, F), self._zeroed("img_back_t", shape_t, F)
        attend = vchitect_ops.attn_temporal64_img(qt[:, :C], qt[:, C:2 * C], qt[:, 2 * C:], tq[:, :C], tq[:, C:2 * C], tq[:, 2 * C:],
                                                  cos, sin, back_v.view(nv, C), back_t.view(nt, C), B, F, Fl, Sl, Ll, H, defer=True)
        # (no op code: the attention is issued by the host closure of the collective it feeds, so a replayed step gets no extra segment)
        dsp.all_to_all_single(recv_v, back_v, sp.group, before=attend)
        sp.exec(recv_v, tv, uv)
        dsp.all_to_all_single(recv_t, back_t, sp.group)
        sp.exec(recv_t, tt, ut)
        return tv.view(B * Fl * S, C), tt.view(B * Fl * L, C)

    def expected_keys(self):
        names = [l for l in self.LINEARS if not (self.context_pre_only and l == "to_add_out")]
        return [f"{l}.{p}" for l in names for p in ("weight", "bias")]

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = "", strict: bool = True):
        missing = [k for k in self.expected_keys() if prefix + k not in sd]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:8]}{'...' if len(missing) > 8 else ''}")
        dev = lambda t: t.detach().to(device=self.device, dtype=torch.bfloat16).contiguous()
        for k in self.expected_keys():
            self.w[k] = dev(sd[prefix + k])
        for name, parts in (("_qkv", ("to_q", "to_k", "to_v")), ("_qkv_temp", ("to_q_temp", "to_k_temp", "to_v_temp")),
                            ("_add_qkv", ("add_q_proj", "add_k_proj", "add_v_proj"))):
            for p in ("weight", "bias"):
                self.w[f"{name}.{p}"] = dev(torch.cat([sd[f"{prefix}{l}.{p}"] for l in parts], 0))
        return self

    def reset_pab_state(self):
        self.spatial_count = self.cross_count = self.temporal_count = 0
        self.last_spatial = self.last_cross = self.last_temporal = None

    def _kv(self, name, batch, kv_len):
        return self._ws.once((name, batch, kv_len), lambda: ops.alloc_kv_buffers64(batch, self.H, kv_len, self.device))

    def _lin(self, x, name, out):
        return ops.gemm(x, self.w[name + ".weight"], self.w[name + ".bias"], out=out)

    @torch.no_grad()
    def forward(self, hidden_states, encoder_hidden_states, batch: int, frames: int, timestep: int = None, frames_global: int = None):
        """hidden_states bf16 [B*F*S, C] rows (b, f, s), encoder_hidden_states bf16 [B*F*L, C] rows (b, f, l) (the normed inputs of
        the block) -> (attn_output [B*F*S, C], context_attn_output [B*F*L, C]); resident buffers, valid until the next call.
        ``timestep``: the Python int the sampler holds (PAB decisions; `int(timestep[0])` of the reference).  Under sequence
        parallelism ``frames`` is the local frame count Fl and ``frames_global`` the F the temporal attention runs over."""
        C, H, B, F = self.C, self.H, batch, frames
        Fa = F if frames_global is None else frames_global
        if self._sp is None and Fa != F:
            raise ValueError("frames_global differs from frames, but the layer is not sharded (enable_parallel)")
        BF = B * F
        Nv, Nt = hidden_states.shape[0], encoder_hidden_states.shape[0]
        if Nv % BF or Nt % BF or hidden_states.shape[1] != C or encoder_hidden_states.shape[1] != C:
            raise ValueError("hidden_states / encoder_hidden_states must hold batch * frames whole frames of `dim` columns")
        S, L = Nv // BF, Nt // BF
        SL = S + L
        if L % B:
            raise ValueError(f"cross attention deals the {L} text keys of frame 0 out over {B} samples (attentions.py:781-786): "
                             f"L must be a multiple of the batch")
        Lk = L // B
        if self._geometry != (B, F, S, L, Fa):     # the caches are views of the resident workspaces: another geometry invalidates them
            self._geometry = (B, F, S, L, Fa)
            self.last_spatial = self.last_cross = self.last_temporal = None
        hs, enc = hidden_states, encoder_hidden_states
        use_pab = pab.enable_pab()
        tq = self._lin(enc, "_add_qkv", self._buf("tq", (Nt, 3 * C)))          # add_q_proj | add_k_proj | add_v_proj
        # ---- temporal attention (:838-858)
        bt = False
        if use_pab:
            bt, self.temporal_count = pab.if_broadcast_temporal(timestep, self.temporal_count)
        if not (bt and self.last_temporal is not None):
            if Fa not in self._rope:
                self._rope[Fa] = rope_tables(Fa, self.device, rope_scaling_factor=self.rope_scaling_factor)
            cos, sin = self._rope[Fa]
            if self._sp is not None:
                tv, tt = self._temporal_sharded(hs, enc, B, F, Fa, S, L, cos, sin)
            else:
                qt = self._lin(hs, "_qkv_temp", self._buf("qkv_temp", (Nv, 3 * C)))
                tv, tt = self._buf("temp_v", (Nv, C)), self._buf("temp_t", (Nt, C))
                vchitect_ops.attn_temporal64(qt[:, :C], qt[:, C:2 * C], qt[:, 2 * C:], tq[:, :C], tq[:, C:2 * C], tq[:, 2 * C:], cos, sin,
                                             tv, tt, B, F, S, L, H)
            self.last_temporal = (self._lin(tv, "to_out_temporal", self._buf("temp_vo", (Nv, C))), tt)
        tvo, tt = self.last_temporal
        # ---- cross attention (:860-878)
        bc = False
        if use_pab:
            bc, self.cross_count = pab.if_broadcast_cross(timestep, self.cross_count)
        if not (bc and self.last_cross is not None):
            qc = self._lin(hs, "to_q_cross", self._buf("q_cross", (Nv, C)))
            kp, vt = self._kv("cross", B, Lk)
            ops.attn_prep_kv64(tq[:L, C:2 * C], tq[:L, 2 * C:], None, None, None, None, 0, kp, vt, B, H, Lk)
            cv, ct = self._buf("cross_v", (Nv, C)), self._buf("cross_t", (Nt, C))
            ops.flash_attn64(qc, None, None, None, None, 0, kp, vt, cv, B, H, F * S, Lk)
            ops.flash_attn64(tq[:, :C], None, None, None, None, 0, kp, vt, ct, B, H, F * L, Lk)
            self.last_cross = (self._lin(cv, "to_out_context", self._buf("cross_vo", (Nv, C))),
                               self._lin(ct, "to_out_context", self._buf("cross_to", (Nt, C))))
        pcv, pct = self.last_cross
        # ---- joint spatial attention (:880-896)
        bs = False
        if use_pab:
            bs, self.spatial_count = pab.if_broadcast_spatial(timestep, self.spatial_count)
        if not (bs and self.last_spatial is not None):
            qs = self._lin(hs, "_qkv", self._buf("qkv", (Nv, 3 * C)))
            # k | v of [video | text] per frame: attn_prep_kv64 wants the S + L keys of a frame in consecutive rows, the two GEMMs
            # write whole tensors, so the rows are gathered by two strided copies (a known cost: DESIGN.md 3.3)
            jkv = self._buf("joint_kv", (BF * SL, 2 * C))
            ops.copy_4d(qs[:, C:], jkv, BF, S, 1, 2 * C, (S * 3 * C, 3 * C, 0), (SL * 2 * C, 2 * C, 0))
            ops.copy_4d(tq[:, C:], jkv[S:], BF, L, 1, 2 * C, (L * 3 * C, 3 * C, 0), (SL * 2 * C, 2 * C, 0))
            kp, vt = self._kv("spatial", BF, SL)
            ops.attn_prep_kv64(jkv[:, :C], jkv[:, C:], None, None, None, None, 0, kp, vt, BF, H, SL)
            sv, st = self._buf("spat_v", (Nv, C)), self._buf("spat_t", (Nt, C))
            ops.flash_attn64(qs[:, :C], None, None, None, None, 0, kp, vt, sv, BF, H, S, SL)
            ops.flash_attn64(tq[:, :C], None, None, None, None, 0, kp, vt, st, BF, H, L, SL)
            self.last_spatial = (sv, st)
        sv, st = self.last_spatial
        # ---- hidden = spatial * 1.1 + cross; output projections; temporal contributions (x 0 at one frame, :909-919)
        hv = vchitect_ops.scale_add_rows(sv, pcv, 1.1, out=self._buf("mix_v", (Nv, C)))
        ht = vchitect_ops.scale_add_rows(st, pct, 1.1, out=self._buf("mix_t", (Nt, C)))
        out_v = self._lin(hv, "to_out.0", self._buf("out_v", (Nv, C)))
        out_t = ht if self.context_pre_only else self._lin(ht, "to_add_out", self._buf("out_t", (Nt, C)))
        if F > 1:
            ops.add_rows(out_v, tvo)
            ops.add_rows(out_t, self._lin(tt, "to_add_out_temporal", self._buf("temp_to", (Nt, C))))
        self.last_decisions = (bt, bc, bs)
        return out_v, out_t

    __call__ = forward


def synth_attention_state_dict(dim: int, context_pre_only: bool = False, seed: int = 777) -> Dict[str, torch.Tensor]:
    """Seeded random weights with the reference's VchitectAttention key names (no pretrained weights offline)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for l in VchitectAttention.LINEARS:
        if context_pre_only and l == "to_add_out":
            continue
        sd[l + ".weight"] = torch.randn(dim, dim, generator=g) * min(0.08, dim ** -0.5)
        sd[l + ".bias"] = torch.randn(dim, generator=g) * 0.02
    return sd


def sincos_2d(embed_dim: int, grid: int, base_size: int) -> torch.Tensor:
    """diffusers get_2d_sincos_pos_embed(embed_dim, grid, base_size=base_size, interpolation_scale=1): fp32 [grid * grid, embed_dim]."""
    g = np.arange(grid, dtype=np.float32) / (grid / base_size)
    gw, gh = np.meshgrid(g, g)          # w goes first
    return torch.from_numpy(np.concatenate([sincos_1d(embed_dim // 2, gw), sincos_1d(embed_dim // 2, gh)], axis=1)).float()


class JointTransformerBlock:
    """vchitect_transformer_3d.py:49-175 on resident 2-D row tensors: video rows [B*F*S, C], text rows [B*F*L, C].  The modulation
    vectors of every block of a step are produced in one launch by the model and handed in as column blocks of one table."""

    def __init__(self, dim, num_attention_heads, attention_head_dim, context_pre_only=False, rope_scaling_factor=1.0, device="cuda"):
        self.C, self.context_pre_only = dim, context_pre_only
        self.attn = VchitectAttention(dim, num_attention_heads, context_pre_only, rope_scaling_factor, device)
        self.w: Dict[str, torch.Tensor] = {}

    LINEARS = ("ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2")

    def expected_keys(self):
        names = ["norm1.linear", "norm1_context.linear"] + [l for l in self.LINEARS if not (self.context_pre_only and "context" in l)]
        return [f"{l}.{p}" for l in names for p in ("weight", "bias")] + ["attn." + k for k in self.attn.expected_keys()]

    def load_state_dict(self, sd, prefix=""):
        dev = lambda t: t.detach().to(device=self.attn.device, dtype=torch.bfloat16).contiguous()
        for k in self.expected_keys():
            if not k.startswith(("attn.", "norm1")):
                self.w[k] = dev(sd[prefix + k])
        self.attn.load_state_dict(sd, prefix + "attn.")
        return self

    def forward(self, x, y, mod_v, mod_c, ms, batch, frames, buf, timestep=None, frames_global=None):
        """x [B*F*S, C], y [B*F*L, C] updated in place (y untouched after a context_pre_only block: the reference returns None).
        mod_v / mod_c: row 0 of this block's modulation columns in the [B*F, ms] table (video: shift_msa, scale_msa, gate_msa,
        shift_mlp, scale_mlp, gate_mlp; context: the same six, or scale | shift of AdaLayerNormContinuous)."""
        C, w = self.C, self.w
        BF = batch * frames
        S, L = x.shape[0] // BF, y.shape[0] // BF
        xn = ops.ln_modulate(x, None, None, mod_v[0:C], mod_v[C:2 * C], S, mod_stride=ms, eps=1e-6, out=buf("xn", x.shape))
        if self.context_pre_only:
            yn = ops.ln_modulate(y, None, None, mod_c[C:2 * C], mod_c[0:C], L, mod_stride=ms, eps=1e-6, out=buf("yn", y.shape))
        else:
            yn = ops.ln_modulate(y, None, None, mod_c[0:C], mod_c[C:2 * C], L, mod_stride=ms, eps=1e-6, out=buf("yn", y.shape))
        av, at = self.attn(xn, yn, batch, frames, timestep, frames_global)
        ops.gate_add_rows(x, av, mod_v[2 * C:3 * C], S, ms)
        xn = ops.ln_modulate(x, None, None, mod_v[3 * C:4 * C], mod_v[4 * C:5 * C], S, mod_stride=ms, eps=1e-6, out=buf("xn", x.shape))
        h = ops.gemm(xn, w["ff.net.0.proj.weight"], w["ff.net.0.proj.bias"], epilogue=ops.EPI_BIAS_GELU, out=buf("ff_h", (x.shape[0], 4 * C)))
        ops.gemm(h, w["ff.net.2.weight"], w["ff.net.2.bias"], epilogue=ops.EPI_GATE_RES, gate=mod_v[5 * C:6 * C], gate_stride=ms,
                 rows_per_sample=S, res=x, out=x)
        if self.context_pre_only:
            return
        ops.gate_add_rows(y, at, mod_c[2 * C:3 * C], L, ms)
        yn = ops.ln_modulate(y, None, None, mod_c[3 * C:4 * C], mod_c[4 * C:5 * C], L, mod_stride=ms, eps=1e-6, out=buf("yn", y.shape))
        h = ops.gemm(yn, w["ff_context.net.0.proj.weight"], w["ff_context.net.0.proj.bias"], epilogue=ops.EPI_BIAS_GELU,
                     out=buf("ffc_h", (y.shape[0], 4 * C)))
        ops.gemm(h, w["ff_context.net.2.weight"], w["ff_context.net.2.bias"], epilogue=ops.EPI_GATE_RES, gate=mod_c[5 * C:6 * C],
                 gate_stride=ms, rows_per_sample=L, res=y, out=y)


class VchitectXLTransformerModel:
    """vchitect_transformer_3d.py:237-590 (constructor config :261-275, state-dict names of the reference / the Vchitect-2.0 checkpoint).

    Batch.  The reference pipeline calls the model one sample at a time; the forward is written for that: `cur_temb = temb.repeat(F, 1)`
    (:548) pairs frame row i with sample i % B, and `norm_out(hidden_states, temb)` (:564) broadcasts only at B = 1.  Here :548 is kept
    literally for every B, and norm_out uses the temb of the sample a row belongs to (the only reading that exists for B > 1; the same
    thing at B = 1).  encoder_hidden_states may be [B, L, D] (every frame of a sample reads its prompt, what the broadcast of
    norm1_context does at B = 1) or [B*F, L, D].

    Sequence parallelism (enable_parallel; module docstring).  A rank embeds its own frames straight from its slice of the latents
    (and of a [B*F, L, D] encoder_hidden_states, which is split by frame), `cur_temb = temb.repeat(Fl, 1)` pairs local row i with
    sample i % B, and the video AND text rows of a frame past F are zero rows written after the embedding (it cannot matter which:
    a padded frame never reaches a real output row).  norm_out, proj_out and unpatchify run on the local frames and the fp32 prediction
    is all-gathered — 256 bytes a token instead of 2 C — into the caller's ``out``, padding dropped."""

    def __init__(self, sample_size=128, patch_size=2, in_channels=16, num_layers=18, attention_head_dim=64, num_attention_heads=18,
                 joint_attention_dim=4096, caption_projection_dim=1152, pooled_projection_dim=2048, out_channels=16,
                 pos_embed_max_size=96, rope_scaling_factor=1.0, device="cuda", dtype=torch.bfloat16):
        from types import SimpleNamespace

        if attention_head_dim != HEAD_DIM:
            raise ValueError("the Vchitect attention kernels are built for head_dim 64")
        if dtype != torch.bfloat16:
            raise ValueError("the MI355X path computes in bf16 (fp32 accumulate)")
        self.out_channels = out_channels if out_channels is not None else in_channels
        self.inner_dim = C = num_attention_heads * attention_head_dim
        if caption_projection_dim != C:
            raise ValueError("caption_projection_dim must equal heads * 64 (the joint blocks add the two streams' projections)")
        if patch_size * patch_size * self.out_channels > 192:
            raise ValueError("proj_out is padded to one 192-column GEMM tile")
        self.config = SimpleNamespace(sample_size=sample_size, patch_size=patch_size, in_channels=in_channels, num_layers=num_layers,
                                      attention_head_dim=attention_head_dim, num_attention_heads=num_attention_heads,
                                      joint_attention_dim=joint_attention_dim, caption_projection_dim=caption_projection_dim,
                                      pooled_projection_dim=pooled_projection_dim, out_channels=self.out_channels,
                                      pos_embed_max_size=pos_embed_max_size, rope_scaling_factor=rope_scaling_factor)
        self.device, self.dtype = torch.device(device), dtype
        self.transformer_blocks = [JointTransformerBlock(C, num_attention_heads, C, i == num_layers - 1, rope_scaling_factor, self.device)
                                   for i in range(num_layers)]
        self.w: Dict[str, torch.Tensor] = {}
        self._ws = Workspace(self.device, dtype)
        self._buf = self._ws.buf   # bound to this Workspace: _ws is cleared, never replaced (rebind _buf with it otherwise)
        self._pos_crop = {}
        self.parallel_manager, self._sp = None, None
        self.use_programs = True     # samplers record a step once and replay it (pipeline_vchitect.py); False: eager issue
        self.pos_embed = sincos_2d(C, pos_embed_max_size, sample_size // patch_size)      # [max * max, C] fp32 (PatchEmbed.pos_embed)

    TOP = ("pos_embed.proj", "time_text_embed.timestep_embedder.linear_1", "time_text_embed.timestep_embedder.linear_2",
           "time_text_embed.text_embedder.linear_1", "time_text_embed.text_embedder.linear_2", "context_embedder", "norm_out.linear",
           "proj_out")

    def expected_keys(self):
        keys = [f"{l}.{p}" for l in self.TOP for p in ("weight", "bias")]
        for i, b in enumerate(self.transformer_blocks):
            keys += [f"transformer_blocks.{i}.{k}" for k in b.expected_keys()]
        return keys

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        missing = [k for k in self.expected_keys() if k not in sd]
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:8]}{'...' if len(missing) > 8 else ''}")
        C, cfg = self.inner_dim, self.config
        dev = lambda t: t.detach().to(device=self.device, dtype=self.dtype).contiguous()
        for l in self.TOP:
            for p in ("weight", "bias"):
                self.w[f"{l}.{p}"] = dev(sd[f"{l}.{p}"].reshape(sd[f"{l}.{p}"].shape[0], -1) if p == "weight" else sd[f"{l}.{p}"])
        if "pos_embed.pos_embed" in sd:          # the checkpoint's persistent buffer [1, max * max, C]
            self.pos_embed = sd["pos_embed.pos_embed"].detach().float().reshape(-1, C).cpu()
            self._pos_crop = {}
        # every linear(silu(temb)) of the blocks in one matrix (video 6C, then context 6C or 2C, per block)
        ws, bs, self._mod_off, off = [], [], [], 0
        for i, b in enumerate(self.transformer_blocks):
            b.load_state_dict(sd, f"transformer_blocks.{i}.")
            pre = f"transformer_blocks.{i}."
            ws += [sd[pre + "norm1.linear.weight"], sd[pre + "norm1_context.linear.weight"]]
            bs += [sd[pre + "norm1.linear.bias"], sd[pre + "norm1_context.linear.bias"]]
            nc = ws[-1].shape[0]
            self._mod_off.append((off, off + 6 * C))
            off += 6 * C + nc
        self.w["_mod.weight"], self.w["_mod.bias"] = dev(torch.cat(ws, 0)), dev(torch.cat(bs, 0))
        # proj_out rows are ordered (dy, dx, c) (the einsum of :578); the unpatchify kernel reads (c, dy, dx): permute once, pad to a tile
        p, co = cfg.patch_size, self.out_channels
        po = torch.zeros(192, C)
        pb = torch.zeros(192)
        po[: p * p * co] = sd["proj_out.weight"].reshape(p, p, co, C).permute(2, 0, 1, 3).reshape(p * p * co, C)
        pb[: p * p * co] = sd["proj_out.bias"].reshape(p, p, co).permute(2, 0, 1).reshape(-1)
        self.w["_proj_out.weight"], self.w["_proj_out.bias"] = dev(po), dev(pb)
        return self

    def enable_parallel(self, dp_size=1, sp_size=1, enable_cp=False, parallel_mgr=None, copy_executor=None):
        """vchitect_transformer_3d.py:326-338.  ``parallel_mgr``: an injected manager (sp_size, sp_group, ...; the group a
        torch.distributed ProcessGroup or an object of dsp's group protocol); without one the mesh dp x cp x sp must be the size of the
        process group initialised in this process, else a NotImplementedError (no group of that size here).  The CFG split (enable_cp
        with more than one rank) is not built."""
        mgr = _resolve_parallel(dp_size, sp_size, enable_cp, parallel_mgr)
        self.parallel_manager = mgr
        if mgr is None:
            self._sp = None
        else:
            kw = {} if copy_executor is None else {"copy_executor": copy_executor}
            self._sp = dsp.SequenceParallel(mgr.sp_group, **kw)
        for i, b in enumerate(self.transformer_blocks):
            b.attn.parallel_manager = mgr
            b.attn.enable_parallel(sp=self._sp, tag=str(i))

    def _local_frames(self, F):
        """(first frame, frames held, real frames among them) of this rank: Fl = ceil(F / P), rank r holds [r Fl, (r + 1) Fl)."""
        sp = self._sp
        if sp is None:
            return 0, F, F
        Fl = -(-F // sp.P)
        f0 = sp.rank * Fl
        return f0, Fl, max(0, min(Fl, F - f0))

    def reset_pab_state(self):
        for b in self.transformer_blocks:
            b.attn.reset_pab_state()

    def step_timesteps(self, rows: int) -> torch.Tensor:
        """The resident fp32 [B * F] buffer the timestep embedding reads.  forward() fills it from ``timestep``; a sampler that replays a
        recorded step writes the step's timestep here instead (the one per-step input besides the latents)."""
        return self._buf("timesteps", (rows,), torch.float32)

    def cropped_pos_embed(self, hp: int, wp: int) -> torch.Tensor:
        """PatchEmbed.cropped_pos_embed: the centre hp x wp window of the max x max table, bf16 [hp * wp, C] on the device."""
        if (hp, wp) not in self._pos_crop:
            m = self.config.pos_embed_max_size
            if hp > m or wp > m:
                raise ValueError(f"a {hp} x {wp} token grid does not fit the {m} x {m} position table")
            top, left = (m - hp) // 2, (m - wp) // 2
            t = self.pos_embed.reshape(m, m, -1)[top:top + hp, left:left + wp].reshape(hp * wp, -1)
            self._pos_crop[(hp, wp)] = t.to(device=self.device, dtype=self.dtype).contiguous()
        return self._pos_crop[(hp, wp)]

    @torch.no_grad()
    def forward(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None, joint_attention_kwargs=None,
                return_dict: bool = True, *, out: torch.Tensor = None):
        """``out`` (an extension): a contiguous fp32 buffer of B * F * out_channels * H * W values the prediction is written to."""
        from types import SimpleNamespace

        w, C, cfg, dev = self.w, self.inner_dim, self.config, self.device
        p = cfg.patch_size
        B, F, cin, Hh, Ww = hidden_states.shape
        Hp, Wp = Hh // p, Ww // p
        S, BF = Hp * Wp, B * F
        enc = encoder_hidden_states.to(device=dev, dtype=self.dtype)
        if enc.shape[0] == B and F > 1:
            enc = enc[:, None].expand(B, F, *enc.shape[1:])
        elif enc.shape[0] != BF:
            raise ValueError("encoder_hidden_states must hold B or B * F samples")
        L = enc.shape[-2]
        enc = enc.reshape(B, F, L, enc.shape[-1])          # (a view: [B * F, L, D] as it lies, or the expanded [B, L, D])
        sp = self._sp
        f0, Fl, nreal = self._local_frames(F)       # single rank: (0, F, F)
        BFl = B * Fl
        # ---- temb = time_text_embed(timestep, pooled) (:540), computed for the B*Fl rows of cur_temb = temb.repeat(Fl, 1) (:548)
        ts = torch.as_tensor(timestep).detach().to("cpu").float().reshape(-1)
        timestep_int = int(ts[0])
        if ts.numel() != B:
            ts = ts.expand(B) if ts.numel() == 1 else ts[:B]
        pooled = pooled_projections.to(device=dev, dtype=self.dtype).reshape(B, -1)
        tsb = self.step_timesteps(BF)            # (the sampler writes B * F rows whatever the shard: the first B * Fl are read)
        tsb.copy_(ts.repeat(F))
        tsb = tsb[:BFl]
        tp = ops.timestep_embedding(tsb, 256)
        te = "time_text_embed.timestep_embedder."
        e1 = ops.linear_small(tp, w[te + "linear_1.weight"], w[te + "linear_1.bias"], act_out=ops.ACT_SILU)
        temb = ops.linear_small(e1, w[te + "linear_2.weight"], w[te + "linear_2.bias"])
        tx = "time_text_embed.text_embedder."
        p1 = ops.linear_small(pooled.repeat(Fl, 1).contiguous(), w[tx + "linear_1.weight"], w[tx + "linear_1.bias"], act_out=ops.ACT_SILU)
        ops.add_rows(temb, ops.linear_small(p1, w[tx + "linear_2.weight"], w[tx + "linear_2.bias"]))     # [B*Fl, C]; rows 0 .. B-1 = temb
        mod = ops.linear_small(temb, w["_mod.weight"], w["_mod.bias"], act_in=ops.ACT_SILU)           # [B*Fl, sum of the blocks' columns]
        ms = mod.shape[1]
        mod_out = ops.linear_small(temb[:B], w["norm_out.linear.weight"], w["norm_out.linear.bias"], act_in=ops.ACT_SILU)   # [B, 2C]: scale | shift
        # ---- patch embed + cropped position table (:483-487), context_embedder (:541)
        z = hidden_states.to(device=dev, dtype=torch.float32)
        x, y = self._buf("x", (BFl * S, C)), self._buf("y", (BFl * L, C))
        if sp is None:
            enc = enc.reshape(BF * L, -1).contiguous()
            cols = ops.im2col_patch(z.contiguous(), B, p)
            ops.gemm(cols, w["pos_embed.proj.weight"], w["pos_embed.proj.bias"], out=x)
            ops.add_bcast_rows(x, self.cropped_pos_embed(Hp, Wp), 1, S)
            ops.gemm(enc, w["context_embedder.weight"], w["context_embedder.bias"], out=y)
        else:
            # this rank's frames of every sample, straight from its slice of the latents and of the text (a view when B = 1: nothing
            # is copied); the rows of the frames past F are zero (set_pad("temporal", F) + split_from_second_dim, :543-546)
            for b in range(B if nreal else 0):
                xb, yb = x[b * Fl * S:(b * Fl + nreal) * S], y[b * Fl * L:(b * Fl + nreal) * L]
                cols = ops.im2col_patch(z[b:b + 1, f0:f0 + nreal].contiguous(), 1, p)
                ops.gemm(cols, w["pos_embed.proj.weight"], w["pos_embed.proj.bias"], out=xb)
                ops.add_bcast_rows(xb, self.cropped_pos_embed(Hp, Wp), 1, S)
                ops.gemm(enc[b, f0:f0 + nreal].reshape(nreal * L, -1).contiguous(), w["context_embedder.weight"],
                         w["context_embedder.bias"], out=yb)
            if nreal < Fl:
                npad = Fl - nreal
                for t, n in ((x, S), (y, L)):       # (a copy of nothing: vsys_copy_4d zero-fills outside n1_valid = 0)
                    ops.copy_4d(t, t[nreal * n:], B, npad * n, 1, C, (0, 0, 0), (Fl * n * C, C, 0), n1_valid=0)
        use_pab = pab.enable_pab()
        for i, blk in enumerate(self.transformer_blocks):
            v0, c0 = self._mod_off[i]
            blk.forward(x, y, mod[0, v0:], mod[0, c0:], ms, B, Fl, self._buf, timestep_int if use_pab else None, F)
        # ---- norm_out (AdaLayerNormContinuous: scale | shift), proj_out, unpatchify (:564-581)
        xo = ops.ln_modulate(x, None, None, mod_out[0, C:2 * C], mod_out[0, 0:C], Fl * S, mod_stride=2 * C, eps=1e-6,
                             out=self._buf("xn", (BFl * S, C)))
        po = ops.gemm(xo, w["_proj_out.weight"], w["_proj_out.bias"], out=self._buf("proj", (BFl * S, 192)))
        if sp is None:
            out = ops.unpatchify_cvx(po, B, F, Hp, Wp, self.out_channels, p, out=out).view(BF, self.out_channels, Hh, Ww)
        else:
            # gather_from_second_dim (:561-562) moved behind the row-wise tail: the fp32 prediction of the local frames travels
            n = self.out_channels * Hh * Ww
            if out is None:
                out = torch.empty(BF * n, dtype=torch.float32, device=dev)
            assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == BF * n
            loc = ops.unpatchify_cvx(po, B, Fl, Hp, Wp, self.out_channels, p, out=self._buf("pred_local", (BFl * n,), torch.float32))
            parts = self._buf("pred_parts", (sp.P * BFl * n,), torch.float32)
            dst, P = out.view(B, F, n), sp.P

            def drop_padding():     # rows (rank, b, f) -> (b, f), frames past F dropped: one strided copy (a view at B = 1)
                dst.copy_(parts.view(P, B, Fl, n).permute(1, 0, 2, 3).reshape(B, P * Fl, n)[:, :F])

            dsp.all_gather_into_tensor(parts, loc, sp.group, after=drop_padding)
            program.keep(out)
            out = out.view(BF, self.out_channels, Hh, Ww)
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)

    __call__ = forward


def synth_state_dict(num_layers=2, num_heads=3, in_channels=16, out_channels=16, patch_size=2, joint_attention_dim=64,
                     pooled_projection_dim=64, seed: int = 777) -> Dict[str, torch.Tensor]:
    """Seeded random weights with the reference's VchitectXLTransformerModel key names (no pretrained weights offline)."""
    g = torch.Generator().manual_seed(seed)
    C = num_heads * HEAD_DIM
    sd: Dict[str, torch.Tensor] = {}

    def lin(name, n_out, n_in, scale=None):
        s = min(0.08, n_in ** -0.5) if scale is None else scale
        sd[name + ".weight"] = torch.randn(n_out, n_in, generator=g) * s
        sd[name + ".bias"] = torch.randn(n_out, generator=g) * 0.02

    sd["pos_embed.proj.weight"] = torch.randn(C, in_channels, patch_size, patch_size, generator=g) * 0.1
    sd["pos_embed.proj.bias"] = torch.randn(C, generator=g) * 0.02
    lin("time_text_embed.timestep_embedder.linear_1", C, 256)
    lin("time_text_embed.timestep_embedder.linear_2", C, C)
    lin("time_text_embed.text_embedder.linear_1", C, pooled_projection_dim)
    lin("time_text_embed.text_embedder.linear_2", C, C)
    lin("context_embedder", C, joint_attention_dim)
    for i in range(num_layers):
        pre, last = f"transformer_blocks.{i}.", i == num_layers - 1
        lin(pre + "norm1.linear", 6 * C, C, 0.02)
        lin(pre + "norm1_context.linear", (2 if last else 6) * C, C, 0.02)
        for k, v in synth_attention_state_dict(C, last, seed=seed + 1 + i).items():
            sd[pre + "attn." + k] = v
        lin(pre + "ff.net.0.proj", 4 * C, C)
        lin(pre + "ff.net.2", C, 4 * C)
        if not last:
            lin(pre + "ff_context.net.0.proj", 4 * C, C)
            lin(pre + "ff_context.net.2", C, 4 * C)
    lin("norm_out.linear", 2 * C, C, 0.02)
    lin("proj_out", patch_size * patch_size * out_channels, C)
    return sd
