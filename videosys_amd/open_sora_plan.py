"""Open-Sora-Plan v1.2 transformer (OpenSoraT2V) on MI355X — host mirror of
videosys/models/transformers/open_sora_plan_v120_transformer_3d.py (OpenSoraT2V :1464-2112, BasicTransformerBlock :1092-1455,
AttnProcessor2_0 :837-961, RoPE3D / PositionGetter3D :39-118, PatchEmbed2D :245-369; AdaLayerNormSingle and the PixArt caption
projection are the ones Latte uses).

Same constructor keyword names, same ``forward(hidden_states, timestep, encoder_hidden_states, attention_mask,
encoder_attention_mask, use_image_num, return_dict)`` and ``[B, out_channels, T, H, W]`` result, same state-dict key names — every
tensor op of the per-step path is a call into libvideosys_amd.so.  What is new for this family is the attention: full 3-D
self-attention over all T * H/p * W/p tokens at head dim 96 with RoPE3D, and masked cross-attention at head dim 96
(vsys_attn_prep_kv96 + vsys_flash_attn_d96, open_sora_plan_ops.py).  Everything else runs on kernels other families use: the
patch-embed kernel (no position table under RoPE: a zero table), the fused-epilogue GEMMs, vsys_ln_modulate, the gate-add and
add-rows kernels, vsys_mod_table, vsys_unpatchify_cvx.  The ``nthwopqc->nctohpwq`` unpatchify (:2099) is B * out_channels calls of
that kernel, one [T, 1, H, W] problem per (sample, channel) — a choice, not a necessity: a dedicated kernel would be one launch
instead of 16 at the production geometry, about 0.1 ms of a 154 ms step, and was not worth a new entry point.

Built: norm_type="ada_norm_single", use_rope=True, downsampler=None, patch_size_t=1, activation_fn="gelu-approximate",
attention_head_dim=96, biased projections, LayerNorms without affine, out_channels in {in_channels, 2 in_channels},
use_image_num=0.  Anything else raises NotImplementedError at construction — nothing is approximated.  The CausalVAE decode, mT5, the
sampler and the pipeline / config classes are vae_open_sora_plan.py and pipeline_open_sora_plan.py; not built (follow-ups): the v1.1 pipeline
(its transformer is open_sora_plan_v110.py), the CFG split (enable_cp).

Sequence parallelism (enable_parallel; :916-941,1716-1728,1896-1900,1975-1979).  The video tokens are split over
the P ranks at rest (split_sequence, dim 1: rank r holds tokens [r Nl, (r + 1) Nl), Nl = N / P — N % P != 0 is a ValueError, as the
reference's assert at comm.py:163, this family has no padding): the patch embedding, the modulation, cross-attention (the text K / V
are replicated for all heads), both projections and the MLP run on the local rows [B * Nl, C]; self-attention swaps sequence for
heads around the attention (all_to_all_comm: H / P heads, all N tokens, RoPE3D over the whole sequence) through dsp.UlyssesParallel
with no text rows; the tail all-gathers the projected rows (192 columns, not the hidden states) and every rank returns the full
prediction.  Three routes for the swap: "rows" over the one-kernel peer-to-peer exchange, "rows" over all_to_all_single (pack, unpack,
pack, unpack around the plain kernels) and "image" over all_to_all_single (vsys_attn_prep_kv96_img / vsys_flash_attn_d96_img read the
receive image as it lies and write the send image of the way back: pack and unpack only) — ``attn_route`` / DEFAULT_A2A_ROUTE.

Differences that do not change results:
  * attn1's to_q / to_k / to_v are one [3C, C] GEMM; attn2's to_k / to_v run once per (prompt, mask) — the text is constant over the
    steps — and their attention layouts are kept per block;
  * the cross-attention mask: the reference adds a bias of -10000 on hidden text keys (:1846); here sample b attends to its first
    kv_lens[b] keys.  exp(-10000 + s - m) underflows to exactly 0 in fp32 (and in bf16 / fp64) whenever one key of the row is visible
    (then m >= that key's logit, and |s| stays far below 10000 - 87), so the hard mask and the bias give the same softmax to below
    fp32 resolution.  The mask must be a prefix of ones with at least one visible key per sample (ValueError otherwise); the host
    check runs once per distinct mask tensor;
  * a video ``attention_mask`` of all ones is dropped, as the reference itself does (:930); any other is NotImplementedError.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict

import torch

from . import dsp
from . import open_sora_plan_ops as oops
from . import ops, pab
from .pipeline import VideoSysPipelineOutput
from .utils import load_weights, same_tensor
from .workspace import Workspace

HEAD_DIM = oops.HEAD_DIM


def rope3d_tables(T: int, H: int, W: int, interpolation_scale_thw=(1.0, 1.0, 1.0), rope_dtype=torch.bfloat16, head_dim: int = HEAD_DIM):
    """The per-token tables the attention kernels take: (cos, sin) fp32 [T*H*W, head_dim] on the CPU, tokens ordered (t, h, w) as
    PositionGetter3D lists them (:47-58), columns [frame | row | column] chunks of head_dim / 3 as RoPE3D.forward applies them
    (:109-117).  RoPE3D.get_cos_sin (:73-82) restated: fp32 angles position / interpolation_scale * 10000^(-2i / D), cast to
    ``rope_dtype`` BEFORE cos / sin, the half-table repeated twice.  ``rope_dtype`` = the dtype the reference model runs in (bf16:
    this project's arithmetic); the values are widened to fp32 for the kernels.

    One property of the reference is kept on purpose: get_cos_sin caches its tables under (D, seq_len, device, dtype) — WITHOUT the
    interpolation scale (:74) — and forward asks for the frame, row and column tables in that order (:109-111).  Two axes of equal
    length therefore share the table of the earlier one, whatever the later one's scale (a square token grid takes the row scale
    for its columns too): that is what the reference computes and what a checkpoint was trained with, so it is restated, and
    tests/golden/osp_v120_fwd_small.pt pins it with T = H = 4 at scales (2, 1.5, 2) against the reference's own class.  NOT
    restated: the cache outlives a forward, so a reference model that has seen another geometry before may also reuse a table
    across calls; the tables here depend on this call's geometry alone (the reference's first forward after construction)."""
    D = head_dim // 3
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    cs, sn, made = [], [], {}
    reps = (H * W, W, 1)
    for axis, n in enumerate((T, H, W)):
        if n not in made:      # the reference's cache key has no scale (see the docstring): an equal length reuses the earlier axis's table
            t = torch.arange(n, dtype=inv_freq.dtype) / interpolation_scale_thw[axis]
            freqs = torch.einsum("i,j->ij", t, inv_freq).to(rope_dtype)
            freqs = torch.cat((freqs, freqs), dim=-1)
            made[n] = (freqs.cos(), freqs.sin())
        # position of token (t, h, w) along this axis: each value repeated over the faster axes, the run tiled over the slower ones
        idx = torch.arange(n).repeat_interleave(reps[axis]).repeat(T * H * W // (n * reps[axis]))
        cs.append(made[n][0][idx])
        sn.append(made[n][1][idx])
    return torch.cat(cs, dim=-1).float().contiguous(), torch.cat(sn, dim=-1).float().contiguous()


class _NoGroupOfThatSize(NotImplementedError, AssertionError):
    """enable_parallel without an injected manager asked for a dp x cp x sp mesh that is not the size of the process group initialised
    in this process (none = 1).  A NotImplementedError for callers written when sequence parallelism was not built; also the
    AssertionError dsp.ParallelManager raises for the same mismatch."""


def _resolve_parallel(dp_size, sp_size, enable_cp, parallel_mgr):
    """:1716-1728 (the reference halves an even sp_size under enable_cp and builds a dp x cp x sp mesh).  Returns the manager to use,
    or None for a single rank.  The CFG split (cp > 1) is not built."""
    import torch.distributed as dist

    if enable_cp:
        raise NotImplementedError("OpenSoraT2V on MI355X: the CFG split (enable_cp) is not built; shard with enable_cp=False")
    if parallel_mgr is not None:
        if getattr(parallel_mgr, "cp_size", 1) > 1:
            raise NotImplementedError("OpenSoraT2V on MI355X: the CFG split (cp_size > 1) is not built")
        return parallel_mgr if parallel_mgr.sp_size > 1 else None
    dp, sp = dp_size or 1, sp_size or 1
    world = dist.get_world_size() if dist.is_initialized() else 1
    if dp * sp != world:
        raise _NoGroupOfThatSize(f"OpenSoraT2V sequence parallelism: there is no process group of {dp} x 1 x {sp} = {dp * sp} ranks in this "
                                 f"process (the initialised world has {world}); initialise torch.distributed with that many ranks, or "
                                 f"hand in a manager (parallel_mgr=)")
    return dsp.ParallelManager(dp, 1, sp) if sp > 1 else None


def _to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


class OpenSoraT2V:
    """Drop-in for the reference OpenSoraT2V at the operator boundary ``transformer(latents, ...)[0]``."""

    def __init__(self, num_attention_heads=16, attention_head_dim=88, in_channels=None, out_channels=None, num_layers=1, dropout=0.0,
                 norm_num_groups=32, cross_attention_dim=None, attention_bias=False, sample_size=None, sample_size_t=None,
                 num_vector_embeds=None, patch_size=None, patch_size_t=None, activation_fn="geglu", num_embeds_ada_norm=None,
                 use_linear_projection=False, only_cross_attention=False, double_self_attention=False, upcast_attention=False,
                 norm_type="layer_norm", norm_elementwise_affine=True, norm_eps=1e-5, attention_type="default", caption_channels=None,
                 interpolation_scale_h=None, interpolation_scale_w=None, interpolation_scale_t=None, use_additional_conditions=None,
                 attention_mode="xformers", downsampler=None, use_rope=False, use_stable_fp32=False, device="cuda",
                 dtype=torch.bfloat16, rope_dtype=torch.bfloat16):
        def unbuilt(what):
            raise NotImplementedError(f"OpenSoraT2V on MI355X: {what} is not built (open_sora_plan.py lists what is)")

        if norm_type != "ada_norm_single":
            unbuilt(f"norm_type={norm_type!r}")
        if not use_rope:
            unbuilt("use_rope=False (absolute position embeddings)")
        if downsampler is not None:
            unbuilt(f"downsampler={downsampler!r}")
        if patch_size_t != 1:
            unbuilt(f"patch_size_t={patch_size_t!r}")
        if activation_fn != "gelu-approximate":
            unbuilt(f"activation_fn={activation_fn!r}")
        if attention_head_dim != HEAD_DIM:
            unbuilt(f"attention_head_dim={attention_head_dim} (the attention kernels are built for 96)")
        if in_channels is None or patch_size is None or sample_size is None or sample_size_t is None:
            raise ValueError("in_channels, patch_size, sample_size and sample_size_t are required (:1569,:1590-1591)")
        out_channels = in_channels if out_channels is None else out_channels
        if out_channels not in (in_channels, 2 * in_channels):
            unbuilt(f"out_channels={out_channels} with in_channels={in_channels}")
        C = num_attention_heads * attention_head_dim
        if norm_elementwise_affine or not attention_bias:
            unbuilt("LayerNorm affine weights / projections without bias")
        if only_cross_attention or double_self_attention or upcast_attention or use_linear_projection or use_stable_fp32:
            unbuilt("only_cross_attention / double_self_attention / upcast_attention / use_linear_projection / use_stable_fp32")
        if attention_type != "default" or num_embeds_ada_norm is not None or num_vector_embeds is not None or dropout:
            unbuilt("gated attention types / ada_norm embeddings / discrete inputs / dropout")
        if cross_attention_dim != C or caption_channels is None:
            unbuilt(f"cross_attention_dim={cross_attention_dim} != {C} or no caption projection")
        if patch_size * patch_size * out_channels > 192 or C % 192:
            unbuilt("proj_out wider than one 192-column GEMM tile, or a hidden size that is no multiple of 192")
        if dtype != torch.bfloat16:
            raise ValueError("the MI355X path computes in bf16 (fp32 accumulate)")
        sample_size = _to_2tuple(sample_size)
        # interpolation scales as _init_patched_inputs derives them (:1600-1617,1658)
        it = ((sample_size_t - 1) // 16 + 1) if sample_size_t % 2 == 1 else sample_size_t / 16
        it = interpolation_scale_t if interpolation_scale_t is not None else it
        ih = interpolation_scale_h if interpolation_scale_h is not None else sample_size[0] / 30
        iw = interpolation_scale_w if interpolation_scale_w is not None else sample_size[1] / 40
        self.interpolation_scale_thw = (it, ih, iw)
        self.config = SimpleNamespace(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim,
                                      in_channels=in_channels, out_channels=out_channels, num_layers=num_layers,
                                      cross_attention_dim=cross_attention_dim, attention_bias=attention_bias, sample_size=sample_size,
                                      sample_size_t=sample_size_t, patch_size=patch_size, patch_size_t=patch_size_t,
                                      activation_fn=activation_fn, norm_type=norm_type, norm_elementwise_affine=norm_elementwise_affine,
                                      norm_eps=norm_eps, caption_channels=caption_channels, interpolation_scale_h=interpolation_scale_h,
                                      interpolation_scale_w=interpolation_scale_w, interpolation_scale_t=interpolation_scale_t,
                                      attention_mode=attention_mode, downsampler=downsampler, use_rope=use_rope, hidden_size=C)
        self.H, self.C, self.L = num_attention_heads, C, num_layers
        self.inner_dim = C
        self.patch_size, self.patch_size_t = patch_size, patch_size_t
        self.in_channels, self.out_channels = in_channels, out_channels
        self.device, self.dtype, self.rope_dtype = torch.device(device), dtype, rope_dtype
        self.w: Dict[str, torch.Tensor] = {}
        self.parallel_manager = SimpleNamespace(sp_size=1, cp_size=1, dp_size=1, dp_rank=0, sp_group=None, cp_group=None)
        self._sp = None
        self.attn_route = None      # None: DEFAULT_A2A_ROUTE; "rows" | "image" force one (_route)
        self.states = [pab.BlockState(i, False) for i in range(num_layers)]
        self.last_decisions = []     # per block of the last forward: (spatial broadcast?, cross broadcast?)
        self._ws = Workspace(self.device, dtype)
        self._buf = self._ws.buf   # bound to this Workspace: _ws is cleared, never replaced (rebind _buf with it otherwise)
        self._text_cache = None
        self._mask_checked = None
        self._video_mask_checked = None

    # ------------------------------------------------------------------ weights
    def expected_shapes(self) -> Dict[str, tuple]:
        """name -> shape of the reference's ``state_dict()`` for this configuration."""
        C, cfg = self.C, self.config
        p = cfg.patch_size
        sh = {"pos_embed.proj.weight": (C, cfg.in_channels, p, p), "pos_embed.proj.bias": (C,)}

        def lin(name, n_out, n_in):
            sh[name + ".weight"], sh[name + ".bias"] = (n_out, n_in), (n_out,)

        for i in range(self.L):
            pre = f"transformer_blocks.{i}"
            sh[pre + ".scale_shift_table"] = (6, C)
            for a in ("attn1", "attn2"):
                for l in ("to_q", "to_k", "to_v", "to_out.0"):
                    lin(f"{pre}.{a}.{l}", C, C)
            lin(pre + ".ff.net.0.proj", 4 * C, C)
            lin(pre + ".ff.net.2", C, 4 * C)
        sh["scale_shift_table"] = (2, C)
        lin("proj_out", cfg.patch_size_t * p * p * cfg.out_channels, C)
        lin("adaln_single.emb.timestep_embedder.linear_1", C, 256)
        lin("adaln_single.emb.timestep_embedder.linear_2", C, C)
        lin("adaln_single.linear", 6 * C, C)
        lin("caption_projection.linear_1", C, cfg.caption_channels)
        lin("caption_projection.linear_2", C, C)
        return sh

    def expected_keys(self):
        return list(self.expected_shapes())

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        shapes = self.expected_shapes()
        for k, s in shapes.items():
            if k in sd and tuple(sd[k].shape) != s:
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)}, expected {s}")
        load_weights(self.w, sd, list(shapes), device=self.device, dtype=self.dtype, strict=strict, reshape=("pos_embed.proj.weight",))
        dev = lambda t: t.detach().to(device=self.device, dtype=self.dtype).contiguous()
        C, cfg = self.C, self.config
        for i in range(self.L):
            p = f"transformer_blocks.{i}"
            self.w[p + ".attn1.qkv.weight"] = dev(torch.cat([sd[f"{p}.attn1.{l}.weight"] for l in ("to_q", "to_k", "to_v")], 0))
            self.w[p + ".attn1.qkv.bias"] = dev(torch.cat([sd[f"{p}.attn1.{l}.bias"] for l in ("to_q", "to_k", "to_v")], 0))
            self.w[p + ".attn2.kv.weight"] = dev(torch.cat([sd[f"{p}.attn2.{l}.weight"] for l in ("to_k", "to_v")], 0))
            self.w[p + ".attn2.kv.bias"] = dev(torch.cat([sd[f"{p}.attn2.{l}.bias"] for l in ("to_k", "to_v")], 0))
        self.w["_all_tables"] = torch.stack([self.w[f"transformer_blocks.{i}.scale_shift_table"].reshape(-1) for i in range(self.L)]).contiguous()
        # proj_out rows are ordered (dy, dx, c) (the einsum of :2099); the unpatchify kernel reads (c, dy, dx): permute once, pad to a tile
        pp, co = cfg.patch_size, cfg.out_channels
        po, pb = torch.zeros(192, C), torch.zeros(192)
        po[: pp * pp * co] = sd["proj_out.weight"].float().reshape(pp, pp, co, C).permute(2, 0, 1, 3).reshape(pp * pp * co, C)
        pb[: pp * pp * co] = sd["proj_out.bias"].float().reshape(pp, pp, co).permute(2, 0, 1).reshape(-1)
        self.w["_proj_out.weight"], self.w["_proj_out.bias"] = dev(po), dev(pb)
        self._text_cache = None
        return self

    # Which self-attention route runs over all_to_all_single when nothing is forced: the image kernels, whose per-rank step (wire
    # stubbed, 29x480p, 32 layers) was 26.97 ms (26.88 .. 27.14) against 27.56 ms (27.47 .. 27.73) at 8 ranks and 48.65 against 49.52 ms
    # at 4 — median below, ranges apart (profiles/osp_sp_timing.json).  "rows" stays reachable through ``attn_route``;
    # the one-kernel peer-to-peer exchange has no receive image and always takes "rows".
    DEFAULT_A2A_ROUTE = "image"

    def enable_parallel(self, dp_size=1, sp_size=1, enable_cp=False, parallel_mgr=None, copy_executor=None):
        """:1716-1728.  Ulysses sequence parallelism over ``sp_size`` ranks (module docstring); the CFG split (enable_cp, or an injected
        manager with cp_size > 1) is not built.  Without a manager the mesh must be the size of the process group initialised in this
        process.  ``copy_executor``: the pack / unpack executor of dsp.UlyssesParallel (default: the HIP copy kernel)."""
        mgr = _resolve_parallel(dp_size, sp_size, enable_cp, parallel_mgr)
        if mgr is None:
            self.parallel_manager = SimpleNamespace(sp_size=1, cp_size=1, dp_size=1, dp_rank=0, sp_group=None, cp_group=None)
            self._sp = None
            return
        if self.H % mgr.sp_size:
            raise ValueError(f"Number of heads {self.H} must be divisible by sequence parallel size {mgr.sp_size}")
        kw = {} if copy_executor is None else {"copy_executor": copy_executor}
        self.parallel_manager = mgr
        self._sp = dsp.UlyssesParallel(mgr.sp_group, text_rows=False, **kw)

    def _route(self):
        """"rows" or "image" for this call."""
        if self._sp.p2p is not None:
            return "rows"
        r = self.attn_route or self.DEFAULT_A2A_ROUTE
        if r not in ("rows", "image"):
            raise ValueError(f"attn_route {r!r}: expected 'rows' or 'image'")
        return r

    def _self_attention(self, qkv, cos, sin, kp, vt, B, N):
        """qkv [B * Nl, 3C] (local rows) -> the attention output [B * Nl, C] of the local rows, all heads."""
        sp, C, H = self._sp, self.C, self.H
        if sp is None:
            oops.attn_prep_kv96(qkv[:, C:2 * C], qkv[:, 2 * C:], cos, sin, kp, vt, B, H, N)
            return oops.flash_attn96(qkv[:, :C], cos, sin, kp, vt, None, self._buf("attn_out", (B * N, C)), B, H, N, N)
        P = sp.P
        Nl, Hl, hw = N // P, H // P, C // P
        out = self._buf("attn_out", (B, Nl, C))
        if self._route() == "rows":      # sequence -> heads, the plain kernels on [B, N, H/P heads], heads -> sequence
            qh = sp.scatter_heads(qkv, B, 0, N, C, out=self._buf("qkv_h", (B, N, 3 * hw)))
            oops.attn_prep_kv96(qh[:, hw:2 * hw], qh[:, 2 * hw:], cos, sin, kp, vt, B, Hl, N)
            ao = oops.flash_attn96(qh[:, :hw], cos, sin, kp, vt, None, self._buf("attn_out_h", (B * N, hw)), B, Hl, N, N)
            return sp.gather_heads(ao, B, 0, N, C, out=out)
        # "image": the kernels read the receive image [P (source)][B][Nl][3][hw] as it lies and write the send image
        # [P (destination)][B][Nl][hw] of the way back
        img = sp.scatter_heads_image(qkv, B, N, C).view(P * B * Nl, 3 * hw)
        oops.attn_prep_kv96_img(img[:, hw:2 * hw], img[:, 2 * hw:], cos, sin, kp, vt, B, Hl, N, Nl, B * Nl)
        send = sp.heads_send_image(B, N, C, qkv)
        oops.flash_attn96_img(img[:, :hw], cos, sin, kp, vt, None, send.view(P * B * Nl, hw), B, Hl, N, N, Nl, B * Nl, B * Nl)
        return sp.gather_heads_image(send, B, N, C, out=out)

    def reset_pab_state(self):
        pab.reset_states(self.states)

    def reset_text_cache(self):
        self._text_cache = None

    # ------------------------------------------------------------------ step-invariant state
    def _check_mask(self, mask, B, Lk):
        """encoder_attention_mask [B, 1, L] (1 = visible) -> per-sample key counts; checked once per distinct mask tensor."""
        c = self._mask_checked
        if c is not None and same_tensor(c[0], mask) and c[1] == (None if mask is None else mask._version):
            return c[2]
        if mask is None:
            lens = [Lk] * B
        else:
            if mask.numel() != B * Lk:
                raise ValueError(f"encoder_attention_mask has {mask.numel()} entries, expected [{B}, 1, {Lk}]")
            m = mask.detach().reshape(B, Lk).to("cpu") != 0
            lens = [int(v) for v in m.sum(dim=1).tolist()]
            for b in range(B):
                if lens[b] == 0 or not bool(m[b, : lens[b]].all()):
                    raise ValueError("encoder_attention_mask must be a prefix of ones with at least one visible key per sample")
        self._mask_checked = (mask, None if mask is None else mask._version, lens)
        return lens

    def _check_video_mask(self, mask):
        """None or all ones (the reference drops such a mask itself, :930); the read-back happens once per distinct mask tensor."""
        c = self._video_mask_checked
        if mask is None or (c is not None and same_tensor(c[0], mask) and c[1] == mask._version):
            return
        if not bool((mask != 0).all()):
            raise NotImplementedError("a video attention_mask that hides tokens is not built (None or all ones)")
        self._video_mask_checked = (mask, mask._version)

    def _encode_text(self, y, mask):
        """Caption projection and every block's text K / V layouts, once per (encoder_hidden_states, mask)."""
        c = self._text_cache
        if (c is not None and same_tensor(c["y"], y) and c["y_version"] == y._version and same_tensor(c["mask"], mask)
                and (mask is None or c["mask_version"] == mask._version)):
            return c
        if y.dim() != 4 or y.shape[1] != 1:
            raise NotImplementedError("encoder_hidden_states must be [B, 1, L, caption_channels] (use_image_num = 0)")
        B, _, Lk, Cc = y.shape
        lens = self._check_mask(mask, B, Lk)
        C, H, w = self.C, self.H, self.w
        yb = y.to(device=self.device, dtype=self.dtype).reshape(B * Lk, Cc).contiguous()
        h = ops.linear_small(yb, w["caption_projection.linear_1.weight"], w["caption_projection.linear_1.bias"], act_out=ops.ACT_GELU_TANH)
        ye = ops.linear_small(h, w["caption_projection.linear_2.weight"], w["caption_projection.linear_2.bias"])
        kv_pad = ops.kv_pad_len(Lk)
        # resident per geometry: a second prompt of the same shape refills the SAME buffers, so a recorded step replays onto them
        kps = self._ws.once(("text_kp", B, Lk), lambda: torch.zeros(self.L, B, H, kv_pad, HEAD_DIM, dtype=self.dtype, device=self.device))
        vts = self._ws.once(("text_vt", B, Lk), lambda: torch.zeros(self.L, B, H, HEAD_DIM, kv_pad, dtype=self.dtype, device=self.device))
        kv_lens = self._ws.once(("text_lens", B, Lk), lambda: torch.zeros(B, dtype=torch.int32, device=self.device))
        kv_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        kv = self._buf("text_kv", (B * Lk, 2 * C))
        for d in range(self.L):
            pre = f"transformer_blocks.{d}.attn2.kv"
            ops.gemm(ye, w[pre + ".weight"], w[pre + ".bias"], out=kv)
            oops.attn_prep_kv96(kv[:, :C], kv[:, C:], None, None, kps[d], vts[d], B, H, Lk)
        self._text_cache = dict(y=y, y_version=y._version, mask=mask, mask_version=None if mask is None else mask._version,
                                lens=lens, kv_lens=kv_lens, kp=kps, vt=vts, Lk=Lk)
        return self._text_cache

    def _rope(self, T, gh, gw):
        def make():
            cos, sin = rope3d_tables(T, gh, gw, self.interpolation_scale_thw, self.rope_dtype, HEAD_DIM)
            return cos.to(self.device), sin.to(self.device)

        return self._ws.once(("rope", T, gh, gw), make)

    def step_timesteps(self, B: int) -> torch.Tensor:
        """The resident fp32 [B] buffer the timestep embedding reads.  forward() fills it from ``timestep``; a sampler that replays a
        recorded step writes the step's timestep here instead."""
        return self._buf("timesteps", (B,), torch.float32)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, hidden_states, timestep=None, encoder_hidden_states=None, added_cond_kwargs=None, class_labels=None,
                cross_attention_kwargs=None, attention_mask=None, encoder_attention_mask=None, use_image_num=0, return_dict=True,
                **kwargs):
        if use_image_num or class_labels is not None or cross_attention_kwargs:
            raise NotImplementedError("image joint training / class labels / cross_attention_kwargs are not built")
        self._check_video_mask(attention_mask)
        w, C, H, cfg, dev = self.w, self.C, self.H, self.config, self.device
        p = cfg.patch_size
        B, cin, T, Hh, Ww = hidden_states.shape
        if encoder_hidden_states.shape[0] != B:
            raise ValueError("batch sizes of latents and encoder_hidden_states do not agree")
        if Hh % p or Ww % p:
            raise ValueError("latent height and width must be multiples of the patch size")
        gh, gw = Hh // p, Ww // p
        N = T * gh * gw            # tokens of a sample, ordered (t, h, w)
        sp = self._sp
        P = 1 if sp is None else sp.P
        if N % P:
            raise ValueError(f"{N} video tokens cannot be split over {P} sequence-parallel ranks (comm.py:163; this family has no padding)")
        Nl = N // P                # ... of which this rank holds [rank Nl, (rank + 1) Nl) at rest
        Hl = H // P                # heads of this rank inside the self-attention
        C6 = 6 * C
        # ---- AdaLayerNormSingle: embedded_timestep and the 6C modulation row; per-block tables added in one kernel
        ts_host = torch.as_tensor(timestep).detach().to("cpu").float().reshape(-1)
        if ts_host.numel() != B:
            if ts_host.numel() != 1:
                raise ValueError("timestep must hold one value or one per sample")
            ts_host = ts_host.expand(B)
        tsb = self.step_timesteps(B)
        tsb.copy_(ts_host)
        f = ops.timestep_embedding(tsb, 256)
        e1 = ops.linear_small(f, w["adaln_single.emb.timestep_embedder.linear_1.weight"],
                              w["adaln_single.emb.timestep_embedder.linear_1.bias"], act_out=ops.ACT_SILU)
        emb = ops.linear_small(e1, w["adaln_single.emb.timestep_embedder.linear_2.weight"],
                               w["adaln_single.emb.timestep_embedder.linear_2.bias"])  # embedded_timestep [B, C]
        t6 = ops.linear_small(emb, w["adaln_single.linear.weight"], w["adaln_single.linear.bias"], act_in=ops.ACT_SILU)
        mod = ops.mod_table(w["_all_tables"], t6, out=self._buf("mod", (self.L, B, C6)))
        txt = self._encode_text(encoder_hidden_states, encoder_attention_mask)
        cos, sin = self._rope(T, gh, gw)
        # ---- PatchEmbed2D without position embedding (use_abs_pos = not use_rope): the patch-embed kernel with a zero table
        xz = hidden_states.to(device=dev, dtype=torch.float32).contiguous()
        if sp is None:
            zero_pos = self._ws.once(("zero_pos", gh * gw), lambda: torch.zeros(gh * gw, C, dtype=self.dtype, device=dev))
            x = ops.patch_embed(xz, w["pos_embed.proj.weight"], w["pos_embed.proj.bias"], zero_pos, B, (1, p, p), C).view(B * N, C)
        else:
            # the local tokens only.  A rank's range of the (t, h, w) order may straddle frames: the T frames are read as ONE frame of
            # T * Hh rows (a patch never crosses a frame: Hh % p == 0), whose token s is token s of the sequence; same arithmetic per token
            zero_pos = self._ws.once(("zero_pos", N), lambda: torch.zeros(N, C, dtype=self.dtype, device=dev))
            x = ops.patch_embed_shard(xz.view(xz.shape[0], cin, 1, T * Hh, Ww), w["pos_embed.proj.weight"], w["pos_embed.proj.bias"],
                                      zero_pos, B, (1, p, p), C, sp.rank * Nl, Nl).view(B * Nl, C)

        use_pab = pab.enable_pab()
        timestep_int = int(ts_host[0]) if use_pab else None
        kp, vt = self._ws.once(("kv_self", B, N, Hl), lambda: oops.alloc_kv_buffers96(B, Hl, N, dev))
        self.last_decisions = []
        for i in range(self.L):
            pre = f"transformer_blocks.{i}"
            st = self.states[i]
            m = mod[i]
            shift_a, scale_a, gate_a = m[0, 0:C], m[0, C:2 * C], m[0, 2 * C:3 * C]
            shift_m, scale_m, gate_m = m[0, 3 * C:4 * C], m[0, 4 * C:5 * C], m[0, 5 * C:6 * C]
            # -- self-attention (:1353-1380)
            bc_s = False
            if use_pab:
                bc_s, st.attn_count = pab.if_broadcast_spatial(timestep_int, st.attn_count)
            if not bc_s:
                xm = ops.ln_modulate(x, None, None, shift_a, scale_a, Nl, mod_stride=C6, eps=cfg.norm_eps, out=self._buf("xm", (B * Nl, C)))
                qkv = ops.gemm(xm, w[pre + ".attn1.qkv.weight"], w[pre + ".attn1.qkv.bias"], out=self._buf("qkv", (B * Nl, 3 * C)))
                ao = self._self_attention(qkv, cos, sin, kp, vt, B, N)
            if use_pab:
                # the cache holds the UN-gated attention output (:1372-1373); it is gated with this step's gate (:1378)
                if not bc_s:
                    if st.last_attn is None or st.last_attn.shape != x.shape:
                        st.last_attn = torch.empty_like(x)
                    ops.gemm(ao, w[pre + ".attn1.to_out.0.weight"], w[pre + ".attn1.to_out.0.bias"], out=st.last_attn)
                ops.gate_add_rows(x, st.last_attn, gate_a, Nl, C6)
            else:
                ops.gemm(ao, w[pre + ".attn1.to_out.0.weight"], w[pre + ".attn1.to_out.0.bias"], epilogue=ops.EPI_GATE_RES, gate=gate_a,
                         gate_stride=C6, rows_per_sample=Nl, res=x, out=x)
            # -- cross-attention on the un-normed x (the PixArt rule, :1399-1402), no gate (:1420); local rows, all heads: no exchange
            bc_c = False
            if use_pab:
                bc_c, st.cross_count = pab.if_broadcast_cross(timestep_int, st.cross_count)
            if not bc_c:
                q = ops.gemm(x, w[pre + ".attn2.to_q.weight"], w[pre + ".attn2.to_q.bias"], out=self._buf("xm", (B * Nl, C)))
                ao = self._buf("attn_out", (B * Nl, C))
                oops.flash_attn96(q, None, None, txt["kp"][i], txt["vt"][i], txt["kv_lens"], ao, B, H, Nl, txt["Lk"])
            if use_pab:
                if not bc_c:
                    if st.last_cross is None or st.last_cross.shape != x.shape:
                        st.last_cross = torch.empty_like(x)
                    ops.gemm(ao, w[pre + ".attn2.to_out.0.weight"], w[pre + ".attn2.to_out.0.bias"], out=st.last_cross)
                ops.add_rows(x, st.last_cross)
            else:
                ops.gemm(ao, w[pre + ".attn2.to_out.0.weight"], w[pre + ".attn2.to_out.0.bias"], epilogue=ops.EPI_GATE_RES, res=x, out=x)
            self.last_decisions.append((bc_s, bc_c))
            # -- feed-forward (:1432-1451)
            xm = ops.ln_modulate(x, None, None, shift_m, scale_m, Nl, mod_stride=C6, eps=cfg.norm_eps, out=self._buf("xm", (B * Nl, C)))
            hb = ops.gemm(xm, w[pre + ".ff.net.0.proj.weight"], w[pre + ".ff.net.0.proj.bias"], epilogue=ops.EPI_BIAS_GELU,
                          out=self._buf("mlp_h", (B * Nl, 4 * C)))
            ops.gemm(hb, w[pre + ".ff.net.2.weight"], w[pre + ".ff.net.2.bias"], epilogue=ops.EPI_GATE_RES, gate=gate_m, gate_stride=C6,
                     rows_per_sample=Nl, res=x, out=x)
        # ---- norm_out, (shift, scale) = scale_shift_table + embedded_timestep, proj_out, unpatchify (:2077-2108)
        fin = ops.mod_table(w["scale_shift_table"], emb, out=self._buf("mod_out", (2, B, C)))     # [shift | scale] x B x C
        xo = ops.ln_modulate(x, None, None, fin[0, 0], fin[1, 0], Nl, mod_stride=C, eps=1e-6, out=self._buf("xm", (B * Nl, C)))
        po = ops.gemm(xo, w["_proj_out.weight"], w["_proj_out.bias"], out=self._buf("proj", (B * Nl, 192)))
        if sp is not None:     # gather_sequence (:1975-1979) on the projected rows: 192 columns travel instead of C
            parts = self._buf("proj_parts", (P, B, Nl, 192))
            dsp.all_gather_into_tensor(parts.view(P * B, Nl, 192), po.view(B, Nl, 192), sp.group)
            gather, _ = dsp.plan_gather(B, 1, Nl, N, 192, P)
            po = self._buf("proj_all", (B * N, 192))
            sp.exec(parts, po, gather)
        co = cfg.out_channels
        out = torch.empty(B, co, T, Hh, Ww, dtype=torch.float32, device=dev)
        for b in range(B):       # rows (t, h, w) x columns (c, dy, dx) -> out[b, c, t, y, x]: one [T, 1, H, W] problem per (b, c)
            for c in range(co):
                ops.unpatchify_cvx(po[b * N:(b + 1) * N, c * p * p:(c + 1) * p * p], 1, T, gh, gw, 1, p, out=out[b, c])
        if not return_dict:
            return (out,)
        return VideoSysPipelineOutput(video=out)

    __call__ = forward


def OpenSoraT2V_ROPE_L_122(**kwargs):
    """:2157-2168 — the 29x480p / 93x480p / 93x720p transformer of v1.2: 32 layers, 24 heads x 96."""
    return OpenSoraT2V(num_layers=32, attention_head_dim=96, num_attention_heads=24, patch_size_t=1, patch_size=2,
                       norm_type="ada_norm_single", caption_channels=4096, cross_attention_dim=2304, **kwargs)


OpenSora_models = {"OpenSoraT2V-ROPE-L/122": OpenSoraT2V_ROPE_L_122}


def synth_state_dict(num_layers=32, num_heads=24, head_dim=HEAD_DIM, caption_channels=4096, in_channels=4, out_channels=4,
                     patch_size=2, seed: int = 1202) -> Dict[str, torch.Tensor]:
    """Seeded random weights (CPU generator, every value bf16-exact, stored as fp32) with the reference's OpenSoraT2V key names
    (no pretrained weights offline)."""
    g = torch.Generator().manual_seed(seed)
    C = num_heads * head_dim
    sd: Dict[str, torch.Tensor] = {}
    bf = lambda t: t.to(torch.bfloat16).float()

    def lin(name, n_out, n_in):
        s = min(0.08, 1.0 / math.sqrt(n_in))
        sd[name + ".weight"] = bf(torch.randn(n_out, n_in, generator=g) * s)
        sd[name + ".bias"] = bf(torch.randn(n_out, generator=g) * 0.02)

    sd["pos_embed.proj.weight"] = bf(torch.randn(C, in_channels, patch_size, patch_size, generator=g) * 0.1)
    sd["pos_embed.proj.bias"] = bf(torch.randn(C, generator=g) * 0.02)
    lin("adaln_single.emb.timestep_embedder.linear_1", C, 256)
    lin("adaln_single.emb.timestep_embedder.linear_2", C, C)
    lin("adaln_single.linear", 6 * C, C)
    lin("caption_projection.linear_1", C, caption_channels)
    lin("caption_projection.linear_2", C, C)
    for i in range(num_layers):
        p = f"transformer_blocks.{i}"
        sd[p + ".scale_shift_table"] = bf(torch.randn(6, C, generator=g) / C**0.5)
        for a in ("attn1", "attn2"):
            for l in ("to_q", "to_k", "to_v", "to_out.0"):
                lin(f"{p}.{a}.{l}", C, C)
        lin(p + ".ff.net.0.proj", 4 * C, C)
        lin(p + ".ff.net.2", C, 4 * C)
    sd["scale_shift_table"] = bf(torch.randn(2, C, generator=g) / C**0.5)
    lin("proj_out", patch_size * patch_size * out_channels, C)
    return sd
