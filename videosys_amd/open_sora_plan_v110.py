"""Open-Sora-Plan v1.1 transformer (LatteT2V with ``use_rope``) on MI355X — host mirror of
videosys/models/transformers/open_sora_plan_v110_transformer_3d.py (LatteT2V :2123-2765, BasicTransformerBlock :1734-2071,
BasicTransformerBlock_ :1370-1712, AttnProcessor2_0 :1125-1267, RoPE2D / RoPE1D and their linear scaling :136-253).

The v1.1 model is the Latte-1 block stack of latte.py with three additions, and this class is latte.LatteT2V with exactly those:
  * ``use_rope``: every spatial self-attention rotates q and k with RoPE2D (the 72 columns of a head are a row half and a column
    half of 36, rotate-half inside each), every temporal one with RoPE1D (rotate-half over all 72), both on linearly scaled positions;
  * position embeddings scaled by ``interpolation_scale_2d = max(sample_size[0] // 64, 1)`` (PatchEmbed's table, :393-400 at the
    model's own grid and :412-421 recomputed for another input size: one formula at a square sample_size, latte.latte_pos_embed_2d,
    float32 on the host and uploaded in bf16 as in latte.py) and ``interpolation_scale_1d`` (temp_pos_embed, :2242-2254);
  * ``encoder_attention_mask`` may be None, and ``encoder_hidden_states`` comes as [B, 1, L, C].

Rotate-half on interleaved kernels.  Attention logits do not change when the same column permutation is applied inside every head to q
and to k, so ``load_state_dict`` permutes the OUTPUT ROWS of to_q / to_k (weights and biases) such that every rotate-half pair
(j, j + half) becomes the neighbours (2p, 2p + 1); v and to_out are untouched.  The temporal attention is then
``ops.attn_temporal`` in its rope-only mode, the spatial attention ``open_sora_plan_v110_ops.attn_prep_kv_rope`` +
``flash_attn_rope``.  With ``use_rope=False`` nothing is permuted and latte.py's plain kernels run.

Tables are built on the host once per geometry, as the reference builds them: inv_freq over D = 36 (2-D) / 72 (1-D) in fp32, the
angles cast to bf16 BEFORE cos / sin (get_cos_sin :144-153: ``freqs.to(dtype)``), positions divided by the scale and truncated back to
integers (LinearScalingRoPE* :190-196, :247-253), the bf16 values widened to fp32.

Built: ada_norm_single, gelu-approximate, biased attention, no norm affine, patch_size_t 1, head dim 72, rope_scaling_type "linear",
compress_kv_factor 1.  Raises NotImplementedError at construction: anything else.  Not built: sequence parallelism and the CFG split
(``enable_parallel`` with more than one rank raises), image joint training, self-attention masks other than all ones."""
from __future__ import annotations

import math
from typing import Dict

import torch

from . import latte, ops, open_sora_plan_v110_ops as vops
from .modules import sincos_1d

HEAD_DIM = ops.HEAD_DIM


# ------------------------------------------------------------------------------------------------ permutations and tables
def head_permutation_2d() -> torch.Tensor:
    """int64 [72]: new column c of a head takes old column perm[c].  Pairs (2p, 2p + 1) = old (p, p + 18) for p < 18 (row half) and
    old (36 + p - 18, 54 + p - 18) for p >= 18 (column half)."""
    perm = []
    for p in range(36):
        a = p if p < 18 else 36 + (p - 18)
        perm += [a, a + 18]
    return torch.tensor(perm, dtype=torch.int64)


def head_permutation_1d() -> torch.Tensor:
    """int64 [72]: pairs (2p, 2p + 1) = old (p, p + 36)."""
    perm = []
    for p in range(36):
        perm += [p, p + 36]
    return torch.tensor(perm, dtype=torch.int64)


def _angles(D: int, positions: torch.Tensor, scale: float, dtype) -> torch.Tensor:
    """get_cos_sin (:144-153 / :207-216) at the scaled positions: [len(positions), D / 2] angles in ``dtype``."""
    pos = (positions.to(torch.int64).float() / scale).to(torch.int64)          # LinearScalingRoPE*: truncated back to integers
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    t = torch.arange(int(pos.max()) + 1, dtype=inv_freq.dtype)
    freqs = torch.einsum("i,j->ij", t, inv_freq).to(dtype)
    return freqs[pos]


def rope_tables_2d(gh: int, gw: int, scale: float, dtype=torch.bfloat16):
    """fp32 (cos, sin) [gh * gw, 36] for vsys_attn_prep_kv_rope / vsys_flash_attn_d72_rope: token s = y * gw + x (PositionGetter2D
    :256-268), entries 0..17 the row-position pairs, 18..35 the column-position pairs."""
    y = torch.arange(gh).repeat_interleave(gw)
    x = torch.arange(gw).repeat(gh)
    ang = torch.cat([_angles(36, y, scale, dtype), _angles(36, x, scale, dtype)], dim=1)
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def rope_tables_1d(T: int, scale: float, dtype=torch.bfloat16):
    """fp32 (cos, sin) [T, 72] in the layout vsys_attn_temporal_d72 reads: pair p at column 2p (and repeated at 2p + 1)."""
    ang = _angles(72, torch.arange(T), scale, dtype)
    return (ang.cos().float().repeat_interleave(2, dim=1).contiguous(), ang.sin().float().repeat_interleave(2, dim=1).contiguous())


def interpolation_scale_1d_default(video_length: int) -> int:
    """:2242-2250."""
    s = (video_length - 1) // 16 if video_length % 2 == 1 else video_length // 16
    return max(s, 1)


class LatteT2V(latte.LatteT2V):
    """Drop-in for the reference's v110 LatteT2V at the operator boundary ``transformer(latent_model_input, ...)[0]``."""

    def __init__(self, num_attention_heads=16, patch_size_t=1, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=28,
                 cross_attention_dim=1152, attention_bias=True, sample_size=(64, 64), patch_size=2, activation_fn="gelu-approximate",
                 norm_type="ada_norm_single", norm_elementwise_affine=False, norm_eps=1e-6, caption_channels=4096, video_length=17,
                 attention_mode="flash", use_rope=True, model_max_length=300, rope_scaling_type="linear", compress_kv_factor=1,
                 interpolation_scale_1d=None, device="cuda", dtype=torch.bfloat16, **unused):
        if compress_kv_factor != 1:
            raise NotImplementedError("compress_kv_factor != 1 (the strided K/V convolution of the second half of the layers) is not built")
        if patch_size_t != 1:
            raise NotImplementedError("patch_size_t != 1 is not built")
        if use_rope and rope_scaling_type != "linear":
            raise NotImplementedError(f"rope_scaling_type {rope_scaling_type!r}: only 'linear' (the reference raises for others too)")
        if isinstance(sample_size, int):
            sample_size = (sample_size, sample_size)
        sample_size = tuple(int(v) for v in sample_size)
        if len(sample_size) != 2 or sample_size[0] != sample_size[1]:
            # the reference's construction-time table is a sqrt(n) x sqrt(n) grid (:397-399): only a square sample_size means what it says
            raise NotImplementedError("sample_size must be a square pair")
        for k in ("num_embeds_ada_norm", "num_vector_embeds"):
            if unused.get(k) is not None:
                raise NotImplementedError(f"{k} is not built")
        # attention_mode: accepted and ignored (one attention implementation here)
        super().__init__(num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim, in_channels=in_channels,
                         out_channels=out_channels, num_layers=num_layers, cross_attention_dim=cross_attention_dim,
                         attention_bias=attention_bias, sample_size=sample_size[0], patch_size=patch_size, activation_fn=activation_fn,
                         norm_type=norm_type, norm_elementwise_affine=norm_elementwise_affine, norm_eps=norm_eps,
                         caption_channels=caption_channels, video_length=video_length, device=device, dtype=dtype)
        self.use_rope = bool(use_rope)
        self.config.sample_size_hw = sample_size
        self.config.model_max_length, self.config.use_rope = model_max_length, self.use_rope
        self.interpolation_scale_2d = max(sample_size[0] // 64, 1)                                   # :2230-2231
        self.interpolation_scale_1d = max(interpolation_scale_1d if interpolation_scale_1d is not None
                                          else interpolation_scale_1d_default(video_length), 1)      # :2242-2250
        self.config.interpolation_scale_1d = self.interpolation_scale_1d
        # get_1d_sincos_pos_embed (:109-112): positions / scale, float32 table (:2251-2254); added in block 0 also with use_rope (:2705-2707)
        pos = (torch.arange(0, video_length).unsqueeze(1) / self.interpolation_scale_1d).numpy()
        self.temp_pos_embed = torch.from_numpy(sincos_1d(self.C, pos)).float().to(device=self.device, dtype=dtype).contiguous()
        self._rope_cache = {}

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """Reference state-dict names; ``caption_projection.y_embedding`` is accepted and unused (the drop-embedding of training)."""
        sd = {k: v for k, v in sd.items() if k != "caption_projection.y_embedding"}
        if self.use_rope:
            sd = dict(sd)
            H = self.H
            for i in range(2 * self.L):
                perm = head_permutation_1d() if i % 2 else head_permutation_2d()
                rows = (torch.arange(H)[:, None] * HEAD_DIM + perm[None]).reshape(-1)
                p = self.block_prefix(i)
                for l in ("to_q", "to_k"):
                    for k in (f"{p}.attn1.{l}.weight", f"{p}.attn1.{l}.bias"):
                        if k in sd:            # (a missing key is the strict check's to name)
                            sd[k] = sd[k][rows]
        return super().load_state_dict(sd, strict=strict)

    def enable_parallel(self, dp_size=None, sp_size=None, enable_cp=None, parallel_mgr=None, copy_executor=None):
        sp = parallel_mgr.sp_size if parallel_mgr is not None else (sp_size or 1)
        if sp > 1 or (parallel_mgr is not None and getattr(parallel_mgr, "cp_size", 1) > 1):
            raise NotImplementedError("Open-Sora-Plan v1.1: sequence parallelism and the CFG split are not built")
        super().enable_parallel(dp_size=dp_size, sp_size=1, enable_cp=False, parallel_mgr=parallel_mgr, copy_executor=copy_executor)

    # ------------------------------------------------------------------ tables
    def rope_tables(self, gh, gw, T):
        """(cos2d, sin2d [gh * gw, 36], cos1d, sin1d [T, 72]) on the device, built once per geometry."""
        key = (gh, gw, T)
        if key not in self._rope_cache:
            tabs = rope_tables_2d(gh, gw, float(self.interpolation_scale_2d), self.dtype) + rope_tables_1d(T, float(self.interpolation_scale_1d), self.dtype)
            self._rope_cache[key] = tuple(t.to(self.device) for t in tabs)
        return self._rope_cache[key]

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, hidden_states, timestep=None, all_timesteps=None, encoder_hidden_states=None, added_cond_kwargs=None,
                class_labels=None, cross_attention_kwargs=None, attention_mask=None, encoder_attention_mask=None,
                use_image_num: int = 0, enable_temporal_attentions: bool = True, return_dict: bool = True):
        if use_image_num or class_labels is not None:
            raise NotImplementedError("image joint training / class labels are not built")
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            raise NotImplementedError("attention_mask must be None or all ones (what the v1.1 pipeline passes)")
        y = encoder_hidden_states
        if y.dim() == 4:                      # "b 1 t d" (:2559-2561)
            if y.shape[1] != 1:
                raise NotImplementedError("image joint training (more than one text per sample) is not built")
            y = y[:, 0]
        m = encoder_attention_mask
        if m is not None and m.dim() == 3:
            if m.shape[1] != 1:
                raise NotImplementedError("image joint training (more than one mask per sample) is not built")
            m = m[:, 0]
        if hidden_states.shape[2] == 1 and enable_temporal_attentions:
            # the reference itself cannot run this: the temporal block's squeeze(1) (:1958) drops the one-frame axis and its attention
            # fails on the 2-D tensor; latte.py would skip temp_pos_embed here, which the v1.1 forward never does (:2705-2707)
            raise NotImplementedError("a single frame with temporal attention is not built (the reference raises on it as well)")
        p = self.patch_size
        gh, gw, Fr = hidden_states.shape[-2] // p, hidden_states.shape[-1] // p, hidden_states.shape[2]
        self._rope = self.rope_tables(gh, gw, Fr) if self.use_rope else None
        return super().forward(hidden_states, timestep=timestep, all_timesteps=all_timesteps, encoder_hidden_states=y,
                               added_cond_kwargs=added_cond_kwargs, cross_attention_kwargs=cross_attention_kwargs,
                               encoder_attention_mask=m, enable_temporal_attentions=enable_temporal_attentions, return_dict=return_dict)

    __call__ = forward

    def _attention(self, qkv, ao, B, Fr, S, temporal):
        """attn1 of one block on the qkv rows (latte.LatteT2V._self_attn_out): with use_rope the rotated kernels on the permuted q / k."""
        if self._rope is None:
            return super()._attention(qkv, ao, B, Fr, S, temporal)
        C, H = self.C, self.H
        cos2, sin2, cos1, sin1 = self._rope
        if temporal:
            ops.attn_temporal(qkv, C, None, None, cos1, sin1, ao, B, Fr, S, H)
        else:
            kp, vt = self._ws.once(("kv_spatial", B * Fr, S), lambda: ops.alloc_kv_buffers(B * Fr, H, S, self.device))
            vops.attn_prep_kv_rope(qkv[:, C:2 * C], qkv[:, 2 * C:], cos2, sin2, kp, vt, B * Fr, H, S)
            vops.flash_attn_rope(qkv[:, :C], cos2, sin2, kp, vt, ao, B * Fr, H, S, S)


def synth_state_dict(num_layers=28, num_heads=16, head_dim=72, caption_channels=4096, in_channels=4, out_channels=8, patch_size=2,
                     seed: int = 1101, qk_gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded random weights with the reference's state-dict names (latte.synth_state_dict's, plus caption_projection.y_embedding).
    ``qk_gain`` scales the attn1.to_q / to_k weights and biases of every block: with default-sized projections the logits are so flat
    that the rotation hardly shows in the output, and a test could not tell a missing rotation from noise."""
    sd = latte.synth_state_dict(num_layers=num_layers, num_heads=num_heads, head_dim=head_dim, caption_channels=caption_channels,
                                in_channels=in_channels, out_channels=out_channels, patch_size=patch_size, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    sd["caption_projection.y_embedding"] = torch.randn(120, caption_channels, generator=g) / math.sqrt(caption_channels)
    if qk_gain != 1.0:
        for k in list(sd):
            if ".attn1.to_q." in k or ".attn1.to_k." in k:
                sd[k] = sd[k] * qk_gain
    return sd
