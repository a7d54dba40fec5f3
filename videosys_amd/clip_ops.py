"""Tensor-level wrappers of the entry points that exist for the CLIP text encoders of Vchitect-2.0 (include/videosys_amd.h:
vsys_clip_attention_d64, vsys_splitk_reduce_bias_act; csrc/clip_ops.hip), on the launch route of videosys_amd.ops
(torch.ops.vsys.launch, op codes 66 and 67; they run once per prompt and nothing records them).  HIP device tensors only, no eager fallback.
Guard-band tests: tests/test_gpu_isolation_clip.py."""
from __future__ import annotations

import torch

from .ops import _bf16, _call, _chk, _p, skinny_split

ACT_NONE, ACT_QUICK_GELU, ACT_GELU = 0, 1, 2   # vsys_splitk_reduce_bias_act


def splitk_reduce_bias_act(part, nsplit, slab, ldp, M, N, out, bias=None, act=ACT_NONE, res=None):
    """out[:M] = bf16(act(bf16(sum_s part[s][m][n] + bias[n])) + res[m][n]) over fp32 partials [s][m][n] (row pitch ldp, slice pitch
    slab): the finish of linear_skinny_bias_act, also callable on its own."""
    _chk(part, out, bias, res)
    _bf16(out, bias, res)
    assert part.dtype == torch.float32 and out.stride(1) == 1 and (res is None or res.stride(1) == 1)
    assert bias is None or (bias.is_contiguous() and bias.numel() == N)
    _call("vsys_splitk_reduce_bias_act", _p(part), nsplit, slab, ldp, _p(res), res.stride(0) if res is not None else 0, _p(out),
          out.stride(0), M, N, _p(bias), act)
    return out


def linear_skinny_bias_act(x, M, w, bias=None, act=ACT_NONE, res=None, out=None, nsplit=None, part=None):
    """linear_skinny's wide path (Mp % 384 == 0) for layers with a bias and an activation (CLIP; T5 has neither and keeps
    linear_skinny): out[:M] = act(x[:M] @ w^T + bias) (+ res[:M]) with the roundings of vsys_splitk_reduce_bias_act."""
    _chk(x, w, bias, res, out, part)
    _bf16(x, w, bias, res, out)
    Mp, K = x.shape
    N = w.shape[0]
    assert Mp % 384 == 0 and M <= Mp and w.shape[1] == K and K % 32 == 0 and x.is_contiguous() and w.is_contiguous()
    nsplit = skinny_split(N, Mp, K, True) if nsplit is None else nsplit
    if part is None:
        part = torch.empty(nsplit * N * Mp, dtype=torch.float32, device=x.device)
    assert part.dtype == torch.float32 and part.numel() >= nsplit * N * Mp and part.is_contiguous()
    if out is None:
        out = torch.empty(Mp, N, dtype=torch.bfloat16, device=x.device)
    assert out.shape[1] == N and (res is None or res.shape[1] == N)
    _call("vsys_gemm_skinny_slices", _p(w), w.stride(0), _p(x), x.stride(0), _p(part), M, Mp, N, K, nsplit)
    return splitk_reduce_bias_act(part, nsplit, Mp * N, N, M, N, out, bias=bias, act=act, res=res)


def clip_attention64(qkv, B, L, heads, out=None):
    """Causal self-attention of CLIPAttention at head dim 64 (vsys_clip_attention_d64): qkv bf16 rows (b, l) holding q | k | v at
    columns 0 | inner | 2 inner (a row-strided view is fine) -> out bf16 [B * L, inner]; L <= 128."""
    _chk(qkv, out)
    _bf16(qkv, out)
    inner = heads * 64
    assert qkv.dim() == 2 and qkv.shape[0] >= B * L and qkv.shape[1] >= 3 * inner and qkv.stride(1) == 1
    if out is None:
        out = torch.empty(B * L, inner, dtype=torch.bfloat16, device=qkv.device)
    assert out.shape[0] >= B * L and out.stride(1) == 1
    _call("vsys_clip_attention_d64", _p(qkv), qkv.stride(0), inner, _p(out), out.stride(0), B, L)
    return out
