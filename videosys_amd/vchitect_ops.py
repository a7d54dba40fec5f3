"""Tensor-level wrappers of the two entry points that exist for Vchitect-2.0 (include/videosys_amd.h: vsys_attn_temporal_d64,
vsys_scale_add_rows), on the launch route of videosys_amd.ops (torch.ops.vsys.launch / ctypes, recorded by program.py).  HIP device
tensors only, no eager fallback.  Guard-band tests: tests/test_gpu_isolation_vchitect.py."""
from __future__ import annotations

import torch

from .ops import _bf16, _call, _chk, _p


def attn_temporal64(q_vid, k_vid, v_vid, q_txt, k_txt, v_txt, rope_cos, rope_sin, out_vid, out_txt, B, T, S, L, heads):
    """Temporal attention of VchitectAttnProcessor (attentions.py:705-764) over the T frames of every video and text token.
    *_vid [B*T*S, >= heads*64] rows ordered (b, t, s), *_txt [B*T*L, >= heads*64] rows ordered (b, t, l): 2-D row-strided views, each
    with its own stride (None where S or L is 0).  rope_cos / rope_sin fp32 [T, 32] (one value per interleaved pair) or None.
    Rounding contract (tests/test_gpu_vchitect_attention.py): q^, k^ = bf16(rotation in fp32), scores, softmax and P V in fp32 (P is
    not rounded; running maximum adopted every 4 keys), one division, one rounding of the output."""
    ts = (q_vid, k_vid, v_vid, q_txt, k_txt, v_txt, out_vid, out_txt)
    _chk(*ts, rope_cos, rope_sin)
    _bf16(*ts)
    for t, n in zip(ts, (S, S, S, L, L, L, S, L)):
        if n > 0:
            assert t is not None and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == B * T * n and t.shape[1] >= heads * 64
    if rope_cos is not None:
        assert rope_cos.dtype == torch.float32 and rope_cos.is_contiguous() and rope_cos.shape == (T, 32)
        assert rope_sin.dtype == torch.float32 and rope_sin.is_contiguous() and rope_sin.shape == (T, 32)
    ld = lambda t: 0 if t is None else t.stride(0)
    _call("vsys_attn_temporal_d64", _p(q_vid), ld(q_vid), _p(k_vid), ld(k_vid), _p(v_vid), ld(v_vid), _p(q_txt), ld(q_txt), _p(k_txt),
          ld(k_txt), _p(v_txt), ld(v_txt), _p(rope_cos), _p(rope_sin), _p(out_vid), ld(out_vid), _p(out_txt), ld(out_txt), B, T, S, L,
          heads)
    return out_vid, out_txt


def scale_add_rows(a, b, scale, out=None):
    """out = bf16(bf16(a * scale) + b) on 2-D row-strided views (``hidden_states * 1.1 + cross_output``, attentions.py:899)."""
    if out is None:
        out = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device)
    _chk(a, b, out)
    _bf16(a, b, out)
    assert a.dim() == 2 and a.shape == b.shape == out.shape and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1
    _call("vsys_scale_add_rows", _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), a.shape[0], a.shape[1], float(scale))
    return out
