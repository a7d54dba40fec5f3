"""Tensor-level wrappers of the two entry points that exist for Open-Sora-Plan v1.1 (include/videosys_amd.h): the head-dim-72 spatial
attention with a per-token rotation of interleaved column pairs, vsys_attn_prep_kv_rope (K side, writes the (kp, vt) pair of
ops.attn_prep_kv) and vsys_flash_attn_d72_rope (Q side, the streaming 32-rows-per-wave flash kernel).  HIP device tensors only, no eager
fallback.

Neither has an op code (the op table is pinned, csrc/gen/program_gen.py NO_OP): the launch goes through ctypes on torch's current stream
and, under a launch-program recorder, is a ``program.host_call`` closure, as in open_sora_plan_ops.py.
Element-wise tests: tests/test_gpu_osp_v110_attention.py; guard bands: tests/test_gpu_isolation_osp_v110.py."""
from __future__ import annotations

import torch

from .open_sora_plan_ops import _issue
from .ops import HEAD_DIM, VT_ROWS, _bf16, _chk, alloc_kv_buffers, kv_pad_len  # noqa: F401  (alloc_kv_buffers, kv_pad_len: re-exported)

PAIRS = HEAD_DIM // 2    # 36 (cos, sin) entries per token: entry p rotates the columns (2p, 2p + 1) of every head


def _tables(rope_cos, rope_sin, rows):
    for t in (rope_cos, rope_sin):
        assert t is not None, "no tables: call ops.attn_prep_kv / ops.flash_attn"
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, PAIRS)


def attn_prep_kv_rope(k, v, rope_cos, rope_sin, kp, vt, batch, heads, kv_len):
    """k, v: 2-D row-strided views [batch * kv_len, >= heads * 72] (head h at column h * 72) -> kp: key s of every batch item and head
    rotated by row s of the fp32 tables [kv_len, 36] (pair p = columns 2p, 2p + 1), the softmax scale folded in, one rounding; vt: V
    transposed with the ones rows.  Exactly the buffers of ops.attn_prep_kv (ops.alloc_kv_buffers)."""
    _chk(k, v, rope_cos, rope_sin, kp, vt)
    _bf16(k, v, kp, vt)
    assert k.dim() == 2 and v.dim() == 2 and k.stride(1) == 1 and v.stride(1) == 1 and kp.is_contiguous() and vt.is_contiguous()
    assert k.shape[0] >= batch * kv_len and v.shape[0] >= batch * kv_len and k.shape[1] >= heads * HEAD_DIM and v.shape[1] >= heads * HEAD_DIM
    kv_pad = kp.shape[-2]
    assert tuple(kp.shape[-3:]) == (heads, kv_pad, HEAD_DIM) and tuple(vt.shape[-3:]) == (heads, VT_ROWS, kv_pad)
    assert kp.numel() == batch * heads * kv_pad * HEAD_DIM and vt.numel() == batch * heads * VT_ROWS * kv_pad and kv_len <= kv_pad
    _tables(rope_cos, rope_sin, kv_len)
    _issue("vsys_attn_prep_kv_rope", (k, v, rope_cos, rope_sin, kp, vt),
           (k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), rope_cos.data_ptr(), rope_sin.data_ptr(), kp.data_ptr(), vt.data_ptr(),
            batch, heads, kv_len, kv_pad))


def flash_attn_rope(q, rope_cos, rope_sin, kp, vt, out, batch, heads, q_len, kv_len):
    """out = softmax(rot(q) kp^T) v on the layouts of attn_prep_kv_rope / ops.attn_prep_kv; q, out: 2-D row-strided views
    [batch * q_len, >= heads * 72]; query s is rotated by row s of the fp32 tables [q_len, 36], one rounding, no q norm.  Always the
    32-rows-per-wave streaming kernel (include/videosys_amd.h)."""
    _chk(q, rope_cos, rope_sin, kp, vt, out)
    _bf16(q, kp, vt, out)
    assert q.dim() == 2 and out.dim() == 2 and q.stride(1) == 1 and out.stride(1) == 1
    assert q.shape[0] >= batch * q_len and out.shape[0] >= batch * q_len and q.shape[1] >= heads * HEAD_DIM and out.shape[1] >= heads * HEAD_DIM
    kv_pad = kp.shape[-2]
    assert kp.numel() == batch * heads * kv_pad * HEAD_DIM and vt.numel() == batch * heads * VT_ROWS * kv_pad and kv_len <= kv_pad
    _tables(rope_cos, rope_sin, q_len)
    _issue("vsys_flash_attn_d72_rope", (q, rope_cos, rope_sin, kp, vt, out),
           (q.data_ptr(), q.stride(0), rope_cos.data_ptr(), rope_sin.data_ptr(), kp.data_ptr(), vt.data_ptr(), out.data_ptr(), out.stride(0),
            batch, heads, q_len, kv_len, kv_pad))
    return out
