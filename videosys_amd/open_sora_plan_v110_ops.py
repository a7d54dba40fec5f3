"""Tensor-level wrappers of the entry points that exist for Open-Sora-Plan v1.1 (include/videosys_amd.h): the head-dim-72 spatial
attention with a per-token rotation of interleaved column pairs, vsys_attn_prep_kv_rope (K side, writes the (kp, vt) pair of
ops.attn_prep_kv) and vsys_flash_attn_d72_rope (Q side, the streaming 32-rows-per-wave flash kernel), and, at the end of the file, the
temporal upsampler of its CausalVAE and its sampler step (vsys_upsample_time2x, vsys_cfg_pndm_step).  HIP device tensors only, no eager
fallback.

Every entry point here has an op code and goes through ``ops._call``, as in open_sora_plan_ops.py: a recorded step replays the two
attention launches inside its vsys_program_run call.
Element-wise tests: tests/test_gpu_osp_v110_attention.py, tests/test_gpu_osp_v110_kernels.py; guard bands:
tests/test_gpu_isolation_osp_v110.py, tests/test_gpu_isolation_osp_v110_pipeline.py."""
from __future__ import annotations

import ctypes

import torch

from . import program
from .ops import HEAD_DIM, VT_ROWS, VaeGrid, _bf16, _call, _chk, _p, alloc_kv_buffers, kv_pad_len  # noqa: F401  (alloc_kv_buffers, kv_pad_len: re-exported)

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
    _call("vsys_attn_prep_kv_rope", _p(k), k.stride(0), _p(v), v.stride(0), _p(rope_cos), _p(rope_sin), _p(kp), _p(vt), batch, heads, kv_len,
          kv_pad)


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
    _call("vsys_flash_attn_d72_rope", _p(q), q.stride(0), _p(rope_cos), _p(rope_sin), _p(kp), _p(vt), _p(out), out.stride(0), batch, heads,
          q_len, kv_len, kv_pad)
    return out


# ------------------------------------------------------------------------------------------------ CausalVAE decode and sampler
# (csrc/vae_osp.hip; as their v1.2 siblings of open_sora_plan_ops.py: the upsampler is recordable, the sampler step refuses to run
#  under a recorder, see there)
def upsample_time2x(x, gs: VaeGrid, y, gd: VaeGrid, C, y_res=None, g_res: VaeGrid = None, alpha: float = 0.0):
    """TimeUpsample2x / TimeUpsampleRes2x up to its conv: x rows over gs -> the interior rows of gd ((1 if T == 1 else 2T - 1) frames of
    the same (H, W)); frame 0 copied, the later frames interpolated by (2, 1, 1) among themselves in fp32, one rounding.  ``y_res`` rows
    over ``g_res`` (same frames, H and W): bf16(alpha * v) from the same fp32 value (include/videosys_amd.h)."""
    assert C % 8 == 0 and 0 < C <= 2048, f"C = {C}: a multiple of 8, at most 2048"
    assert (gd.n, gd.T, gd.H, gd.W) == (gs.n, 1 if gs.T == 1 else 2 * gs.T - 1, gs.H, gs.W), "grid_dst does not match grid_src"
    assert x.shape == (gs.rows, C) and y.shape == (gd.rows, C) and x.is_contiguous() and y.is_contiguous()
    if y_res is not None:
        assert g_res is not None and (g_res.n, g_res.T, g_res.H, g_res.W) == (gd.n, gd.T, gd.H, gd.W), "grid_res does not match grid_dst"
        assert y_res.shape == (g_res.rows, C) and y_res.is_contiguous()
    _chk(x, y, y_res)          # (after the argument checks: a wrong call is refused as such on any device, before any launch)
    _bf16(x, y, y_res)
    _call("vsys_upsample_time2x", _p(x), gs._c, _p(y), gd._c, _p(y_res), None if y_res is None else g_res._c, float(alpha), gs.n, C)
    return y


def cfg_pndm_step(model_out, model_in, z_out, guidance, c_base, cz, ca=None, base=None, srcs=(), e_out=None, aux_out=None):
    """One launch per sampler call (vsys_cfg_pndm_step): e = u + guidance (c - u) with u = model_out[b], c = model_out[b + Bz] on the first
    Cin of the 2 Cin channels of model_out fp32 [2 Bz, 2 Cin, ...]; over S = (e, *srcs) (up to four fp32 tensors like z_out, None = absent)
    z_out = c_base base + sum cz[i] S[i], aux_out = sum ca[i] S[i], e_out = e, both halves of model_in bf16 [2 Bz, Cin, ...] = the same
    form as z_out rounded to bf16.  fp64 arithmetic on the fp32 operands, one rounding per stored value FROM THE fp64 VALUE (model_in
    is not the fp32 z_out rounded again).  ``base`` may be ``z_out``, ``aux_out`` may be one of ``srcs``.
    ``cz`` / ``ca``: up to five host floats each (missing ones are 0)."""
    srcs = tuple(srcs) + (None,) * (4 - len(srcs))
    assert len(srcs) == 4, "at most four sources"
    # (the weights are per-call scalars in a host array and the source / output pointers rotate from call to call: a recorded copy
    #  would replay the values and addresses of the call it was recorded on)
    assert program.active() is None, "vsys_cfg_pndm_step: its scalars and pointers change every call, launch it after the replay"
    Bz, Cin = z_out.shape[:2]
    thw = z_out[0, 0].numel()
    assert model_out.dtype == torch.float32 and model_out.is_contiguous()
    assert model_out.shape[1] == 2 * Cin, f"model_out has {model_out.shape[1]} channels, not 2 x {Cin} (learned sigma)"
    assert tuple(model_out.shape) == (2 * Bz, 2 * Cin) + tuple(z_out.shape[2:]), (tuple(model_out.shape), tuple(z_out.shape))
    assert model_in.is_contiguous() and tuple(model_in.shape) == (2 * Bz,) + tuple(z_out.shape[1:])
    for t in (z_out, base, e_out, aux_out) + srcs:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == z_out.shape)
    outs = [t for t in (z_out, e_out, aux_out) if t is not None]
    assert len({t.data_ptr() for t in outs}) == len(outs), "the outputs must be distinct buffers"
    cz = [float(v) for v in cz] + [0.0] * (5 - len(cz))
    ca = [float(v) for v in (ca or ())] + [0.0] * (5 - len(ca or ()))
    assert len(cz) == 5 and len(ca) == 5
    for k, t in enumerate(srcs):
        assert t is not None or (cz[k + 1] == 0.0 and (ca[k + 1] == 0.0 or aux_out is None)), f"a non-zero weight on source {k}, which is None"
    assert base is not None or float(c_base) == 0.0, "a non-zero c_base, but no base"
    _chk(model_out, model_in, z_out, base, e_out, aux_out, *srcs)       # (after the argument checks, as above)
    _bf16(model_in)
    coef = (ctypes.c_double * 12)(float(guidance), float(c_base), *cz, *ca)
    _call("vsys_cfg_pndm_step", _p(model_out), _p(e_out), *[_p(t) for t in srcs], _p(base), _p(z_out), _p(aux_out), _p(model_in), Bz, Cin,
          2 * Cin, thw, coef)
    return z_out, model_in
