"""Tensor-level wrappers of the entry points that exist for Open-Sora-Plan v1.2 (include/videosys_amd.h): the head-dim-96 attention
(vsys_attn_prep_kv96, vsys_flash_attn_d96 and their forms on a sequence-parallel exchange image, vsys_attn_prep_kv96_img,
vsys_flash_attn_d96_img) and, at the end of the file, the CausalVAE decode and sampler kernels
(vsys_upsample_trilinear2x, vsys_cfg_ancestral_step, vsys_pixels_to_u8_trunc).  HIP device tensors only, no eager fallback.

Every entry point here has an op code and goes through ``ops._call`` like the wrappers of ops.py: issued through
torch.ops.vsys.launch, and under a launch-program recorder logged as a vsys_cmd, so a recorded step replays the attention launches
inside its vsys_program_run call.  The per-sample key counts of the cross-attention are read by the kernel from device memory, so a
replay carries no count.
Element-wise tests: tests/test_gpu_osp_attention.py, tests/test_gpu_osp_attention_img.py; guard bands: tests/test_gpu_isolation_osp.py,
tests/test_gpu_isolation_osp_img.py."""
from __future__ import annotations

import torch

from . import program
from .ops import VaeGrid, _bf16, _call, _chk, _p, kv_pad_len

HEAD_DIM = 96


def alloc_kv_buffers96(batch, heads, kv_len, device):
    """(kp [batch, heads, kv_pad, 96], vt [batch, heads, 96, kv_pad]) for kv_len keys, kv_pad = the next multiple of 64."""
    kv_pad = kv_pad_len(kv_len)
    kp = torch.zeros(batch, heads, kv_pad, HEAD_DIM, dtype=torch.bfloat16, device=device)
    vt = torch.zeros(batch, heads, HEAD_DIM, kv_pad, dtype=torch.bfloat16, device=device)
    return kp, vt


def _tables(rope_cos, rope_sin, rows):
    if rope_cos is None:
        assert rope_sin is None
        return
    for t in (rope_cos, rope_sin):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, HEAD_DIM)


def attn_prep_kv96(k, v, rope_cos, rope_sin, kp, vt, batch, heads, kv_len):
    """k, v: 2-D row-strided views [batch * kv_len, >= heads * 96] -> kp (RoPE3D rotation with the per-token fp32 tables
    [kv_len, 96], None = none; softmax scale folded in; one rounding) and vt (transposed); keys past kv_len are written as zeros."""
    _chk(k, v, rope_cos, rope_sin, kp, vt)
    _bf16(k, v, kp, vt)
    assert k.dim() == 2 and v.dim() == 2 and k.stride(1) == 1 and v.stride(1) == 1 and kp.is_contiguous() and vt.is_contiguous()
    assert k.shape[0] >= batch * kv_len and v.shape[0] >= batch * kv_len and k.shape[1] >= heads * HEAD_DIM and v.shape[1] >= heads * HEAD_DIM
    kv_pad = kp.shape[-2]
    assert tuple(kp.shape[-3:]) == (heads, kv_pad, HEAD_DIM) and tuple(vt.shape[-3:]) == (heads, HEAD_DIM, kv_pad)
    assert kp.numel() == vt.numel() == batch * heads * kv_pad * HEAD_DIM
    _tables(rope_cos, rope_sin, kv_len)
    _call("vsys_attn_prep_kv96", _p(k), k.stride(0), _p(v), v.stride(0), _p(rope_cos), _p(rope_sin), _p(kp), _p(vt), batch, heads, kv_len,
          kv_pad)


def flash_attn96(q, rope_cos, rope_sin, kp, vt, kv_lens, out, batch, heads, q_len, kv_len):
    """out = softmax(rope(q) k^T / sqrt(96)) v on the layouts of attn_prep_kv96.  q, out: 2-D row-strided views [batch * q_len, >=
    heads * 96]; rope tables fp32 [q_len, 96] or None; kv_lens: device int32 [batch] (sample b sees its first kv_lens[b] keys, every
    count >= 1 — the caller's to guarantee) or None."""
    _chk(q, rope_cos, rope_sin, kp, vt, kv_lens, out)
    _bf16(q, kp, vt, out)
    assert q.dim() == 2 and out.dim() == 2 and q.stride(1) == 1 and out.stride(1) == 1
    assert q.shape[0] >= batch * q_len and out.shape[0] >= batch * q_len and q.shape[1] >= heads * HEAD_DIM and out.shape[1] >= heads * HEAD_DIM
    kv_pad = kp.shape[-2]
    assert kp.numel() == vt.numel() == batch * heads * kv_pad * HEAD_DIM and kv_len <= kv_pad
    _tables(rope_cos, rope_sin, q_len)
    if kv_lens is not None:
        assert kv_lens.dtype == torch.int32 and kv_lens.is_contiguous() and kv_lens.numel() == batch
    _call("vsys_flash_attn_d96", _p(q), q.stride(0), _p(rope_cos), _p(rope_sin), _p(kp), _p(vt), _p(kv_lens), _p(out), out.stride(0),
          batch, heads, q_len, kv_len, kv_pad)
    return out


def _image(t, batch, heads, length, seg_len, slab_rows):
    """The slab checks of the image entry points: ``t`` is a 2-D row-strided view that holds every slab of ``length`` tokens."""
    assert t.dim() == 2 and t.stride(1) == 1 and t.shape[1] >= heads * HEAD_DIM
    assert seg_len >= 1
    if seg_len >= length:        # one slab: samples seg_len rows apart, the slab stride is unused
        assert t.shape[0] >= (batch - 1) * seg_len + length
        return
    assert slab_rows >= batch * seg_len, "a slab holds at least batch * seg_len rows"
    nslab = -(-length // seg_len)
    last = length - (nslab - 1) * seg_len
    assert t.shape[0] >= (nslab - 1) * slab_rows + (batch - 1) * seg_len + last


def attn_prep_kv96_img(k, v, rope_cos, rope_sin, kp, vt, batch, heads, kv_len, seg_len, slab_rows):
    """attn_prep_kv96 on an exchange image (vsys_attn_prep_kv96_img): token s of sample b is row (s // seg_len) * slab_rows + b * seg_len
    + s % seg_len of k and of v (the receive image [P (source)][B][Nl][...] of the Ulysses all-to-all: seg_len = Nl, slab_rows = B * Nl).
    Same bits as attn_prep_kv96 on the gathered rows; rows that belong to no token are neither read nor written."""
    _chk(k, v, rope_cos, rope_sin, kp, vt)
    _bf16(k, v, kp, vt)
    assert kp.is_contiguous() and vt.is_contiguous()
    _image(k, batch, heads, kv_len, seg_len, slab_rows), _image(v, batch, heads, kv_len, seg_len, slab_rows)
    kv_pad = kp.shape[-2]
    assert tuple(kp.shape[-3:]) == (heads, kv_pad, HEAD_DIM) and tuple(vt.shape[-3:]) == (heads, HEAD_DIM, kv_pad)
    assert kp.numel() == vt.numel() == batch * heads * kv_pad * HEAD_DIM
    _tables(rope_cos, rope_sin, kv_len)
    _call("vsys_attn_prep_kv96_img", _p(k), k.stride(0), _p(v), v.stride(0), _p(rope_cos), _p(rope_sin), _p(kp), _p(vt), batch, heads,
          kv_len, kv_pad, seg_len, slab_rows)


def flash_attn96_img(q, rope_cos, rope_sin, kp, vt, kv_lens, out, batch, heads, q_len, kv_len, seg_len, q_slab_rows, out_slab_rows):
    """flash_attn96 with q and out as exchange images (vsys_flash_attn_d96_img): query token s of sample b is row (s // seg_len) *
    slab_rows + b * seg_len + s % seg_len, q and out each with its own slab stride and row stride — q the receive image of the way
    there, out the send image of the way back.  Same bits as flash_attn96 on the gathered rows."""
    _chk(q, rope_cos, rope_sin, kp, vt, kv_lens, out)
    _bf16(q, kp, vt, out)
    _image(q, batch, heads, q_len, seg_len, q_slab_rows), _image(out, batch, heads, q_len, seg_len, out_slab_rows)
    kv_pad = kp.shape[-2]
    assert kp.numel() == vt.numel() == batch * heads * kv_pad * HEAD_DIM and kv_len <= kv_pad
    _tables(rope_cos, rope_sin, q_len)
    if kv_lens is not None:
        assert kv_lens.dtype == torch.int32 and kv_lens.is_contiguous() and kv_lens.numel() == batch
    _call("vsys_flash_attn_d96_img", _p(q), q.stride(0), _p(rope_cos), _p(rope_sin), _p(kp), _p(vt), _p(kv_lens), _p(out), out.stride(0),
          batch, heads, q_len, kv_len, kv_pad, seg_len, q_slab_rows, out_slab_rows)
    return out


# ------------------------------------------------------------------------------------------------ CausalVAE decode and sampler
# (csrc/vae_osp.hip.  The two decode kernels are recordable like the other VAE kernels; the sampler step refuses to run under a
#  recorder, see there.  Element-wise tests: tests/test_gpu_osp_vae_kernels.py; guard bands: tests/test_gpu_isolation_osp_pipeline.py)
def upsample_trilinear2x(x, gs: VaeGrid, y, gd: VaeGrid, C):
    """Spatial2xTime2x3DUpsample up to its conv: x rows over gs -> the interior rows of gd ((1 if T == 1 else 2T - 1) frames of
    (2H, 2W)); F.interpolate(mode="trilinear") of frame 0 by (1, 2, 2) and of the later frames by (2, 2, 2) among themselves, the eight
    taps accumulated in fp32 and rounded once (include/videosys_amd.h)."""
    _chk(x, y)
    _bf16(x, y)
    assert x.shape == (gs.rows, C) and y.shape == (gd.rows, C) and x.is_contiguous() and y.is_contiguous()
    _call("vsys_upsample_trilinear2x", _p(x), gs._c, _p(y), gd._c, gs.n, C)
    return y


def cfg_ancestral_step(z, model_out, noise, model_in, guidance, dt, sigma_up, in_scale):
    """z fp32 [Bz, Cin, ...] in place: z + dt (u + guidance (c - u)) + sigma_up noise with u = model_out[b], c = model_out[b + Bz] on
    the first Cin of the 2 Cin channels of model_out fp32 [2 Bz, 2 Cin, ...]; model_in bf16 [2 Bz, Cin, ...]: both halves
    bf16(z' * in_scale).  ``noise``: fp32 like z, or None when sigma_up == 0."""
    _chk(z, model_out, noise, model_in)
    _bf16(model_in)
    # (dt, sigma_up and guidance are per-call scalars: a recorded copy would replay the values of the step it was recorded on)
    assert program.active() is None, "vsys_cfg_ancestral_step: its scalars change every call, launch it after the replay"
    Bz, Cin = z.shape[:2]
    thw = z[0, 0].numel()
    assert z.dtype == torch.float32 and model_out.dtype == torch.float32 and z.is_contiguous() and model_out.is_contiguous()
    assert tuple(model_out.shape) == (2 * Bz, 2 * Cin) + tuple(z.shape[2:]), (tuple(model_out.shape), tuple(z.shape))
    assert model_in.is_contiguous() and tuple(model_in.shape) == (2 * Bz,) + tuple(z.shape[1:])
    if noise is not None:
        assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.shape == z.shape
    else:
        assert sigma_up == 0.0, "no noise tensor, but sigma_up != 0"
    _call("vsys_cfg_ancestral_step", _p(z), _p(model_out), _p(noise), _p(model_in), Bz, Cin, 2 * Cin, thw, float(guidance), float(dt),
          float(sigma_up), float(in_scale))
    return z, model_in


def pixels_to_u8_trunc(x, g: VaeGrid, out, f0):
    """first 3 channels of the interior rows of grid g (x [g.rows, ldx] bf16, row-strided) -> out uint8 [Ftot, H, W, 3], frames
    f0 .. f0 + g.n * g.T - 1: trunc(bf16(clamp(bf16(bf16(x / 2) + 0.5), 0, 1) * 255)), the reference pipeline's own post-process."""
    _chk(x, out)
    _bf16(x)
    assert x.dim() == 2 and x.shape[0] == g.rows and x.stride(1) == 1 and x.shape[1] >= 3
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 4 and tuple(out.shape[1:]) == (g.H, g.W, 3)
    _call("vsys_pixels_to_u8_trunc", _p(x), g._c, g.n, x.stride(0), _p(out), out.shape[0], f0)
    return out
