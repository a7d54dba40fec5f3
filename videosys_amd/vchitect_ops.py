"""Tensor-level wrappers of the entry points that exist for Vchitect-2.0 (include/videosys_amd.h: vsys_attn_temporal_d64,
vsys_attn_temporal_d64_img, vsys_scale_add_rows of the transformer; vsys_vae_first_im2col_nc, vsys_pixels_to_u8 of the SD3 VAE decode), on the launch route of
videosys_amd.ops (torch.ops.vsys.launch / ctypes, recorded by program.py).  The one exception is vsys_attn_temporal_d64_img, whose 26
integer / pointer arguments do not fit a vsys_cmd (24): see attn_temporal64_img.  HIP device tensors only, no eager fallback.  Guard-band tests: tests/test_gpu_isolation_vchitect.py,
tests/test_gpu_isolation_vchitect_pipeline.py."""
from __future__ import annotations

import torch

from . import _lib, program
from .ops import VaeGrid, _bf16, _call, _chk, _p


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


def attn_temporal64_img(q_vid, k_vid, v_vid, q_txt, k_txt, v_txt, rope_cos, rope_sin, out_vid, out_txt, B, T, Tl, S, L, heads,
                        defer=False):
    """attn_temporal64 on the receive image of the frame -> token switch (vsys_attn_temporal_d64_img): *_vid [nslab * B * Tl * S, >=
    heads*64] rows ordered (slab, b, t % Tl, s) with nslab >= ceil(T / Tl) (an image has one slab per rank, also for the ranks that
    hold only padded frames), *_txt likewise with L; frames past T are neither read nor written, and out_* is the image the return
    collective sends.  Same bits as attn_temporal64 on the un-imaged rows.
    The entry point takes 26 integer / pointer arguments and a vsys_cmd holds VSYS_CMD_MAX_INT = 24, so it is the one launch entry
    point without an op code (csrc/gen/program_gen.py NO_OP): the launch goes through ctypes on torch's current stream, and code
    under a launch-program recorder issues it from a ``program.host_call`` closure (the collective's, dsp.all_to_all_single(before=)),
    never bare: ``defer=True`` checks the arguments now and returns the closure that launches."""
    ts = (q_vid, k_vid, v_vid, q_txt, k_txt, v_txt, out_vid, out_txt)
    _chk(*ts, rope_cos, rope_sin)
    _bf16(*ts)
    nslab = -(-T // Tl)
    for t, n in zip(ts, (S, S, S, L, L, L, S, L)):
        if n > 0:
            assert t is not None and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] >= heads * 64
            assert t.shape[0] >= nslab * B * Tl * n and t.shape[0] % (B * Tl * n) == 0
    if rope_cos is not None:
        assert rope_cos.dtype == torch.float32 and rope_cos.is_contiguous() and rope_cos.shape == (T, 32)
        assert rope_sin.dtype == torch.float32 and rope_sin.is_contiguous() and rope_sin.shape == (T, 32)
    ld = lambda t: 0 if t is None else t.stride(0)
    dp = lambda t: None if t is None else t.data_ptr()
    program.keep(ts), program.keep((rope_cos, rope_sin))
    args = (dp(q_vid), ld(q_vid), dp(k_vid), ld(k_vid), dp(v_vid), ld(v_vid), dp(q_txt), ld(q_txt), dp(k_txt), ld(k_txt), dp(v_txt),
            ld(v_txt), dp(rope_cos), dp(rope_sin), dp(out_vid), ld(out_vid), dp(out_txt), ld(out_txt), B, T, Tl, B * Tl * S, B * Tl * L, S, L,
            heads)
    fn = _lib.load().vsys_attn_temporal_d64_img

    def issue():
        _lib.check(fn(*args, torch.cuda.current_stream().cuda_stream), "vsys_attn_temporal_d64_img")

    if defer:
        return issue
    assert program.active() is None, "vsys_attn_temporal_d64_img does not fit a vsys_cmd: under a recorder issue it from a host_call closure (defer=True)"
    issue()
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


def vae_first_im2col_nc(z_f32, kcols, scaling_factor, shift_factor):
    """z fp32 [F, Cz, H, W] (Cz <= 32) -> bf16 [F*H*W, kcols] rows of a 3 x 3 conv over bf16(bf16(bf16(z) / scaling_factor) +
    shift_factor): column tap * Cz + c, zero outside the image and from column 9 Cz on (include/videosys_amd.h)."""
    _chk(z_f32)
    assert z_f32.dtype == torch.float32 and z_f32.dim() == 4 and z_f32.is_contiguous()
    F, Cz, H, W = z_f32.shape
    out = torch.empty(F * H * W, kcols, dtype=torch.bfloat16, device=z_f32.device)
    _call("vsys_vae_first_im2col_nc", _p(z_f32), F, Cz, H, W, kcols, float(scaling_factor), float(shift_factor), _p(out))
    return out


def pixels_to_u8(x, g: VaeGrid, out, f0):
    """first 3 channels of the interior rows of grid g (x [g.rows, ldx] bf16, row-strided) -> out uint8 [Ftot, H, W, 3], frames
    f0 .. f0 + g.n * g.T - 1: round-half-even(clamp(bf16(bf16(x / 2) + 0.5), 0, 1) * 255) (include/videosys_amd.h)."""
    _chk(x, out)
    _bf16(x)
    assert x.dim() == 2 and x.shape[0] == g.rows and x.stride(1) == 1 and x.shape[1] >= 3
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 4 and tuple(out.shape[1:]) == (g.H, g.W, 3)
    _call("vsys_pixels_to_u8", _p(x), g._c, g.n, x.stride(0), _p(out), out.shape[0], f0)
    return out
