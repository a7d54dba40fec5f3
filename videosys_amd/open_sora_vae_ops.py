"""Tensor-level wrapper of the entry point that exists for the Open-Sora v1.2 VAE's ENCODER (include/videosys_amd.h):
vsys_conv_causal_tdown2_bf16, the stride-(2, 1, 1) CausalConv3d of VAE_Temporal's encoder (csrc/conv_causal_tdown_bf16.hip).  HIP device
tensors only, no eager fallback.

The entry point has no op code: ``conv_causal_tdown2`` calls it through ctypes from a ``program.host_call`` closure, as
``open_sora_plan_ops.conv_down2`` does (which serves the three spatial stride-2 layers of the same encoder in its kt = 1 mode).
Element-wise test and guard bands: tests/test_gpu_conv_causal_tdown.py."""
from __future__ import annotations

import torch

from . import _lib, program
from .ops import VaeGrid, _bf16, _chk


def causal_tdown2_grid(grid: VaeGrid) -> VaeGrid:
    """The dense output grid of ``conv_causal_tdown2`` over ``grid``: T // 2 frames of the same H x W."""
    return VaeGrid(grid.n, grid.T // 2, grid.H, grid.W, 0, 0)


def conv_causal_tdown2(x, grid: VaeGrid, w, bias, cin, out=None):
    """The 3 x 3 x 3 convolution of the voxels of ``grid`` (rows ``x``, any pad / tf: borders and front frames are NOT read) with stride
    2 in time behind ONE ZERO frame — tap a of output frame t' reads frame 2 t' + a - 1 — and one implicit zero row / column on every
    side.  ``w`` [cout, 27 cin] (k = tap * cin + channel), ``bias`` [cout] or None.  Returns the dense rows of
    ``causal_tdown2_grid(grid)`` [rows, cout]; grid.T >= 2, an odd T leaves its last frame unread.  No op code: issued through ctypes,
    under a recorder from a host closure."""
    _chk(x, w, bias, out)
    _bf16(x, w, bias, out)
    assert x.shape[0] == grid.rows and x.stride(1) == 1 and x.shape[1] >= cin and w.shape[1] == 27 * cin and w.stride(1) == 1
    og = causal_tdown2_grid(grid)
    if out is None:
        out = torch.empty(og.rows, w.shape[0], dtype=torch.bfloat16, device=x.device)
    assert out.shape[0] == og.rows and out.shape[1] >= w.shape[0] and out.stride(1) == 1
    program.keep((x, w, bias, out, grid))
    args = (x.data_ptr(), x.stride(0), grid._c, grid.n, w.data_ptr(), w.stride(0), None if bias is None else bias.data_ptr(),
            out.data_ptr(), out.stride(0), cin, w.shape[0])
    fn = _lib.load().vsys_conv_causal_tdown2_bf16
    program.host_call(lambda: _lib.check(fn(torch.cuda.current_stream().cuda_stream, *args), "vsys_conv_causal_tdown2_bf16"))
    return out
