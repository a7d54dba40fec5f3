"""The K/V column order of the spatial qkv site (csrc/vsys_internal.h qkv_kv_column; ops.qkv_kv_column_order is its host mirror, and
tests/test_gpu_fused_kv.py holds the device side to it): a permutation of the 216 heads output features into 96-column windows such
that every K head lies whole inside ONE window — the column window of one GEMM wave — so that its RMS norm needs no other wave."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def order(heads):
    from videosys_amd import ops

    return ops.qkv_kv_column_order(heads)


@pytest.mark.parametrize("heads", [8, 16, 24])
def test_column_order_is_a_bijection_with_whole_k_heads(heads):
    C = 72 * heads
    col = order(heads)
    assert col.dtype == torch.int64 and col.shape == (3 * C,)
    assert torch.equal(torch.sort(col).values, torch.arange(3 * C)), "not a bijection of 0 .. 3C - 1"
    assert torch.equal(col[:C], torch.arange(C)), "Q keeps the checkpoint's order"
    nq = C // 96
    assert C % 96 == 0 and (3 * C) % 192 == 0 and 3 * C // 96 == nq + heads + heads // 2
    # every K head: columns 0 .. 71 of exactly one window, one head per window
    wins = set()
    for h in range(heads):
        kc = col[C + 72 * h:C + 72 * (h + 1)]
        w = int(kc[0]) // 96
        assert torch.equal(kc, w * 96 + torch.arange(72)), f"K head {h} is not columns 0-71 of one window"
        assert w == nq + h
        wins.add(w)
    assert len(wins) == heads
    # every V feature appears once: 24 per K window (columns 72-95), the rest in windows of their own, in feature order
    vc = col[2 * C:]
    assert len(set(vc.tolist())) == C and int(vc.min()) >= nq * 96
    for h in range(heads):
        assert torch.equal(vc[24 * h:24 * (h + 1)], (nq + h) * 96 + 72 + torch.arange(24))
    assert torch.equal(vc[24 * heads:], (nq + heads) * 96 + torch.arange(C - 24 * heads))


@pytest.mark.parametrize("heads", [8, 16])
def test_permuting_and_unpermuting_site_tensors_round_trips(heads):
    """W', cs, cv written through the order (row n at column order[n]) and read back through it are the originals."""
    N, K = 216 * heads, 96
    g = torch.Generator().manual_seed(heads)
    W, cs, cv = torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)
    col = order(heads)
    Wp, csp, cvp = torch.empty_like(W), torch.empty_like(cs), torch.empty_like(cv)
    Wp[col], csp[col], cvp[col] = W, cs, cv
    assert torch.equal(Wp[col], W) and torch.equal(csp[col], cs) and torch.equal(cvp[col], cv)
    inv = torch.empty_like(col)
    inv[col] = torch.arange(N)
    assert torch.equal(Wp, W[inv]) and torch.equal(col[inv], torch.arange(N))
    assert not torch.equal(Wp, W)


def test_entry_point_is_declared_bound_and_recordable():
    from videosys_amd import _lib, _opcodes

    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    m = re.search(r"\nint vsys_gemm_bf16_ln_qkv_kv\(([^;]*?)\);", hdr, flags=re.S)
    assert m is not None and m.group(1).strip().endswith("void* stream")
    nargs = len(m.group(1).split(","))
    assert len(_lib.SIGNATURES["vsys_gemm_bf16_ln_qkv_kv"]) == nargs
    assert "vsys_gemm_bf16_ln_qkv_kv" in _opcodes.OPCODES, "the fused launch must be recordable in a launch program"
    assert "vsys_gemm_bf16_ln_qkv_kv_dispatched" not in _opcodes.OPCODES   # a host-side query, not a launch


def test_switch_is_read_once_and_models_start_from_it():
    from videosys_amd import ops
    from videosys_amd.stdit3 import STDiT3, STDiT3Config

    assert isinstance(ops.FUSED_KV, bool)
    m = STDiT3(STDiT3Config(depth=1, hidden_size=576, num_heads=8, caption_channels=64, model_max_length=16), device="cpu")
    assert m.fused_kv == ops.FUSED_KV
    # shapes the fused entry does not take keep the two-kernel path: frames of 16 tokens, or a sequence-parallel layout
    assert not m._fused_kv_ok(2 * 5 * 16, 16)
