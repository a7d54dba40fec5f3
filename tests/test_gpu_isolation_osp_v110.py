"""-m gpu: guard-band tests (tests/isolation.py) of the two entry points of Open-Sora-Plan v1.1's spatial attention:
open_sora_plan_v110_ops.attn_prep_kv_rope and open_sora_plan_v110_ops.flash_attn_rope (csrc/attention.hip).  Exact assertions only,
under both guard fills: same bits as the call on tight operands, every guard byte untouched, every input unchanged.

Operand forms: q / k / v are column slices of wider parents of their own, so both neighbours of every operand are guard; the RoPE
tables [N, 36] are tight (the rows behind the last token are guard: a token index past the end would read them); Kp / Vt tight with
one 64-key tile of every (batch, head) image as extra guard, Vt rows 73-75 and 77-95 the caller's zeros (ops.alloc_kv_buffers); ``out``
row-strided with live guard columns on both sides.  heads = 3; 72 tokens (one full 64-key tile + 8, one partial 128-row query block)
and 130 (two tiles + 2, a second query block of two rows), and 512 (eight whole tiles: the flash launcher's three-workgroup
instantiation, the kernel of the real model's 1 024 keys per frame).  The flash kernel masks the keys behind kv_len, so the pad keys of Kp / Vt
hold the zeros the prep kernel wrote (finite, as include/videosys_amd.h asks)."""
import pytest
import torch

import isolation as iso
from isolation import Operand

pytestmark = pytest.mark.gpu

HD, PAIRS, VT_ROWS, H, B = 72, 36, 96, 3, 2


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rnd(shape, seed, offset=0.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev()) + offset).to(torch.bfloat16)


def strided(data, pad_l, pad_r):
    return Operand(data, parent=(data.shape[0], pad_l + data.shape[1] + pad_r), at=(0, pad_l))


def tables(n, seed):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(n, PAIRS, generator=g) * 6.0
    return ang.cos().contiguous().to(dev()), ang.sin().contiguous().to(dev())


def vt_callers(vt):
    m = torch.zeros_like(vt, dtype=torch.bool)
    m[:, :, 73:76] = True
    m[:, :, 77:] = True
    return m


@pytest.mark.parametrize("N", [72, 130, 512])
def test_isolation_attn_prep_kv_rope(N):
    from videosys_amd import open_sora_plan_v110_ops as vops

    C = H * HD
    kv_pad = vops.kv_pad_len(N)
    cos, sin = tables(N, N)
    vt0 = torch.zeros(B, H, VT_ROWS, kv_pad, dtype=torch.bfloat16, device=dev())
    o = {"k": strided(rnd((B * N, C), N), 8, 16), "v": strided(rnd((B * N, C), N + 1, 0.5), 16, 8), "cos": Operand(cos), "sin": Operand(sin),
         "kp": Operand(torch.zeros(B, H, kv_pad, HD, dtype=torch.bfloat16, device=dev()), guard_elems=B * H * 64 * HD),
         "vt": Operand(vt0, callers=vt_callers(vt0), guard_elems=B * H * VT_ROWS * 64)}

    def fn(t):
        vops.attn_prep_kv_rope(t["k"], t["v"], t["cos"], t["sin"], t["kp"], t["vt"], B, H, N)

    iso.check_isolated(fn, o, ["kp", "vt"], what=f"attn_prep_kv_rope N={N}")


@pytest.mark.parametrize("N", [72, 130, 512])
def test_isolation_flash_attn_rope(N):
    from videosys_amd import open_sora_plan_v110_ops as vops

    C = H * HD
    cos, sin = tables(N, N)
    kv = rnd((B * N, 2 * C), N + 5)
    kv[:, C:] += 0.5
    kp, vt = vops.alloc_kv_buffers(B, H, N, dev())
    vops.attn_prep_kv_rope(kv[:, :C], kv[:, C:], cos, sin, kp, vt, B, H, N)
    torch.cuda.synchronize()
    o = {"q": strided(rnd((B * N, C), N + 2), 16, 8), "cos": Operand(cos), "sin": Operand(sin),
         "kp": Operand(kp, guard_elems=B * H * 64 * HD), "vt": Operand(vt, guard_elems=B * H * VT_ROWS * 64),
         "out": strided(torch.zeros(B * N, C, dtype=torch.bfloat16, device=dev()), 8, 24)}

    def fn(t):
        vops.flash_attn_rope(t["q"], t["cos"], t["sin"], t["kp"], t["vt"], t["out"], B, H, N, N)

    iso.check_isolated(fn, o, ["out"], what=f"flash_attn_rope N={N}")
