"""-m gpu: guard-band tests (tests/isolation.py) of the two head-dim-96 entry points of Open-Sora-Plan v1.2:
open_sora_plan_ops.attn_prep_kv96 and open_sora_plan_ops.flash_attn96 (attention96.hip).  Exact assertions only, under both guard
fills: same bits as the call on tight operands, every guard byte untouched, every input unchanged.

Operand forms: q / k / v are column slices of wider parents of their own, so both neighbours of every operand are guard; the RoPE
tables are tight (rows behind the last token are guard: a token index past the end would read them); Kp / Vt tight with one 64-key
tile of every (batch, head) image as extra guard; ``out`` row-strided with live guard columns on both sides.  heads = 3; 72 tokens (one
full 64-key tile + 8, one partial 128-row query block) and 130 (two tiles + 2, a second query block of two rows); the cross form
reads kv_lens = [5, 130] on the device (its guard holds other VALID counts).  The keys a count hides are ordinary finite data: the
contract asks that of masked keys (their V is multiplied by a zero probability)."""
import pytest
import torch

import isolation as iso
from isolation import Operand

pytestmark = pytest.mark.gpu

HD, H, B = 96, 3, 2


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
    ang = (torch.rand(n, 3, 16, generator=g) * 6.0).repeat(1, 1, 2).reshape(n, HD)
    return ang.cos().contiguous().to(dev()), ang.sin().contiguous().to(dev())


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("N", [72, 130])
def test_isolation_attn_prep_kv96(N, rope):
    from videosys_amd import open_sora_plan_ops as oops

    C = H * HD
    kv_pad = oops.kv_pad_len(N)
    o = {"k": strided(rnd((B * N, C), N), 8, 16), "v": strided(rnd((B * N, C), N + 1, 0.5), 16, 8),
         # every element of both images is written (pad keys: zeros): pure outputs
         "kp": Operand(torch.zeros(B, H, kv_pad, HD, dtype=torch.bfloat16, device=dev()), guard_elems=B * H * 64 * HD),
         "vt": Operand(torch.zeros(B, H, HD, kv_pad, dtype=torch.bfloat16, device=dev()), guard_elems=B * H * 64 * HD)}
    if rope:
        cos, sin = tables(N, N)
        o["cos"], o["sin"] = Operand(cos), Operand(sin)

    def fn(t):
        oops.attn_prep_kv96(t["k"], t["v"], t.get("cos"), t.get("sin"), t["kp"], t["vt"], B, H, N)

    iso.check_isolated(fn, o, ["kp", "vt"], what=f"attn_prep_kv96 N={N} rope={rope}")


@pytest.mark.parametrize("form", ["self", "cross"])
@pytest.mark.parametrize("N", [72, 130])
def test_isolation_flash_attn96(N, form):
    from videosys_amd import open_sora_plan_ops as oops

    C = H * HD
    Lk = N if form == "self" else 130
    cos, sin = tables(N, N) if form == "self" else (None, None)
    kv = rnd((B * Lk, 2 * C), Lk + 5)
    kv[:, C:] += 0.5
    kp, vt = oops.alloc_kv_buffers96(B, H, Lk, dev())
    oops.attn_prep_kv96(kv[:, :C], kv[:, C:], cos if Lk == N else None, sin if Lk == N else None, kp, vt, B, H, Lk)
    torch.cuda.synchronize()
    o = {"q": strided(rnd((B * N, C), N + 2), 16, 8), "kp": Operand(kp, guard_elems=B * H * 64 * HD),
         "vt": Operand(vt, guard_elems=B * H * 64 * HD), "out": strided(torch.zeros(B * N, C, dtype=torch.bfloat16, device=dev()), 8, 24)}
    if form == "self":
        o["cos"], o["sin"] = Operand(cos), Operand(sin)
    else:
        o["lens"] = Operand(torch.tensor([5, 130], dtype=torch.int32, device=dev()), int_guard=[7, 64, 1, 129])

    def fn(t):
        oops.flash_attn96(t["q"], t.get("cos"), t.get("sin"), t["kp"], t["vt"], t.get("lens"), t["out"], B, H, N, Lk)

    iso.check_isolated(fn, o, ["out"], what=f"flash_attn96 {form} N={N}")
