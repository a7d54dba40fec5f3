"""-m gpu: vae_blocks.vae_flash_attn (csrc/attention_vae.hip: key blocks of 32, query blocks of 128) element-wise against float64 with
the bound of numerics.attention_ref, at the block edges and just past 8192 keys; then one call inside guard bands (tests/isolation.py).
diffuse: randn q, k, v = randn + 0.5.  retrieval: keys of norm sqrt(C), query i = 3 x a key of the LAST key block (its logit leads by
>= 22 nats; the running maximum moves in the last block).  Pad rows of q / k are NaN (never read), pad columns of V^T hold 7."""
import math

import pytest
import torch

import isolation as iso
import numerics as nm
from isolation_cases import rnd, strided

pytestmark = pytest.mark.gpu

KB, QB = 32, 128                 # key block, query block of the kernel
LOG2E = math.log2(math.e)
SHAPES = [(1, 1, 128), (2, 6, 128), (1, KB + 1, 128), (2, 200, 256), (1, QB + 1, 256), (1, 8200, 8320)]   # (n, L, Lp)
CASES = [(n, L, Lp, C) for n, L, Lp in SHAPES for C in (128, 512) if L <= 8192 or C == 128]


def reference(family, n, L, C, device):
    """Operands and the float64 reference of the rows that are compared: all of them, at L = 8200 the first and the last 64."""
    g = torch.Generator().manual_seed(1000 * L + C + n)
    k, v, targets = torch.randn(n, L, C, generator=g), torch.randn(n, L, C, generator=g) + 0.5, None
    if family == "diffuse":
        q = torch.randn(n, L, C, generator=g)
    else:
        k = k * (C**0.5 / k.norm(dim=-1, keepdim=True))
        last = (L - 1) // KB * KB
        t = last + torch.arange(L) % (L - last)
        q, targets = 3.0 * k.to(torch.bfloat16).float()[:, t], t[None, :, None].expand(n, L, 1)
    q, k, v = (x.to(torch.bfloat16) for x in (q, k, v))
    rows = torch.arange(L) if L <= 4096 else torch.cat([torch.arange(64), torch.arange(L - 64, L)])
    ref = nm.attention_ref(q[:, rows].to(device).double(), k.to(device).double(), v.to(device).double(), log2_scale=C**-0.5 * LOG2E,
                           denominator="fp32", targets=None if targets is None else targets[:, rows].to(device), tile=KB)
    assert ref.vacuous == 0, f"{family} n{n} L{L} C{C}: {ref.vacuous} rows of the reference have no finite bound"
    assert targets is None or ref.weight.min().item() >= 1 - 2.0**-12, "the retrieval construction is too weak"
    return q, k, v, rows, ref


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("n,L,Lp,C", CASES)
def test_vae_flash_attn_elementwise(n, L, Lp, C, family):
    from videosys_amd import vae_blocks

    dev = torch.device("cuda:0")
    q, k, v, rows, ref = reference(family, n, L, C, dev)
    qd, kd = (torch.full((n, Lp, C), float("nan"), dtype=torch.bfloat16, device=dev) for _ in range(2))
    vt = torch.full((n, C, Lp), 7.0, dtype=torch.bfloat16, device=dev)
    qd[:, :L], kd[:, :L], vt[:, :, :L] = q.to(dev), k.to(dev), v.to(dev).transpose(1, 2)
    out = torch.full((n * Lp, C), float("nan"), dtype=torch.bfloat16, device=dev)
    vae_blocks.vae_flash_attn(qd.view(n * Lp, C), kd.view(n * Lp, C), vt, n, L, Lp, C**-0.5, out=out)
    torch.cuda.synchronize()
    o = out.view(n, Lp, C)
    nm.check_elementwise(o[:, rows.to(dev)], ref.out, ref.bound, f"vae_flash_attn {family} n{n} L{L} Lp{Lp} C{C}")
    assert bool(o[:, L:].isnan().all()), "rows L .. Lp - 1 of the output were written"


def test_vae_flash_attn_isolated():
    """Column slices of wider buffers.  Pad rows of q / k are guard under both fills; pad columns of V^T are read and must be finite
    (the documented contract), so their guard holds the ``max`` fill only."""
    from videosys_amd import vae_blocks

    dev, n, L, Lp, C = torch.device("cuda:0"), 2, 200, 256, 512
    pad_rows = (torch.arange(n * Lp, device=dev) % Lp >= L)[:, None].expand(n * Lp, C).contiguous()
    pad_keys = (torch.arange(Lp, device=dev) >= L).expand(n, C, Lp).contiguous()
    o = {name: strided(rnd(dev, (n * Lp, C), seed)) for name, seed in (("q", 1), ("k", 2))}
    o["q"].interior = o["k"].interior = pad_rows
    o["vt"] = iso.Operand(rnd(dev, (n, C, Lp), 3, 1.0, 0.5), parent=(n, C, Lp + 16), at=(0, 0, 8), interior=pad_keys, interior_fills=("max",))
    o["out"] = strided(torch.zeros(n * Lp, C, dtype=torch.bfloat16, device=dev))
    o["out"].callers = pad_rows

    def fn(t):
        vae_blocks.vae_flash_attn(t["q"], t["k"], t["vt"], n, L, Lp, C**-0.5, out=t["out"])

    iso.check_isolated(fn, o, ["out"], [], what="vae_flash_attn C=512 n=2 L=200 Lp=256")
