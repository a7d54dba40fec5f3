"""-m gpu: guard-band test (tests/isolation.py) of ops.attn_temporal past 64 frames: qkv and out are column slices of wider buffers
(row strides > 3 C and > C), everything around them is guard.  Same bits as the call on tight operands, no guard byte touched."""
import pytest
import torch

import isolation as iso
from isolation_cases import HD, rnd, strided

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T,S,heads,norm_rope", [(65, 9, 2, True), (97, 37, 6, False), (300, 9, 3, True)])
def test_isolation_temporal_long(T, S, heads, norm_rope):
    from videosys_amd import ops

    dev, B, C = torch.device("cuda:0"), 2, heads * HD
    o = {"qkv": strided(rnd(dev, (B * T * S, 3 * C), T * 100 + S)),
         "out": strided(torch.zeros(B * T * S, C, dtype=torch.bfloat16, device=dev))}
    if norm_rope:
        o["qw"], o["kw"] = iso.Operand(rnd(dev, (HD,), 1, 0.2, 1.0)), iso.Operand(rnd(dev, (HD,), 2, 0.2, 1.0))
        ang = torch.rand(T, HD // 2, generator=torch.Generator().manual_seed(T)) * 6.0
        o["cos"] = iso.Operand(ang.cos().repeat_interleave(2, -1).contiguous().to(dev))
        o["sin"] = iso.Operand(ang.sin().repeat_interleave(2, -1).contiguous().to(dev))

    def fn(t):
        ops.attn_temporal(t["qkv"], C, t.get("qw"), t.get("kw"), t.get("cos"), t.get("sin"), t["out"], B, T, S, heads)

    iso.check_isolated(fn, o, ["out"], [], what=f"attn_temporal T={T} S={S} heads={heads} norm+rope={norm_rope}")
