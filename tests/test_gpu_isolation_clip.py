"""-m gpu: guard-band tests (tests/isolation.py) of the two kernels of the CLIP text encoders (csrc/clip_ops.hip):
vsys_clip_attention_d64 and vsys_splitk_reduce_bias_act.  Exact assertions only, under both guard fills: same bits as the call on
tight operands, every guard byte untouched, every input unchanged.

Operand forms.  Attention: qkv is a [B * L, 3 * inner] view of rows that are wider (row_stride > 3 * inner), so the slack of every row
is a guard INSIDE the buffer, on top of the bands in front and behind (a key row read past B * L, or past the sample's L rows in the
last sample, lands there); the output is a pure output with a row pitch of its own.  L = 17 (one row past a 16-row block: 15 rows of
the second block do not exist) and L = 77 (the production length, 13-row tail), B = 2.  Reduce: fp32 partials tight (a pure input
that must come back unchanged), bias tight, res and out with ldr, ldo > N."""
import pytest
import torch

import isolation as iso
from isolation import Operand

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("L", [17, 77])
def test_isolation_clip_attention(L):
    from videosys_amd import clip_ops

    B, heads = 2, 2
    inner = 64 * heads
    g = torch.Generator().manual_seed(L)
    qkv = torch.randn(B * L, 3 * inner, generator=g).to(torch.bfloat16).to(dev())
    o = {"qkv": Operand(qkv, parent=(B * L, 3 * inner + 64), at=(0, 32)),
         "out": Operand(torch.zeros(B * L, inner, dtype=torch.bfloat16, device=dev()), parent=(B * L, inner + 24), at=(0, 8))}

    def fn(t):
        clip_ops.clip_attention64(t["qkv"], B, L, heads, out=t["out"])

    iso.check_isolated(fn, o, ["out"], what=f"clip_attention_d64 L={L}")


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,N,S", [(77, 128, 3), (1, 768, 1)])
def test_isolation_splitk_reduce_bias_act(M, N, S, act):
    from videosys_amd import clip_ops

    g = torch.Generator().manual_seed(M + N + act)
    d = dev()
    o = {"part": Operand(torch.randn(S, M, N, generator=g).to(d)),
         "bias": Operand(torch.randn(N, generator=g).to(torch.bfloat16).to(d)),
         "res": Operand(torch.randn(M, N, generator=g).to(torch.bfloat16).to(d), parent=(M, N + 16), at=(0, 8)),
         "out": Operand(torch.zeros(M, N, dtype=torch.bfloat16, device=d), parent=(M, N + 40), at=(0, 16))}

    def fn(t):
        clip_ops.splitk_reduce_bias_act(t["part"], S, M * N, N, M, N, t["out"], bias=t["bias"], act=act, res=t["res"])

    iso.check_isolated(fn, o, ["out"], what=f"splitk_reduce_bias_act {M}x{N} S={S} act={act}")
