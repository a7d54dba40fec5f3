"""-m gpu: guard-band tests (tests/isolation.py) of the two Vchitect-2.0 entry points: vchitect_ops.attn_temporal64
(attention_t64.hip) and vchitect_ops.scale_add_rows (rowwise.hip).  Exact assertions only, under both guard fills: same bits as the
call on tight operands, every guard byte untouched, every input unchanged.

Operand forms: video q / k / v as the three column blocks of ONE fused [rows, 3 C] buffer is what the model would pass; here each is
a column slice of a wider parent of its own so that both neighbours of every operand are guard; text q / k / v likewise with another
width; the RoPE tables tight (rows behind T are guard: a frame index past T would read them); both outputs row-strided with live guard
columns on both sides.  T = 3 (a partial 4-key group), 33 (a second K / V chunk of one key: rows 1 .. 31 of the chunk lie behind the
operand), 65 (a second query pass of one query).  heads = 5: the second workgroup of a token has one head and three idle waves, whose
columns would lie behind the row."""
import pytest
import torch

import isolation as iso
from isolation import Operand

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rnd(shape, seed, offset=0.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev()) + offset).to(torch.bfloat16)


def strided(data, pad_l, pad_r):
    return Operand(data, parent=(data.shape[0], pad_l + data.shape[1] + pad_r), at=(0, pad_l))


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("T", [3, 33, 65])
def test_isolation_attn_temporal64(T, rope):
    from videosys_amd import vchitect_ops as vops

    import vchitect_ref as vr

    B, S, L, H = 2, 9, 4, 5
    C = H * 64
    o = {}
    for i, n in enumerate(("q", "k", "v")):
        o[n + "_vid"] = strided(rnd((B * T * S, C), 10 * T + i, 0.5 * (n == "v")), 8, 16)
        o[n + "_txt"] = strided(rnd((B * T * L, C), 10 * T + 3 + i, 0.5 * (n == "v")), 16, 8)
    o["out_vid"] = strided(torch.zeros(B * T * S, C, dtype=torch.bfloat16, device=dev()), 8, 8)
    o["out_txt"] = strided(torch.zeros(B * T * L, C, dtype=torch.bfloat16, device=dev()), 24, 8)
    if rope:
        cos, sin = vr.rope_tables(T)
        o["cos"], o["sin"] = Operand(cos.to(dev())), Operand(sin.to(dev()))

    def fn(t):
        vops.attn_temporal64(t["q_vid"], t["k_vid"], t["v_vid"], t["q_txt"], t["k_txt"], t["v_txt"], t.get("cos"), t.get("sin"),
                             t["out_vid"], t["out_txt"], B, T, S, L, H)

    iso.check_isolated(fn, o, ["out_vid", "out_txt"], what=f"attn_temporal64 T={T} rope={rope}")


@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("rows,C", [(1, 8), (37, 192), (300, 1536)])
def test_isolation_scale_add_rows(rows, C, inplace):
    from videosys_amd import vchitect_ops as vops

    o = {"a": strided(rnd((rows, C), rows + C), 8, 8), "b": strided(rnd((rows, C), rows + C + 1), 16, 0)}
    if not inplace:
        o["out"] = strided(torch.zeros(rows, C, dtype=torch.bfloat16, device=dev()), 8, 24)

    def fn(t):
        vops.scale_add_rows(t["a"], t["b"], 1.1, out=t["a"] if inplace else t["out"])

    outs = ["a"] if inplace else ["out"]
    iso.check_isolated(fn, o, outs, inplace=outs if inplace else (), what=f"scale_add_rows rows={rows} C={C} inplace={inplace}")
