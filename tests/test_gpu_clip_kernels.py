"""-m gpu: the two kernels of the CLIP text encoders (csrc/clip_ops.hip) on their own.

vsys_clip_attention_d64, element-wise against float64 (tests/numerics.py): every query row against attention_ref on its OWN key
prefix (keys 0 .. i), logits log2(e) / 8 q.k, ``denominator="fp32"`` (w_j = bf16(p_j / l) from the unrounded p_j).  B = 2, 2 heads,
L in {1, 16, 17, 77, 128}: one block, an exact block, one past a block, the production length with its ragged 13-row tail, the limit.
No row may be vacuous (an infinite bound).

Causality, exact.  L = 77.  (a) k and v at positions >= j replaced by other finite values, j in {1, 16, 17, 64}: output rows < j keep
their bits.  (b) v at positions > i filled with +inf: rows <= i stay finite and keep their bits — a key block above the diagonal that
was multiplied by zero weights instead of skipped would turn them into NaN.  i runs over the last row of every 16-row block below
the tail (15, 31, 47, 63): INSIDE the diagonal block the masked weights are exact zeros that do meet V on the matrix pipe, as they do
in the reference's own `softmax(...) @ v`, so 0 x inf is NaN there for any implementation that multiplies matrices.

vsys_splitk_reduce_bias_act.  bias = NULL, act = 0: the bits of vsys_splitk_reduce.  bias, act = 0: bit-exact against the fp32
emulation ((p_0 + p_1) + ...) + bias, rounded, + res, rounded (IEEE adds: torch on the CPU gives the same bits).  act 1 / 2: y is
known exactly from that emulation; the activation in float64 on y and the bound from the contract's roundings:
  quick_gelu  a = bf16(1.702 y): rnd(a) + 2^-24 |a| (the fp32 constant); through the sigmoid (slope <= 1/4) + U_EXP s + rnd(s) for
              bf16(sigmoid) (U_EXP for the exponential, 2 x 2^-24 for the add and the division); times |y|, + rnd(y s) for the product;
  gelu        one rounding rnd(r) + the fp32 evaluation: erf to U_EXP absolute (|erf| <= 1), the add (<= 2 x 2^-24 absolute) and two
              multiplies (2 x 2^-24 of a factor <= 2): U_EXP + 6 x 2^-24, times |y| / 2 (1 + erf cancels for negative y: the error is
              absolute there);
  + res       the error so far + rnd(value + res).
M in {1, 77, 154}, N in {128, 768}, nsplit in {1, 3}, with and without res (ldr, ldo > N), once with out aliased to res; |y| up to 12."""
import math

import pytest
import torch

import numerics as nm

pytestmark = pytest.mark.gpu

B, HEADS = 2, 2
INNER = 64 * HEADS
LOG2_SCALE = math.log2(math.e) / 8


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------- attention
_QKV = {}


def qkv_case(L):
    """bf16 qkv [B * L, 3 * INNER] (unit normal) on the CPU, made once per length."""
    if L not in _QKV:
        g = torch.Generator().manual_seed(1000 + L)
        _QKV[L] = torch.randn(B * L, 3 * INNER, generator=g).to(torch.bfloat16)
    return _QKV[L]


_REF = {}


def attention_reference(L):
    """(out, bound) float64 [B * L, INNER] of the causal attention on qkv_case(L), and the number of vacuous rows; made once."""
    if L not in _REF:
        x = qkv_case(L).double().view(B, L, 3, HEADS, 64)
        out = torch.zeros(B, L, HEADS, 64, dtype=torch.float64)
        bound = torch.zeros_like(out)
        vac = 0
        for i in range(L):   # all (b, h) slices of a row share the prefix length: one stacked call per row
            q, k, v = (x[:, :i + 1, c].permute(0, 2, 1, 3) for c in range(3))           # [B, H, i + 1, 64]
            r = nm.attention_ref(q[:, :, i:i + 1], k, v, log2_scale=LOG2_SCALE, denominator="fp32")
            out[:, i], bound[:, i] = r.out[:, :, 0], r.bound[:, :, 0]
            vac += r.vacuous
        _REF[L] = (out.view(B * L, INNER), bound.view(B * L, INNER), vac)
    return _REF[L]


def run_attention(qkv, L, row_stride=None):
    from videosys_amd import clip_ops

    x = qkv.to(dev())
    if row_stride is not None:
        wide = torch.full((x.shape[0], row_stride), float("nan"), dtype=torch.bfloat16, device=dev())
        wide[:, :x.shape[1]] = x
        x = wide[:, :3 * INNER]
    out = clip_ops.clip_attention64(x, B, L, HEADS)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("L", [1, 16, 17, 77, 128])
def test_attention_elementwise_against_fp64(L):
    ref, bound, vacuous = attention_reference(L)
    assert vacuous == 0, f"{vacuous} rows of the reference have an infinite bound: the seed does not test them"
    out = run_attention(qkv_case(L), L)
    assert out.shape == (B * L, INNER) and out.dtype == torch.bfloat16
    nm.check_elementwise(out, ref, bound, f"clip_attention_d64 L={L}")


def test_attention_reads_strided_rows():
    """row_stride > 3 inner (NaN in the slack): the same bits as the tight call."""
    L = 77
    assert torch.equal(run_attention(qkv_case(L), L, row_stride=3 * INNER + 64), run_attention(qkv_case(L), L))


@pytest.mark.parametrize("j", [1, 16, 17, 64])
def test_attention_is_causal_later_keys_do_not_reach_earlier_rows(j):
    L = 77
    base = qkv_case(L)
    want = run_attention(base, L)
    other = base.clone().view(B, L, 3 * INNER)
    g = torch.Generator().manual_seed(j)
    other[:, j:, INNER:] = (torch.randn(B, L - j, 2 * INNER, generator=g) * 3).to(torch.bfloat16)
    got = run_attention(other.view(B * L, 3 * INNER), L)
    rows = lambda t: t.view(B, L, INNER)[:, :j]
    assert torch.equal(rows(got).view(torch.int16), rows(want).view(torch.int16))
    assert not torch.equal(got.view(B, L, INNER)[:, j:], want.view(B, L, INNER)[:, j:])       # (the later rows do see them)


@pytest.mark.parametrize("i", [15, 31, 47, 63])
def test_attention_skips_key_blocks_above_the_diagonal(i):
    L = 77
    base = qkv_case(L)
    want = run_attention(base, L)
    poisoned = base.clone().view(B, L, 3 * INNER)
    poisoned[:, i + 1:, 2 * INNER:] = float("inf")
    got = run_attention(poisoned.view(B * L, 3 * INNER), L).view(B, L, INNER)
    assert bool(torch.isfinite(got[:, :i + 1].float()).all()), "a row at or below i met a value row above the diagonal"
    assert torch.equal(got[:, :i + 1].view(torch.int16), want.view(B, L, INNER)[:, :i + 1].view(torch.int16))


# ---------------------------------------------------------------------------------------------------- split-K finish
def reduce_case(M, N, S):
    """Partials fp32 [S, M, N] whose sums (+ bias) cover [-12, 12] and the bulk around zero; bias and res bf16."""
    g = torch.Generator().manual_seed(M * 7 + N + S)
    y = torch.where(torch.rand(M, N, generator=g) < 0.5, torch.randn(M, N, generator=g), (torch.rand(M, N, generator=g) - 0.5) * 24)
    y.view(-1)[:4] = torch.tensor([12.0, -12.0, 6.0, -6.0])          # both tails, whatever the draw
    parts = torch.randn(S, M, N, generator=g)
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    parts[0] += (y - bias.float()) - parts.sum(0)
    res = (torch.randn(M, N, generator=g) * 2).to(torch.bfloat16)
    return parts.contiguous(), bias, res


def emulate_sum(parts, bias):
    """fp32, slices in ascending order from 0.f as the kernel starts, bias last — IEEE adds, the kernel's bits."""
    acc = torch.zeros_like(parts[0])
    for s in range(parts.shape[0]):
        acc = acc + parts[s]
    return acc + bias.float() if bias is not None else acc


def run_reduce(parts, bias, act, res, alias=False, pitch=64):
    from videosys_amd import clip_ops

    S, M, N = parts.shape
    d = dev()
    out = torch.full((M, N + pitch), float("nan"), dtype=torch.bfloat16, device=d)[:, :N]
    r = None
    if res is not None:
        r = torch.full((M, N + 2 * pitch), float("nan"), dtype=torch.bfloat16, device=d)[:, :N]
        r.copy_(res)
    if alias:
        out = r
    clip_ops.splitk_reduce_bias_act(parts.to(d), S, M * N, N, M, N, out, bias=None if bias is None else bias.to(d), act=act, res=r)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [128, 768])
@pytest.mark.parametrize("M", [1, 77, 154])
def test_reduce_bias_act(M, N, S):
    from videosys_amd import ops

    parts, bias, res = reduce_case(M, N, S)
    d = dev()
    # bias = NULL, act = 0: the bits of vsys_splitk_reduce, with and without the residual
    for r in (None, res):
        plain = torch.empty(M, N, dtype=torch.bfloat16, device=d)
        rd = None if r is None else r.to(d)
        ops._call("vsys_splitk_reduce", ops._p(parts.to(d)), S, M * N, N, ops._p(rd), N if r is not None else 0, ops._p(plain), N, M, N)
        torch.cuda.synchronize()
        assert torch.equal(run_reduce(parts, None, 0, r).view(torch.int16), plain.cpu().view(torch.int16))
    # bias, act = 0: bit-exact against the emulation
    y32 = emulate_sum(parts, bias)
    want = y32.to(torch.bfloat16)
    assert torch.equal(run_reduce(parts, bias, 0, None), want)
    want_res = (want.float() + res.float()).to(torch.bfloat16)
    assert torch.equal(run_reduce(parts, bias, 0, res), want_res)
    assert torch.equal(run_reduce(parts, bias, 0, res, alias=True), want_res)          # in place on the residual stream
    # activations: y exact, the activation within the contract's roundings
    y = want.double()
    assert float(y.min()) <= -11.5 and float(y.max()) >= 11.5       # both tails of the activations are hit
    a = 1.702 * y
    s = torch.sigmoid(a)
    quick = y * s
    e_a = nm.rnd(a) + nm.U_F32 * a.abs()
    e_s = 0.25 * e_a + (nm.U_EXP + 2 * nm.U_F32) * s + nm.rnd(s)
    e_quick = y.abs() * e_s + nm.rnd(quick)
    erf = torch.erf(y / math.sqrt(2.0))
    gelu = 0.5 * y * (1 + erf)
    e_gelu = nm.rnd(gelu) + 0.5 * y.abs() * (nm.U_EXP + 6 * nm.U_F32)
    for act, ref, err in ((1, quick, e_quick), (2, gelu, e_gelu)):
        nm.check_elementwise(run_reduce(parts, bias, act, None), ref, err, f"splitk_reduce_bias_act act={act} {M}x{N} S={S}")
        total = ref + res.double()
        nm.check_elementwise(run_reduce(parts, bias, act, res), total, err + nm.rnd(total) + nm.rnd(err),
                             f"splitk_reduce_bias_act act={act} + res {M}x{N} S={S}")


def test_linear_skinny_bias_act_runs_the_streaming_gemm_into_the_finish():
    """clip_ops.linear_skinny_bias_act = vsys_gemm_skinny_slices + the finish: against the fp32 matmul of the bf16 operands, rows past M
    of the padded activations poisoned with NaN (they must not reach a result row)."""
    from videosys_amd import clip_ops

    M, N, K = 77, 160, 256
    g = torch.Generator().manual_seed(9)
    x = torch.full((384, K), float("nan"))
    x[:M] = torch.randn(M, K, generator=g)
    xb, wb = x.to(torch.bfloat16), (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    out = clip_ops.linear_skinny_bias_act(xb.to(dev()), M, wb.to(dev()), bias=bias.to(dev()))
    torch.cuda.synchronize()
    ref, ref_abs = nm.matmul_ref(xb[:M], wb)
    ref = ref + bias.double()
    nm.check_elementwise(out[:M].cpu(), ref, nm.acc(K + 2, ref_abs + bias.double().abs()) + nm.rnd(ref), "linear_skinny_bias_act")
