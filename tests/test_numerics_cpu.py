"""The element-wise bound of tests/numerics.py on synthetic data (no GPU): a correctly rounded result and a result with one
rounding fewer than the contract pass; each of four planted defects fails, and the failure names the tile."""
import pytest
import torch

import numerics as nm

M, N, K = 1024, 384, 1024


def _operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K**0.5).to(torch.bfloat16)
    # a bias of the accumulator's own scale: the epilogue's sum then cancels on many elements, where an extra rounding shows
    b = torch.randn(N, generator=g).to(torch.bfloat16)
    return a, w, b


def _bias_case(seed=0):
    """Contract: out = bf16(a @ w^T + b), fp32 accumulation.  Chain: acc(K) + one rounding of the output."""
    a, w, b = _operands(seed)
    ref, s = nm.matmul_ref(a, w)
    ref = ref + b.double()
    bound = nm.acc(K, s + b.double().abs()) + nm.rnd(ref)
    return a, w, b, ref, bound


def _check(out, ref, bound, what="synthetic"):
    nm.Bound(what).add(out, ref, bound).check()


def test_correctly_rounded_result_passes():
    a, w, b, ref, bound = _bias_case()
    _check(ref.to(torch.bfloat16), ref, bound)
    # the fp32-accumulated form the kernels compute passes too
    _check((a.float() @ w.float().t() + b.float()).to(torch.bfloat16), ref, bound)


def test_element_two_ulps_off_fails():
    a, w, b, ref, bound = _bias_case()
    out = ref.to(torch.bfloat16)
    bits = out.view(torch.int16)
    r, c = 700, 200
    bits[r, c] += 2                      # two ulps away from the correctly rounded value (same sign, same binade or the next)
    with pytest.raises(AssertionError, match=r"1 of .* worst at \(row 700, col 200\) \[256-row tile 2, 128-row tile 5, 192-col tile 1\]"):
        _check(out, ref, bound)


def test_partial_sums_rounded_to_bf16_every_64_terms_fail():
    a, w, b, ref, bound = _bias_case()
    part = torch.zeros(M, N, dtype=torch.bfloat16)
    for k0 in range(0, K, 64):
        part = (part.float() + a[:, k0:k0 + 64].float() @ w[:, k0:k0 + 64].float().t()).to(torch.bfloat16)
    out = (part.float() + b.float()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="outside the bound"):
        _check(out, ref, bound)


def test_extra_rounding_in_the_epilogue_fails():
    """bf16(bf16(acc) + b): the accumulator rounded before the bias is added (the contract adds in fp32, then rounds once)."""
    a, w, b, ref, bound = _bias_case()
    accum = (a.float() @ w.float().t()).to(torch.bfloat16)
    out = (accum.float() + b.float()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="outside the bound"):
        _check(out, ref, bound)


def test_unwritten_256_row_tile_fails_and_is_named():
    a, w, b, ref, bound = _bias_case()
    out = ref.to(torch.bfloat16)
    out[512:768] = 0
    with pytest.raises(AssertionError, match=r"98\d\d\d of .* \[256-row tile 2,"):
        _check(out, ref, bound)


def test_chunked_check_reports_global_rows():
    a, w, b, ref, bound = _bias_case()
    out = ref.to(torch.bfloat16)
    out[900, 17] = float("nan")
    rep = nm.Bound("chunks")
    for r0, r1 in nm.row_chunks(M, 256):
        rep.add(out[r0:r1], ref[r0:r1], bound[r0:r1], row0=r0)
    with pytest.raises(AssertionError, match=r"1 of 393216 .* \(row 900, col 17\)"):
        rep.check()


def test_gate_residual_chain_accepts_one_rounding_fewer():
    """Contract x + g * proj(a) = bf16(x + bf16(g * bf16(a W^T + b))): three roundings.  The bound built from that chain accepts
    the contract itself, the two-rounding form the GEMM epilogue computes (bf16(x + bf16(g (acc + b)))) and a single rounding."""
    a, w, b = _operands(1)
    g = torch.Generator().manual_seed(2)
    b = (b.float() * 0.1).to(torch.bfloat16)
    gate = torch.randn(N, generator=g).to(torch.bfloat16)
    x = torch.randn(M, N, generator=g).to(torch.bfloat16)
    p, s = nm.matmul_ref(a, w)
    p = p + b.double()
    gd, xd = gate.double(), x.double()
    ref = xd + gd * p
    bound = gd.abs() * (nm.acc(K, s + b.double().abs()) + nm.rnd(p)) + nm.rnd(gd * p) + nm.rnd(ref)
    acc32 = a.float() @ w.float().t() + b.float()
    three = (x.float() + (gate.float() * acc32.to(torch.bfloat16).float()).to(torch.bfloat16).float()).to(torch.bfloat16)
    two = (x.float() + (gate.float() * acc32).to(torch.bfloat16).float()).to(torch.bfloat16)
    one = ref.to(torch.bfloat16)
    for out in (three, two, one):
        _check(out, ref, bound, "gate + residual")
    # ... and the gate of the neighbouring sample on one 128-row tile does not pass
    bad = two.clone()
    gate2 = torch.randn(N, generator=g).to(torch.bfloat16)
    bad[256:384] = (x[256:384].float() + (gate2.float() * acc32[256:384]).to(torch.bfloat16).float()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match=r"128-row tile 2,"):
        _check(bad, ref, bound, "gate + residual")
