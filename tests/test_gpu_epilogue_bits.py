"""-m gpu: the gate + residual epilogues of the 16x16x32 GEMM kernels store the SAME BITS as their 32x32x16 forms.

The 16x16x32 epilogues (gemm_bf16.hip, ``MF``) are written for instruction count: descriptor addressing with hardware bounds instead of
per-unit 64-bit arithmetic and row clamps, packed fp32 arithmetic, no multiply for a null gate, one gate row per wave where its 64 rows
lie in one sample.  Every value, rounding point and summation order is that of the 32x32x16 kernels, which are the reference here:
``vsys_tune_gemm_variant`` 8 forces them, 16 the 8-wave 16x16x32 kernel, 113 / 119 its 128-row forms.  Outputs, the PAB slab and the
statistics buffer are compared with torch.equal on the raw bits, and so are the padding columns and the rows behind M of every buffer
(nothing outside the operands may be written).

Shapes are the smallest at which these epilogues can go wrong: M = 1 (a single row), 65 (one row past a 64-row wave), 257 (one row past a
tile), 300 (a ragged second tile); N = 192 / 384 (one / two column tiles); K = 128.  rows_per_sample = 100 puts sample boundaries inside
a wave's 64 rows and inside a 16-row token block (the per-token gate form) and leaves whole waves inside one sample (the one-row form).
The statistics-emitting epilogue and the folded PAB operands take the 128-row kernels at these sizes whatever the id, so their
reference is composed: the stored rows of the plain 32x32x16 epilogue (+ the bf16 additions of the PAB operands, done by torch), and the
row pass (ln_row_stats) over the stored rows, which accumulates the same 48-column halves in the same order.  One shape with >= 400
tiles puts the 8-wave kernels of the denoise step themselves (id 16 against id 8) through both."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K = 128
RPS = 100
PAD_ROWS = 3


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


@pytest.fixture(scope="module")
def lib():
    from videosys_amd import _lib

    return _lib.load()


class Problem:
    """Inputs of one (M, N) on the device; ``rows(ld)`` hands out a fresh [M + PAD_ROWS, ld] copy of the residual image (its first N
    columns of the first M rows are the residual, everything else is a recognisable filler)."""

    def __init__(self, M, N, seed, on_device=False):
        g = torch.Generator(device=dev() if on_device else "cpu").manual_seed(seed)
        kw = dict(generator=g, device=dev() if on_device else "cpu")
        self.M, self.N = M, N
        self.x = torch.randn(M, K, **kw).to(torch.bfloat16).to(dev())
        self.w = (torch.randn(N, K, **kw) / math.sqrt(K)).to(torch.bfloat16).to(dev())
        self.b = (torch.randn(N, **kw) * 0.1).to(torch.bfloat16).to(dev())
        self.nsamp = -(-M // RPS)
        self.mod = torch.randn(self.nsamp, 2 * N, **kw).to(torch.bfloat16).to(dev())   # per sample: gate | alternative gate
        self.res = (torch.randn(M, N, **kw) * 2.0 + 3.0).to(torch.bfloat16).to(dev())
        self.add1 = torch.randn(M, N, **kw).to(torch.bfloat16).to(dev())
        self.add2 = torch.randn(M, N, **kw).to(torch.bfloat16).to(dev())

    def rows(self, ld, src=None):
        buf = torch.full((self.M + PAD_ROWS, ld), -7.25, dtype=torch.bfloat16, device=dev())
        if src is not None:
            buf[:self.M, :self.N] = src
        return buf

    def gate_kw(self, gated):
        return dict(gate=self.mod[0, :self.N], gate_stride=2 * self.N, rows_per_sample=RPS) if gated else {}


def _plain(ops, lib, pr, variant, *, bias, gate, ldr, ldo, aux=False):
    """EPI_GATE_RES under ``variant``; gate: None / "sample" / "segment" (two gate vectors per sample, seg_split = 40).
    ldo == 0: in place.  Returns the whole out buffer (padding included) and the whole aux buffer or None."""
    res = pr.rows(ldr, pr.res)
    out = res if ldo == 0 else pr.rows(ldo)
    auxb = pr.rows(ldr) if aux else None
    rv, ov = res[:pr.M, :pr.N], out[:pr.M, :pr.N]
    av = auxb[:pr.M, :pr.N] if aux else None
    assert lib.vsys_tune_gemm_variant(variant) == 0
    try:
        if gate == "segment":
            ops.gemm_gate2(pr.x, pr.w, bias, pr.mod[0, :pr.N], 2 * pr.N, RPS, 40, pr.N, rv, ov, aux=av)
        else:
            ops.gemm(pr.x, pr.w, bias, epilogue=ops.EPI_GATE_RES, res=rv, aux=av, out=ov, **pr.gate_kw(gate == "sample"))
    finally:
        lib.vsys_tune_gemm_variant(0)
    return out, auxb


@pytest.mark.parametrize("N", [192, 384])
@pytest.mark.parametrize("M", [1, 65, 257, 300])
def test_gate_residual_epilogue_same_bits(ops, lib, M, N):
    pr = Problem(M, N, seed=1000 * N + M)
    for bias in (None, pr.b):
        for gate in (None, "sample", "segment"):
            for ldr, ldo, aux in ((N + 8, 0, False), (N + 8, N + 64, True)):   # strided and in place / two leading dimensions + PAB slab
                want, want_aux = _plain(ops, lib, pr, 8, bias=bias, gate=gate, ldr=ldr, ldo=ldo, aux=aux)
                for variant in (16, 113, 119):
                    got, got_aux = _plain(ops, lib, pr, variant, bias=bias, gate=gate, ldr=ldr, ldo=ldo, aux=aux)
                    what = f"id {variant}, M {M}, N {N}, bias {bias is not None}, gate {gate}, ldr {ldr}, ldo {ldo}"
                    assert torch.equal(got, want), f"{what}: stored bits (or bytes outside the operand) differ from the 32x32x16 kernel"
                    if aux:
                        assert torch.equal(got_aux, want_aux), f"{what}: PAB slab differs"
    # no residual at all: gate (acc + bias) alone
    for variant in (8, 16):
        out = pr.rows(N + 8)
        assert lib.vsys_tune_gemm_variant(variant) == 0
        try:
            ops.gemm(pr.x, pr.w, pr.b, epilogue=ops.EPI_GATE_RES, out=out[:M, :N], **pr.gate_kw(True))
        finally:
            lib.vsys_tune_gemm_variant(0)
        if variant == 8:
            want = out
    assert torch.equal(out, want)


def _row_stats(ops, pr, buf):
    st = ops.ln_stats_buffer(pr.M, pr.N, dev())
    st.fill_(float("nan"))
    return ops.ln_row_stats(buf[:pr.M, :pr.N].contiguous(), st)


@pytest.mark.parametrize("N", [192, 384])
@pytest.mark.parametrize("M", [1, 65, 257, 300])
def test_statistics_epilogue_same_bits(ops, lib, M, N):
    pr = Problem(M, N, seed=2000 * N + M)
    for bias in (None, pr.b):
        for gated in (False, True):
            want, _ = _plain(ops, lib, pr, 8, bias=bias, gate="sample" if gated else None, ldr=N + 8, ldo=0)
            for variant in (16,):   # (at these sizes the dispatch takes the 128-row 16x16x32 kernel whatever the id)
                buf = pr.rows(N + 8, pr.res)
                st = ops.ln_stats_buffer(M + PAD_ROWS, N, dev())
                st.fill_(float("nan"))
                assert lib.vsys_tune_gemm_variant(variant) == 0
                try:
                    ops.gemm_stats(pr.x, pr.w, bias, st, res=buf[:M, :N], out=buf[:M, :N], **pr.gate_kw(gated))
                finally:
                    lib.vsys_tune_gemm_variant(0)
                what = f"id {variant}, M {M}, N {N}, bias {bias is not None}, gate {gated}"
                assert torch.equal(buf, want), f"{what}: the statistics epilogue stores other bits than the plain 32x32x16 epilogue"
                assert torch.equal(st[:, :M], _row_stats(ops, pr, buf)), f"{what}: partials differ from the row pass over the stored rows"
                assert torch.isnan(st[:, M:]).all(), f"{what}: partials written for rows past M"


@pytest.mark.parametrize("N", [192, 384])
@pytest.mark.parametrize("M", [1, 65, 257, 300])
def test_folded_pab_operands_same_bits(ops, lib, M, N):
    """EPI_GATE_RES with the PAB slab, with add1 / add2 and with the statistics beside them: the general store phase keeps its bits."""
    pr = Problem(M, N, seed=3000 * N + M)
    ld = N + 8
    plain, slab = _plain(ops, lib, pr, 8, bias=pr.b, gate="sample", ldr=ld, ldo=0, aux=True)
    a1, a2 = pr.rows(ld, pr.add1), pr.rows(ld, pr.add2)
    for nadds, with_stats, with_aux in ((1, False, True), (2, True, False), (0, True, True), (2, True, True)):
        want = plain.clone()
        for a in (a1, a2)[:nadds]:   # one bf16 rounding per folded addition, in order
            want[:M, :N] = (want[:M, :N].float() + a[:M, :N].float()).to(torch.bfloat16)
        for variant in (16,):   # (the 128-row 16x16x32 kernel at these sizes)
            buf = pr.rows(ld, pr.res)
            auxb = pr.rows(ld) if with_aux else None
            st = None
            if with_stats:
                st = ops.ln_stats_buffer(M, N, dev())
                st.fill_(float("nan"))
            assert lib.vsys_tune_gemm_variant(variant) == 0
            try:
                ops.gemm_gate_res_add(pr.x, pr.w, pr.b, res=buf[:M, :N], aux=auxb[:M, :N] if with_aux else None,
                                      adds=tuple(a[:M, :N] for a in (a1, a2)[:nadds]), stats=st, out=buf[:M, :N], **pr.gate_kw(True))
            finally:
                lib.vsys_tune_gemm_variant(0)
            what = f"id {variant}, M {M}, N {N}, adds {nadds}, stats {with_stats}, aux {with_aux}"
            assert torch.equal(buf, want), f"{what}: stored bits differ"
            if with_aux:
                assert torch.equal(auxb, slab), f"{what}: PAB slab differs"
            if with_stats:
                assert torch.equal(st, _row_stats(ops, pr, buf)), f"{what}: partials differ from the row pass over the stored rows"


def test_eight_wave_kernels_same_bits(ops, lib):
    """>= 400 tiles: the statistics epilogue and the folded PAB operands run on the 8-wave kernels of the denoise step, id 16 (16x16x32)
    against id 8 (32x32x16) directly.  M is one row past a tile; rows_per_sample is a multiple of 64 (one gate row per wave, as on the
    denoise path) in the first pass and 100 (gate rows per token) in the second."""
    M, N = 25857, 1152
    pr = Problem(M, N, seed=7, on_device=True)
    ld = N + 8
    a1 = pr.rows(ld, pr.add1)
    for rps in (12928, 100):
        mod = torch.randn(-(-M // rps), 2 * N, generator=torch.Generator(device=dev()).manual_seed(rps), device=dev()).to(torch.bfloat16)
        kw = dict(gate=mod[0, :N], gate_stride=2 * N, rows_per_sample=rps)
        got = {}
        for variant in (8, 16):
            b_st, b_pab, slab = pr.rows(ld, pr.res), pr.rows(ld, pr.res), pr.rows(ld)
            st, st2 = ops.ln_stats_buffer(M, N, dev()), ops.ln_stats_buffer(M, N, dev())
            st.fill_(float("nan"))
            st2.fill_(float("nan"))
            assert lib.vsys_tune_gemm_variant(variant) == 0
            try:
                ops.gemm_stats(pr.x, pr.w, pr.b, st, res=b_st[:M, :N], out=b_st[:M, :N], **kw)
                ops.gemm_gate_res_add(pr.x, pr.w, pr.b, res=b_pab[:M, :N], aux=slab[:M, :N], adds=(a1[:M, :N],), stats=st2,
                                      out=b_pab[:M, :N], **kw)
            finally:
                lib.vsys_tune_gemm_variant(0)
            got[variant] = (b_st, st, b_pab, slab, st2)
        for name, a, b in zip(("stored rows", "partials", "stored rows (PAB)", "PAB slab", "partials (PAB)"), got[8], got[16]):
            assert torch.equal(a, b), f"rows_per_sample {rps}: {name} of the 16x16x32 kernel differ from the 32x32x16 kernel"

