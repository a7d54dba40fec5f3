"""-m gpu: parity of the HIP path (called through the C ABI via videosys_amd.ops) against the CPU oracle, the
reference-minted golden fixtures, and size-independent properties at BASELINE config-2 sizes.

Tolerances (stated here, SURVEY.md §8c — the reference's own tests pin nothing):
  * bf16 kernel vs fp32 oracle on the same bf16-rounded inputs: max|err| <= 2^-7 * max|ref| per op;
  * whole small model (2 block pairs) vs reference fp32 output: max|err| <= 3e-2 * max|ref| and cosine >= 0.999;
  * integer / layout work (copies, permutation GEMM): bit exact.
"""
import math

import pytest
import torch

from conftest import load_golden
from oracle import stdit3_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2.0**-7


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def bf(t):
    return t.to(torch.bfloat16).to(dev())


def rel_err(out, ref):
    out = out.float().cpu()
    ref = ref.float().cpu()
    return ((out - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def check(out, ref, tol=TOL, what=""):
    e = rel_err(out, ref)
    assert e <= tol, f"{what}: max|err|/max|ref| = {e:.3e} > {tol:.3e}"


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("variant", [0, 8, 16, 20, 24])
@pytest.mark.parametrize("M,N,K", [(300, 192, 64), (1000, 576, 576), (257, 384, 128), (2048, 1152, 1152)])
def test_gemm_bias(ops, M, N, K, variant):
    from videosys_amd import _lib

    assert _lib.load().vsys_tune_gemm_variant(variant) == 0, f"variant {variant} rejected: the default would be tested instead"
    try:
        _gemm_bias(ops, M, N, K)
    finally:
        _lib.load().vsys_tune_gemm_variant(0)


def _gemm_bias(ops, M, N, K):
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
    ref = x.float() @ w.float().t() + b.float()
    out = ops.gemm(x.to(dev()), w.to(dev()), b.to(dev()))
    check(out, ref, what=f"gemm {M}x{N}x{K}")
    out = ops.gemm(x.to(dev()), w.to(dev()), b.to(dev()), epilogue=ops.EPI_BIAS_GELU)
    check(out, O.gelu_tanh(ref), what="gemm+gelu")


@pytest.mark.parametrize("variant", [3, 6, 8, 9, 16, 20, 24, 28, 30, 34, 103, 106, 113, 118, 119])
def test_gemm_pipeline_variants(ops, variant):
    """Every main-loop schedule of the GEMM (LDS-DMA burst / interleaved, 2-stage / 3+2-slot, 8-wave / 4-wave geometry)
    must give the same result;
    K = 64 (one tile), 128 (two), 1152 (18) and an M tail exercise prologue / steady state / epilogue of each."""
    from videosys_amd import _lib

    lib = _lib.load()
    g = torch.Generator().manual_seed(40 + variant)
    try:
        assert lib.vsys_tune_gemm_variant(variant) == 0, f"variant {variant} rejected: the default would be tested instead"
        for M, N, K in ((515, 192, 64), (300, 384, 128), (1000, 576, 1152), (777, 576, 192), (600, 1152, 320)):
            x = torch.randn(M, K, generator=g).to(torch.bfloat16)
            w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
            b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
            ref = x.float() @ w.float().t() + b.float()
            out = ops.gemm(x.to(dev()), w.to(dev()), b.to(dev()))
            check(out, ref, what=f"variant {variant} gemm {M}x{N}x{K}")
        K = 576
        x = torch.randn(700, K, generator=g).to(torch.bfloat16)
        perm = torch.randperm(K, generator=g)
        w = torch.zeros(K, K)
        w[torch.arange(K), perm] = 1.0
        out = ops.gemm(x.to(dev()), w.to(torch.bfloat16).to(dev()), None).cpu()
        assert torch.equal(out, x[:, perm]), f"variant {variant}: permutation GEMM not bit exact"
    finally:
        lib.vsys_tune_gemm_variant(0)


def test_gemm_is_transpose_exact(ops):
    """Permutation weight: out must be a bit-exact column permutation of x (catches any fragment/epilogue
    row<->col swap; asymmetric by construction)."""
    M, K = 777, 576
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    perm = torch.randperm(K, generator=g)
    w = torch.zeros(K, K)
    w[torch.arange(K), perm] = 1.0
    out = ops.gemm(x.to(dev()), w.to(torch.bfloat16).to(dev()), None).cpu()
    assert torch.equal(out, x[:, perm])


@pytest.mark.parametrize("variant", [0, 8, 16, 20, 24, 103, 113, 118, 119])
def test_gemm_gate_residual_aux(ops, variant):
    """variant 0 = the shape dispatch (small problems take the 128-row geometry); 8 / 20 / 103 force each kernel family
    through the gate + residual + aux epilogue."""
    from videosys_amd import _lib

    assert _lib.load().vsys_tune_gemm_variant(variant) == 0, f"variant {variant} rejected: the default would be tested instead"
    try:
        _gate_residual_aux(ops)
        _gate_residual_aux(ops, M=1100, rps=448)   # sample length a multiple of 64 rows, as on the denoise path
        _gate_residual_aux(ops, M=2048, rps=1024, N=1152)
    finally:
        _lib.load().vsys_tune_gemm_variant(0)


def _gate_residual_aux(ops, M=1100, N=576, K=1152, rps=400):
    # default: 3 samples, tiles straddle sample boundaries
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16)
    nb = -(-M // rps)
    mod = torch.randn(nb, 6 * N, generator=g).to(torch.bfloat16)
    gate = mod[:, 2 * N:3 * N]
    u = (x.float() @ w.float().t() + b.float()) * gate.float().repeat_interleave(rps, 0)[:M]
    modd = mod.to(dev())
    xr = res.to(dev()).clone()
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    out = ops.gemm(x.to(dev()), w.to(dev()), b.to(dev()), epilogue=ops.EPI_GATE_RES, gate=modd[0, 2 * N:3 * N],
                   gate_stride=6 * N, rows_per_sample=rps, res=xr, aux=aux, out=xr)  # in place, like the model
    check(aux, u, what="aux (PAB slab)")
    check(out, res.float() + u, what="gate+residual")
    # gate = None (cross-attention projection)
    xr2 = res.to(dev()).clone()
    out2 = ops.gemm(x.to(dev()), w.to(dev()), b.to(dev()), epilogue=ops.EPI_GATE_RES, res=xr2, out=xr2)
    check(out2, res.float() + x.float() @ w.float().t() + b.float(), what="residual only")


@pytest.mark.parametrize("K", [1152, 4608])
def test_gemm_split_k_few_tiles(ops, K):
    """One rank of an 8-way DSP group: 4864 rows x 1152 columns = 228 tiles of 128 rows on 256 CUs.  Id 123 runs TWO workgroups per tile, each over
    half of K, the first handing its fp32 sums to the second through L2 (gemm_bf16.hip KS; measured slower than one workgroup per tile, so
    opt-in).  Against the one-workgroup kernel (id 113): every epilogue within one bf16 neighbour on a small fraction of the elements (the summation order of
    two fp32 partials), deterministic from launch to launch, flags lowered again (a second and third launch see the same result), and
    the same under a recorded launch program replayed twice (identical arguments every replay)."""
    from videosys_amd import _lib, program

    lib = _lib.load()
    M, N = 4864, 1152
    g = torch.Generator().manual_seed(K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev())
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(dev())
    b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).to(dev())
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev())
    gate = (torch.randn(2, 6 * N, generator=g) * 0.3).to(torch.bfloat16).to(dev())

    def run_all():
        outs = [ops.gemm(x, w, b), ops.gemm(x, w, b, epilogue=ops.EPI_BIAS_GELU)]
        r = res.clone()
        ops.gemm(x, w, b, epilogue=ops.EPI_GATE_RES, gate=gate[0, 2 * N:3 * N], gate_stride=6 * N, rows_per_sample=M // 2, res=r, out=r)
        outs.append(r)
        r2, st = res.clone(), ops.ln_stats_buffer(M, N, dev())
        ops.gemm_stats(x, w, b, st, res=r2, out=r2)
        outs += [r2, st]
        return outs

    try:
        assert lib.vsys_tune_gemm_variant(113) == 0
        ref = run_all()
        assert lib.vsys_tune_gemm_variant(123) == 0
        got = run_all()
        again = run_all()
    finally:
        lib.vsys_tune_gemm_variant(0)
    for a, c, r in zip(got, again, ref):
        assert torch.equal(a, c), "split K is not deterministic / a flag stayed up"
        if a.dtype == torch.bfloat16:
            d = (a.float() - r.float()).abs()
            assert float((d > 0).float().mean()) < 5e-3 and float(d.max()) <= 2.0 ** -6 * float(r.float().abs().max())
    want = ops.ln_stats_buffer(M, N, dev())
    ops.ln_row_stats(got[3], want)
    assert torch.equal(got[4], want), "the partials of the split-K statistics epilogue are not the statistics of what it stored"
    # recorded + replayed twice: the same commands, the flags must have been lowered by the consuming workgroups every time
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    try:
        assert lib.vsys_tune_gemm_variant(123) == 0
        with program.Recorder() as rec:
            ops.gemm(x, w, b, out=out)
        prog = rec.finish()
        first = out.clone()
        for _ in range(2):
            out.zero_()
            prog.run()
            assert torch.equal(out, first)
    finally:
        lib.vsys_tune_gemm_variant(0)
    assert torch.equal(first, got[0])


def test_gemm_rejects_bad_shapes(ops):
    from videosys_amd._lib import VsysError

    x = torch.zeros(64, 100, dtype=torch.bfloat16, device=dev())
    w = torch.zeros(192, 100, dtype=torch.bfloat16, device=dev())
    with pytest.raises(VsysError):
        ops.gemm(x, w, None)
    with pytest.raises(VsysError):
        ops.gemm(torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(192, 64, dtype=torch.bfloat16), None)  # CPU tensors


def test_gemm_config2_shapes_linearity(ops):
    """Full BASELINE config-2 token count (N = 38912) for the four weight shapes: checked against torch fp32 on
    sampled rows, then on EVERY row against float64 (tests/numerics.py: acc(K) + one rounding of the output), and through
    linearity gemm(x1 + x2) ~= gemm(x1) + gemm(x2) with bias = 0, where x1 / x2 split the entries of x (x1 + x2 = x exactly):
    |gemm(x) - (gemm(x1) + gemm(x2))| <= bound(x) + 2^-8 (1 + 2^-7) (|gemm(x1)| + |gemm(x2)|) + acc(K) of x1 and x2."""
    import numerics as nm

    M = 38912
    g = torch.Generator().manual_seed(1)
    for N, K in ((3456, 1152), (1152, 1152), (4608, 1152), (1152, 4608)):
        x = (torch.randn(M, K, generator=g)).to(torch.bfloat16).to(dev())
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(dev())
        out = ops.gemm(x, w, None)
        rows = torch.randint(0, M, (64,), generator=g).to(dev())
        ref = x[rows].float() @ w.float().t()
        check(out[rows], ref, what=f"c2 gemm {N}x{K} sampled rows")
        assert torch.isfinite(out.float()).all()
        # last / first tile rows exact position check
        ref_edge = x[-3:].float() @ w.float().t()
        check(out[-3:], ref_edge, what="tail rows")
        half = torch.rand(M, K, generator=g).to(dev()) < 0.5
        x1 = torch.where(half, x, torch.zeros_like(x))
        x2 = x - x1
        o1, o2 = ops.gemm(x1, w, None), ops.gemm(x2, w, None)
        every, lin = nm.Bound(f"c2 gemm {N}x{K} every row"), nm.Bound(f"c2 gemm {N}x{K} linearity")
        for r0, r1 in nm.row_chunks(M, 4096):
            ref, s = nm.matmul_ref(x[r0:r1], w)
            bound = nm.acc(K, s) + nm.rnd(ref)
            every.add(out[r0:r1], ref, bound, r0)
            parts = o1[r0:r1].double() + o2[r0:r1].double()
            lin.add(out[r0:r1].double() - parts, torch.zeros_like(ref),
                    2 * nm.acc(K, s) + nm.rnd(ref) + nm.U_BF16 * (1 + 2.0**-7) * (o1[r0:r1].double().abs() + o2[r0:r1].double().abs()), r0)
        every.check()
        lin.check()


def test_linear_small(ops):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 264, generator=g).to(torch.bfloat16)
    w = (torch.randn(37, 264, generator=g) / 16).to(torch.bfloat16)
    b = torch.randn(37, generator=g).to(torch.bfloat16)
    ref = x.float() @ w.float().t() + b.float()
    check(ops.linear_small(bf(x), bf(w), bf(b)), ref, what="linear_small")
    check(ops.linear_small(bf(x), bf(w), bf(b), act_out=ops.ACT_SILU), torch.nn.functional.silu(ref), what="silu out")
    xs = torch.nn.functional.silu(x.float()).to(torch.bfloat16).float()
    check(ops.linear_small(bf(x), bf(w), bf(b), act_in=ops.ACT_SILU), xs @ w.float().t() + b.float(), what="silu in")
    check(ops.linear_small(bf(x), bf(w), bf(b), act_out=ops.ACT_GELU_TANH), O.gelu_tanh(ref), what="gelu out")


# ------------------------------------------------------------------------------------------------ row-wise
def test_adaln_golden(ops, golden_ops):
    f = golden_ops["adaln"]
    B, n, C = f["x"].shape
    mod = torch.zeros(B, 6 * C)
    mod[:, :C] = f["shift"][:, 0]
    mod[:, C:2 * C] = f["scale"][:, 0]
    modd = bf(mod)
    out = ops.adaln_modulate(bf(f["x"]).view(B * n, C), modd[0, :C], modd[0, C:2 * C], n, 6 * C)
    check(out.view(B, n, C), f["out"], what="adaln vs reference")


def test_adaln_config2_property(ops):
    """Full-size rows (38912 x 1152): with scale = 0, shift = 0 every output row has mean ~0 and variance ~1."""
    N, C = 38912, 1152
    x = (torch.randn(N, C, device=dev()) * 3 + 1).to(torch.bfloat16)
    z = torch.zeros(2, 6 * C, dtype=torch.bfloat16, device=dev())
    out = ops.adaln_modulate(x, z[0, :C], z[0, C:2 * C], N // 2, 6 * C).float()
    assert out.mean(-1).abs().max().item() < 2e-2
    assert (out.var(-1, unbiased=False) - 1).abs().max().item() < 3e-2


def test_adaln_width_1152_vs_torch(ops):
    """C = 1152 takes the two-rows-per-wave kernel: an odd row count (the last wave has one row), two samples with different
    modulation vectors, against LayerNorm + modulate in fp32."""
    C, rps = 1152, 334
    rows = 2 * rps - 1
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.3).to(torch.bfloat16)
    mod = (torch.randn(2, 6 * C, generator=g) * 0.3).to(torch.bfloat16)
    out = ops.adaln_modulate(bf(x), bf(mod)[0, :C], bf(mod)[0, C:2 * C], rps, 6 * C)
    xf = x.float()
    ln = torch.nn.functional.layer_norm(xf, (C,), eps=1e-6)
    sample = (torch.arange(rows) // rps)
    ref = ln * (1 + mod[sample, C:2 * C].float()) + mod[sample, :C].float()
    check(out, ref, what="adaln 1152")


def test_mod_table_and_embeddings(ops, golden_ops):
    g = torch.Generator().manual_seed(4)
    table = torch.randn(6, 6 * 64, generator=g).to(torch.bfloat16)
    tm = torch.randn(2, 6 * 64, generator=g).to(torch.bfloat16)
    out = ops.mod_table(bf(table), bf(tm)).cpu()
    ref = (table[:, None, :] + tm[None]).to(torch.bfloat16)  # bf16 add, as the reference's tensors
    assert torch.equal(out, ref)
    f = golden_ops["embed"]
    te = ops.timestep_embedding(f["t"].to(dev()), 256)
    check(te, f["t_freq"], tol=2.0**-8, what="timestep embedding")


def test_patch_embed_and_final(ops, golden_ops):
    g = torch.Generator().manual_seed(6)
    C, Cin = 576, 4
    z = torch.randn(1, Cin, 3, 9, 7, generator=g)  # odd H/W: exercises the zero pad + CFG duplicate (B=2 from Bz=1)
    w = (torch.randn(C, Cin, 1, 2, 2, generator=g) * 0.1).to(torch.bfloat16)
    b = (torch.randn(C, generator=g) * 0.02).to(torch.bfloat16)
    pos = O.pos_embed_2d(C, 5, 4, 0.25, 4)[0].to(torch.bfloat16)
    sd = {"x_embedder.proj.weight": w.float(), "x_embedder.proj.bias": b.float()}
    zz = z.to(torch.bfloat16).float()
    ref = O.patch_embed(torch.cat([zz, zz]), sd).view(2, 3, 20, C) + pos.float()
    out = ops.patch_embed(z.to(dev()), bf(w.reshape(C, -1)), bf(b), bf(pos), 2, (1, 2, 2), C)
    check(out, ref, what="patch embed")

    f = golden_ops["final"]
    B, n, C = f["x"].shape
    T, Hp, Wp = 3, 4, 4
    out = ops.final_layer(bf(f["x"]).view(B * n, C), bf(f["table"]), bf(f["t"]), bf(f["w"]), bf(f["b"]), B, T, Hp, Wp, 8, 8,
                          (1, 2, 2), 8)
    ref = O.unpatchify(f["out"], T, Hp, Wp, T, 8, 8, (1, 2, 2), 8)
    check(out, ref, what="final layer + unpatchify vs reference")
    # cropped variant (odd latent size)
    out2 = ops.final_layer(bf(f["x"]).view(B * n, C), bf(f["table"]), bf(f["t"]), bf(f["w"]), bf(f["b"]), B, T, Hp, Wp, 7, 5,
                           (1, 2, 2), 8)
    check(out2, ref[:, :, :, :7, :5], what="final layer cropped")


def test_patch_embed_and_final_on_sequence_shards(ops, golden_ops):
    """The S-shard forms used by a sequence-parallel rank (vsys_patch_embed_shard, vsys_final_layer_tokens +
    vsys_unpatchify_tokens) must reproduce the whole-frame entry points bit for bit: every rank's rows of the embedding (zero rows
    past the frame's last token), and the pixels scattered from the gathered per-token outputs — for a shard size that does not
    divide the token count (S = 20 over P = 3: 7 + 7 + 6, one padding row) and one that does."""
    g = torch.Generator().manual_seed(6)
    C, Cin = 576, 4
    z = torch.randn(1, Cin, 3, 9, 7, generator=g).to(dev())     # Hp x Wp = 5 x 4 = 20 tokens per frame, odd H / W
    w = bf((torch.randn(C, Cin, 1, 2, 2, generator=g) * 0.1).to(torch.bfloat16).reshape(C, -1))
    b = bf((torch.randn(C, generator=g) * 0.02).to(torch.bfloat16))
    pos = bf(O.pos_embed_2d(C, 5, 4, 0.25, 4)[0].to(torch.bfloat16))
    full = ops.patch_embed(z, w, b, pos, 2, (1, 2, 2), C)          # [2, 3, 20, C]
    for P in (3, 4):
        Sl = -(-20 // P)
        for r in range(P):
            part = ops.patch_embed_shard(z, w, b, pos, 2, (1, 2, 2), C, r * Sl, Sl)
            valid = max(0, min(Sl, 20 - r * Sl))
            assert torch.equal(part[:, :, :valid], full[:, :, r * Sl:r * Sl + valid]), f"P={P} rank {r}"
            assert not part[:, :, valid:].any(), "rows past the last token must be zero"

    f = golden_ops["final"]
    B, n, C = f["x"].shape
    T, Hp, Wp = 3, 4, 4
    x = bf(f["x"]).view(B, T, Hp * Wp, C)
    args = (bf(f["table"]), bf(f["t"]), bf(f["w"]), bf(f["b"]))
    for (H, W) in ((8, 8), (7, 5)):
        whole = ops.final_layer(x.reshape(B * n, C), *args, B, T, Hp, Wp, H, W, (1, 2, 2), 8)
        for P in (3, 4):
            Sl = -(-(Hp * Wp) // P)
            toks = []
            for r in range(P):
                xs = torch.zeros(B, T, Sl, C, dtype=torch.bfloat16, device=dev())
                valid = max(0, min(Sl, Hp * Wp - r * Sl))
                xs[:, :, :valid] = x[:, :, r * Sl:r * Sl + valid]
                toks.append(ops.final_layer_tokens(xs.view(B * T * Sl, C), *args, B, T, Sl))
            out = ops.unpatchify_tokens(torch.stack(toks).contiguous(), P, B, T, Sl, Hp, Wp, H, W, (1, 2, 2), 8)
            assert torch.equal(out, whole), f"P={P} {H}x{W}: sharded final layer differs from the whole-frame one"


def test_cfg_euler_and_add(ops):
    g = torch.Generator().manual_seed(8)
    z = torch.randn(1, 4, 3, 8, 8, generator=g)
    mo = torch.randn(2, 8, 3, 8, 8, generator=g)
    ref = z + (mo[1:, :4] + 7.0 * (mo[:1, :4] - mo[1:, :4])) * 0.0625
    out = ops.cfg_euler_step(z.to(dev()).clone(), mo.to(dev()), 7.0, 0.0625)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-6, atol=1e-6)
    a = torch.randn(1000, 64, generator=g).to(torch.bfloat16)
    b = torch.randn(1000, 64, generator=g).to(torch.bfloat16)
    out = ops.add_rows(bf(a).clone(), bf(b)).cpu()
    assert torch.equal(out, (a.float() + b.float()).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ attention
def _run_flash(ops, q2d, k2d, v2d, qw, kw_, batch, heads, q_len, kv_len, k_norm_bound=None, keys_exact=False):
    kp, vt = ops.alloc_kv_buffers(batch, heads, kv_len, dev())
    ops.attn_prep_kv(k2d, v2d, kw_, kp, vt, batch, heads, kv_len)
    out = torch.full((batch * q_len, heads * 72), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.flash_attn(q2d, qw, kp, vt, out, batch, heads, q_len, kv_len, k_norm_bound=k_norm_bound, keys_exact=keys_exact)
    return out


def test_attn_spatial_golden(ops, golden_ops):
    f = golden_ops["attn_spatial"]
    Bp, N, C = f["x"].shape
    H = f["heads"]
    qkv = bf(f["qkv"]).view(Bp * N, 3 * C)
    out = _run_flash(ops, qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], bf(f["q_norm"]), bf(f["k_norm"]), Bp, H, N, N)
    check(out.view(Bp, N, C), f["attn_out"], what="spatial attention vs reference (pre-proj)")


def test_attn_cross_golden(ops, golden_ops):
    f = golden_ops["attn_cross"]
    B, N, C = f["x"].shape
    H, L = f["heads"], f["y_lens"][0]
    q = bf(f["q"]).view(B * N, C)
    kv = bf(f["kv"]).view(B * L, 2 * C)
    out = _run_flash(ops, q, kv[:, :C], kv[:, C:], None, None, B, H, N, L)
    check(out.view(B, N, C), f["attn_out"], what="cross attention vs reference (pre-proj)")


@pytest.mark.parametrize("name", ["attn_temporal", "attn_temporal38"])
def test_attn_temporal_golden(ops, golden_ops, name):
    f = golden_ops[name]
    Bp, T, C = f["x"].shape  # (B S) T C
    H = f["heads"]
    # lay the sequences out as the model does: rows ordered (b, t, s) with B=1, S=Bp
    qkv = f["qkv"].view(Bp, T, 3 * C).permute(1, 0, 2).reshape(T * Bp, 3 * C)
    cos, sin = O.rope_table(f["rope_freqs"], T)
    out = torch.empty(T * Bp, C, dtype=torch.bfloat16, device=dev())
    ops.attn_temporal(bf(qkv), C, bf(f["q_norm"]), bf(f["k_norm"]), cos.float().contiguous().to(dev()),
                      sin.float().contiguous().to(dev()), out, 1, T, Bp, H)
    ref = f["attn_out"].view(Bp, T, C).permute(1, 0, 2).reshape(T * Bp, C)
    check(out, ref, what=f"{name} vs reference (pre-proj)")


@pytest.mark.parametrize("B,T,S,H,norm,rope", [(2, 19, 64, 16, True, True), (1, 5, 33, 3, True, False), (1, 32, 16, 4, False, True),
                                                 (1, 1, 8, 2, True, True), (1, 16, 40, 16, False, False), (2, 38, 16, 5, True, True),
                                                 (1, 33, 9, 16, True, True), (1, 64, 12, 4, False, True), (2, 40, 300, 16, True, False),
                                                 (1, 2, 70, 8, True, True), (2, 19, 128, 16, True, True), (1, 11, 300, 12, False, True),
                                                 (1, 32, 600, 16, True, True), (2, 10, 37, 4, False, False)])
def test_attn_temporal_kernels_agree_with_oracle(ops, B, T, S, H, norm, rope):
    """The temporal kernels — matrix-pipe (default; attention_t3.hip: one 32-frame tile for T <= 32, two key / query blocks for
    T <= 64), VALU two-pass (flash variant 4, T <= 40) and online-softmax (variant 9) — against the fp32 oracle and each other: with /
    without qk-norm and RoPE (Latte runs without either), head counts that leave waves idle, T = 1 (output = v), T = 33 (one frame in
    the second block), T = 38 (720p x 128f), T = 40 on a grid large enough to run one workgroup per token, T = 64 (both blocks full)."""
    from videosys_amd import _lib

    lib = _lib.load()
    C = H * 72
    g = torch.Generator().manual_seed(33 + T)
    qkv = torch.randn(B * T * S, 3 * C, generator=g).to(torch.bfloat16)
    qw = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16) if norm else None
    kw_ = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16) if norm else None
    freqs = 1.0 / (10000 ** (torch.arange(0, 72, 2).float() / 72))
    cos = sin = None
    if rope:
        cos, sin = (t.float().contiguous().to(dev()) for t in O.rope_table(freqs, T))
    # oracle: q, k, v [B*S, H, T, 72] from the (b, t, s)-ordered rows
    x = qkv.float().view(B, T, S, 3, H, 72).permute(3, 0, 2, 4, 1, 5).reshape(3, B * S, H, T, 72)
    q, k, v = x[0].to(torch.bfloat16), x[1].to(torch.bfloat16), x[2]
    if norm:
        q, k = O.rms_norm(q, qw.float()), O.rms_norm(k, kw_.float())
    q, k = q.float(), k.float()
    if rope:
        q, k = O.rope_rotate(q, freqs), O.rope_rotate(k, freqs)
    ref = (O.sdpa(q, k, v) if T > 1 else v).view(B, S, H, T, 72).permute(0, 3, 1, 2, 4).reshape(B * T * S, C)
    outs = {}
    # (0 = the default: one rounding per q / k element in front of the matrix product; 21 = the same kernels with every rounding point
    #  of the reference's bf16 run; 4 / 9 = the VALU two-pass and online-softmax kernels)
    # (22 = the per-lane-load kernel where 0 runs the round-6 cooperative LDS-DMA form — heads in groups of four, T <= 32: same
    #  fragments, same matrix products, so the SAME BITS are required below)
    for fv in (0, 22, 21, 4, 9) if T <= 40 else (0, 22, 21, 9):
        assert lib.vsys_tune_flash_variant(fv) == 0
        try:
            out = torch.full((B * T * S, C), 7.0, dtype=torch.bfloat16, device=dev())
            ops.attn_temporal(bf(qkv), C, None if qw is None else qw.to(dev()), None if kw_ is None else kw_.to(dev()), cos, sin,
                              out, B, T, S, H)
            outs[fv] = out.float().cpu()
        finally:
            lib.vsys_tune_flash_variant(0)
        check(outs[fv], ref, what=f"temporal kernel variant {fv} vs oracle")
    scale = ref.abs().max().item()
    assert (outs[0] - outs[9]).abs().max().item() <= 2.0 ** -6 * scale
    assert (outs[0] - outs[21]).abs().max().item() <= 2.0 ** -6 * scale
    assert torch.equal(outs[0], outs[22]), "the LDS-DMA form of the temporal kernel must reproduce the per-lane-load kernel bit for bit"
    # (the oracle above carries the reference's own cast-before-weight rounding, so the stage-by-stage form may sit a little closer
    #  to it than the single-rounding default: both are held to the same tolerance, neither to the other's bits)


@pytest.mark.parametrize("q_len,kv_len,heads,batch,norm", [
    (1024, 1024, 4, 3, True),    # spatial shape: 16 KV tiles, 4 query blocks of 256
    (700, 300, 2, 2, False),     # cross shape: ragged last tile (300 = 4 x 64 + 44), ragged query block
    (100, 64, 2, 1, True),       # one tile, fewer rows than one wave group
    (256, 129, 1, 2, True),      # 3 tiles, the last with one key
    (333, 448, 3, 1, False),     # 7 tiles: ring of five stages wraps
    (257, 192, 2, 2, True),      # 3 tiles = exactly the prologue depth; second query block has one row
    (2000, 300, 16, 2, False),   # resident kernel: chunks = 8 workgroups per (batch, head) walk 8 query blocks unevenly, ragged tail
    (1500, 320, 40, 7, True),    # more (batch, head) pairs than CUs: one chunk each, 6 query blocks, five full tiles
])
def test_flash_resident_matches_streaming_and_torch(ops, q_len, kv_len, heads, batch, norm):
    """flash variant 8 (resident K/V: every KV tile staged once per workgroup, query blocks walked without DMA or barriers) does the
    arithmetic of the streaming kernel (variant 10) in the same order per query row: results must be BIT-identical to it, for every
    prologue / ragged-tail / chunking case; and against torch fp32 SDPA."""
    from videosys_amd import _lib

    lib = _lib.load()
    C = heads * 72
    g = torch.Generator().manual_seed(q_len + kv_len)
    q = torch.randn(batch * q_len, C, generator=g).to(torch.bfloat16).to(dev())
    k = torch.randn(batch * kv_len, C, generator=g).to(torch.bfloat16).to(dev())
    v = torch.randn(batch * kv_len, C, generator=g).to(torch.bfloat16).to(dev())
    qw = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev()) if norm else None
    kw_ = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev()) if norm else None
    try:
        assert lib.vsys_tune_flash_variant(10) == 0          # the streaming kernel (two-stage ring, one barrier per tile)
        base = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        assert lib.vsys_tune_flash_variant(8) == 0           # resident K/V (kv_len <= 320; otherwise the streaming kernel again)
        res = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        assert lib.vsys_tune_flash_variant(23) == 0          # three workgroups per CU with the LDS-DMA pieces IN FRONT of the tile (the A/B
        front = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)   # partner of the shipped placement behind the first QK MFMAs)
        torch.cuda.synchronize()
    finally:
        lib.vsys_tune_flash_variant(0)
    assert torch.equal(res, base), f"resident-K/V flash differs from the streaming kernel: max {float((res.float() - base.float()).abs().max()):.3e}"
    assert torch.equal(front, base), "the placement of the LDS-DMA pieces inside the tile must not change a bit"
    for bi in range(batch):
        for h in range(heads):
            qq = q[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72]
            kk = k[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72]
            vv = v[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72].float()
            if norm:
                qq, kk = O.rms_norm(qq, qw.float()), O.rms_norm(kk, kw_.float())
            ref = O.sdpa(qq.float()[None], kk.float()[None], vv[None])[0]
            # P and the output are bf16: 2^-6 of max|ref| over up to 280 (batch, head) slices (the two kernels agree bit for bit)
            check(res[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72], ref, tol=2.0 ** -6, what=f"flash b{bi} h{h}")


@pytest.mark.parametrize("q_len,kv_len,heads,batch,qscale,mode", [
    (19456, 300, 16, 2, 1.0, "typical"),    # the cross attention of config 2 (text K / V prepared for exactly 300 keys)
    (2000, 300, 16, 2, 0.3, "typical"),     # small logits: the padding keys' logit 0 is inside the real range
    (1500, 120, 40, 7, 1.0, "typical"),     # two tiles, 56 padding keys in the second
    (1024, 44, 16, 2, 1.0, "typical"),      # ONE tile: the padding keys take part in the first tile's max adoption
    (1500, 320, 16, 2, 1.0, "typical"),     # whole tiles: the promise changes nothing
    (2000, 300, 16, 2, 1.0, "all_far_negative"),   # every real logit ~ -300 (exp2 domain): the guard recomputes with the mask
])
def test_flash_keys_exact_promise(ops, q_len, kv_len, heads, batch, qscale, mode):
    """vsys_flash_attn_d72_exact (K / Vt prepared for exactly kv_len on zeroed buffers: no mask on the ragged last tile of the
    resident-K/V kernel) against the masked kernel and torch fp32.  Whole tiles: same bits.  Ragged: the same tolerance against
    fp32, and the same bits wherever no padding key raises a tile's max past the rescale threshold (typical logits); rows whose real
    logits all lie far below the padding keys' 0 are recomputed with the mask (same bits as the masked kernel)."""
    C = heads * 72
    g = torch.Generator().manual_seed(q_len + kv_len)
    q = (torch.randn(batch * q_len, C, generator=g) * qscale).to(torch.bfloat16)
    k = (torch.randn(batch * kv_len, C, generator=g) * qscale).to(torch.bfloat16)
    if mode == "all_far_negative":     # q = u + noise, k = -u + noise with |u|^2 / sqrt(72) * log2(e) ~ 300
        u = torch.randn(1, 72, generator=g)
        u = u / u.norm() * (300.0 * 72 ** 0.5 / 1.4427) ** 0.5
        q = (u.repeat(1, heads) + 0.1 * torch.randn(batch * q_len, C, generator=g)).to(torch.bfloat16)
        k = (-u.repeat(1, heads) + 0.1 * torch.randn(batch * kv_len, C, generator=g)).to(torch.bfloat16)
    v = torch.randn(batch * kv_len, C, generator=g).to(torch.bfloat16)
    q, k, v = q.to(dev()), k.to(dev()), v.to(dev())
    base = _run_flash(ops, q, k, v, None, None, batch, heads, q_len, kv_len)
    res = _run_flash(ops, q, k, v, None, None, batch, heads, q_len, kv_len, keys_exact=True)
    torch.cuda.synchronize()
    assert torch.isfinite(res.float()).all()
    if kv_len % 64 == 0 or mode == "all_far_negative":
        assert torch.equal(res, base), float((res.float() - base.float()).abs().max())
    else:
        differing = (res != base).float().mean().item()
        assert differing <= (0.25 if kv_len < 64 or qscale < 1.0 else 1e-3), differing    # (a different rounding scale of P where a padding key raised a max)
    if mode == "all_far_negative":
        return      # (logits of -300: the single bf16 rounding of the scaled K already moves P by tens of percent — both kernels alike;
                    # what this case pins is the guard: the masked kernel's bits)
    for bi in range(0, batch, max(1, batch - 1)):
        for h in range(0, heads, max(1, heads - 1)):
            sl = slice(bi * q_len, bi * q_len + min(q_len, 2048))
            qq = q[sl, h * 72:(h + 1) * 72].float()
            kk = k[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72].float()
            vv = v[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72].float()
            ref = O.sdpa(qq[None], kk[None], vv[None])[0]
            check(res[sl, h * 72:(h + 1) * 72], ref, tol=2.0 ** -6, what=f"exact-keys flash b{bi} h{h}")


@pytest.mark.parametrize("q_len,kv_len,heads,batch,norm,qscale", [
    (1024, 1024, 4, 3, True, 1.0),     # the spatial shape of config 2: 16 KV tiles, 4 workgroups of 256 rows per (frame, head)
    (700, 300, 2, 2, False, 1.0),      # ragged last tile (300 keys), ragged last workgroup
    (512, 448, 3, 1, False, 1.0),      # odd tile count
    (300, 256, 2, 2, True, 1.0),       # 4 tiles: no trip of the unrolled loop; second workgroup has 44 rows
    (600, 3600, 2, 1, True, 1.0),      # the spatial shape of 720p: 57 tiles, the last with 16 keys
    (512, 1024, 2, 2, False, 2.5),     # un-normed q, k scaled up: logits of +-60, the deferred-rescale branch fires on most tiles
])
def test_flash_w64_matches_default_and_torch(ops, q_len, kv_len, heads, batch, norm, qscale):
    """flash variant 14 (attention_w64.hip: 64 query rows per wave, one wave per SIMD, the tile loop one hand-allocated asm
    statement) against the 32-rows-per-wave kernels (variant 15) and torch fp32 SDPA.  Per query row the two kernels do the same
    arithmetic in the same order as long as the deferred rescale fires for the same tiles; the decision is taken per 64 rows there
    and per 32 rows here, so bit equality is asserted on the inputs whose logits stay inside the threshold (RMS-normed q, k) and a
    tolerance everywhere."""
    from videosys_amd import _lib

    lib = _lib.load()
    C = heads * 72
    g = torch.Generator().manual_seed(q_len + kv_len)
    q = (torch.randn(batch * q_len, C, generator=g) * qscale).to(torch.bfloat16).to(dev())
    k = (torch.randn(batch * kv_len, C, generator=g) * qscale).to(torch.bfloat16).to(dev())
    v = torch.randn(batch * kv_len, C, generator=g).to(torch.bfloat16).to(dev())
    qw = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev()) if norm else None
    kw_ = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev()) if norm else None
    try:
        assert lib.vsys_tune_flash_variant(15) == 0
        base = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        assert lib.vsys_tune_flash_variant(14) == 0
        res = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        res2 = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        torch.cuda.synchronize()
    finally:
        lib.vsys_tune_flash_variant(0)
    assert torch.equal(res, res2), "two launches of the w64 kernel differ (a race)"
    if norm:
        assert torch.equal(res, base), f"w64 differs from the 32-row kernel: max {float((res.float() - base.float()).abs().max()):.3e}"
    for bi in range(batch):
        for h in range(heads):
            qq = q[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72]
            kk = k[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72]
            vv = v[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72].float()
            if norm:
                qq, kk = O.rms_norm(qq, qw.float()), O.rms_norm(kk, kw_.float())
            ref = O.sdpa(qq.float()[None], kk.float()[None], vv[None])[0]
            check(res[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72], ref, tol=2.0 ** -6, what=f"w64 flash b{bi} h{h}")
            check(base[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72], ref, tol=2.0 ** -6, what=f"32-row flash b{bi} h{h}")


@pytest.mark.parametrize("q_len,kv_len,heads,batch,wscale,fv", [
    (1024, 1024, 16, 40, 1.0, 18),     # config-2 spatial shape, persistent walk (2560 items)
    (1024, 1024, 16, 40, 1.0, 0),      # ... whatever the dispatch picks when the promise is given (the 32-row kernel ignores it)
    (600, 3600, 2, 1, 1.0, 17),        # 720p frame: one item per workgroup, ragged last tile and last query block
    (700, 2304, 4, 2, 1.6, 0),         # larger norm weights (logit bound ~45): default dispatch from 2048 keys
    (512, 512, 8, 40, 0.3, 18),        # small weights: the bound is far above nothing, P stays well inside bf16's range
    (1000, 3648, 16, 6, 1.0, 18),      # 57 tiles on the persistent walk (odd: the ring position of tile 0 rotates from item to item)
    (512, 320, 8, 40, 1.0, 18),        # 5 tiles per item
])
def test_flash_w64_without_running_max(ops, q_len, kv_len, heads, batch, wscale, fv):
    """vsys_flash_attn_d72_kb: with the caller's bound on the key norms (ops.rms_key_bound, from the norm weights) the w64
    kernels subtract m_i = |q_i| k_bound instead of a running maximum (flash72_gen.py variant 5).  Softmax does not depend on the
    subtracted constant, so the result must agree with the running-max kernels to the tolerance both have against fp32 torch; forced
    one-item (17) / persistent (18) forms and the default dispatch."""
    from videosys_amd import _lib

    lib = _lib.load()
    C = heads * 72
    g = torch.Generator().manual_seed(q_len + kv_len + heads + fv)
    q = torch.randn(batch * q_len, C, generator=g).to(torch.bfloat16).to(dev())
    k = torch.randn(batch * kv_len, C, generator=g).to(torch.bfloat16).to(dev())
    v = torch.randn(batch * kv_len, C, generator=g).to(torch.bfloat16).to(dev())
    qw = (wscale * (1 + 0.1 * torch.randn(72, generator=g))).to(torch.bfloat16).to(dev())
    kw_ = (wscale * (1 + 0.1 * torch.randn(72, generator=g))).to(torch.bfloat16).to(dev())
    kb = ops.rms_key_bound(qw, kw_)
    assert kb is not None and kb > 0
    try:
        assert lib.vsys_tune_flash_variant(15) == 0
        base = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        assert lib.vsys_tune_flash_variant(fv) == 0
        res = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len, k_norm_bound=kb)
        res2 = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len, k_norm_bound=kb)
        torch.cuda.synchronize()
    finally:
        lib.vsys_tune_flash_variant(0)
    assert torch.isfinite(res.float()).all()
    assert torch.equal(res, res2), "two launches differ (a race)"
    scale = base.float().abs().max().item()
    assert (res.float() - base.float()).abs().max().item() <= 2.0 ** -6 * scale
    for bi, h in ((0, 0), (batch - 1, heads - 1)):
        qq = O.rms_norm(q[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72], qw.float())
        kk = O.rms_norm(k[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72], kw_.float())
        vv = v[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72].float()
        ref = O.sdpa(qq.float()[None], kk.float()[None], vv[None])[0]
        sl = (slice(bi * q_len, (bi + 1) * q_len), slice(h * 72, (h + 1) * 72))
        e_new, e_old = (res[sl].float().cpu() - ref.cpu()).abs().max().item(), (base[sl].float().cpu() - ref.cpu()).abs().max().item()
        check(res[sl], ref, tol=2.0 ** -6, what=f"flash without running max b{bi} h{h}")
        assert e_new <= 1.5 * e_old + 1e-3, (e_new, e_old)
    # weights the promise cannot be derived from: no bound
    assert ops.rms_key_bound(qw * 8, kw_ * 8) is None


@pytest.mark.parametrize("q_len,kv_len,heads,batch,norm,qscale", [
    (1024, 1024, 16, 10, True, 1.0),    # 640 items on 256 workgroups: every workgroup walks 2-3 items, K / Vt change inside a walk
    (700, 512, 16, 12, False, 1.0),     # 576 items, ragged last query block of every (batch, head)
    (512, 256, 8, 40, True, 1.0),       # 4 tiles per item: the descriptor switch happens before the first tile of every item
    (600, 448, 8, 24, True, 1.0),       # 7 tiles per item: the ring position of tile 0 changes from item to item
    (1024, 1024, 2, 2, False, 2.5),     # fewer items than CUs; the deferred-rescale branch fires
])
def test_flash_w64_persistent_matches_one_item_kernel(ops, q_len, kv_len, heads, batch, norm, qscale):
    """flash variant 16 (the persistent form of the w64 kernel: one workgroup per CU walks (batch, head, query block) items, the tail
    of an item's tile loop prefetches the next item's tiles and Q rows) against variant 14 (one item per workgroup, same instruction
    stream per tile): the same bits, whatever the walk; and torch fp32 SDPA on sampled (batch, head) pairs."""
    from videosys_amd import _lib

    lib = _lib.load()
    C = heads * 72
    g = torch.Generator().manual_seed(q_len + kv_len + heads)
    q = (torch.randn(batch * q_len, C, generator=g) * qscale).to(torch.bfloat16).to(dev())
    k = (torch.randn(batch * kv_len, C, generator=g) * qscale).to(torch.bfloat16).to(dev())
    v = torch.randn(batch * kv_len, C, generator=g).to(torch.bfloat16).to(dev())
    qw = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev()) if norm else None
    kw_ = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev()) if norm else None
    try:
        assert lib.vsys_tune_flash_variant(14) == 0
        base = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        assert lib.vsys_tune_flash_variant(16) == 0
        res = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        res2 = _run_flash(ops, q, k, v, qw, kw_, batch, heads, q_len, kv_len)
        torch.cuda.synchronize()
    finally:
        lib.vsys_tune_flash_variant(0)
    assert torch.equal(res, res2), "two launches of the persistent kernel differ (a race)"
    assert torch.equal(res, base), f"persistent form differs from the one-item kernel: max {float((res.float() - base.float()).abs().max()):.3e}"
    for bi, h in ((0, 0), (batch - 1, heads - 1), (batch // 2, heads // 2)):
        qq = q[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72]
        kk = k[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72]
        vv = v[bi * kv_len:(bi + 1) * kv_len, h * 72:(h + 1) * 72].float()
        if norm:
            qq, kk = O.rms_norm(qq, qw.float()), O.rms_norm(kk, kw_.float())
        ref = O.sdpa(qq.float()[None], kk.float()[None], vv[None])[0]
        check(res[bi * q_len:(bi + 1) * q_len, h * 72:(h + 1) * 72], ref, tol=2.0 ** -6, what=f"persistent w64 flash b{bi} h{h}")


def test_attn_config2_sizes_vs_torch(ops):
    """Config-2 geometry for one CFG sample slice: spatial (frames x 1024 tokens, 16 heads) vs torch fp32 SDPA on the
    GPU for sampled (frame, head) pairs, plus the softmax-of-constant-V property on everything."""
    frames, S, H, C = 38, 1024, 16, 1152
    g = torch.Generator().manual_seed(21)
    qkv = (torch.randn(frames * S, 3 * C, generator=g)).to(torch.bfloat16).to(dev())
    qw = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev())
    kw_ = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16).to(dev())
    out = _run_flash(ops, qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], qw, kw_, frames, H, S, S)
    for fr, h in ((0, 0), (17, 5), (37, 15)):
        blk = qkv[fr * S:(fr + 1) * S].float()
        q = O.rms_norm(blk[:, h * 72:(h + 1) * 72].to(torch.bfloat16), qw.float()).float()
        k = O.rms_norm(blk[:, C + h * 72:C + (h + 1) * 72].to(torch.bfloat16), kw_.float()).float()
        v = blk[:, 2 * C + h * 72:2 * C + (h + 1) * 72]
        ref = O.sdpa(q[None], k[None], v[None])[0]
        check(out[fr * S:(fr + 1) * S, h * 72:(h + 1) * 72], ref, what=f"c2 spatial attn frame {fr} head {h}")
    # property: V constant per (frame, head, dim) => output equals that constant for every query
    qkv2 = qkv.clone()
    const = torch.randn(frames, 1, C, generator=g).to(torch.bfloat16).to(dev())
    qkv2.view(frames, S, 3 * C)[:, :, 2 * C:] = const
    out2 = _run_flash(ops, qkv2[:, :C], qkv2[:, C:2 * C], qkv2[:, 2 * C:], qw, kw_, frames, H, S, S)
    check(out2.view(frames, S, C), const.expand(frames, S, C), tol=2.0**-7, what="constant-V property")


def test_attn_temporal_config2_vs_torch(ops):
    B, T, S, H, C = 2, 19, 1024, 16, 1152
    g = torch.Generator().manual_seed(22)
    qkv = torch.randn(B * T * S, 3 * C, generator=g).to(torch.bfloat16).to(dev())
    qw = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16)
    kw_ = (1 + 0.1 * torch.randn(72, generator=g)).to(torch.bfloat16)
    freqs = 1.0 / (10000 ** (torch.arange(0, 72, 2).float() / 72))
    cos, sin = O.rope_table(freqs, T)
    out = torch.empty(B * T * S, C, dtype=torch.bfloat16, device=dev())
    ops.attn_temporal(qkv, C, bf(qw), bf(kw_), cos.contiguous().to(dev()), sin.contiguous().to(dev()), out, B, T, S, H)
    v5 = qkv.view(B, T, S, 3, H, 72)
    for (b, s, h) in ((0, 0, 0), (1, 513, 7), (1, 1023, 15)):
        q = O.rope_rotate(O.rms_norm(v5[b, :, s, 0, h].cpu(), qw.float()).float()[None], freqs)
        k = O.rope_rotate(O.rms_norm(v5[b, :, s, 1, h].cpu(), kw_.float()).float()[None], freqs)
        v = v5[b, :, s, 2, h].cpu().float()[None]
        ref = O.sdpa(q, k, v)[0]
        got = out.view(B, T, S, H, 72)[b, :, s, h]
        check(got, ref, what=f"c2 temporal attn (b={b}, s={s}, h={h})")


# ------------------------------------------------------------------------------------------------ DSP plans on device
def test_dsp_plans_hip_executor(ops):
    """The pack/unpack plans executed by the HIP copy kernel for every rank of a P-way group, with the collective
    replaced by an in-process exchange, must reproduce the reference all_to_all_with_pad semantics (oracle)."""
    from videosys_amd import dsp

    B, T, S, C, P = 2, 5, 12, 64, 4
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, T, S, C, generator=g).to(torch.bfloat16)
    shards_ref = O.dsp_split_sequence(x.float(), P, dim=2)
    Sl = shards_ref[0].shape[2]
    local = []
    for r in range(P):
        ops_, shape = dsp.plan_split(B, T, S, C, P, r)
        out = torch.empty(shape, dtype=torch.bfloat16, device=dev())
        dsp.hip_copy_executor(bf(x), out, ops_)
        assert torch.equal(out.cpu().float(), shards_ref[r])
        local.append(out)
    t_ref = O.dsp_all_to_all(shards_ref, 1, 2, O.dsp_pad(T, P), O.dsp_pad(S, P))
    pack, unpack, sshape, oshape = dsp.plan_switch_to_temporal_shard(B, T, Sl, S, C, P)
    sends = []
    for r in range(P):
        send = torch.empty(sshape, dtype=torch.bfloat16, device=dev())
        dsp.hip_copy_executor(local[r], send, pack)
        sends.append(send)
    t_local = []
    for r in range(P):
        recv = torch.stack([sends[src][r] for src in range(P)])  # all_to_all_single semantics
        out = torch.empty(oshape, dtype=torch.bfloat16, device=dev())
        dsp.hip_copy_executor(recv, out, unpack)
        assert torch.equal(out.cpu().float(), t_ref[r]), f"to_temporal_shard rank {r}"
        t_local.append(out)
    Tp = oshape[1]
    pack, unpack, sshape, oshape = dsp.plan_switch_to_spatial_shard(B, Tp, T, S, Sl, C, P)
    sends = []
    for r in range(P):
        send = torch.empty(sshape, dtype=torch.bfloat16, device=dev())
        dsp.hip_copy_executor(t_local[r], send, pack)
        sends.append(send)
    for r in range(P):
        recv = torch.stack([sends[src][r] for src in range(P)])
        out = torch.empty(oshape, dtype=torch.bfloat16, device=dev())
        dsp.hip_copy_executor(recv, out, unpack)
        assert torch.equal(out.cpu().float(), shards_ref[r]), f"to_spatial_shard rank {r}"


# ------------------------------------------------------------------------------------------------ whole model
def _small_model(fx):
    from videosys_amd.stdit3 import STDiT3, STDiT3Config

    cfg = fx["cfg"]
    sd = O.synth_state_dict(**cfg, seed=fx["seed"])
    sd = {k: (v if k == "rope.freqs" else v.to(torch.bfloat16).float()) for k, v in sd.items()}
    m = STDiT3(STDiT3Config(**cfg), device=dev())
    m.load_state_dict(sd)
    return m


def _model_check(out, ref, what):
    out = out.float().cpu()
    e = rel_err(out, ref)
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
    assert e <= 3e-2 and cos >= 0.999, f"{what}: rel max err {e:.3e}, cosine {cos:.6f}"


def test_stdit3_forward_golden():
    fx = load_golden("stdit3_fwd_small.pt")
    m = _small_model(fx)
    i = fx["inputs"]
    out = m(i["x"], i["timestep"], i["y"], mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"])
    _model_check(out, fx["out"], "STDiT3 small forward vs reference")
    # second call hits the text/kv caches and must give the same answer
    out2 = m(i["x"], i["timestep"], i["y"], mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"])
    assert torch.equal(out.cpu(), out2.cpu())


def test_stdit3_launch_program_replay_equals_eager():
    """Launch programs (videosys_amd/program.py, vsys_program_run): a step recorded once and replayed through the C loop must give
    the bits of the step issued launch by launch from Python — across changing inputs and timesteps (they live in the program's
    device buffers), and per PAB decision pattern (each pattern is its own program; a pattern seen for the first time is
    recorded while it runs eagerly)."""
    from videosys_amd import pab

    fx = load_golden("stdit3_pab_small.pt")
    i = fx["inputs"]
    kw = dict(mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"])
    g = torch.Generator().manual_seed(77)
    xs = [i["x"]] + [torch.randn(i["x"].shape, generator=g).to(torch.bfloat16).float() for _ in range(3)]
    ts = [900.0, 640.0, 333.0, 120.0]

    def run(use_programs, with_pab):
        m = _small_model(fx)
        m.use_programs = use_programs
        outs = []
        if with_pab:
            p = fx["pab"]
            pab.set_pab_manager(pab.PABConfig(spatial_broadcast=True, spatial_threshold=list(p["spatial"][:2]), spatial_range=p["spatial"][2],
                                              temporal_broadcast=True, temporal_threshold=list(p["temporal"][:2]), temporal_range=p["temporal"][2],
                                              cross_broadcast=True, cross_threshold=list(p["cross"][:2]), cross_range=p["cross"][2]))
            pab.update_steps(fx["steps"])
        try:
            if with_pab:
                for rep in range(2):          # the schedule twice: the second pass replays every pattern of the first
                    m.reset_pab_state()
                    for t in fx["timesteps"]:
                        outs.append(m(i["x"], torch.tensor([t, t]), i["y"], **kw).float().cpu())
            else:
                for x, t in zip(xs, ts):
                    outs.append(m(x, torch.tensor([t, t]), i["y"], **kw).float().cpu())
        finally:
            pab.set_pab_manager(None)
        torch.cuda.synchronize()
        return outs, dict(m.program_stats)

    for with_pab in (False, True):
        eager, st0 = run(False, with_pab)
        prog, st1 = run(True, with_pab)
        assert st0["replayed"] == 0 and st0["recorded"] == 0
        assert st1["replayed"] >= (len(fx["timesteps"]) if with_pab else 3), st1
        for k, (a, b) in enumerate(zip(eager, prog)):
            assert torch.equal(a, b), f"pab={with_pab} call {k}: replayed step differs from the eager step ({st1})"
        if not with_pab:   # the outputs handed back are the caller's: a later replay must not overwrite them
            assert not torch.equal(prog[0], prog[1])


def test_stdit3_pab_slab_elision_is_exact():
    """A computed attention output is written to its PAB slab only when the block's next call will broadcast it
    (STDiT3._pab_plan).  Keeping every output (the reference's behaviour) and keeping only the needed ones must give the same bits
    at every step of the schedule, two videos back to back."""
    from videosys_amd import pab

    fx = load_golden("stdit3_pab_small.pt")
    i = fx["inputs"]
    kw = dict(mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"])
    p = fx["pab"]
    sched = [int(t) for t in fx["timesteps"]]

    def run(elide):
        m = _small_model(fx)
        m.pab_elide_unused = elide
        pab.set_pab_manager(pab.PABConfig(spatial_broadcast=True, spatial_threshold=list(p["spatial"][:2]), spatial_range=p["spatial"][2],
                                          temporal_broadcast=True, temporal_threshold=list(p["temporal"][:2]), temporal_range=p["temporal"][2],
                                          cross_broadcast=True, cross_threshold=list(p["cross"][:2]), cross_range=p["cross"][2]))
        pab.update_steps(fx["steps"])
        outs = []
        try:
            for rep in range(2):
                m.reset_pab_state()
                for t in fx["timesteps"]:
                    outs.append(m(i["x"], torch.tensor([t, t]), i["y"], all_timesteps=sched, **kw).float().cpu())
        finally:
            pab.set_pab_manager(None)
        torch.cuda.synchronize()
        return outs

    a, b = run(False), run(True)
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), f"step {k}: eliding unused slab writes changed the result"
    for t, ref, out in zip(fx["timesteps"], fx["outs"], b):
        _model_check(out, ref, f"PAB (elided slabs) step t={t}")


def test_stdit3_pab_golden():
    from videosys_amd import pab

    fx = load_golden("stdit3_pab_small.pt")
    m = _small_model(fx)
    p = fx["pab"]
    cfg = pab.PABConfig(spatial_broadcast=True, spatial_threshold=list(p["spatial"][:2]), spatial_range=p["spatial"][2],
                        temporal_broadcast=True, temporal_threshold=list(p["temporal"][:2]), temporal_range=p["temporal"][2],
                        cross_broadcast=True, cross_threshold=list(p["cross"][:2]), cross_range=p["cross"][2])
    pab.set_pab_manager(cfg)
    pab.update_steps(fx["steps"])
    try:
        i = fx["inputs"]
        for t, ref in zip(fx["timesteps"], fx["outs"]):
            tt = torch.tensor([t, t])
            out = m(i["x"], tt, i["y"], mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"])
            _model_check(out, ref, f"PAB step t={t}")
    finally:
        pab.set_pab_manager(None)


def test_stdit3_pab_mlp_broadcast_golden():
    """Full PAB incl. the MLP broadcast (pab_mgr.py:93-174, open_sora_transformer_3d.py:232-280) against the reference model run
    with ``all_timesteps`` handed to its blocks (oracle/make_golden_pab_mlp.py): windows opening at 900 / 640 (spatial) and 800
    (temporal), replayed blocks, entries dropped at the window's end."""
    from videosys_amd import pab

    fx = load_golden("stdit3_pab_mlp_small.pt")
    m = _small_model(fx)
    p = fx["pab"]
    cfg = pab.PABConfig(spatial_broadcast=True, spatial_threshold=list(p["spatial"][:2]), spatial_range=p["spatial"][2],
                        temporal_broadcast=True, temporal_threshold=list(p["temporal"][:2]), temporal_range=p["temporal"][2],
                        cross_broadcast=True, cross_threshold=list(p["cross"][:2]), cross_range=p["cross"][2],
                        mlp_broadcast=True, mlp_spatial_broadcast_config=fx["mlp_spatial"],
                        mlp_temporal_broadcast_config=fx["mlp_temporal"])
    pab.set_pab_manager(cfg)
    pab.update_steps(fx["steps"])
    try:
        i = fx["inputs"]
        with pytest.raises(ValueError):   # the schedule is required (the reference dies with TypeError here)
            m(i["x"], torch.tensor([900.0, 900.0]), i["y"], mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"])
        m.reset_pab_state()
        for t, ref in zip(fx["timesteps"], fx["outs"]):
            tt = torch.tensor([float(t), float(t)])
            out = m(i["x"], tt, i["y"], mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"],
                    all_timesteps=fx["timesteps"])
            _model_check(out, ref, f"PAB + MLP broadcast step t={t}")
        assert (len(cfg.mlp_spatial_outputs), len(cfg.mlp_temporal_outputs)) == tuple(fx["stored_left"])
    finally:
        pab.set_pab_manager(None)


def test_rflow_golden():
    from videosys_amd.rflow import RFLOW

    fx = load_golden("rflow_small.pt")
    m = _small_model(fx)
    sched = RFLOW(num_sampling_steps=fx["steps"], cfg_scale=fx["cfg_scale"], use_timestep_transform=True)
    margs = dict(y=fx["y"], mask=fx["mask"], height=fx["height"], width=fx["width"], num_frames=fx["num_frames"],
                 fps=fx["fps"])
    ts = sched.prepare_timesteps(1, margs)
    assert [int(t[0]) for t in ts] == fx["all_timesteps"]  # the golden model is fp32: int(t.to(float32))
    z = sched.sample(m, fx["z0"], margs, fx["y_null"])
    out = z.float().cpu()
    # (1) Against the oracle fed the timesteps a bf16 model really sees: STDiT3.forward casts timestep to the model dtype
    # (open_sora_transformer_3d.py:562), e.g. 626.3 -> 628, and CFG (x7) amplifies that input change; the fp32 golden
    # below used the un-rounded value.
    cfg = fx["cfg"]
    sd = O.synth_state_dict(**cfg, seed=fx["seed"])
    sd = {k: (v if k == "rope.freqs" else v.to(torch.bfloat16).float()) for k, v in sd.items()}
    om = O.STDiT3Oracle(sd, cfg["depth"], cfg["hidden_size"], cfg["num_heads"])
    zref = O.rflow_sample(om, fx["z0"], fx["y"], fx["y_null"], fx["mask"], fx["fps"], fx["height"], fx["width"],
                          fx["num_frames"], num_sampling_steps=fx["steps"], cfg_scale=fx["cfg_scale"],
                          model_dtype=torch.bfloat16)
    e = rel_err(out, zref)
    cos = torch.nn.functional.cosine_similarity(out.flatten(), zref.flatten(), dim=0).item()
    assert e <= 5e-2 and cos >= 0.999, f"RFLOW 4-step latents vs oracle(bf16 timesteps): rel err {e:.3e}, cosine {cos:.6f}"
    # (2) Against the reference's fp32 run (golden): looser, dominated by the timestep rounding (oracle-vs-golden with
    # only that change already differs by 6.4e-2 / cosine 0.9980).
    e = rel_err(out, fx["z_out"])
    cos = torch.nn.functional.cosine_similarity(out.flatten(), fx["z_out"].flatten(), dim=0).item()
    assert e <= 1e-1 and cos >= 0.995, f"RFLOW 4-step latents vs reference fp32 golden: rel err {e:.3e}, cosine {cos:.6f}"


# ------------------------------------------------------------------------------------------------ image / video conditioning
def test_stdit3_x_mask_golden_and_sharded():
    """STDiT3.forward with a conditioning mask (open_sora_transformer_3d.py:181-184,198-200,220-222,262-273,578-582 and the final
    layer's twice-normalised timestep-0 branch :82-85) against the fixture minted from the reference; an all-True mask must
    be the plain step bit for bit; four sequence-parallel ranks in process must reproduce the single-process output bit for
    bit (the modulation row of a frame does not depend on where its tokens live)."""
    from tools.local_group import LocalWorld
    from types import SimpleNamespace

    fx = load_golden("stdit3_xmask_small.pt")
    m = _small_model(fx)
    i = fx["inputs"]
    kw = dict(mask=i["mask"], fps=i["fps"], height=i["height"], width=i["width"])
    out = m(i["x"], i["timestep"], i["y"], x_mask=fx["x_mask"], **kw)
    _model_check(out, fx["out"], "STDiT3 small forward with x_mask vs reference")
    # the masked frames really took the other branch: against the all-True output they differ as much as the reference's do
    plain = m(i["x"], i["timestep"], i["y"], **kw)
    ones = m(i["x"], i["timestep"], i["y"], x_mask=torch.ones(2, 5, dtype=torch.bool), **kw)
    assert torch.equal(ones, plain)
    _model_check(ones, fx["out_all_true"], "STDiT3 small forward with an all-True x_mask vs reference")
    sel = fx["x_mask"][:, None, :, None, None].expand_as(fx["out"])
    d_hip = (out.float().cpu() - plain.float().cpu())[~sel].abs().mean().item()
    d_ref = (fx["out"] - fx["out_all_true"])[~sel].abs().mean().item()
    assert abs(d_hip - d_ref) <= 0.05 * d_ref, (d_hip, d_ref)
    # (the masked call runs eagerly; the all-True mask IS the plain step: recorded by the plain call, replayed for the mask)
    assert m.program_stats["eager"] == 1 and m.program_stats["recorded"] == 1 and m.program_stats["replayed"] == 1

    P = 4

    def rank_fn(r, group):
        torch.cuda.set_device(0)
        mm = _small_model(fx)
        pm = SimpleNamespace(sp_size=P, cp_size=1, dp_size=1, dp_rank=0, sp_rank=r, cp_rank=0, sp_group=group, cp_group=None)
        res = []
        for scatter, overlap in (("flat", False), ("sample", True)):
            mm.enable_parallel(parallel_mgr=pm, overlap=overlap)
            mm._scatter = scatter
            o = mm(i["x"], i["timestep"], i["y"], x_mask=fx["x_mask"], **kw)
            torch.cuda.synchronize()
            res.append(bool(torch.equal(o, out)))
        return res

    for r, res in enumerate(LocalWorld(P, timeout=300).run(rank_fn)):
        assert all(res), f"rank {r}: sharded x_mask output differs from the single-process output {res}"


def test_rflow_masked_sampling_vs_oracle():
    """RFLOW.sample(mask=...) (scheduling_rflow_open_sora.py:215-236,254-255): same seeded noise into the HIP sampler and the
    oracle (bf16 timesteps as the bf16 model sees them); the held frame must come back bit for bit, the edited frame must have
    joined, and the latents must agree at the sampler tolerance of test_rflow_golden."""
    from videosys_amd.rflow import RFLOW

    fx = load_golden("stdit3_xmask_small.pt")
    s = fx["sample"]
    m = _small_model(fx)
    sched = RFLOW(num_sampling_steps=s["steps"], cfg_scale=s["cfg_scale"], use_timestep_transform=True)
    margs = dict(y=s["y"], mask=s["mask"], height=s["height"], width=s["width"], num_frames=s["num_frames"], fps=s["fps"])
    seen = []

    class Spy:   # (STDiT3.__call__ is bound on the class: wrap the object rather than patching an attribute)
        def __getattr__(self, k):
            return getattr(m, k)

        def __call__(self, *a, **k):
            seen.append(None if k.get("x_mask") is None else k["x_mask"].clone().cpu())
            return m(*a, **k)

    g = torch.Generator().manual_seed(77)
    noises = [torch.randn(s["z0"].shape, generator=g) for _ in range(s["steps"])]
    it = iter(noises)
    z = sched.sample(Spy(), s["z0"], margs, s["y_null"], mask=s["cond_mask"], noise_fn=lambda shape: next(it)).float().cpu()
    assert [None if v is None else v.tolist() for v in seen] == [v.tolist() for v in s["x_masks"]]   # never all-True here
    assert torch.equal(z[:, :, 0], s["z0"][:, :, 0]) and not torch.equal(z[:, :, 1], s["z0"][:, :, 1])

    cfg = fx["cfg"]
    sd = O.synth_state_dict(**cfg, seed=fx["seed"])
    sd = {k: (v if k == "rope.freqs" else v.to(torch.bfloat16).float()) for k, v in sd.items()}
    om = O.STDiT3Oracle(sd, cfg["depth"], cfg["hidden_size"], cfg["num_heads"])
    it2 = iter(noises)
    zref = O.rflow_sample(om, s["z0"], s["y"], s["y_null"], s["mask"], s["fps"], s["height"], s["width"], s["num_frames"],
                          num_sampling_steps=s["steps"], cfg_scale=s["cfg_scale"], model_dtype=torch.bfloat16,
                          cond_mask=s["cond_mask"], noise_fn=lambda shape: next(it2))
    e = rel_err(z, zref)
    cos = torch.nn.functional.cosine_similarity(z.flatten(), zref.flatten(), dim=0).item()
    assert e <= 5e-2 and cos >= 0.999, f"masked RFLOW latents vs oracle(bf16 timesteps): rel err {e:.3e}, cosine {cos:.6f}"
