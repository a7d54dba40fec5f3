"""-m gpu: the GEMM family (gemm_bf16.hip, gemm2_bf16.hip, the AdaLN fold) against a float64 reference, element by element on every
row and column (tests/numerics.py), at the shapes the model launches and on both sides of every branch of the shape dispatch.

Variant 0 is the shipped dispatch; variant 8 forces schedule 8 (32x32x16) wherever launch_gemm honours it — the anchor the
same-bits tests of tests/test_gpu_adaln_fold.py compare against, so both sides of those tests have an oracle of their own.

Rounding chains (the reference = the model run in bf16; each rounding a worst case 2^-8 |v|, fp32 sums K 2^-24 sum|a_k b_k|):
  * store-only  (cross-q):      bf16(a W^T + b)                                    acc + rnd(p)
  * GELU        (fc1 unfused):  bf16(gelu(bf16(a W^T + b)))                        1.13 (acc + rnd(p)) + rnd(gelu) (+ fp32 exp2 / rcp)
  * gate + res  (proj, fc2):    bf16(x + bf16(g * bf16(a W^T + b)))                |g| (acc + rnd(p)) + rnd(g p) + rnd(x + g p)
    (the epilogue rounds twice: bf16(x + bf16(g (acc + b))); a form with one rounding fewer passes the same bound)
  * residual    (cross-proj):   bf16(x + bf16(a W^T + b))                          acc + rnd(p) + rnd(x + p)
  * PAB adds:                   every ``x += cached`` one more rounding of the running sum; the slab copy = bf16(g p)
  * LayerNorm fold (qkv, fc1):  Linear(LN(x) (1 + scale) + shift), LN in fp32 (test_gemm_ln_vs_fp32_and_unfused); the fold
    rounds W (1 + scale) to bf16 where the model rounds the modulated activations, sums x Wp and x-independent sum_k Wp in fp32
    and combines rstd (acc - mu cs) + cv:  rstd (rnd(W (1+s)) . |x - mu| + acc(x Wp) + |mu| acc(Wp)) + acc(shift W + b)
    + stats (mu / rstd to 2^-20 relative) + rnd(out), then GELU as above.

Second half: the GEMM work only Latte, CogVideoX, the two Open-Sora-Plans and Vchitect-2.0 do (tests/gemm_numerics_cases.py: the tables, the
per-row two-segment gate, the GELU bound from the activation's image interval, linear_small).  Every one of those tests names the kernel
its launch reaches (from the restated dispatch rule) and prints the worst |err| / bound.
"""
import contextlib
import math

import pytest
import torch

import gemm_numerics_cases as gc
import numerics as nm

pytestmark = pytest.mark.gpu

CHUNK = 4096
GELU_SLOPE = 1.13          # max |d gelu_tanh / dx|
STATS_REL = 2.0**-20       # LayerNorm statistics from fp32 partials (mean / M2 per 96 columns, merged)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


@contextlib.contextmanager
def variant(v):
    from videosys_amd import _lib

    lib = _lib.load()
    assert lib.vsys_tune_gemm_variant(v) == 0, f"variant {v} rejected: the default would be tested instead"
    try:
        yield
    finally:
        lib.vsys_tune_gemm_variant(0)


def randn(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev()) * scale + offset).to(torch.bfloat16)


def operands(M, N, K, seed):
    return randn((M, K), seed), randn((N, K), seed + 1, 1.0 / math.sqrt(K)), randn((N,), seed + 2, 0.1)


def gelu64(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v**3)))


def gate_rows(gate, gate_stride, rps, r0, r1, N):
    """Gate of rows r0 .. r1-1: the row of sample r // rps at gate + sample * gate_stride (float64 [r1 - r0, N])."""
    base = torch.as_strided(gate, (-(-r1 // rps), N), (gate_stride, 1))
    return base.double()[torch.arange(r0, r1, device=gate.device) // rps]


def check_gemm(out, x, w, b, what, *, gelu=False, gate=None, gate_stride=0, rps=0, res=None, adds=(), aux=None):
    """out (and aux, the slab copy of g p) against the float64 reference of the GEMM site, chunk by chunk over the rows."""
    M, K = x.shape
    N = w.shape[0]
    bd = b.double() if b is not None else torch.zeros(N, dtype=torch.float64, device=x.device)
    rep, rep_aux = nm.Bound(what), nm.Bound(what + " [aux slab]")
    for r0, r1 in nm.row_chunks(M, CHUNK):
        p, s = nm.matmul_ref(x[r0:r1], w)
        p = p + bd
        e = nm.acc(K, s + bd.abs())
        if gelu:
            ref = gelu64(p)
            bound = GELU_SLOPE * (e + nm.rnd(p)) + nm.rnd(ref) + 2.0**-16 * ref.abs()
        elif res is None:
            ref, bound = p, e + nm.rnd(p)
        else:
            if gate is not None:
                g = gate_rows(gate, gate_stride, rps, r0, r1, N)
                u, eu = g * p, g.abs() * (e + nm.rnd(p)) + nm.rnd(g * p)
            else:
                u, eu = p, e + nm.rnd(p)
            if aux is not None:
                rep_aux.add(aux[r0:r1], u, eu, r0)
            ref = res[r0:r1].double() + u
            bound = eu + nm.rnd(ref)
            for a in adds:
                ref = ref + a[r0:r1].double()
                bound = bound + nm.rnd(ref)
        rep.add(out[r0:r1], ref, bound, r0)
    rep.check()
    if aux is not None:
        rep_aux.check()


def prescale(ops, W, bias, shift, scale):
    """One-site vsys_adaln_prescale (shift | scale laid out like one row of the modulation table): Wp = bf16(W (1 + scale)),
    cs = sum_k Wp, cv = W shift + bias."""
    N, K = W.shape
    mod = torch.cat([shift, scale]).contiguous()
    Wp = torch.empty_like(W)
    cs = torch.empty(N, dtype=torch.float32, device=W.device)
    cv = torch.empty(N, dtype=torch.float32, device=W.device)
    sites = torch.tensor([[W.data_ptr(), bias.data_ptr(), Wp.data_ptr(), cs.data_ptr(), cv.data_ptr(), 0, K, N, K, 0]],
                         dtype=torch.int64).to(W.device)
    ops.adaln_prescale(sites, -(-N // 4), mod)
    return Wp, cs, cv


def check_gemm_ln(out, x, W, Wp, bias, shift, scale, what, *, gelu=False, eps=1e-6):
    """out = [gelu](Linear(LN(x) (1 + scale) + shift)) (the model) against float64, with the fold's chain (module docstring)."""
    M, K = x.shape
    sd, cd = shift.double(), 1.0 + scale.double()
    Wd, Wpd, bd = W.double(), Wp.double(), bias.double()
    Wm = Wd * cd[None, :]                      # W (1 + scale), exact
    cv = Wd @ sd + bd
    cv_err = nm.acc(K, Wd.abs() @ sd.abs() + bd.abs())
    cs_abs = Wpd.abs().sum(1)
    rep = nm.Bound(what)
    for r0, r1 in nm.row_chunks(M, CHUNK):
        xd = x[r0:r1].double()
        mu = xd.mean(1, keepdim=True)
        rstd = torch.rsqrt(((xd - mu) ** 2).mean(1, keepdim=True) + eps)
        c = xd - mu
        p = rstd * (c @ Wm.t()) + cv
        cw = c.abs() @ Wm.abs().t()
        e = rstd * (nm.U_BF16 * cw + nm.acc(K, xd.abs() @ Wpd.abs().t()) + nm.acc(K, mu.abs() * cs_abs)) \
            + cv_err + STATS_REL * rstd * (cw + mu.abs() * cs_abs)
        if gelu:
            ref = gelu64(p)
            bound = GELU_SLOPE * (e + nm.rnd(p)) + nm.rnd(ref) + 2.0**-16 * ref.abs()
        else:
            ref, bound = p, e + nm.rnd(p)
        rep.add(out[r0:r1], ref, bound, r0)
    rep.check()


# ------------------------------------------------------------------------------------------------ the sites as the model calls them
C = 1152
SHAPES = [(38912, 19456), (4864, 2432)]    # config 2 (2 x 19 x 1024 tokens, one sample = T S) | one rank of eight


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("M,rps", SHAPES)
def test_site_qkv_and_fc1_layernorm_fold(ops, M, rps, v):
    """qkv (N = 3456) and fc1 + GELU (N = 4608): gemm_ln on weights from adaln_prescale, statistics from ln_row_stats."""
    x = randn((M, C), 10, offset=0.0)
    x = (x.float() * 1.5 + randn((M, 1), 11, 2.0).float()).to(torch.bfloat16)     # a per-row offset, as residual rows carry
    st = ops.ln_stats_buffer(M, C, dev())
    ops.ln_row_stats(x, st)
    for N, gelu, seed in ((3 * C, False, 20), (4 * C, True, 30)):
        W, b = randn((N, C), seed, 1.0 / math.sqrt(C)), randn((N,), seed + 1, 0.1)
        shift, scale = randn((C,), seed + 2, 0.3), randn((C,), seed + 3, 0.3)
        Wp, cs, cv = prescale(ops, W, b, shift, scale)
        with variant(v):
            out = ops.gemm_ln(x, Wp, cs, cv, st, gelu=gelu)
        check_gemm_ln(out, x, W, Wp, b, shift, scale, f"gemm_ln M={M} N={N} gelu={gelu} variant {v}", gelu=gelu)


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("M,rps", SHAPES)
def test_site_cross_q_and_cross_proj(ops, M, rps, v):
    """cross-attention q (store-only, N = K = 1152) and its projection (residual only, gate = None, in place)."""
    a, w, b = operands(M, C, C, 40)
    res = randn((M, C), 43, 1.0, 0.5)
    x = res.clone()
    with variant(v):
        q = ops.gemm(a, w, b)
        ops.gemm(a, w, b, epilogue=ops.EPI_GATE_RES, res=x, out=x)
    check_gemm(q, a, w, b, f"cross-q M={M} variant {v}")
    check_gemm(x, a, w, b, f"cross-proj M={M} variant {v}", res=res)


MOD_ROWS = {19456: 2, 1024: 38, 2432: 2, 128: 38}


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("M,rps", SHAPES + [(38912, 1024), (4864, 128)])
def test_site_proj_gate_from_modulation_table(ops, M, rps, v):
    """Self-attention proj: x += gate_msa * proj(a), in place, gate_msa = column block 2 of a [samples, 6 C] modulation table
    (gate_stride = 6 C).  rows_per_sample: T S (config 2), S (x_mask: one gate row per frame), and their rank-of-eight forms 2432
    (straddles 256-row tiles) and 128 (a new gate row on every 128-row tile)."""
    a, w, b = operands(M, C, C, 50)
    mod = randn((MOD_ROWS[rps], 6 * C), 53, 0.5)
    res = randn((M, C), 54, 1.0, 0.25)
    x = res.clone()
    with variant(v):
        ops.gemm(a, w, b, epilogue=ops.EPI_GATE_RES, gate=mod[0, 2 * C:3 * C], gate_stride=6 * C, rows_per_sample=rps, res=x, out=x)
    check_gemm(x, a, w, b, f"proj M={M} rps={rps} variant {v}", gate=mod[0, 2 * C:], gate_stride=6 * C, rps=rps, res=res)


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("M,rps", SHAPES)
def test_site_fc2_gate_residual_with_statistics(ops, M, rps, v):
    """fc2: x += gate_mlp * fc2(h), K = 4608, through gemm_stats (the statistics-emitting epilogue the fold uses); the partials are
    the statistics of the stored rows (float64 mean / variance of every row from the combined partials)."""
    a, w, b = operands(M, C, 4 * C, 60)
    mod = randn((MOD_ROWS[rps], 6 * C), 63, 0.5)
    res = randn((M, C), 64, 1.0, -0.5)
    x = res.clone()
    st = ops.ln_stats_buffer(M, C, dev())
    st.fill_(float("nan"))
    with variant(v):
        ops.gemm_stats(a, w, b, st, gate=mod[0, 5 * C:], gate_stride=6 * C, rows_per_sample=rps, res=x, out=x)
    check_gemm(x, a, w, b, f"fc2 M={M} variant {v}", gate=mod[0, 5 * C:], gate_stride=6 * C, rps=rps, res=res)
    mean_b, m2_b = st[..., 0].double(), st[..., 1].double()
    mu = mean_b.mean(0)
    var = (m2_b.sum(0) + 96.0 * ((mean_b - mu[None]) ** 2).sum(0)) / C
    xd = x.double()
    assert torch.allclose(mu, xd.mean(1), rtol=0, atol=1e-5 * xd.abs().max().item())
    assert torch.allclose(var, xd.var(1, unbiased=False), rtol=2e-5, atol=0)


@pytest.mark.parametrize("v", [0, 8])
def test_proj_with_slab_and_pab_adds_at_config2(ops, v):
    """The PAB forms at M = 38912: the slab copy (aux = bf16(g p)) beside the gated residual, and gemm_gate_res_add with one and two
    folded broadcasts (every ``x += cached`` one more rounding)."""
    M, rps = 38912, 19456
    a, w, b = operands(M, C, C, 70)
    mod = randn((2, 6 * C), 73, 0.5)
    res = randn((M, C), 74)
    a1, a2 = randn((M, C), 75, 0.5), randn((M, C), 76, 0.5, 1.0)
    gk = dict(gate=mod[0, 2 * C:3 * C], gate_stride=6 * C, rows_per_sample=rps)
    ck = dict(gate=mod[0, 2 * C:], gate_stride=6 * C, rps=rps, res=res)
    x, aux = res.clone(), torch.full_like(res, float("nan"))
    with variant(v):
        ops.gemm(a, w, b, epilogue=ops.EPI_GATE_RES, res=x, aux=aux, out=x, **gk)
    check_gemm(x, a, w, b, f"proj + slab variant {v}", aux=aux, **ck)
    for adds in ((a1,), (a1, a2)):
        x, aux = res.clone(), torch.full_like(res, float("nan"))
        with variant(v):
            ops.gemm_gate_res_add(a, w, b, res=x, aux=aux, adds=adds, out=x, **gk)
        check_gemm(x, a, w, b, f"proj + slab + {len(adds)} PAB adds variant {v}", aux=aux, adds=adds, **ck)


# ------------------------------------------------------------------------------------------------ every branch of the shape dispatch
def dispatch_rule(M, N, K, epi, v, cu):
    """Which kernel launch_gemm (gemm_bf16.hip) picks for a store-only ("bias") or gated ("gate") epilogue — the rule restated:
    fewer than 400 tiles of 256 rows -> the 128-row geometry (launch_rows128: the three-stage ring, schedule 9, when its tile count
    fits the CUs and K / 64 >= 3, else schedule 3); otherwise variant 8 = schedule 8, and the shipped dispatch sends a store-only
    epilogue with K <= 1536 to the two-workgroup kernel and everything else to schedule 8.  (Variant 8 forces schedule 8 on these
    plain epilogues before the tile count is looked at.)"""
    if v == 8:
        return "sched8"
    if -(-M // 256) * (N // 192) < 400:
        return "rows128 ring" if -(-M // 128) * (N // 192) <= cu and K // 64 >= 3 else "rows128 sched3"
    return "gemm2" if epi == "bias" and K <= 1536 else "sched8"


def branch_cases(cu):
    # (name, M, N, K, {epilogue: expected kernel under variant 0}) — the table is asserted against dispatch_rule below
    t399 = 399 * 256
    return [
        ("256-row tiles 399", t399, 192, 64, {"bias": "rows128 sched3", "gate": "rows128 sched3"}),
        ("256-row tiles 400", t399 + 1, 192, 64, {"bias": "gemm2", "gate": "sched8"}),
        ("128-row tiles = CUs", cu * 128, 192, 192, {"bias": "rows128 ring", "gate": "rows128 ring"}),
        ("128-row tiles = CUs + 1", cu * 128 + 1, 192, 192, {"bias": "rows128 sched3", "gate": "rows128 sched3"}),
        ("K / 64 = 2", 1000, 384, 128, {"bias": "rows128 sched3", "gate": "rows128 sched3"}),
        ("K / 64 = 3", 1000, 384, 192, {"bias": "rows128 ring", "gate": "rows128 ring"}),
        ("M = 1", 1, 192, 1152, {"bias": "rows128 ring", "gate": "rows128 ring"}),
        ("M = 17", 17, 192, 1152, {"bias": "rows128 ring", "gate": "rows128 ring"}),
        ("M = 127", 127, 192, 1152, {"bias": "rows128 ring", "gate": "rows128 ring"}),
        ("M = 129", 129, 192, 1152, {"bias": "rows128 ring", "gate": "rows128 ring"}),
    ]


def test_dispatch_table_matches_rule():
    for cu in (256, 304, 80):
        for name, M, N, K, want in branch_cases(cu):
            for epi, kern in want.items():
                assert dispatch_rule(M, N, K, epi, 0, cu) == kern, (cu, name, epi)
    # both sides of each boundary land in different kernels
    cases = {c[0]: c for c in branch_cases(256)}
    for lo, hi in (("256-row tiles 399", "256-row tiles 400"), ("128-row tiles = CUs", "128-row tiles = CUs + 1"),
                   ("K / 64 = 2", "K / 64 = 3")):
        assert cases[lo][4] != cases[hi][4]


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("case", range(10))
def test_dispatch_branches(ops, case, v):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    name, M, N, K, want = branch_cases(cu)[case]
    a, w, b = operands(M, N, K, 100 + case)
    rps = max(1, M // 3 + 5)             # three samples, boundaries inside tiles
    gate = randn((3 + 1, N), 200 + case, 0.7)
    res = randn((M, N), 300 + case)
    x = res.clone()
    with variant(v):
        out = ops.gemm(a, w, b)
        ops.gemm(a, w, b, epilogue=ops.EPI_GATE_RES, gate=gate[0], gate_stride=N, rows_per_sample=rps, res=x, out=x)
    tag = f"{name} (M={M} N={N} K={K}, variant {v}: {dispatch_rule(M, N, K, 'bias', v, cu)} | {dispatch_rule(M, N, K, 'gate', v, cu)})"
    check_gemm(out, a, w, b, "store-only " + tag)
    check_gemm(x, a, w, b, "gate + residual " + tag, gate=gate, gate_stride=N, rps=rps, res=res)


# ================================================================================================ the other models' sites
# Tables, operands, references and bounds: tests/gemm_numerics_cases.py (meta-tests and planted defects: tests/test_numerics_cpu.py).
def nan_out(M, N):
    return torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def reached(M, N, K, epi, v, want=None, aux=False):
    """The kernel of this launch by the restated rule; under id 0 it must be the one the case's table promises."""
    kern = gc.kernel_of(M, N, K, epi, v, cus(), aux)
    if v == 0 and want is not None:
        assert kern == gc.expected(want, cus()), f"the table promises {gc.expected(want, cus())}, the rule gives {kern}"
    return f"id {v}: {kern}"


def test_other_models_tables_match_rule():
    gc.assert_tables_match_rule()


@pytest.mark.parametrize("case", range(len(gc.GELU_SITES)), ids=[c[0].replace(" ", "_") for c in gc.GELU_SITES])
def test_gelu_sites(ops, case):
    """EPI_BIAS_GELU (fc1 of Latte, CogVideoX, both Open-Sora-Plans, Vchitect) in the production kernel of every (N, K), on both sides of
    the K <= 1536 branch and on the few-tile kernels, with pre-activations beyond +-12 in every case."""
    name, M, N, K, want = gc.GELU_SITES[case]
    a, w, b = gc.gelu_operands(M, N, K, 400 + 3 * case, dev())
    out = nan_out(M, N)
    ops.gemm(a, w, b, epilogue=ops.EPI_BIAS_GELU, out=out)
    gc.check_gemm(out, a, w, b, f"GELU {name} ({M} x {N} x {K}, {reached(M, N, K, 'gelu', 0, want)})", gelu=True, tails=True)


_ID8 = {}


def _id8(ops, i):
    """Operands of ID_SHAPES[i] and the bits id 8 stores for them (GELU, store-only): computed once."""
    if i not in _ID8:
        M, N, K = gc.ID_SHAPES[i]
        a, w, b = gc.gelu_operands(M, N, K, 440 + i, dev())
        with variant(8):
            _ID8[i] = (a, w, b, ops.gemm(a, w, b, epilogue=ops.EPI_BIAS_GELU, out=nan_out(M, N)), ops.gemm(a, w, b, out=nan_out(M, N)))
    return _ID8[i]


@pytest.mark.parametrize("v", gc.ACCEPTED_IDS)
def test_every_accepted_id_gelu_and_store_only(ops, v):
    """Every id vsys_tune_gemm_variant accepts: GELU and store-only element-wise, and the same bits as id 8 (include/videosys_amd.h)."""
    for i, (M, N, K) in enumerate(gc.ID_SHAPES):
        a, w, b, gelu8, store8 = _id8(ops, i)
        with variant(v):
            out_g = ops.gemm(a, w, b, epilogue=ops.EPI_BIAS_GELU, out=nan_out(M, N))
            out_s = ops.gemm(a, w, b, out=nan_out(M, N))
        gc.check_gemm(out_g, a, w, b, f"GELU {M} x {N} x {K}, {reached(M, N, K, 'gelu', v)}", gelu=True, tails=True)
        gc.check_gemm(out_s, a, w, b, f"store-only {M} x {N} x {K}, {reached(M, N, K, 'bias', v)}")
        assert torch.equal(out_g, gelu8), f"id {v}: GELU bits differ from id 8 at {M} x {N} x {K}"
        assert torch.equal(out_s, store8), f"id {v}: store-only bits differ from id 8 at {M} x {N} x {K}"


@pytest.mark.parametrize("case", range(len(gc.GATE2_SMALL)), ids=[f"M{c[0]}_rps{c[1]}_split{c[2]}" for c in gc.GATE2_SMALL])
def test_two_segment_gate_small(ops, case):
    """vsys_gemm_bf16_gate2 at segment / sample boundaries inside a 16-row block, on wave and tile edges, with many samples in a wave:
    with and without bias, in place and with out / aux slab on leading dimensions of their own, under every id of GATE2_IDS (and the
    same bits as id 8).  The modulation row is gate | junk | alternative gate (gate_alt = 2 N)."""
    M, rps, split, what = gc.GATE2_SMALL[case]
    N, K = gc.GATE2_N, gc.GATE2_K
    a, w, b = gc.operands(M, N, K, 500 + 3 * case, dev())
    mod = gc.randn((-(-M // rps), 3 * N), 530 + case, dev())
    res = gc.randn((M, N), 540 + case, dev(), 1.0, 0.5)
    gate = mod[0, :N]
    for bias in (b, None):
        for slab in (False, True):
            bits8 = None
            for v in (8,) + tuple(i for i in gc.GATE2_IDS if i != 8):
                rv, rbuf = gc.padded(M, N, N + 8, dev(), res)
                (ov, obuf), (av, abuf) = (gc.padded(M, N, N + 64, dev()), gc.padded(M, N, N + 136, dev())) if slab else ((rv, rbuf), (None, None))
                with variant(v):
                    ops.gemm_gate2(a, w, bias, gate, 3 * N, rps, split, 2 * N, rv, ov, aux=av)
                tag = (f"gate2 M={M} rps={rps} split={split} bias={bias is not None} {'out + slab' if slab else 'in place'} "
                       f"({what}; {reached(M, N, K, 'gate', v, aux=slab)})")
                gc.check_gemm(ov, a, w, bias, tag, gate=gate, gate_stride=3 * N, rps=rps, seg_split=split, gate_alt=2 * N, res=res, aux=av)
                assert torch.isnan(obuf[:, N:]).all() and (abuf is None or torch.isnan(abuf[:, N:]).all()), f"{tag}: padding columns written"
                if v == 8:
                    bits8 = (ov, av)
                else:
                    assert torch.equal(ov, bits8[0]) and (av is None or torch.equal(av, bits8[1])), f"{tag}: other bits than id 8"
            if split in (0, rps):       # one segment only: ops.gemm with the gate pointer (moved on by gate_alt) stores the same bits
                x = res.clone()
                ops.gemm(a, w, bias, epilogue=ops.EPI_GATE_RES, gate=mod[0, 2 * N:] if split else gate, gate_stride=3 * N, rows_per_sample=rps,
                         res=x, out=x)
                assert torch.equal(x, bits8[0]), f"gate2 with seg_split = {split} differs from ops.gemm with the (moved) gate pointer"


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("case", range(len(gc.GATE2_PROD)), ids=[c[0].replace(" ", "_") for c in gc.GATE2_PROD])
def test_two_segment_gate_production_dispatch(ops, case, v):
    """The two-segment gate in the kernels a CogVideoX step runs (>= 400 tiles of 256 rows: schedule 8) and on the long K loop of the 5b
    fc2 on few tiles; in place, with the slab copy."""
    name, M, N, K, rps, split, want = gc.GATE2_PROD[case]
    a, w, b = gc.operands(M, N, K, 600 + 3 * case, dev())
    mod = gc.randn((-(-M // rps), 3 * N), 630 + case, dev(), 0.7)
    res = gc.randn((M, N), 640 + case, dev(), 1.0, 0.25)
    x, aux = res.clone(), nan_out(M, N)
    with variant(v):
        ops.gemm_gate2(a, w, b, mod[0, :N], 3 * N, rps, split, 2 * N, x, x, aux=aux)
    gc.check_gemm(x, a, w, b, f"gate2 {name} ({M} x {N} x {K}, rps {rps}, split {split}; {reached(M, N, K, 'gate', v, want, aux=True)})",
                  gate=mod[0, :N], gate_stride=3 * N, rps=rps, seg_split=split, gate_alt=2 * N, res=res, aux=aux)


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("rps", gc.SHORT_RPS)
@pytest.mark.parametrize("M,N,K,want", gc.SHORT_SHAPES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in gc.SHORT_SHAPES])
def test_short_samples(ops, M, N, K, want, rps, v):
    """ops.gemm(EPI_GATE_RES) with samples shorter than a wave's 64 rows (Vchitect gates per frame and per prompt), down to a gate row
    per token; the last sample is short wherever rps does not divide M."""
    a, w, b = gc.operands(M, N, K, 700 + rps, dev())
    mod = gc.randn((-(-M // rps), N), 710 + rps, dev(), 0.7)
    res = gc.randn((M, N), 720 + rps, dev(), 1.0, -0.25)
    x = res.clone()
    with variant(v):
        ops.gemm(a, w, b, epilogue=ops.EPI_GATE_RES, gate=mod[0], gate_stride=N, rows_per_sample=rps, res=x, out=x)
    gc.check_gemm(x, a, w, b, f"short samples {M} x {N} x {K} rps={rps} ({reached(M, N, K, 'gate', v, want)})", gate=mod[0], gate_stride=N, rps=rps,
                  res=res)


@pytest.mark.parametrize("v", [0, 8])
@pytest.mark.parametrize("case", range(len(gc.REMAINING)), ids=[c[0].replace(" ", "_") for c in gc.REMAINING])
def test_remaining_store_only_sites(ops, case, v):
    """The N = 192 proj_out launches (long K loops on few tiles) and the widest store-only GEMM (Open-Sora-Plan's qkv)."""
    name, M, N, K, want = gc.REMAINING[case]
    a, w, b = gc.operands(M, N, K, 800 + 3 * case, dev())
    out = nan_out(M, N)
    with variant(v):
        ops.gemm(a, w, b, out=out)
    gc.check_gemm(out, a, w, b, f"store-only {name} ({M} x {N} x {K}, {reached(M, N, K, 'bias', v, want)})")


# ------------------------------------------------------------------------------------------------ linear_small
def _acts(ops):
    return {"none": ops.ACT_NONE, "silu": ops.ACT_SILU, "gelu": ops.ACT_GELU_TANH}


@pytest.mark.parametrize("name", list(gc.LS_CASES))
def test_linear_small_elementwise(ops, name):
    """linear_small_kernel (every model's timestep embedding, caption projection and modulation table) against
    numerics.linear_small_ref; x, w and out on leading dimensions with slack, whose sentinel must keep its bits."""
    c = gc.ls_case(name, dev())
    assert c["tie"] is None or c["tie"].share() <= gc.TIE_CAP
    out, buf = c["run"](ops.linear_small, _acts(ops))
    rep = nm.Bound(f"linear_small {name} {gc.LS_CASES[name][:5]}").add(out, c["ref"], c["bound"])
    print(rep.message())
    rep.check()
    assert gc.slack_untouched(buf, c["N"]), f"linear_small {name}: the columns behind N were written"
    assert c["operands_intact"](), f"linear_small {name}: x or w (or the slack behind their rows) changed"


def test_linear_small_out_column_slice_and_row_slice_of_x(ops):
    """The ``out=`` form writing a column slice of a wider buffer, from the first rows of a taller x (norm_out's temb[:B])."""
    name = "m3_n72_k4096_silu_in"
    c = gc.ls_case(name, dev())
    M, N, K = c["M"], c["N"], c["K"]
    tall = torch.full((M + 4, K), 3.0, dtype=torch.bfloat16, device=dev())
    tall[:M] = c["x"]
    wide = torch.full((M, N + 100), gc.LS_SENTINEL, dtype=torch.bfloat16, device=dev())
    wide[:, 40:40 + N] = float("nan")
    ops.linear_small(tall[:M], c["w"], c["b"], act_in=ops.ACT_SILU, out=wide[:, 40:40 + N])
    rep = nm.Bound(f"linear_small {name}, out = a column slice, x = a row slice").add(wide[:, 40:40 + N], c["ref"], c["bound"])
    print(rep.message())
    rep.check()
    assert bool((wide[:, :40] == gc.LS_SENTINEL).all()) and bool((wide[:, 40 + N:] == gc.LS_SENTINEL).all())
