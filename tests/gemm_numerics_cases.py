"""TEST INFRASTRUCTURE: the cases of the GEMM family's element-wise checks beyond what STDiT3 launches — the sites of Latte, CogVideoX,
Open-Sora-Plan v1.1 / v1.2 and Vchitect-2.0 on gemm_bf16.hip / gemm2_bf16.hip and linear_small_kernel.  Importable without a GPU: every
function works on the device of the tensors it is handed.  tests/test_gpu_numerics_gemm.py runs the HIP kernels on these tables,
tests/test_numerics_cpu.py the restatements of tests/gemm_cpu_emul.py (and their planted defects) on scaled-down rows of them.

Rounding chains (tests/numerics.py; the reference = the model run in bf16, every term a worst case):
  * store-only        bf16(a W^T + b)                          acc(K, s + |b|) + rnd(p)
  * GELU (fc1)        bf16(gelu_tanh(bf16(a W^T + b)))         d = acc(K, s + |b|) + rnd(p);  the IMAGE of [p - d, p + d] under gelu_tanh
                                                               (numerics.act_image) + rnd(gelu) + 2^-16 |gelu| (the fast exp2 / reciprocal)
  * gate + residual   bf16(x + bf16(g_r bf16(a W^T + b)))      |g_r| (acc + rnd(p)) + rnd(g_r p) + rnd(x + g_r p);  aux slab = bf16(g_r p);
                      g_r = the gate row of token r (row_gates: sample r // rows_per_sample, the alternative vector gate_alt elements on
                      for the first seg_split rows of a sample — CogVideoX's text tokens)
  * linear_small      numerics.linear_small_ref

GELU operands: row r of A is scaled by (1, 1, 4, 16)[r % 4], so that every case holds pre-activations beyond +-12, where exp2 in the
kernels' gelu_tanh overflows to +inf and the result must be -0 (or p itself on the positive side): asserted on the float64 reference
before the kernel's output is looked at.  The image bound is tight there (the slope is next to zero), where a global slope 1.13 would
allow 1.13 2^-8 |p| = 0.05 around a value that must be 0.

Near-tie shares of the linear_small cases whose input goes through SiLU (numerics.Tie; a condition on the INPUTS, asserted <= TIE_CAP by
tests/test_numerics_cpu.py): 0 at K = 8 (the seeds are searched for it), 0.1 - 0.3 % at K >= 256.
"""
import functools
import math

import torch

import numerics as nm

BF = torch.bfloat16
CHUNK = 4096
TIE_CAP = 0.05
FAST_MATH = 2.0**-16        # the GELU epilogue's exp2 + reciprocal, relative to the output (as tests/test_gpu_numerics_gemm.py has it)
TAIL = 12.0                 # |p| from which the exp2 of gelu_tanh has left fp32's range on the negative side
ROW_SCALE = (1.0, 1.0, 4.0, 16.0)

ACCEPTED_IDS = (0, 3, 6, 8, 9, 16, 20, 24, 28, 30, 34, 103, 106, 113, 118, 119)
GATE2_IDS = (0, 8, 16, 20, 24, 103, 113, 119)


# ------------------------------------------------------------------------------------------------ operands
def randn(shape, seed, device, scale=1.0, offset=0.0):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=device) * scale + offset).to(BF)


def operands(M, N, K, seed, device):
    return randn((M, K), seed, device), randn((N, K), seed + 1, device, 1.0 / math.sqrt(K)), randn((N,), seed + 2, device, 0.1)


def gelu_operands(M, N, K, seed, device):
    """operands() with row r of A scaled by ROW_SCALE[r % 4] (powers of two: exact in bf16)."""
    a, w, b = operands(M, N, K, seed, device)
    sc = torch.tensor(ROW_SCALE, device=device)[torch.arange(M, device=device) % 4]
    return (a.float() * sc[:, None]).to(BF), w, b


def padded(rows, cols, ld, device, src=None, fill=float("nan")):
    """A [rows, cols] view of a fresh [rows, ld] buffer filled with ``fill`` (NaN: an output the epilogue does not read), holding ``src``."""
    buf = torch.full((rows, ld), fill, dtype=BF, device=device)
    if src is not None:
        buf[:, :cols] = src
    return buf[:, :cols], buf


# ------------------------------------------------------------------------------------------------ references
def row_gates(gate, gate_stride, rows_per_sample, seg_split, gate_alt, r0, r1, N):
    """Gate of rows r0 .. r1-1, float64 [r1 - r0, N]: row r of sample b = r // rows_per_sample reads gate + b gate_stride, and gate_alt
    elements further on when seg_split > 0 and r - b rows_per_sample < seg_split.  ``gate`` is a view that starts at sample 0's vector."""
    ns = -(-r1 // rows_per_sample)
    r = torch.arange(r0, r1, device=gate.device)
    b = r // rows_per_sample
    g = torch.as_strided(gate, (ns, N), (gate_stride, 1)).double()[b]
    if seg_split > 0:
        alt = torch.as_strided(gate, (ns, N), (gate_stride, 1), gate.storage_offset() + gate_alt).double()[b]
        g = torch.where((r - b * rows_per_sample < seg_split)[:, None], alt, g)
    return g


def gemm_bounds(out, x, w, b, what, *, gelu=False, gate=None, gate_stride=0, rps=0, seg_split=0, gate_alt=0, res=None, aux=None,
                tails=False):
    """The Bound objects (output, then the aux slab if any) of one GEMM site against its float64 reference, chunk by chunk over the
    rows.  ``tails``: assert on the reference that the case holds p <= -TAIL and p >= TAIL before ``out`` is looked at."""
    M, K = x.shape
    N = w.shape[0]
    bd = b.double() if b is not None else torch.zeros(N, dtype=torch.float64, device=x.device)
    refs = []
    lo, hi = float("inf"), float("-inf")
    for r0, r1 in nm.row_chunks(M, CHUNK):
        p, s = nm.matmul_ref(x[r0:r1], w)
        p = p + bd
        e = nm.acc(K, s + bd.abs())
        u = eu = None
        if gelu:
            lo, hi = min(lo, float(p.min())), max(hi, float(p.max()))
            ref, img = nm.act_image("gelu", p, e + nm.rnd(p))
            bound = img + nm.rnd(ref) + FAST_MATH * ref.abs()
        elif res is None:
            ref, bound = p, e + nm.rnd(p)
        else:
            if gate is not None:
                g = row_gates(gate, gate_stride, rps, seg_split, gate_alt, r0, r1, N)
                u, eu = g * p, g.abs() * (e + nm.rnd(p)) + nm.rnd(g * p)
            else:
                u, eu = p, e + nm.rnd(p)
            ref = res[r0:r1].double() + u
            bound = eu + nm.rnd(ref)
        refs.append((r0, r1, ref, bound, u, eu))
    if tails:
        assert gelu and lo <= -TAIL and hi >= TAIL, f"{what}: the case does not reach the tails of gelu_tanh (p in [{lo:.3g}, {hi:.3g}])"
    rep, rep_aux = nm.Bound(what), nm.Bound(what + " [aux slab]")
    for r0, r1, ref, bound, u, eu in refs:
        rep.add(out[r0:r1], ref, bound, r0)
        if aux is not None:
            rep_aux.add(aux[r0:r1], u, eu, r0)
    return [rep] + ([rep_aux] if aux is not None else [])


def check_gemm(out, x, w, b, what, **kw):
    """gemm_bounds, printed (the worst |err| / bound of every output) and asserted."""
    reps = gemm_bounds(out, x, w, b, what, **kw)
    for rep in reps:
        print(rep.message())
    for rep in reps:
        rep.check()
    return reps


# ------------------------------------------------------------------------------------------------ which kernel a launch reaches
def dispatch_rule(M, N, K, epi, cu):
    """launch_gemm's shape dispatch (gemm_bf16.hip, id 0) restated for a store-only ("bias"), GELU ("gelu") or gated ("gate") epilogue:
    fewer than 400 tiles of 256 rows -> the 128-row geometry (the three-stage ring when its tile count fits the CUs and K / 64 >= 3, else
    schedule 3); otherwise an un-gated epilogue with K <= 1536 -> the two-workgroup kernel, everything else schedule 8."""
    if -(-M // 256) * (N // 192) < 400:
        return "rows128 ring" if -(-M // 128) * (N // 192) <= cu and K // 64 >= 3 else "rows128 sched3"
    return "gemm2" if epi != "gate" and K <= 1536 else "sched8"


def kernel_of(M, N, K, epi, v, cu, aux=False):
    """The kernel id ``v`` of vsys_tune_gemm_variant selects at this launch (the switch of launch_gemm restated).  Id 0 is the shape
    dispatch, whose kernels are the 16x16x32 forms; of the forced ids the 32x32x16 forms are marked mf32, the others are 16x16x32."""
    gated = epi == "gate"
    fixed = {3: "sched3 mf32", 6: "sched6 mf32", 8: "sched8 mf32", 9: "sched8 mf32 row-major", 16: "sched8", 20: "gemm2 mf32",
             103: "rows128 sched3 mf32", 106: "rows128 sched6 mf32", 113: "rows128 sched3", 118: "rows128 sched8", 119: "rows128 ring"}
    if v == 0:
        return dispatch_rule(M, N, K, epi, cu)
    if v in fixed:
        return fixed[v]
    if v == 24:
        return "sched8" if gated and aux else "gemm2"
    if v == 28:
        return "sched8 mf32" if gated else "sched8 mf32 + producers"
    if v == 30:
        return "gemm2 mf32 256x384" if N % 384 == 0 else "sched8 mf32"
    if v == 34:
        return "gemm2 256x384" if N % 384 == 0 and not (gated and aux) else "sched8"
    raise KeyError(v)


def _ring(tiles128):
    """Expected kernel of a few-tile case with K / 64 >= 3: the ring where the 128-row tiles fit the CUs."""
    return lambda cu: "rows128 ring" if tiles128 <= cu else "rows128 sched3"


def expected(want, cu):
    return want(cu) if callable(want) else want


# (name, M, N, K, kernel under id 0): the GELU sites at the smallest M that lands in the production kernel of (N, K), both sides of the
# K <= 1536 branch, and the few-tile side of fc1 at C = 1152.  M = 1600 is the site's; 1613 repeats it ragged against 64 rows.
GELU_SITES = [
    ("Latte / Vchitect fc1", 4300, 4608, 1152, "gemm2"),
    ("CogVideoX-2b fc1", 2400, 7680, 1920, "sched8"),
    ("Open-Sora-Plan fc1", 2100, 9216, 2304, "sched8"),
    ("CogVideoX-5b fc1", 1600, 12288, 3072, "sched8"),
    ("CogVideoX-5b fc1, ragged", 1613, 12288, 3072, "sched8"),
    ("K = 1536", 4300, 4608, 1536, "gemm2"),
    ("K = 1600", 4300, 4608, 1600, "sched8"),
    ("fc1 on few tiles", 700, 4608, 1152, _ring(6 * 24)),
    ("fc1, more 128-row tiles than CUs", 1700, 4608, 1152, "rows128 sched3"),
]
ID_SHAPES = [(515, 384, 192), (300, 192, 64)]
# (M, rows_per_sample, seg_split, what it reaches) at N = 384, K = 128
GATE2_N, GATE2_K = 384, 128
GATE2_SMALL = [
    (600, 300, 226, "the boundary two rows into a 16-row block of a wave"),
    (515, 256, 64, "segment and sample boundaries on wave and tile edges: one gate row per wave, with and without the alternative"),
    (515, 100, 40, "the shape of test_gpu_epilogue_bits.py"),
    (130, 7, 3, "many samples inside one wave"),
    (257, 257, 0, "all rows take the plain gate"),
    (257, 257, 257, "all rows take the alternative gate"),
]
# (name, M, N, K, rows_per_sample, seg_split, kernel under id 0)
GATE2_PROD = [
    ("400 tiles", 102401, 192, 64, 1576, 226, "sched8"),
    ("CogVideoX-2b out-proj", 10252, 1920, 1920, 5126, 226, "sched8"),
    ("CogVideoX-2b fc2", 10252, 1920, 7680, 5126, 226, "sched8"),
    ("CogVideoX-5b fc2 on few tiles", 1100, 3072, 12288, 550, 226, _ring(9 * 16)),
]
SHORT_RPS = (1, 7, 77, 100)     # Vchitect gates per frame and per prompt; the last sample is short wherever rps does not divide M
SHORT_SHAPES = [(300, 384, 128, "rows128 sched3"), (102401, 192, 64, "sched8")]
# (name, M, N, K, kernel under id 0), store-only
REMAINING = [
    ("CogVideoX-2b proj_out", 5126, 192, 1920, _ring(41)),
    ("Open-Sora-Plan proj_out", 2100, 192, 2304, _ring(17)),
    ("Open-Sora-Plan qkv", 2100, 6912, 2304, "rows128 sched3"),
]


def table_rows():
    """Every (M, N, K, epilogue, expected kernel under id 0) the tables above promise."""
    rows = [(M, N, K, "gelu", want) for _, M, N, K, want in GELU_SITES]
    rows += [(M, N, K, "gate", want) for _, M, N, K, _, _, want in GATE2_PROD]
    rows += [(M, N, K, "gate", want) for M, N, K, want in SHORT_SHAPES]
    rows += [(M, GATE2_N, GATE2_K, "gate", "rows128 sched3") for M, _, _, _ in GATE2_SMALL]
    rows += [(M, N, K, "bias", want) for _, M, N, K, want in REMAINING]
    rows += [(515, 384, 192, e, "rows128 ring") for e in ("bias", "gelu")] + [(300, 192, 64, e, "rows128 sched3") for e in ("bias", "gelu")]
    return rows


def assert_tables_match_rule():
    """Every table row names the kernel the restated dispatch rule gives it, on 80, 256 and 304 CUs; every M is ragged against the 256-
    and 128-row tiles and — but for the CogVideoX-5b site's own 1600, which 1613 repeats — against a wave's 64 rows."""
    for cu in (80, 256, 304):
        for M, N, K, epi, want in table_rows():
            assert dispatch_rule(M, N, K, epi, cu) == expected(want, cu), (cu, M, N, K, epi)
            assert kernel_of(M, N, K, epi, 0, cu) == expected(want, cu)
    for M, N, K, epi, want in table_rows():
        assert M % 256 and M % 128 and (M % 64 or M == 1600), (M, N, K)
    site = {name: want for name, _, _, _, want in GELU_SITES}
    assert site["K = 1536"] != site["K = 1600"]                                       # both sides of the K <= 1536 branch
    assert expected(site["fc1 on few tiles"], 256) != site["fc1, more 128-row tiles than CUs"]
    for v in ACCEPTED_IDS:                                                            # every id has a restated kernel at every ID_SHAPES launch
        for M, N, K in ID_SHAPES:
            assert kernel_of(M, N, K, "gelu", v, 256)


# ------------------------------------------------------------------------------------------------ linear_small
# name: (M, N, K, act_in, act_out, bias).  M in {1, 2, 3, 600}, N in {1, 3, 5, 72, 1152} ((M N) % 4 != 0 reaches the tail waves that
# return early), K in {8, 256, 512, 520, 4096} (one lane active | one full pass | one lane with a second pass), every (act_in, act_out)
# pair a model uses.  Every operand and the output sit in buffers with slack behind the row (ldx = K + 8, ldw = K + 16, ldo = N + 3).
LS_CASES = {
    "m1_n1_k8": (1, 1, 8, "none", "none", True),
    "m1_n3_k8_silu_in": (1, 3, 8, "silu", "none", True),
    "m3_n5_k8_silu_in": (3, 5, 8, "silu", "none", False),
    "m2_n72_k8_silu_out": (2, 72, 8, "none", "silu", True),
    "m2_n3_k256_gelu": (2, 3, 256, "none", "gelu", True),
    "m3_n1_k256_silu_in": (3, 1, 256, "silu", "none", True),
    "m1_n1152_k256_silu_out": (1, 1152, 256, "none", "silu", True),
    "m3_n5_k512_silu_out": (3, 5, 512, "none", "silu", True),
    "m2_n5_k512_silu_in": (2, 5, 512, "silu", "none", True),
    "m2_n5_k520": (2, 5, 520, "none", "none", False),
    "m3_n5_k520_silu_in": (3, 5, 520, "silu", "none", True),
    "m2_n1152_k520_gelu": (2, 1152, 520, "none", "gelu", True),
    "m3_n72_k4096_silu_in": (3, 72, 4096, "silu", "none", True),
    "m3_n5_k4096_gelu": (3, 5, 4096, "none", "gelu", True),
    "m600_n5_k8": (600, 5, 8, "none", "none", True),
    "m600_n72_k256_silu_out": (600, 72, 256, "none", "silu", True),
    "m600_n1152_k4096_gelu": (600, 1152, 4096, "none", "gelu", True),       # the caption projection's fc1
    "modulation_table": (2, 6 * 1152 * 5, 1152, "silu", "none", True),        # _mod.weight: N = (2 L + 1) 6 C at L = 2
}
LS_SENTINEL = -7.25


def _ls_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 2).to(BF)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    b = (torch.randn(N, generator=g) * 0.5).to(BF)
    return x, w, b


@functools.lru_cache(maxsize=None)
def _ls_cpu(name):
    """CPU operands of a case.  Where SiLU is applied to few inputs (M K <= 64: one flagged element would already be several per cent)
    the seed is the first from the case's own on whose x no element is flagged by the near-tie rule."""
    M, N, K, act_in, act_out, bias = LS_CASES[name]
    seed = sum((i + 1) * ord(ch) for i, ch in enumerate(name))
    while True:
        x, w, b = _ls_operands(M, N, K, seed)
        if act_in != "silu" or M * K > 64:
            break
        v = nm.silu64(x.double())
        if nm.Tie(v, v.abs() * (nm.U_LIBM + nm.U_RCP + 3 * nm.U_F32)).share() == 0.0:
            break
        seed += 1
    return x, w, b if bias else None


def ls_case(name, device="cpu", max_rows=None, max_cols=None):
    """x, w, bias as strided views on ``device`` (slack columns hold the sentinel), ref / bound / tie (float64 on ``device``) and
    ``run(linear_small, acts) -> (out view, whole out buffer)`` with NaN in the output and the sentinel behind every row.  ``max_rows`` /
    ``max_cols``: the first rows of x / of w only (the CPU restatements' scaled-down form of the same operands)."""
    M, N, K, act_in, act_out, _ = LS_CASES[name]
    x, w, b = (t.to(device) if t is not None else None for t in _ls_cpu(name))
    if max_rows is not None and M > max_rows:
        M, x = max_rows, x[:max_rows].contiguous()
    if max_cols is not None and N > max_cols:
        N, w, b = max_cols, w[:max_cols].contiguous(), b[:max_cols].contiguous() if b is not None else None
    xv, xbuf = padded(M, K, K + 8, device, x, LS_SENTINEL)
    wv, wbuf = padded(N, K, K + 16, device, w, LS_SENTINEL)
    ref, bound, tie = nm.linear_small_ref(x, w, b, act_in, act_out)

    def run(linear_small, acts):
        ov, obuf = padded(M, N, N + 3, device, fill=LS_SENTINEL)
        ov.fill_(float("nan"))
        linear_small(xv, wv, b, act_in=acts[act_in], act_out=acts[act_out], out=ov)
        return ov, obuf

    def operands_intact():
        """x and w hold their values and the sentinel behind every row after the launch."""
        return torch.equal(xv, x) and torch.equal(wv, w) and slack_untouched(xbuf, K) and slack_untouched(wbuf, K)

    return dict(M=M, N=N, K=K, act_in=act_in, act_out=act_out, x=xv, w=wv, b=b, ref=ref, bound=bound, tie=tie, run=run, operands_intact=operands_intact)


def slack_untouched(buf, cols):
    return bool((buf[:, cols:] == LS_SENTINEL).all())
