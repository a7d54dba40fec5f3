"""GPU: the kernels under the four VAE paths — conv_kernel (tap-shifted conv and the plain 128-column GEMM, csrc/conv_bf16.hip) and the
GroupNorm / SpatialNorm / softmax / first-layer kernels of csrc/vae_ops.hip — element by element against a float64 reference, each
element under the bound of its own rounding chain (tests/numerics.py; cases, operands and junk fills: tests/vae_numerics_cases.py; the
bounds' own meta-tests: tests/test_numerics_cpu.py).  Every test prints the worst |err| / bound of its family.

Shapes are the smallest that reach the branch they name (case tables in vae_numerics_cases.py), not the decoders' own."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import numerics as nm
import vae_numerics_cases as vc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def _ops():
    from videosys_amd import ops

    return ops


def _worse(a, b):
    return b if a is None or b.worst[0] > a.worst[0] else a


# ------------------------------------------------------------------------------------------------ tap-shifted conv
def run_conv(c):
    """ops.conv on a CONV_CASES entry -> the voxels of the output [n T H W, cout] on the CPU."""
    ops = _ops()
    a = vc.grid_rows(c["a_buf"].to(dev()), c["g"])
    res = vc.conv_res_rows(c, c["res_buf"].to(dev())) if c["res_buf"] is not None else None
    out = ops.conv(a, c["g"], c["w"].to(dev()), c["b"].to(dev()), c["cin"], c["kt"], c["ks"], res=res)
    torch.cuda.synchronize()
    return out, nm.grid_interior(out.cpu(), c["og"], c["cout"]).reshape(-1, c["cout"])


@pytest.mark.parametrize("name", list(vc.CONV_CASES))
def test_conv_tap_shift_elementwise(name):
    c = vc.conv_case(name)
    _, got = run_conv(c)
    rep = nm.Bound(f"conv {name} {vc.CONV_CASES[name][:9]}").add(got, c["ref"], c["bound"])
    print(rep.message())
    rep.check()


# ------------------------------------------------------------------------------------------------ gemm128
def _gemm(a, w, bias=None, res=None, **kw):
    d = lambda t: None if t is None else t.to(dev())
    out = _ops().gemm128(d(a), d(w), d(bias), d(res), **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("K", vc.GEMM_K)
def test_gemm128_elementwise_k_tiles_and_row_tails(K):
    """N = 128, every M of GEMM_M, bias and residual each on and off (K = 32: the nt == 1 prologue; 64, 96, 224: 2, 3, 7 k-tiles, where the
    three-slot A ring and the two-slot W ring wrap at different periods; 4096: the T5 feed-forward width)."""
    worst = None
    for M in vc.GEMM_M:
        a, w, b, r = vc.gemm_operands(M, 128, K, 1000 * K + M)
        for bias, res in ((None, None), (b, None), (None, r), (b, r)):
            ref, bound = nm.linear_ref(a, w, bias, res)
            rep = nm.Bound(f"gemm128 M={M} N=128 K={K} bias={bias is not None} res={res is not None}").add(_gemm(a, w, bias, res), ref, bound)
            rep.check()
            worst = _worse(worst, rep)
    print(worst.message())


def test_gemm128_elementwise_three_column_tiles_and_strided_out():
    worst = None
    for K, M in vc.GEMM_THIN:
        a, w, b, r = vc.gemm_operands(M, 384, K, 77 * K + M)
        ref, bound = nm.linear_ref(a, w, b, r)
        rep = nm.Bound(f"gemm128 M={M} N=384 K={K}").add(_gemm(a, w, b, r), ref, bound)
        rep.check()
        worst = _worse(worst, rep)
    # a strided out (ldo > N): columns 64 .. 191 of a 320-wide tensor; the columns beside them keep their fill
    M, K = 257, 96
    a, w, b, r = vc.gemm_operands(M, 128, K, 5)
    wide = torch.full((M, 320), vc.DST_FILL, dtype=BF, device=dev())
    _ops().gemm128(a.to(dev()), w.to(dev()), b.to(dev()), out=wide[:, 64:192])
    torch.cuda.synchronize()
    wide = wide.cpu()
    ref, bound = nm.linear_ref(a, w, b)
    rep = nm.Bound("gemm128 strided out").add(wide[:, 64:192], ref, bound)
    rep.check()
    assert bool((wide[:, :64] == vc.DST_FILL).all()) and bool((wide[:, 192:] == vc.DST_FILL).all())
    print(_worse(worst, rep).message())


@pytest.mark.parametrize("M", [128, 100])
def test_gemm128_elementwise_broadcast_batch(M):
    """batch = 3 with batch_a = 0 (V^T = W_v X^T of the mid-block attention) at a whole and at a ragged M: a batch entry's output ends
    where the next one's begins, so a row stored past M would land in the neighbour (or, after the last, in the fill behind it)."""
    nb, L, C = 3, 256, 64
    gen = torch.Generator().manual_seed(M)
    wv = torch.randn(M, C, generator=gen).to(BF)
    x = torch.randn(nb, L, C, generator=gen).to(BF)
    out = torch.full((nb * M + 64, L), vc.DST_FILL, dtype=BF, device=dev())
    _ops().gemm128(wv.to(dev()), x.to(dev()), out=out[:nb * M].view(nb, M, L), batch=nb, batch_a=0, batch_w=L * C, batch_o=M * L, M=M)
    torch.cuda.synchronize()
    out = out.cpu()
    rep = nm.Bound(f"gemm128 batch=3 batch_a=0 M={M}")
    for i in range(nb):
        ref, bound = nm.linear_ref(wv, x[i])
        rep.add(out[i * M:(i + 1) * M], ref, bound, row0=i * M)
    print(rep.message())
    rep.check()
    assert bool((out[nb * M:] == vc.DST_FILL).all())


def score_case():
    """The fp32 score form of the mid-block attention: L = 200 query rows of frames padded to Lp = 256, out_scale = 0.125."""
    nb, L, Lp, C = 2, 200, 256, 64
    gen = torch.Generator().manual_seed(200)
    q = torch.randn(nb, Lp, C, generator=gen).to(BF)
    k = torch.randn(nb, Lp, C, generator=gen).to(BF)
    return nb, L, Lp, C, q, k


def run_scores():
    nb, L, Lp, C, q, k = score_case()
    s = torch.full((nb, Lp, Lp), vc.DST_FILL, dtype=torch.float32, device=dev())
    _ops().gemm128(q.to(dev()), k.to(dev()), out_f32=s, out_scale=0.125, batch=nb, batch_a=Lp * C, batch_w=Lp * C, batch_o=Lp * Lp, M=L)
    torch.cuda.synchronize()
    return s.cpu()


def check_scores(s, what):
    nb, L, Lp, C, q, k = score_case()
    rep = nm.Bound(what)
    for i in range(nb):
        ref, bound = nm.linear_ref(q[i, :L], k[i], out_scale=0.125)
        rep.add(s[i, :L], ref, bound, row0=i * Lp)
    rep.check()
    assert bool((s[:, L:] == vc.DST_FILL).all()), f"{what}: rows behind M were written"
    return rep


def test_gemm128_elementwise_fp32_scores_and_split_k():
    rep = check_scores(run_scores(), "gemm128 fp32 scores, out_scale 0.125, 200 of 256 rows")
    # the K= sub-range form (ops.linear_skinny, the T5 encoder's few-row linears: one K slice per batch entry, fp32 partials)
    N, Mp, K, nsplit = 128, 128, 256, 4
    Ks = K // nsplit
    w, x, _, _ = vc.gemm_operands(N, Mp, K, 9)       # (the WEIGHT is the row operand there)
    part = torch.empty(nsplit, N, Mp, dtype=torch.float32, device=dev())
    _ops().gemm128(w.to(dev()), x.to(dev()), out_f32=part, batch=nsplit, batch_a=Ks, batch_w=Ks, batch_o=N * Mp, M=N, K=Ks)
    torch.cuda.synchronize()
    part = part.cpu()
    rep2 = nm.Bound("gemm128 K= sub-range (split-K partials)")
    for i in range(nsplit):
        ref, bound = nm.linear_ref(w[:, i * Ks:(i + 1) * Ks], x[:, i * Ks:(i + 1) * Ks], out_scale=1.0)
        rep2.add(part[i], ref, bound, row0=i * N)
    rep2.check()
    print(_worse(rep, rep2).message())


# ------------------------------------------------------------------------------------------------ GroupNorm / SpatialNorm
def _norm_check(c, y_after, what):
    C, gd, r = c["C"], c["gd"], c["r"]
    got = nm.grid_interior(vc.grid_rows(y_after, gd), gd).reshape(-1, C)
    rep = nm.Bound(what)
    for r0, r1 in nm.row_chunks(got.shape[0], 1 << 15):
        rep.add(got[r0:r1], r.ref.reshape(-1, C)[r0:r1], r.bound.reshape(-1, C)[r0:r1], row0=r0)
    print(rep.message())
    rep.check()
    assert vc.outside_interior_unchanged(y_after, c["y_buf"], gd, C), f"{what}: the destination changed outside its interior"


@pytest.mark.parametrize("name", list(vc.GN_CASES))
def test_group_norm_elementwise(name):
    ops = _ops()
    c = vc.gn_case(name, ops._GN_NBLK)
    x_buf, y_buf = c["x_buf"].to(dev()), c["y_buf"].to(dev())
    ops.group_norm(vc.grid_rows(x_buf, c["gs"]), c["gs"], vc.grid_rows(y_buf, c["gd"]), c["gd"], c["C"], c["gamma"].to(dev()), c["beta"].to(dev()),
                   vc.GN_EPS, c["silu"], groups=c["groups"])
    torch.cuda.synchronize()
    if name == "offset_mean8":
        print(f"offset case: the rstd (cancellation) term takes up to {c['r'].cancel_share():.3f} of an element's bound at {c['r'].n_t} positions "
              f"per thread (a 64-frame decode has thousands: not covered here)")
    _norm_check(c, y_buf.cpu(), f"group norm {name} {vc.GN_CASES[name][:6]} silu={c['silu']}")


def _run_spatial_norm(c, what):
    ops = _ops()
    C = c["C"]
    x_buf, y_buf = c["x_buf"].to(dev()), c["y_buf"].to(dev())
    ops.spatial_norm_silu(vc.grid_rows(x_buf, c["gs"]), c["gs"], vc.grid_rows(y_buf, c["gd"]), c["gd"], C, c["gamma"].to(dev()), c["beta"].to(dev()),
                          c["yb"].to(dev()), c["zdims"])
    torch.cuda.synchronize()
    _norm_check(c, y_buf.cpu(), what)


@pytest.mark.parametrize("T,zT,C", vc.SN_CASES)
def test_spatial_norm_silu_elementwise(T, zT, C):
    _run_spatial_norm(vc.sn_case(T, zT, C, _ops()._GN_NBLK), f"spatial norm n=2 T={T} zT={zT} C={C}")


def test_spatial_norm_silu_grid_stride_lap():
    """More image rows (2 x 32776) than the 65536 blocks of spatial_norm_apply_kernel's grid: the last 16 rows are a block's second lap."""
    _run_spatial_norm(vc.sn_case(nblk=_ops()._GN_NBLK, **vc.SN_LAP), "spatial norm, 65 552 image rows")


# ------------------------------------------------------------------------------------------------ softmax_rows, first layer
@pytest.mark.parametrize("case", vc.SOFTMAX_CASES, ids=lambda c: f"{c[0]}x{c[1]}of{c[2]}")
def test_softmax_rows_elementwise(case):
    rows, n, ld, kinds = case
    s = vc.softmax_scores(rows, n, ld, kinds)
    p = _ops().softmax_rows(s.to(dev()), n=n)
    torch.cuda.synchronize()
    rep = vc.check_softmax(p.cpu(), s, n, f"softmax_rows {rows} x {n} of {ld} ({kinds})")
    print(rep.message())


@pytest.mark.parametrize("kt,kcols", [(3, 128), (1, 64)])
def test_first_layer_elementwise(kt, kcols):
    z, params, ref, bound, mask = vc.first_case(kt, kcols)
    out = _ops().vae_first_im2col(z.to(dev()), kt, kcols, params)
    torch.cuda.synchronize()
    rep = vc.check_first(out.cpu(), ref, bound, mask, f"first layer kt={kt} kcols={kcols}")
    print(rep.message())


# ------------------------------------------------------------------------------------------------ the 32x32x16 fallback form
FALLBACK_CONV = "27taps_M312"
FALLBACK_GEMM = (257, 128, 96)


def fallback_outputs():
    """Three conv / gemm128 launches from fixed seeds: a 27-tap conv with residual, a bias + residual GEMM with a row tail, the fp32 scores."""
    _, conv = run_conv(vc.conv_case(FALLBACK_CONV))
    a, w, b, r = vc.gemm_operands(*FALLBACK_GEMM, 31)
    return dict(conv=conv, gemm=_gemm(a, w, b, r), scores=run_scores())


def test_fallback_mfma_form_gives_the_same_bits():
    """VSYS_GEMM_MF16=0 selects conv_kernel<*, 0> (32x32x16 MFMA); it is read once per process, so one fresh child interpreter runs the three
    launches with it set.  Same bits as the default form, and the child's outputs pass the same element-wise bounds."""
    mine = fallback_outputs()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fallback.pt")
        env = dict(os.environ, VSYS_GEMM_MF16="0")
        # the limit is the child's own: a cold interpreter + torch + library load (tens of seconds at worst) and three small launches
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fallback-child", path], env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        theirs = torch.load(path)
    assert theirs["mf16_env"] == "0"
    for k in mine:
        assert torch.equal(mine[k], theirs[k]), f"{k}: the 32x32x16 form differs from the 16x16x32 form"
    c = vc.conv_case(FALLBACK_CONV)
    rep = nm.Bound("fallback conv").add(theirs["conv"], c["ref"], c["bound"])
    rep.check()
    a, w, b, r_ = vc.gemm_operands(*FALLBACK_GEMM, 31)
    rep2 = nm.Bound("fallback gemm128").add(theirs["gemm"], *nm.linear_ref(a, w, b, r_))
    rep2.check()
    rep3 = check_scores(theirs["scores"], "fallback fp32 scores")
    print(_worse(_worse(rep, rep2), rep3).message())


if __name__ == "__main__":      # the child of test_fallback_mfma_form_gives_the_same_bits
    assert sys.argv[1] == "--fallback-child"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = fallback_outputs()
    res["mf16_env"] = os.environ.get("VSYS_GEMM_MF16")
    torch.save(res, sys.argv[2])
