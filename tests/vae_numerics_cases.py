"""TEST INFRASTRUCTURE: the cases of the VAE element-wise checks — shapes, seeded bf16 operands on the CPU, padded storage with junk
where the contract says nothing is read, and the float64 reference + bound of tests/numerics.py.  tests/test_gpu_numerics_vae.py runs
the HIP kernels on them, tests/test_numerics_cpu.py the restatements of tests/vae_cpu_emul.py (and their planted defects).

Storage of a grid (ops.VaeGrid.alloc): [guard + rows + guard, C].  The guard rows hold GUARD_JUNK (large, finite: a conv reads them only
for the border rows of its output, which nobody compares); rows and columns the contract calls never read hold UNREAD; the border
pixels and front frames of a CONV INPUT are zero (they are the convolution's padding)."""
import math

import torch

import numerics as nm

GUARD_JUNK = 1.0e4
UNREAD = 3.0
BF = torch.bfloat16


def _grid(*a, **k):
    from videosys_amd.ops import VaeGrid

    return VaeGrid(*a, **k)


def storage(x5, g, border, lda=None):
    """x5 [n, T, H, W, C] -> bf16 storage [guard + rows + guard, lda] of grid g: voxels = x5, border pixels and front frames = ``border``,
    slack rows and columns C.. = UNREAD, guard rows = GUARD_JUNK."""
    C = x5.shape[-1]
    lda = C if lda is None else lda
    buf = torch.full((g.rows + 2 * g.guard, lda), GUARD_JUNK, dtype=BF)
    rows = buf[g.guard:g.guard + g.rows]
    rows.fill_(UNREAD)
    v = rows.view(g.n, g.sample_rows, lda)[:, :(g.T + g.tf) * g.plane].view(g.n, g.T + g.tf, g.Hp, g.Wp, lda)
    v[..., :C] = border
    v[:, g.tf:, g.pad:g.pad + g.H, g.pad:g.pad + g.W, :C] = x5.to(BF)
    return buf


def grid_rows(buf, g):
    return buf[g.guard:g.guard + g.rows]


def outside_interior_unchanged(after, before, g, C):
    """True when storage ``after`` equals ``before`` everywhere but on the voxels of grid g (first C columns)."""
    a, b = after.clone(), before.clone()
    for t in (a, b):
        rows = grid_rows(t, g)
        v = rows.view(g.n, g.sample_rows, -1)[:, :(g.T + g.tf) * g.plane].view(g.n, g.T + g.tf, g.Hp, g.Wp, -1)
        v[:, g.tf:, g.pad:g.pad + g.H, g.pad:g.pad + g.W, :C] = 0
    return torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ tap-shifted conv
#             n, T, H,  W,  cin, cout, kt, ks, res,   pad, lda,  res_wide
CONV_CASES = {
    "M35_9tiles":       (1, 1, 5, 3, 32, 128, 1, 3, False, 1, None, False),    # one partial row tile, cshift = 0, 9 k-tiles
    "two_samples":      (2, 1, 9, 7, 64, 256, 1, 3, True, 1, None, True),      # two samples, two column tiles, M = 198; residual = a column slice
    "27taps_M312":      (1, 2, 10, 11, 32, 128, 3, 3, True, 1, None, False),   # two row tiles with a ragged tail
    "cshift2_108tiles": (1, 3, 6, 5, 128, 256, 3, 3, False, 1, None, False),
    "time_only_pad0":   (1, 4, 4, 4, 256, 128, 3, 1, True, 0, None, False),    # kt = 3, ks = 1: taps_hw = 1
    "time_only_pad1":   (1, 3, 5, 5, 512, 128, 3, 1, False, 1, None, False),
    "xcd_27tiles":      (1, 1, 46, 46, 32, 384, 1, 3, False, 1, None, False),  # 9 row tiles x 3 column tiles
    "lda_gt_cin":       (1, 1, 6, 5, 64, 128, 1, 3, False, 1, 128, False),     # cin = 64 read from 128-wide rows (the wrapper allows it; no caller in the product does it)
}


def conv_case(name):
    """Operands (CPU bf16), grids, float64 reference and bound [n T H W, cout] of one CONV_CASES entry."""
    n, T, H, W, cin, cout, kt, ks, has_res, pad, lda, res_wide = CONV_CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    K = cin * kt * ks * ks
    x5 = torch.randn(n, T, H, W, cin, generator=gen).to(BF)
    w = (torch.randn(cout, K, generator=gen) / math.sqrt(K)).to(BF)
    b = (0.5 * torch.randn(cout, generator=gen)).to(BF)
    g = _grid(n, T, H, W, pad, kt - 1)
    og = g.conv_out()
    a_buf = storage(x5, g, border=0.0, lda=lda)
    res_buf = res_cols = None
    r5 = None
    if has_res:
        r5 = torch.randn(n, T, H, W, cout, generator=gen).to(BF)
        res_buf = storage(r5, og, border=UNREAD)
        if res_wide:      # the residual as a column slice of a wider tensor: its own row stride
            wide = torch.full((res_buf.shape[0], cout + 192), GUARD_JUNK, dtype=BF)
            wide[:, 64:64 + cout] = res_buf
            res_buf, res_cols = wide, (64, 64 + cout)
    A = nm.conv_gather(grid_rows(a_buf, g), g, cin, kt, ks)
    ref, bound = nm.linear_ref(A, w, b, None if r5 is None else r5.reshape(-1, cout))
    return dict(name=name, g=g, og=og, cin=cin, cout=cout, kt=kt, ks=ks, a_buf=a_buf, w=w, b=b, res_buf=res_buf, res_cols=res_cols, r5=r5,
                x5=x5, ref=ref, bound=bound)


def conv_res_rows(c, buf=None):
    """The residual's row view [og.rows, cout] inside its storage (None without a residual)."""
    buf = c["res_buf"] if buf is None else buf
    if buf is None:
        return None
    rows = grid_rows(buf, c["og"])
    return rows if c["res_cols"] is None else rows[:, c["res_cols"][0]:c["res_cols"][1]]


# ------------------------------------------------------------------------------------------------ gemm128
GEMM_K = (32, 64, 96, 224, 4096)      # 1, 2, 3, 7 and 128 k-tiles: the nt == 1 prologue, the wraps of the 3-slot A ring and the 2-slot W ring
GEMM_M = (1, 17, 255, 256, 257, 700)
# the K= sub-range form of ops.gemm128 (fp32 split-K partials) has one caller, ops.linear_skinny (T5): tested in test_gpu_numerics_vae.py
GEMM_THIN = ((32, 17), (32, 700), (224, 257), (96, 700))     # (K, M) at N = 384


def gemm_operands(M, N, K, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=gen).to(BF)
    w = (torch.randn(N, K, generator=gen) / math.sqrt(K)).to(BF)
    b = torch.randn(N, generator=gen).to(BF)
    r = torch.randn(M, N, generator=gen).to(BF)
    return a, w, b, r


# ------------------------------------------------------------------------------------------------ GroupNorm / SpatialNorm
#            n, T, H,    W,  C,    groups, silu,  src_pad, dense, offset
GN_CASES = {
    "two_samples_cg4":  (2, 1, 3, 5, 128, 32, True, 1, False, False),        # sample 1 scaled by 3 and offset; C / groups = 4: a chunk straddles two groups
    "cg12_idle":        (1, 2, 4, 3, 384, 32, False, 0, True, False),        # 256 % 48 != 0: idle threads; C / groups = 12: chunks straddle groups
    "c1024":            (1, 1, 3, 3, 1024, 32, True, 0, False, False),
    "c2048_lanes1":     (1, 1, 2, 3, 2048, 32, False, 1, True, False),
    "8_per_thread":     (1, 4, 64, 64, 128, 32, True, 1, False, False),
    "65552_rows":       (1, 17, 3856, 1, 8, 2, False, 0, True, False),       # more image rows than the 65536-block grid: the grid-stride lap
    "offset_mean8":     (1, 4, 64, 64, 128, 32, True, 0, True, True),        # x ~ N(8, 0.5): the cancellation of E[x^2] - mu^2
    "cg12_silu_pad":    (1, 2, 4, 3, 384, 32, True, 1, False, False),
}
GN_CPU_SCALE = {"65552_rows": (1, 17, 40, 1, 8, 2, False, 0, True, False)}    # (the CPU restatement: same path, fewer rows)
GN_EPS = 1e-6
DST_FILL = 5.0


def gn_case(name, nblk, small=False):
    n, T, H, W, C, groups, silu, src_pad, dense, offset = (GN_CPU_SCALE.get(name) if small and name in GN_CPU_SCALE else GN_CASES[name])
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if offset:
        x5 = 8.0 + 0.5 * torch.randn(n, T, H, W, C, generator=gen)
    else:
        x5 = torch.randn(n, T, H, W, C, generator=gen) * 1.5 + 0.7
    if n > 1:
        x5[1] = 3.0 * x5[1] - 2.0     # a sample mix-up shows
    x5 = x5.to(BF)
    gamma = (1 + 0.3 * torch.randn(C, generator=gen)).to(BF)
    beta = (0.3 * torch.randn(C, generator=gen)).to(BF)
    gs = _grid(n, T, H, W, src_pad, 0)
    gd = _grid(n, T, H, W, 0, 0, sample_rows=T * H * W + 5) if dense else _grid(n, T, H, W, 1, 2)
    x_buf = storage(x5, gs, border=UNREAD)
    y_buf = torch.full((gd.rows + 2 * gd.guard, C), DST_FILL, dtype=BF)
    r = nm.group_norm_ref(x5.double(), groups, gamma, beta, GN_EPS, nblk, silu=silu)
    return dict(name=name, x5=x5, gamma=gamma, beta=beta, gs=gs, gd=gd, x_buf=x_buf, y_buf=y_buf, C=C, groups=groups, silu=silu, r=r)


SN_CASES = [(T, zT, C) for T, zT in ((1, 1), (2, 2), (5, 3), (9, 3)) for C in (128, 256)]


SN_LAP = dict(T=1, zT=1, C=128, H=32776, W=1, zH=3, zW=1, dense=True)    # 2 x 32776 = 65 552 image rows: the grid-stride lap of the apply kernel


def sn_case(T, zT, C, nblk, H=6, W=10, zH=3, zW=4, dense=False):
    n, groups = 2, 32
    gen = torch.Generator().manual_seed(T * 100 + zT * 10 + C)
    x5 = torch.randn(n, T, H, W, C, generator=gen) * 1.3 + 0.4
    x5[1] = 3.0 * x5[1] - 2.0
    x5 = x5.to(BF)
    gamma = (1 + 0.3 * torch.randn(C, generator=gen)).to(BF)
    beta = (0.3 * torch.randn(C, generator=gen)).to(BF)
    yb = torch.cat([1 + 0.5 * torch.randn(n * zT * zH * zW, C, generator=gen), 0.5 * torch.randn(n * zT * zH * zW, C, generator=gen)], 1).to(BF)
    gs = _grid(n, T, H, W, 1, 0)
    gd = _grid(n, T, H, W, 0, 0, sample_rows=T * H * W + 5) if dense else _grid(n, T, H, W, 1, 2)
    x_buf = storage(x5, gs, border=UNREAD)
    y_buf = torch.full((gd.rows + 2 * gd.guard, C), DST_FILL, dtype=BF)
    maps = nm.spatial_norm_maps(yb, n, C, (zT, zH, zW), (T, H, W))
    r = nm.group_norm_ref(x5.double(), groups, gamma, beta, GN_EPS, nblk, yb=maps)
    return dict(x5=x5, gamma=gamma, beta=beta, yb=yb, zdims=(zT, zH, zW), gs=gs, gd=gd, x_buf=x_buf, y_buf=y_buf, C=C, groups=groups, r=r, n=n)


# ------------------------------------------------------------------------------------------------ softmax_rows
#                 rows, n, ld, kinds of the rows
SOFTMAX_CASES = [(3, 4, 4, "pcs"), (5, 200, 256, "pcsrr"), (3, 1024, 1024, "pcs"), (3, 1028, 1152, "pcs"), (2, 4092, 4096, "ps"),
                 (2, 5000, 8192, "cp"), (2, 8192, 8192, "sp")]
SOFTMAX_CPU_SCALE = {(2, 8192, 8192, "sp"): (2, 2048, 2048, "sp"), (2, 5000, 8192, "cp"): (2, 1500, 2048, "cp"), (2, 4092, 4096, "ps"): (2, 1276, 1280, "ps")}


def softmax_scores(rows, n, ld, kinds):
    """fp32 scores [rows, ld]: p = peaked (the LAST valid column 30 above the rest), c = constant, s = shifted by -1e4, r = plain random;
    columns n.. hold GUARD_JUNK (never read)."""
    gen = torch.Generator().manual_seed(rows * 7 + n)
    s = 3.0 * torch.randn(rows, ld, generator=gen)
    for r, kind in enumerate(kinds):
        if kind == "p":
            s[r, :n] = torch.randn(n, generator=gen)
            s[r, n - 1] = s[r, :n].max() + 30.0
        elif kind == "c":
            s[r, :n] = 1.75
        elif kind == "s":
            s[r, :n] -= 1.0e4
    s[:, n:] = GUARD_JUNK
    return s


def check_softmax(out, s, n, what):
    """The element-wise bound on columns < n and EXACT zeros behind them; returns the Bound (already checked)."""
    ref, bound = nm.softmax_rows_ref(s, n)
    rep = nm.Bound(what).add(out[:, :n], ref, bound)
    rep.check()
    assert int((out[:, n:].float() != 0).sum()) == 0, f"{what}: columns n .. ld - 1 are not exactly zero"
    return rep


# ------------------------------------------------------------------------------------------------ first layer
FIRST_PARAMS = [3.85, 2.32, 2.33, 3.06] + [-0.10, 0.34, 0.27, 0.98]


def first_case(kt, kcols):
    gen = torch.Generator().manual_seed(17 + kt)
    z = torch.randn(4, 3, 4, 5, generator=gen).to(BF)
    params = FIRST_PARAMS + (0.5 * torch.randn(16, generator=gen)).tolist() + (0.1 * torch.randn(4, generator=gen)).tolist()
    ref, bound, mask = nm.first_im2col_ref(z, kt, kcols, params)
    return z, params, ref, bound, mask


def check_first(out, ref, bound, mask, what):
    rep = nm.Bound(what).add(out, ref, torch.where(mask, bound, torch.zeros_like(bound)))
    rep.check()
    assert int((out.float()[~mask] != 0).sum()) == 0, f"{what}: not exactly zero outside the volume / behind column 36 kt"
    return rep
