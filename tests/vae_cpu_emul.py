"""TEST INFRASTRUCTURE: torch restatements, on CPU tensors, of the VAE kernel wrappers of videosys_amd.ops (same signatures, same
row / grid layouts, bf16 storage, fp32 arithmetic) so that the HOST composition of vae_open_sora.py — which grids, paddings,
strides and weights it hands to which launch — can be checked against the oracle without a GPU.  The product never imports
this (it has no CPU path, tests/test_host_cpu.py::test_no_cpu_fallback); the kernels themselves are checked on the GPU against
torch in tests/test_gpu_vae.py."""
import contextlib

import torch
import torch.nn.functional as F


def _v5(rows, g, C=None):
    """rows over grid g -> view [n, T + tf, Hp, Wp, C]"""
    C = rows.shape[1] if C is None else C
    return rows.view(g.n, g.sample_rows, -1)[:, :(g.T + g.tf) * g.plane].view(g.n, g.T + g.tf, g.Hp, g.Wp, -1)[..., :C]


def _interior(rows, g, C=None):
    return _v5(rows, g, C)[:, g.tf:, g.pad:g.pad + g.H, g.pad:g.pad + g.W]


def vae_first_im2col(z, kt, kcols, params):
    scale, shift = torch.tensor(params[0:4]), torch.tensor(params[4:8])
    pw, pb = torch.tensor(params[8:24]).view(4, 4), torch.tensor(params[24:28])
    _, Fr, H, W = z.shape
    x = z.float() * scale[:, None, None, None] + shift[:, None, None, None]
    x = torch.einsum("oc,cfhw->ofhw", pw, x) + pb[:, None, None, None]
    x = x.to(torch.bfloat16).float()
    xp = F.pad(x, (1, 1, 1, 1, kt - 1, 0))                                  # zeros AFTER the 1x1 (the conv's own padding)
    cols = []
    for a in range(kt):
        for dy in range(3):
            for dx in range(3):
                cols.append(xp[:, a:a + Fr, dy:dy + H, dx:dx + W])           # [4, F, H, W] per tap, k = tap * 4 + c
    m = torch.stack(cols, 0).permute(2, 3, 4, 0, 1).reshape(Fr * H * W, kt * 36)
    out = torch.zeros(Fr * H * W, kcols)
    out[:, :kt * 36] = m
    return out.to(torch.bfloat16)


def gemm128(a, w, bias=None, res=None, out=None, out_f32=None, out_scale=1.0, batch=1, batch_a=0, batch_w=0, batch_o=0, M=None):
    assert batch == 1 and out_f32 is None and out_scale == 1.0, "the encode host flow uses the plain form only"
    y = a.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if res is not None:
        y = y + res.float()
    y = y.to(torch.bfloat16)
    if out is not None:
        out.copy_(y)
        return out
    return y


def conv(a, grid, w, bias, cin, kt, ks, out=None, res=None):
    assert grid.tf == kt - 1 and (ks == 1 or grid.pad == 1) and a.shape[0] == grid.rows
    og = grid.conv_out()
    x = _v5(a, grid, cin).permute(0, 4, 1, 2, 3).float()                      # [n, C, T + tf, Hp, Wp], borders are the padding
    wt = w.float().view(w.shape[0], kt, ks, ks, cin).permute(0, 4, 1, 2, 3)
    y = F.conv3d(x, wt, None if bias is None else bias.float())               # valid: [n, N, T, H, W]
    o = torch.zeros(og.rows, w.shape[0])
    (_interior(o, og) if ks == 3 else _v5(o, og)).copy_(y.permute(0, 2, 3, 4, 1))     # (ks = 1 on a bordered grid: every pixel is a row)
    if res is not None:
        o = o + res.float()
    o = o.to(torch.bfloat16)
    if out is not None:
        out.copy_(o)
        return out
    return o


def group_norm(x, gs, y, gd, C, gamma, beta, eps, silu_act, groups=32):
    v = _interior(x, gs, C).permute(0, 4, 1, 2, 3).float()
    h = F.group_norm(v, groups, gamma.float(), beta.float(), eps)
    if silu_act:
        h = F.silu(h)
    _interior(y, gd, C).copy_(h.permute(0, 2, 3, 4, 1).to(torch.bfloat16))
    return y


def regrid(x, gs, y, gd, C, up=0, tmode=0):
    assert up == 0 and tmode == 0
    _interior(y, gd, C).copy_(_interior(x, gs, C))
    return y


def subsample(x, gs, y, gd, C, t_stride=1, s_stride=1, t_first=0, s_first=0):
    src = _interior(x, gs, C)[:, t_first::t_stride, s_first::s_stride, s_first::s_stride]
    _interior(y, gd, C).copy_(src[:, :gd.T, :gd.H, :gd.W])
    return y


def extract_planar(x, g, nc, tskip, out, f0):
    assert 1 <= nc <= 4 and x.stride(0) % 4 == 0 and out.is_contiguous()       # the kernel's contract
    v = _interior(x, g, nc)                                                    # [n, T, H, W, nc]
    fr = v.reshape(g.n * g.T, g.H, g.W, nc)[tskip:]
    out[:, f0:f0 + fr.shape[0]] = fr.permute(3, 0, 1, 2)
    return out


def attention_2d(x, g, A):
    """VaeBlocks._attention with ``A`` an AttnWeights (the batched-GEMM / softmax composition is the decode path's, checked on the GPU): plain torch."""
    from videosys_amd.ops import VaeGrid

    C, L, n = 512, g.H * g.W, g.n
    t = _interior(x, g, C).reshape(n, L, C).float()
    hn = F.group_norm(t.transpose(1, 2), 32, A.norm.g.float(), A.norm.b.float(), A.norm.eps).transpose(1, 2)
    hn = hn.to(torch.bfloat16).float()
    q = (hn @ A.wq.float().t() + A.bq.float()).to(torch.bfloat16).float()
    k = (hn @ A.wk.float().t() + A.bk.float()).to(torch.bfloat16).float()
    v = (hn @ A.wv.float().t()).to(torch.bfloat16).float()
    p = torch.softmax(q @ k.transpose(1, 2) / (C ** 0.5), dim=-1).to(torch.bfloat16).float()
    o = (p @ v).to(torch.bfloat16).float()
    y = (o @ A.wo.float().t() + A.bo.float() + t).to(torch.bfloat16)
    gd = VaeGrid(n, 1, g.H, g.W, 0, 0)
    return y.reshape(n * L, C), gd


@contextlib.contextmanager
def emulated_vae_ops():
    from videosys_amd import ops
    from videosys_amd.vae_blocks import VaeBlocks

    mine = dict(vae_first_im2col=vae_first_im2col, gemm128=gemm128, conv=conv, group_norm=group_norm, regrid=regrid,
                subsample=subsample, extract_planar=extract_planar)
    saved = {k: getattr(ops, k) for k in mine}
    saved_attn = VaeBlocks._attention
    for k, v in mine.items():
        setattr(ops, k, v)
    VaeBlocks._attention = lambda self, x, g, aw: attention_2d(x, g, aw)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        VaeBlocks._attention = saved_attn


def cpu_vae(state_dict, encoder=True):
    """An OpenSoraVAE object on CPU tensors for the emulated host-flow test (bypasses the constructor's device check)."""
    from videosys_amd.vae_open_sora import OpenSoraVAE

    v = OpenSoraVAE.__new__(OpenSoraVAE)
    v.device = torch.device("cpu")
    v.micro_frame_size, v.micro_batch_size, v.frames_per_launch = 17, 4, 16
    v.micro_z_frame_size = 5
    v._padded = {}
    v._init_temporal(state_dict, v.device)
    v._init_spatial(state_dict, v.device, "spatial_vae.module.")
    v.has_encoder = encoder
    if encoder:
        v._init_encoders(state_dict, v.device)
    return v


# ------------------------------------------------------------------------------------------------ kernel-order restatements
# For the element-wise bounds of tests/numerics.py (tests/test_numerics_cpu.py): the same contracts restated in the ORDER the kernels
# work in (fp32 arithmetic, bf16 storage), each with the defects the bounds have to catch.  ``defect`` None = the contract.
def conv_taps(a, grid, w, bias, cin, kt, ks, res=None, defect=None):
    """conv_kernel as flat row shifts: output row r of grid.conv_out() adds, tap by tap, row r + a plane + b Wp + c of the buffer that
    starts (Wp + 1) rows before the grid (ks = 3).  n = 1.  Defects: "bf16_partials" (the running sum rounded to bf16 after every tap),
    "ktile_left" (the second 32-channel k-tile — the only one at cin = 32 — of the centre tap of the LAST frame plane, which always sees
    data, read one row = one pixel to the left),
    "res_next_row" (the residual of row r + 1)."""
    assert grid.n == 1 and grid.tf == kt - 1 and (ks == 1 or grid.pad == 1)
    og = grid.conv_out()
    M, N = og.rows, w.shape[0]
    lead = grid.Wp + 1 if ks == 3 else 0
    buf = torch.zeros(lead + grid.rows + lead, cin)
    buf[lead:lead + grid.rows] = a[:, :cin].float()
    wt = w.float().view(N, kt * ks * ks, cin)
    y = torch.zeros(M, N)
    bad_tap = kt * ks * ks - (5 if ks == 3 else 1)
    for tap in range(kt * ks * ks):
        ta, r = divmod(tap, ks * ks)
        b, c = divmod(r, ks)
        off = ta * grid.plane + b * grid.Wp + c
        x = buf[off:off + M].clone()
        if defect == "ktile_left" and tap == bad_tap:
            k0 = 32 if cin > 32 else 0
            x[1:, k0:k0 + 32] = buf[off:off + M - 1, k0:k0 + 32]
        y = y + x @ wt[:, tap].t()
        if defect == "bf16_partials":
            y = y.to(torch.bfloat16).float()
    if bias is not None:
        y = y + bias.float()
    y = y.to(torch.bfloat16)
    if res is not None:
        r32 = res.float()
        if defect == "res_next_row":
            r32 = torch.cat([r32[1:], r32[-1:]])
        y = (y.float() + r32).to(torch.bfloat16)
    return y


def gn_stats_geometry(x5, groups, eps, nblk, defect=None):
    """(mean, rstd) [n, groups] fp32 the way gn_partial_kernel / gn_finalize_kernel form them: thread (block, lane, 8-channel chunk) adds
    its positions block lanes + lane + k nblk lanes in fp32, one (sum, sum of squares) pair per 4-channel half; the lanes of a block
    are added in fp32 in lane order; blocks and the halves of a group in double; var = E[x^2] - mean^2.  x5 [n, T, H, W, C] bf16 values.
    Defect "q_bf16": the sums of squares held in bf16."""
    n, T, H, W, C = x5.shape
    P = T * H * W
    lanes = 256 // (C // 8)
    n_t = -(-P // (nblk * lanes))
    x = torch.zeros(n, n_t * nblk * lanes, C // 4, 4)
    x[:, :P] = x5.float().reshape(n, P, C // 4, 4)
    x = x.view(n, n_t, nblk, lanes, C // 4, 4)
    s = torch.zeros(n, nblk, lanes, C // 4)
    q = torch.zeros(n, nblk, lanes, C // 4)
    for k in range(n_t):
        f = x[:, k]
        s = s + ((f[..., 0] + f[..., 1]) + (f[..., 2] + f[..., 3]))
        f2 = f * f
        q = q + ((f2[..., 0] + f2[..., 1]) + (f2[..., 2] + f2[..., 3]))
        if defect == "q_bf16":
            q = q.to(torch.bfloat16).float()
    sb, qb = torch.zeros(n, nblk, C // 4), torch.zeros(n, nblk, C // 4)
    for l in range(lanes):
        sb, qb = sb + s[:, :, l], qb + q[:, :, l]
        if defect == "q_bf16":
            qb = qb.to(torch.bfloat16).float()
    cnt = float(P * (C // groups))
    sg = sb.double().sum(dim=1).view(n, groups, -1).sum(dim=2)
    qg = qb.double().sum(dim=1).view(n, groups, -1).sum(dim=2)
    mean = sg / cnt
    var = (qg / cnt - mean * mean).clamp_min(0.0)
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float()


def _silu32(x):
    return x / (1.0 + torch.exp(-x))


def gn_apply_chunks(x5, mean, rstd, groups, gamma, beta, silu_act, yb=None, defect=None):
    """gn_apply_kernel / spatial_norm_apply_kernel: per 8-channel chunk, elements 0..3 take the statistics of the group of channel 8 ch,
    elements 4..7 those of channel 8 ch + 4.  yb = (Y, B) [n, T, H, W, C] already gathered.  Defects: "upper_half_stats" (elements 4..7
    take the lower half's group), "sample0_stats" (every sample normalised with sample 0's statistics)."""
    n, T, H, W, C = x5.shape
    cg = C // groups
    ch = torch.arange(C)
    lower = (ch // 8 * 8) // cg
    upper = (ch // 8 * 8 + 4) // cg
    grp = torch.where(ch % 8 < 4, lower, lower if defect == "upper_half_stats" else upper)
    if defect == "sample0_stats":
        mean, rstd = mean[:1].expand(n, -1), rstd[:1].expand(n, -1)
    mu, rs = mean[:, grp][:, None, None, None, :], rstd[:, grp][:, None, None, None, :]
    o = ((x5.float() - mu) * rs * gamma.float() + beta.float()).to(torch.bfloat16).float()
    if yb is not None:
        o = ((o * yb[0].float()).to(torch.bfloat16).float() + yb[1].float()).to(torch.bfloat16).float()
        silu_act = True
    if silu_act:
        o = _silu32(o)
    return o.to(torch.bfloat16)


def spatial_norm_gather(yb_rows, n, C, zdims, size, defect=None):
    """(Y, B) [n, T, H, W, C] from the [Y | B] rows of the latent grid by the kernel's integer index (zt with the first-frame split for an
    odd T > 1, zh = h zH / H, zw = w zW / W).  Defect "zw_plus_1": the latent voxel one to the right (clamped)."""
    zT, zH, zW = zdims
    T, H, W = size
    z = yb_rows.view(n, zT, zH, zW, 2 * C)
    t = torch.arange(T)
    if T > 1 and T % 2 == 1:
        zt = torch.where(t == 0, torch.zeros_like(t), 1 + ((t - 1) * (zT - 1)) // max(T - 1, 1))
    else:
        zt = (t * zT) // T
    zh = (torch.arange(H) * zH) // H
    zw = (torch.arange(W) * zW) // W
    if defect == "zw_plus_1":
        zw = (zw + 1).clamp_max(zW - 1)
    g = z[:, zt][:, :, zh][:, :, :, zw]
    return g[..., :C], g[..., C:]


def softmax_rows(s, n, defect=None):
    """softmax_rows_kernel in fp32: the maximum over the first n columns, exp, the row sum, one reciprocal, bf16; columns n.. = 0.
    Defects: "sum_first_1024" (columns >= 1024 left out of the row sum: a thread's later column groups forgotten), "pad_not_zeroed"
    (columns n.. hold exp(s - m) / l of whatever the score buffer had there)."""
    rows, ld = s.shape
    x = s.float()
    m = x[:, :n].amax(dim=1, keepdim=True)
    e = torch.exp(x - m)
    if defect != "pad_not_zeroed":
        e[:, n:] = 0.0
    l = (e[:, :min(n, 1024)] if defect == "sum_first_1024" else e[:, :n]).sum(dim=1, keepdim=True)
    return (e * (1.0 / l)).to(torch.bfloat16)
