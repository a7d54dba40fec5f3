"""-m gpu: vsys_conv_time_down2_bf16 (csrc/conv_time_down_bf16.hip) element-wise against float64 on the same bf16 operands and the same
fp32 a3 the kernel gets: p = conv3d(x', w_s, stride (2, 1, 1), padding (0, 1, 1)) + b_s + a3 (x0 + x1 + x2), x' = x behind two copies of
its first frame.  Bound: acc(27 C + 4, s) + rnd(p), s the same expression on absolute values (27 C products, the bias, the three pooled
terms: fp32 throughout, one rounding).  Pool-only mode (w = None): the exact float64 mean, bound rnd(m) + acc(4, mean |x|) (two adds and
a multiply by fp32(1 / 3)).  The source's border pixels, front frames and slack hold junk (vae_numerics_cases.storage) and the never-read
last frame of an even T holds NaN: the padding must come from the addressing.  A tile is 256 output voxels: 15 x 17 gives 255 a frame
(the first tile runs from output frame 0 into 1, frames straddle tiles), 17 x 17 gives 289 (a ragged last tile); both also run inside
the guard bands of tests/isolation.py, the source's border pixels being guard."""
import functools

import pytest
import torch
import torch.nn.functional as F

import isolation as iso
import numerics as nm
import vae_numerics_cases as vc

pytestmark = pytest.mark.gpu

#                n  T  H   W   C   pad tf  alpha
CASES = {
    "T1_2x2":    (2, 1, 2, 2, 128, 0, 0, 0.31),       # one voxel row of four: every edge tap, all three time taps on frame 0
    "T2_even":   (2, 2, 7, 5, 128, 1, 0, 0.47),       # even T: one output frame, frame 1 unread
    "T3":        (2, 3, 7, 9, 128, 1, 0, 0.93),       # two output frames
    "T5_255":    (2, 5, 15, 17, 128, 1, 2, 0.58),     # 255 voxels a frame: the first tile wraps from output frame 0 into 1, frames straddle tiles
    "T4_289":    (2, 4, 17, 17, 128, 1, 0, 0.72),     # 289 voxels a frame, ragged last tile
    "T5_C256":   (1, 5, 17, 15, 256, 0, 0, 0.28),     # two column tiles: the residual columns follow col0; eight chunks per tap
}
POOL = {"T1_2x2": 128, "T2_even": 128, "T5_255": 128, "T3": 32}        # pool-only: case -> C (the first C columns of the same source)


@functools.lru_cache(maxsize=None)
def case(name):
    """CPU operands, source grid and storage, float64 reference and bound [n To H W, C] of both modes."""
    n, T, H, W, C, pad, tf, alpha = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    K = 27 * C
    x5 = torch.randn(n, T, H, W, C, generator=gen).to(vc.BF)
    w = torch.randn(C, K, generator=gen) / K**0.5
    b = 0.5 * torch.randn(C, generator=gen)
    keep = torch.tensor(1.0 - alpha, dtype=torch.float32)
    w_s, b_s = (w * keep).to(vc.BF), (b * keep).to(vc.BF)                        # scaled in fp32, one rounding
    a3 = float(torch.tensor(alpha / 3.0, dtype=torch.float32))
    g = vc._grid(n, T, H, W, pad, tf)
    read = x5[:, :T - 1] if T % 2 == 0 else x5                                   # an even T leaves its last frame unread ...
    stored = x5.clone()
    if T % 2 == 0:
        stored[:, T - 1] = float("nan")                                          # ... so it may hold anything
    x = read.double().permute(0, 4, 1, 2, 3)
    x = torch.cat([x[:, :, :1], x[:, :, :1], x], dim=2)                          # [n, C, T + 2, H, W]
    wk = w_s.double().view(C, 3, 3, 3, C).permute(0, 4, 1, 2, 3)
    rows = lambda v: v.permute(0, 2, 3, 4, 1).reshape(-1, v.shape[1])
    conv = lambda v, k: rows(F.conv3d(v, k, stride=(2, 1, 1), padding=(0, 1, 1)))
    pool3 = lambda v: rows(F.avg_pool3d(v, (3, 1, 1), stride=(2, 1, 1))) * 3.0   # x0 + x1 + x2
    p = conv(x, wk) + b_s.double() + a3 * pool3(x)
    s = conv(x.abs(), wk.abs()) + b_s.double().abs() + a3 * pool3(x.abs())
    m, ma = pool3(x) / 3.0, pool3(x.abs()) / 3.0
    return dict(C=C, g=g, buf=vc.storage(stored, g, border=vc.UNREAD), w_s=w_s, b_s=b_s, a3=a3, ref=p, bound=nm.acc(K + 4, s) + nm.rnd(p),
                pool_ref=m, pool_bound=nm.rnd(m) + nm.acc(4, ma))


@pytest.mark.parametrize("name", list(CASES))
def test_conv_time_down2_elementwise(name):
    from videosys_amd import open_sora_plan_v110_ops as ops

    c, dev = case(name), torch.device("cuda:0")
    assert ops.time_down2_grid(c["g"]).rows == c["ref"].shape[0] > 0
    out = ops.conv_time_down2(vc.grid_rows(c["buf"].to(dev), c["g"]), c["g"], c["w_s"].to(dev), c["b_s"].to(dev), c["C"], c["a3"])
    torch.cuda.synchronize()
    rep = nm.Bound(f"conv_time_down2 {name} {CASES[name]}").add(out.cpu(), c["ref"], c["bound"])
    print(rep.message())
    rep.check()


@pytest.mark.parametrize("name", list(POOL))
def test_time_pool_down2_elementwise(name):
    from videosys_amd import open_sora_plan_v110_ops as ops

    c, C, dev = case(name), POOL[name], torch.device("cuda:0")
    out = ops.conv_time_down2(vc.grid_rows(c["buf"].to(dev), c["g"]), c["g"], None, None, C, 1.0 / 3.0)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (c["pool_ref"].shape[0], C)
    rep = nm.Bound(f"time_pool_down2 {name} C={C}").add(out.cpu(), c["pool_ref"][:, :C], c["pool_bound"][:, :C])
    print(rep.message())
    rep.check()


@pytest.mark.parametrize("name", ["T5_255", "T4_289"])
def test_conv_time_down2_inside_guard_bands(name):
    from videosys_amd import open_sora_plan_v110_ops as ops

    c, dev = case(name), torch.device("cuda:0")
    g, rows, C = c["g"], c["ref"].shape[0], c["C"]
    voxel = torch.zeros(g.rows, 1, dtype=torch.bool)
    nm.grid_interior(voxel, g)[...] = True
    operands = dict(x=iso.Operand(vc.grid_rows(c["buf"], g).to(dev), interior=~voxel.to(dev).expand(-1, C)),
                    w=iso.Operand(c["w_s"].to(dev)), b=iso.Operand(c["b_s"].to(dev)),
                    out=iso.Operand(torch.zeros(rows, C, dtype=vc.BF, device=dev), parent=(rows, C + 192), at=(0, 64)))
    iso.check_isolated(lambda t: ops.conv_time_down2(t["x"], g, t["w"], t["b"], C, c["a3"], out=t["out"]), operands, ("out",),
                       what=f"conv_time_down2 {name}")
