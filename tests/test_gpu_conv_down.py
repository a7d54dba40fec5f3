"""-m gpu: vsys_conv_down2_bf16 (csrc/conv_down_bf16.hip) element-wise against a float64 conv2d / conv3d (stride 2) of the same bf16
operands on the EXPLICITLY padded input: F.pad (0, 1, 0, 1), and for the causal mode two copies of the first frame in front.  Bound: the
stride-1 convolution's (numerics.linear_ref: acc(K + 1, sum |a w| + |b|) + rnd(p)), the accumulation length per output being the same.
The source's border pixels, front frames and slack hold junk (vae_numerics_cases.storage): the padding must come from the addressing.
A tile is 256 output voxels: 30 x 34 gives 255 per frame (a ragged second tile), 34 x 30 x 3 frames 765 (frames straddle tiles).  One
case per mode also runs inside the guard bands of tests/isolation.py, the source's border pixels being guard."""
import functools

import pytest
import torch
import torch.nn.functional as F

import isolation as iso
import numerics as nm
import vae_numerics_cases as vc

pytestmark = pytest.mark.gpu

#        kt n  T  H   W   cin  cout pad tf
CASES = {
    "s_2x2":        (1, 2, 1, 2, 2, 32, 128, 0, 0),      # one output voxel: its kh = 2 and kw = 2 taps are both padding
    "s_odd":        (1, 2, 3, 7, 5, 32, 128, 1, 0),      # odd sizes: the zero row / column is never reached
    "s_edge":       (1, 2, 2, 30, 34, 32, 128, 1, 2),    # 510 voxels per sample, bordered grid with (unread) front frames
    "s_cin128_n2":  (1, 1, 1, 34, 30, 128, 256, 0, 0),   # two column tiles, four channel chunks per tap
    "s_cin96":      (1, 1, 2, 6, 33, 96, 128, 0, 0),     # a chunk count that is no power of two; W odd, H even
    "st_T1":        (3, 2, 1, 2, 2, 32, 128, 0, 0),      # every tap reads frame 0
    "st_T2_odd":    (3, 2, 2, 7, 9, 32, 128, 1, 0),      # one output frame, frame 1 unread
    "st_T3_edge":   (3, 2, 3, 30, 34, 32, 128, 1, 0),    # output frames 0 (replicated front) and 1 in one tile
    "st_T5_cin128": (3, 1, 5, 34, 30, 128, 256, 0, 0),   # three output frames over three row tiles, two column tiles
    "st_T5_wrap":   (3, 2, 5, 34, 34, 32, 128, 1, 0),    # 289 voxels a frame: the tile at voxel 256 starts in output frame 0 and runs into
                                                         # frame 1, which reads source frame 0 from its start again (lower rows than the tile's first)
}


@functools.lru_cache(maxsize=None)
def case(name):
    """CPU operands, source grid and storage, float64 reference and bound [n To Ho Wo, cout]."""
    kt, n, T, H, W, cin, cout, pad, tf = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    K = 9 * kt * cin
    x5 = torch.randn(n, T, H, W, cin, generator=gen).to(vc.BF)
    w = (torch.randn(cout, K, generator=gen) / K**0.5).to(vc.BF)
    b = (0.5 * torch.randn(cout, generator=gen)).to(vc.BF)
    g = vc._grid(n, T, H, W, pad, tf)
    buf = vc.storage(x5, g, border=vc.UNREAD)
    x = F.pad(x5.double().permute(0, 4, 1, 2, 3), (0, 1, 0, 1))                    # [n, cin, T, H + 1, W + 1]
    if kt == 3:
        x = torch.cat([x[:, :, :1], x[:, :, :1], x], dim=2)
        wk = w.double().view(cout, 3, 3, 3, cin).permute(0, 4, 1, 2, 3)
        p, s = F.conv3d(x, wk, stride=2), F.conv3d(x.abs(), wk.abs(), stride=2)
    else:
        x = x.permute(0, 2, 1, 3, 4).reshape(n * T, cin, H + 1, W + 1)
        wk = w.double().view(cout, 3, 3, cin).permute(0, 3, 1, 2)
        p, s = (v.view(n, T, cout, H // 2, W // 2).permute(0, 2, 1, 3, 4) for v in (F.conv2d(x, wk, stride=2), F.conv2d(x.abs(), wk.abs(), stride=2)))
    rows = lambda v: v.permute(0, 2, 3, 4, 1).reshape(-1, cout)
    p, s = rows(p) + b.double(), rows(s) + b.double().abs()
    return dict(kt=kt, cin=cin, cout=cout, g=g, buf=buf, w=w, b=b, ref=p, bound=nm.acc(K + 1, s) + nm.rnd(p))


@pytest.mark.parametrize("name", list(CASES))
def test_conv_down2_elementwise(name):
    from videosys_amd import open_sora_plan_ops as ops

    c, dev = case(name), torch.device("cuda:0")
    assert c["g"].down2(c["kt"]).rows == c["ref"].shape[0] > 0
    out = ops.conv_down2(vc.grid_rows(c["buf"].to(dev), c["g"]), c["g"], c["w"].to(dev), c["b"].to(dev), c["cin"], c["kt"])
    torch.cuda.synchronize()
    rep = nm.Bound(f"conv_down2 {name} {CASES[name]}").add(out.cpu(), c["ref"], c["bound"])
    print(rep.message())
    rep.check()


@pytest.mark.parametrize("name", ["s_edge", "st_T3_edge"])
def test_conv_down2_inside_guard_bands(name):
    from videosys_amd import open_sora_plan_ops as ops

    c, dev = case(name), torch.device("cuda:0")
    g, og = c["g"], c["g"].down2(c["kt"])
    voxel = torch.zeros(g.rows, 1, dtype=torch.bool)
    nm.grid_interior(voxel, g)[...] = True
    operands = dict(x=iso.Operand(vc.grid_rows(c["buf"], g).to(dev), interior=~voxel.to(dev).expand(-1, c["cin"])),
                    w=iso.Operand(c["w"].to(dev)), b=iso.Operand(c["b"].to(dev)),
                    out=iso.Operand(torch.zeros(og.rows, c["cout"], dtype=vc.BF, device=dev), parent=(og.rows, c["cout"] + 192), at=(0, 64)))
    iso.check_isolated(lambda t: ops.conv_down2(t["x"], g, t["w"], t["b"], c["cin"], c["kt"], out=t["out"]), operands, ("out",),
                       what=f"conv_down2 {name}")
