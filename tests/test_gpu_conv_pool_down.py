"""-m gpu: vsys_conv_pool_down2_bf16 (csrc/conv_pool_down_bf16.hip) element-wise against float64: p = conv2d(pad(m64), w64, stride 2)
+ b, m64 the EXACT float64 mean of each frame pair (of the lone first frame when T is odd) of the same bf16 operands, F.pad (0, 1, 0, 1).
Bound: conv_down2's stride-2 bound acc(K + 1, s) + rnd(p), s the same convolution of |m64| and |w| plus |b|, K = 9 cin — plus
conv2d(pad(rnd(m64)), |w|, stride 2), which pays for the one bf16 rounding of the pooled operand.  The wrapper takes w / 2 (exact in
bf16); the reference uses w.  The source's border pixels, front frames and slack hold junk (vae_numerics_cases.storage): the padding
must come from the addressing.  A tile is 256 output voxels: ``T5_edge`` (255 a frame, T odd) has lone and paired voxels in its first
tile and frames that straddle tiles, ``T4_wrap`` (289 a frame) a ragged last tile; both also run inside the guard bands of
tests/isolation.py, the source's border pixels being guard."""
import functools

import pytest
import torch
import torch.nn.functional as F

import isolation as iso
import numerics as nm
import vae_numerics_cases as vc

pytestmark = pytest.mark.gpu

#                 n  T  H   W   cin  cout pad tf
CASES = {
    "T1_2x2":       (2, 1, 2, 2, 32, 128, 0, 0),      # one voxel: lone frame, both padding taps
    "T2_odd":       (2, 2, 7, 5, 32, 128, 1, 0),      # even T, one pair; the zero row and column are never reached
    "T3_odd":       (2, 3, 7, 9, 32, 128, 1, 0),      # lone frame 0, then pair (1, 2)
    "T5_edge":      (2, 5, 30, 34, 32, 128, 1, 2),    # 255 voxels a frame: the first tile holds lone and paired voxels, frames straddle tiles
    "T4_wrap":      (2, 4, 34, 34, 32, 128, 1, 0),    # 289 voxels a frame, even T, ragged last tile
    "T5_cin128_n2": (1, 5, 34, 30, 128, 256, 0, 0),   # two column tiles, four chunks per tap
    "T3_cin96":     (1, 3, 6, 33, 96, 128, 0, 0),     # a chunk count that is no power of two
}


@functools.lru_cache(maxsize=None)
def case(name):
    """CPU operands, source grid and storage, float64 reference and bound [n To Ho Wo, cout]."""
    n, T, H, W, cin, cout, pad, tf = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    K = 9 * cin
    x5 = torch.randn(n, T, H, W, cin, generator=gen).to(vc.BF)
    w = (torch.randn(cout, K, generator=gen) / K**0.5).to(vc.BF)
    b = (0.5 * torch.randn(cout, generator=gen)).to(vc.BF)
    g = vc._grid(n, T, H, W, pad, tf)
    odd = T % 2
    xd = x5.double()
    m = torch.cat([xd[:, :odd], (xd[:, odd::2] + xd[:, odd + 1::2]) / 2], dim=1)                 # [n, To, H, W, cin], exact
    To = m.shape[1]
    wk = w.double().view(cout, 3, 3, cin).permute(0, 3, 1, 2)
    conv = lambda v, k: F.conv2d(F.pad(v.permute(0, 1, 4, 2, 3).reshape(n * To, cin, H, W), (0, 1, 0, 1)), k, stride=2) \
        .permute(0, 2, 3, 1).reshape(-1, cout)
    p, s = conv(m, wk) + b.double(), conv(m.abs(), wk.abs()) + b.double().abs()
    bound = nm.acc(K + 1, s) + nm.rnd(p) + conv(nm.rnd(m), wk.abs())
    return dict(cin=cin, cout=cout, g=g, buf=vc.storage(x5, g, border=vc.UNREAD), w_half=(w.float() * 0.5).to(vc.BF), b=b, ref=p,
                bound=bound, rows=n * To * (H // 2) * (W // 2))


@pytest.mark.parametrize("name", list(CASES))
def test_conv_pool_down2_elementwise(name):
    from videosys_amd import vae_blocks as vb

    c, dev = case(name), torch.device("cuda:0")
    assert vb.pool_down2_grid(c["g"]).rows == c["rows"] == c["ref"].shape[0] > 0
    out = vb.conv_pool_down2(vc.grid_rows(c["buf"].to(dev), c["g"]), c["g"], c["w_half"].to(dev), c["b"].to(dev), c["cin"])
    torch.cuda.synchronize()
    rep = nm.Bound(f"conv_pool_down2 {name} {CASES[name]}").add(out.cpu(), c["ref"], c["bound"])
    print(rep.message())
    rep.check()


@pytest.mark.parametrize("name", ["T5_edge", "T4_wrap"])
def test_conv_pool_down2_inside_guard_bands(name):
    from videosys_amd import vae_blocks as vb

    c, dev = case(name), torch.device("cuda:0")
    g = c["g"]
    voxel = torch.zeros(g.rows, 1, dtype=torch.bool)
    nm.grid_interior(voxel, g)[...] = True
    operands = dict(x=iso.Operand(vc.grid_rows(c["buf"], g).to(dev), interior=~voxel.to(dev).expand(-1, c["cin"])),
                    w=iso.Operand(c["w_half"].to(dev)), b=iso.Operand(c["b"].to(dev)),
                    out=iso.Operand(torch.zeros(c["rows"], c["cout"], dtype=vc.BF, device=dev), parent=(c["rows"], c["cout"] + 192), at=(0, 64)))
    iso.check_isolated(lambda t: vb.conv_pool_down2(t["x"], g, t["w"], t["b"], c["cin"], out=t["out"]), operands, ("out",),
                       what=f"conv_pool_down2 {name}")
