"""-m gpu: vsys_conv_causal_tdown2_bf16 (csrc/conv_causal_tdown_bf16.hip) element-wise against a float64 conv3d on the same bf16
operands: p = conv3d(x', w, stride (2, 1, 1), padding (0, 1, 1)) + b, x' = x behind ONE explicit ZERO frame.  Bound: acc(27 cin + 1, s)
+ rnd(p), s the same expression on absolute values (27 cin products and the bias in fp32, one rounding): tests/numerics.py, as
tests/test_gpu_conv_time_down.py.  The source's border pixels and front frames (pad = 1, tf = 2 case) and the never-read last frame of
an odd T hold NaN: the padding must come from the addressing.  On every case the output also equals, bit for bit, the route the kernel
replaces (stride-1 vsys_conv_bf16 over a zero-bordered copy, vsys_subsample of the odd frames): the tile engine keeps that kernel's k
order.  One case runs inside the guard bands of tests/isolation.py.  At the encoder level: OpenSoraVAE's moments against the golden of
the reference with the strided route, which must not touch vsys_subsample, while VSYS_VAE_ENCODE_STRIDED=0 must."""
import functools

import pytest
import torch
import torch.nn.functional as F

import isolation as iso
import numerics as nm
import vae_numerics_cases as vc
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

#             T  H   W   pad tf
SHAPES = {
    "T2_8x8":     (2, 8, 8, 0, 0),       # one partial tile of 64 voxels; only t' = 0 exists: every output has a zero time tap
    "T4_12x12":   (4, 12, 12, 0, 0),     # 288 voxels, two tiles: the first straddles output frames 0 and 1
    "T5_5x7":     (5, 5, 7, 0, 0),       # odd extents, the last frame unread
    "T4_15x17_p": (4, 15, 17, 1, 2),     # a conv-output grid (NaN border and front frames); 255 voxels a frame: frames straddle tiles, ragged tail
}
CHANNELS = [(32, 128), (128, 128), (128, 256)]


@functools.lru_cache(maxsize=None)
def case(shape, n, cin, cout):
    """CPU operands, source grid and storage, float64 reference and bound [n To H W, cout] with and without the bias."""
    T, H, W, pad, tf = SHAPES[shape]
    gen = torch.Generator().manual_seed(sum(map(ord, shape)) + 7 * n + cin + cout)
    K = 27 * cin
    x5 = torch.randn(n, T, H, W, cin, generator=gen).to(vc.BF)
    w = (torch.randn(cout, K, generator=gen) / K**0.5).to(vc.BF)
    b = (0.5 * torch.randn(cout, generator=gen)).to(vc.BF)
    g = vc._grid(n, T, H, W, pad, tf)
    stored = x5.clone()
    if T % 2:
        stored[:, T - 1] = float("nan")                                          # an odd T leaves its last frame unread
    x = x5[:, :T - T % 2].double().permute(0, 4, 1, 2, 3)
    x = torch.cat([torch.zeros_like(x[:, :, :1]), x], dim=2)                     # ONE zero frame in front
    wk = w.double().view(cout, 3, 3, 3, cin).permute(0, 4, 1, 2, 3)
    conv = lambda v, k: F.conv3d(v, k, stride=(2, 1, 1), padding=(0, 1, 1)).permute(0, 2, 3, 4, 1).reshape(-1, cout)
    p, s = conv(x, wk), conv(x.abs(), wk.abs())
    pb, sb = p + b.double(), s + b.double().abs()
    return dict(g=g, x5=x5, buf=vc.storage(stored, g, border=float("nan")), w=w, b=b,
                ref={False: p, True: pb}, bound={False: nm.acc(K + 1, s) + nm.rnd(p), True: nm.acc(K + 1, sb) + nm.rnd(pb)})


def composed(x4, w, b):
    """One sample [T, H, W, cin] on the route the kernel replaces: zero-bordered copy, stride-1 conv, every second frame from frame 1."""
    from videosys_amd import ops

    T, H, W, cin = x4.shape
    gp = ops.VaeGrid(1, T, H, W, 1, 2)
    _, xp = gp.alloc(cin, DEV, zero=True)
    xp.view(T + 2, H + 2, W + 2, cin)[2:, 1:-1, 1:-1] = x4
    g2 = ops.VaeGrid(1, T // 2, H, W, 0, 0)
    out = torch.empty(g2.rows, w.shape[0], dtype=vc.BF, device=DEV)
    ops.subsample(ops.conv(xp, gp, w, b, cin, 3, 3), gp.conv_out(), out, g2, w.shape[0], 2, 1, 1, 0)
    return out


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("cin, cout", CHANNELS)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_conv_causal_tdown2_elementwise_and_equal_to_the_composed_route(shape, n, cin, cout, bias):
    from videosys_amd import open_sora_vae_ops as vops

    c = case(shape, n, cin, cout)
    w, b = c["w"].to(DEV), (c["b"].to(DEV) if bias else None)
    assert vops.causal_tdown2_grid(c["g"]).rows == c["ref"][bias].shape[0] > 0
    out = vops.conv_causal_tdown2(vc.grid_rows(c["buf"].to(DEV), c["g"]), c["g"], w, b, cin)
    torch.cuda.synchronize()
    rep = nm.Bound(f"conv_causal_tdown2 {shape} n={n} {cin}->{cout} bias={bias}").add(out.cpu(), c["ref"][bias], c["bound"][bias])
    print(rep.message())
    rep.check()
    old = torch.cat([composed(c["x5"][i, :SHAPES[shape][0] - SHAPES[shape][0] % 2].to(DEV), w, b) for i in range(n)])
    assert torch.equal(iso.bits(out), iso.bits(old)), f"{int((iso.bits(out) != iso.bits(old)).sum())} elements differ from the composed route"


def test_conv_causal_tdown2_inside_guard_bands():
    from videosys_amd import open_sora_vae_ops as vops

    cin, cout = 128, 128
    c = case("T4_15x17_p", 2, cin, cout)
    g, rows = c["g"], c["ref"][True].shape[0]
    voxel = torch.zeros(g.rows, 1, dtype=torch.bool)
    nm.grid_interior(voxel, g)[...] = True
    operands = dict(x=iso.Operand(vc.grid_rows(c["buf"], g).to(DEV), interior=~voxel.to(DEV).expand(-1, cin)),
                    w=iso.Operand(c["w"].to(DEV)), b=iso.Operand(c["b"].to(DEV)),
                    out=iso.Operand(torch.zeros(rows, cout, dtype=vc.BF, device=DEV), parent=(rows, cout + 192), at=(0, 64)))
    iso.check_isolated(lambda t: vops.conv_causal_tdown2(t["x"], g, t["w"], t["b"], cin, out=t["out"]), operands, ("out",),
                       what="conv_causal_tdown2 T4_15x17_p")


# ---------------------------------------------------------------------------------------------------- encoder level
@functools.lru_cache(maxsize=None)
def encoder():
    from videosys_amd.vae_open_sora import OpenSoraVAE_V1_2

    gold = load_golden("opensora_vae_encode_small.pt")
    return gold, OpenSoraVAE_V1_2(from_pretrained=f"synthetic-full:{gold['seed']}", device=DEV)


def moments(gold, vae):
    fr = gold["x"][0].permute(1, 0, 2, 3)[:4]                                     # [4 frames, 3, 32, 48]
    m2d = vae._spatial_encode(fr.permute(1, 0, 2, 3).to(vc.BF).to(DEV).contiguous()).float().cpu()
    mt = vae._temporal_encode(gold["xz17"][0].to(vc.BF).to(DEV).contiguous()).float().cpu()
    return m2d.permute(1, 0, 2, 3), mt[None]


def test_encode_on_the_strided_route_matches_the_reference_golden():
    """The bound of tests/test_gpu_vae.py's encode test: rel rms <= 1.5 x the reference's own bf16 run + 1e-3, cosine >= 0.999."""
    gold, vae = encoder()
    rms = lambda t: t.pow(2).mean().sqrt().item()
    for out, key in zip(moments(gold, vae), ("frames4_moments", "xz17_moments")):
        ref, ref16 = gold[key], gold[key + "_bf16"]
        floor, mine = rms(ref16.float() - ref) / rms(ref), rms(out - ref) / rms(ref)
        cos = F.cosine_similarity(out.flatten(), ref.flatten(), dim=0).item()
        print(f"{key}: rel rms {mine:.4f} vs floor {floor:.4f}, cosine {cos:.5f}")
        assert mine <= 1.5 * floor + 1e-3 and cos >= 0.999, f"{key}: rel rms {mine:.4f} vs floor {floor:.4f}, cosine {cos:.5f}"


def test_default_route_makes_no_sampled_stride1_convolution(monkeypatch):
    from videosys_amd import ops

    gold, vae = encoder()

    def refuse(*a, **k):
        raise AssertionError("vsys_subsample on the strided route")

    monkeypatch.setattr(ops, "subsample", refuse)
    monkeypatch.delenv("VSYS_VAE_ENCODE_STRIDED", raising=False)
    assert all(bool(torch.isfinite(m).all()) for m in moments(gold, vae))
    monkeypatch.setenv("VSYS_VAE_ENCODE_STRIDED", "0")
    with pytest.raises(AssertionError, match="vsys_subsample"):
        moments(gold, vae)
