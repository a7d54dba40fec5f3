"""-m gpu: the three kernels of csrc/vae_osp.hip against their contracts (include/videosys_amd.h).

  * vsys_upsample_trilinear2x: element-wise against float64 F.interpolate(mode="trilinear") of frame 0 by (1, 2, 2) and of the later
    frames by (2, 2, 2).  Bound: ONE rounding of the exact value to bf16, rnd(ref) (the fp32 accumulation of the eight taps, 2^-24
    relative, disappears in the room rnd leaves over half an ulp and in numerics.FLOOR).  The destination is the interior of a padded
    grid whose border and front frames must keep their bits.
  * vsys_cfg_ancestral_step: against float64 on the fp32 operands; |z' - ref| <= 4 2^-24 (|z| + |dt eps| + |sigma_up n|) per element,
    model_in within half a bf16 ulp of z' in_scale plus that slack, both CFG halves bit-equal, NaN in the learned-sigma channels
    without influence, noise = None with sigma_up = 0.
  * vsys_pixels_to_u8_trunc: bit-equal to the contract evaluated with torch bf16 tensor ops on the CPU."""
import pytest
import torch
import torch.nn.functional as F

import numerics as nm

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def trilinear_ref(x):
    """x [1, C, T, H, W] float64 -> Spatial2xTime2x3DUpsample's interpolation (autoencoder_kl_open_sora_plan_v120.py:349-357)."""
    if x.size(2) > 1:
        a = F.interpolate(x[:, :, :1], scale_factor=(1, 2, 2), mode="trilinear")
        r = F.interpolate(x[:, :, 1:], scale_factor=(2, 2, 2), mode="trilinear")
        return torch.cat([a, r], dim=2)
    return F.interpolate(x, scale_factor=(1, 2, 2), mode="trilinear")


@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("T,H,W", [(1, 3, 5), (2, 3, 5), (3, 2, 2), (4, 5, 3)])
def test_upsample_trilinear2x(C, T, H, W):
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd.ops import VaeGrid

    x = torch.randn(T * H * W, C, generator=torch.Generator().manual_seed(C + T)).to(torch.bfloat16)
    gs = VaeGrid(1, T, H, W, 1, 0)                      # a conv-output grid, as the decoder hands it over
    T2 = 1 if T == 1 else 2 * T - 1
    gd = VaeGrid(1, T2, 2 * H, 2 * W, 1, 2)
    xs = torch.full((gs.rows, C), float("nan"), dtype=torch.bfloat16)
    nm.grid_interior(xs, gs)[:] = x.view(1, T, H, W, C)   # (a NaN border: a tap that left the interior would show)
    sentinel = 123.0
    y = torch.full((gd.rows, C), sentinel, dtype=torch.bfloat16, device=dev())
    oops.upsample_trilinear2x(xs.to(dev()), gs, y, gd, C)
    torch.cuda.synchronize()
    y = y.cpu()
    x5 = x.double().view(1, T, H, W, C).permute(0, 4, 1, 2, 3)
    ref = trilinear_ref(x5).permute(0, 2, 3, 4, 1)                          # [1, T2, 2H, 2W, C]
    out = nm.grid_interior(y, gd)
    nm.check_elementwise(out.reshape(-1, C), ref.reshape(-1, C), nm.rnd(ref).reshape(-1, C), f"upsample_trilinear2x C={C} T={T} {H}x{W}")
    # border pixels and the two front frames are the conv's padding: never written
    full = nm.grid_view(y.clone(), gd)
    nm.grid_interior(full.reshape(gd.rows, C), gd)[:] = sentinel
    assert torch.equal(full, torch.full_like(full, sentinel)), "the kernel wrote outside the interior of the destination grid"


@pytest.mark.parametrize("Bz", [1, 2])
@pytest.mark.parametrize("thw", [1, 7, 4096 + 3])
@pytest.mark.parametrize("with_noise", [True, False])
def test_cfg_ancestral_step(Bz, thw, with_noise):
    from videosys_amd import open_sora_plan_ops as oops

    Cin = 4
    g = torch.Generator().manual_seed(Bz * 100 + thw)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    guidance, dt, in_scale = f32(7.5), f32(-0.731), f32(1.0 / (1.0 + 2.3**2) ** 0.5)
    sigma_up = f32(0.417) if with_noise else 0.0
    z = torch.randn(Bz, Cin, thw, 1, 1, generator=g)
    mo = torch.randn(2 * Bz, 2 * Cin, thw, 1, 1, generator=g)
    noise = torch.randn(Bz, Cin, thw, 1, 1, generator=g) if with_noise else None
    u, c = mo[:Bz, :Cin].double(), mo[Bz:, :Cin].double()
    eps = u + guidance * (c - u)
    ref = z.double() + dt * eps + (sigma_up * noise.double() if with_noise else 0.0)
    slack = 4 * 2.0**-24 * (z.double().abs() + (dt * eps).abs() + ((sigma_up * noise.double()).abs() if with_noise else 0.0))
    mo[:, Cin:] = float("nan")                           # the learned-sigma half must have no influence
    zd, mi = z.clone().to(dev()), torch.full((2 * Bz, Cin, thw, 1, 1), 9.0, dtype=torch.bfloat16, device=dev())
    oops.cfg_ancestral_step(zd, mo.to(dev()), noise.to(dev()) if with_noise else None, mi, guidance, dt, sigma_up, in_scale)
    torch.cuda.synchronize()
    zo, mi = zd.cpu(), mi.cpu()
    what = f"cfg_ancestral_step Bz={Bz} thw={thw} noise={with_noise}"
    nm.check_elementwise(zo.reshape(Bz, -1), ref.reshape(Bz, -1), slack.reshape(Bz, -1), what + " z'")
    want = ref * in_scale
    half_ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0**-120))) - 8)   # bf16: 8 significant bits
    nm.check_elementwise(mi[:Bz].reshape(Bz, -1), want.reshape(Bz, -1), (half_ulp + slack * abs(in_scale)).reshape(Bz, -1), what + " model_in")
    assert torch.equal(mi[:Bz].view(torch.int16), mi[Bz:].view(torch.int16)), "the two CFG halves of model_in differ"


def u8_contract(x_bf16):
    """pipeline_open_sora_plan.py:1186-1188 on a bf16 tensor, with torch's own bf16 tensor ops."""
    return ((x_bf16 / 2.0 + 0.5).clamp(0, 1) * 255).to(dtype=torch.uint8)


def boundary_values():
    """-1, 1, 127.5 / 255 and every x whose d * 255 lands on k + 0.5 (d = (2k + 1) / 510 is not a bf16 value for most k: take the bf16
    neighbours of the x that would give it, both sides)."""
    k = torch.arange(0, 255, dtype=torch.float64)
    d = (2 * k + 1) / 510.0
    x = (d - 0.5) * 2.0
    xb = x.to(torch.bfloat16)
    up = (xb.view(torch.int16) + 1).view(torch.bfloat16)
    dn = (xb.view(torch.int16) - 1).view(torch.bfloat16)
    fixed = torch.tensor([-1.0, 1.0, 0.0, -1.5, 1.5, 127.5, 2 * 127.5 / 255 - 1, -0.0], dtype=torch.bfloat16)
    return torch.cat([fixed, xb, up, dn])


@pytest.mark.parametrize("N,H,W,f0,Ftot", [(12, 4, 6, 1, 14), (18, 3, 5, 1, 20)], ids=["dword-stores", "byte-stores"])
def test_pixels_to_u8_trunc(N, H, W, f0, Ftot):
    """Enough frames of each grid to hold the whole boundary set; the rest of the values are random in [-1.5, 1.5]."""
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd.ops import VaeGrid

    ldx = 128
    g = VaeGrid(N, 1, H, W, 1, 0)
    npx = N * H * W * 3
    vals = (torch.rand(npx, generator=torch.Generator().manual_seed(H)) * 3.0 - 1.5).to(torch.bfloat16)
    bv = boundary_values()
    assert bv.numel() <= npx
    vals[:bv.numel()] = bv
    pix = vals.view(N, 1, H, W, 3)
    x = torch.full((g.rows, ldx), float("nan"), dtype=torch.bfloat16)
    nm.grid_interior(x, g)[..., :3] = pix
    out = torch.full((Ftot, H, W, 3), 77, dtype=torch.uint8, device=dev())
    oops.pixels_to_u8_trunc(x.to(dev()), g, out, f0)
    torch.cuda.synchronize()
    out = out.cpu()
    want = u8_contract(pix).view(N, H, W, 3)
    assert torch.equal(out[f0:f0 + N], want), f"{int((out[f0:f0 + N] != want).sum())} bytes differ from the bf16 contract"
    assert bool((out[:f0] == 77).all()) and bool((out[f0 + N:] == 77).all()), "frames outside [f0, f0 + N) were written"


def test_pixels_to_u8_trunc_every_bf16_value():
    """Every finite bf16 value in [-2, 2] through the kernel on one long grid row set: the contract is a function of 16 bits."""
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd.ops import VaeGrid

    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    vals = allb[torch.isfinite(allb.float()) & (allb.float().abs() <= 2.0)]
    n = vals.numel() // 12 * 12
    vals = vals[:n]
    H, W = 2, 2
    N = n // (H * W * 3)
    g = VaeGrid(N, 1, H, W, 0, 0)
    x = torch.zeros(g.rows, 4, dtype=torch.bfloat16)
    x[:, :3] = vals.view(-1, 3)
    out = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev())
    oops.pixels_to_u8_trunc(x.to(dev()), g, out, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(-1), u8_contract(vals))
