"""-m gpu: guard-band tests (tests/isolation.py) of the three kernels of the Open-Sora-Plan v1.2 pipeline (csrc/vae_osp.hip):
vsys_upsample_trilinear2x, vsys_cfg_ancestral_step and vsys_pixels_to_u8_trunc.  Exact assertions only, under both guard fills: same
bits as the call on tight operands, every guard byte untouched, every input unchanged.

Operand forms.  upsample_trilinear2x: the source rows over a conv-output grid (pad 1) with an INTERIOR guard on its border pixels — a
clamped tap that slipped past the edge would read it — and the destination over the padded input grid of the conv that follows (pad 1,
two front frames), a pure output with an INTERIOR guard on its border pixels and both front frames, which belong to the host.
cfg_ancestral_step: z in place, the learned-sigma half of model_out an interior guard, model_in a pure output; with and without the
noise operand.  pixels_to_u8_trunc: as tests/test_gpu_isolation_vchitect_pipeline.py does for vsys_pixels_to_u8 (border rows and the
channels from 3 on are guard; the frames outside [f0, f0 + N) keep their bytes); the 3 x 5 grid with f0 = 1 takes the byte-store path."""
import pytest
import torch

import isolation as iso
from isolation import Operand

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def border_mask(g, C, front=True):
    """True on every element of the rows of grid ``g`` that is not an interior voxel (border pixels, front frames)."""
    m = torch.ones(g.n, g.T + g.tf, g.Hp, g.Wp, C, dtype=torch.bool, device=dev())
    m[:, g.tf:, g.pad:g.pad + g.H, g.pad:g.pad + g.W] = False
    return m.view(g.rows, C)


@pytest.mark.parametrize("C,T,H,W", [(32, 1, 3, 5), (128, 3, 2, 2), (32, 4, 5, 3)])
def test_isolation_upsample_trilinear2x(C, T, H, W):
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd.ops import VaeGrid

    gs = VaeGrid(1, T, H, W, 1, 0)
    gd = VaeGrid(1, 1 if T == 1 else 2 * T - 1, 2 * H, 2 * W, 1, 2)
    x = torch.randn(gs.rows, C, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16).to(dev())
    o = {"x": Operand(x, interior=border_mask(gs, C)),
         "y": Operand(torch.zeros(gd.rows, C, dtype=torch.bfloat16, device=dev()), interior=border_mask(gd, C))}

    def fn(t):
        oops.upsample_trilinear2x(t["x"], gs, t["y"], gd, C)

    iso.check_isolated(fn, o, ["y"], what=f"upsample_trilinear2x C={C} T={T} {H}x{W}")


@pytest.mark.parametrize("Bz,thw,with_noise", [(1, 7, True), (2, 4096 + 3, True), (2, 7, False)])
def test_isolation_cfg_ancestral_step(Bz, thw, with_noise):
    from videosys_amd import open_sora_plan_ops as oops

    Cin = 4
    g = torch.Generator().manual_seed(thw)
    z = torch.randn(Bz, Cin, thw, generator=g).to(dev())
    mo = torch.randn(2 * Bz, 2 * Cin, thw, generator=g).to(dev())
    sigma = torch.zeros(2 * Bz, 2 * Cin, thw, dtype=torch.bool, device=dev())
    sigma[:, Cin:] = True
    o = {"z": Operand(z), "mo": Operand(mo, interior=sigma),
         "mi": Operand(torch.zeros(2 * Bz, Cin, thw, dtype=torch.bfloat16, device=dev()))}
    if with_noise:
        o["noise"] = Operand(torch.randn(Bz, Cin, thw, generator=g).to(dev()))

    def fn(t):
        oops.cfg_ancestral_step(t["z"], t["mo"], t.get("noise"), t["mi"], 7.5, -0.731, 0.417 if with_noise else 0.0, 0.4)

    iso.check_isolated(fn, o, ["z", "mi"], inplace=["z"], what=f"cfg_ancestral_step Bz={Bz} thw={thw} noise={with_noise}")


@pytest.mark.parametrize("N,H,W,f0,Ftot", [(2, 4, 6, 1, 4), (2, 3, 5, 1, 3)], ids=["dword-stores", "byte-stores"])
def test_isolation_pixels_to_u8_trunc(N, H, W, f0, Ftot):
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd.ops import VaeGrid

    ldx = 128
    g = VaeGrid(N, 1, H, W, 1, 0)
    x = (torch.rand(g.rows, ldx, generator=torch.Generator().manual_seed(H)) * 3.0 - 1.5).to(torch.bfloat16).to(dev())
    guard = torch.ones(N, H + 2, W + 2, ldx, dtype=torch.bool, device=dev())
    guard[:, 1:-1, 1:-1, :3] = False
    out = torch.full((Ftot, H, W, 3), 77, dtype=torch.uint8, device=dev())
    o = {"x": Operand(x, interior=guard.view(g.rows, ldx)),
         "out": Operand(out, int_guard=torch.tensor([0x5A, 0xA5, 0x3C], dtype=torch.uint8))}

    def fn(t):
        oops.pixels_to_u8_trunc(t["x"], g, t["out"], f0)

    iso.check_isolated(fn, o, ["out"], inplace=["out"], what=f"pixels_to_u8_trunc {N}x{H}x{W} f0={f0}")
