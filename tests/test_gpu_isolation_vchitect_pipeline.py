"""-m gpu: guard-band tests (tests/isolation.py) of the two decode kernels of the Vchitect-2.0 pipeline (csrc/vae_sd3.hip):
vsys_vae_first_im2col_nc and vsys_pixels_to_u8.  Exact assertions only, under both guard fills: same bits as the call on tight
operands, every guard byte untouched, every input unchanged.

Operand forms.  first_im2col_nc: the fp32 latents tight (bands in front and behind: a tap past the image would read them), the bf16
rows a pure output (pre-filled with the guard pattern: an unwritten pad column shows).  pixels_to_u8: the conv-output rows [rows, ldx]
with an INTERIOR guard — every border row of the padded grid and, in the interior rows, every channel from 3 on — so a border pixel
or a fourth channel that reached a byte would show under either fill; the uint8 frames are an integer tensor, which the harness takes
in place only (the frames outside [f0, f0 + N) are the caller's and must keep their bytes; that every byte of the written frames IS
written is tests/test_gpu_vchitect_vae.py's part).  The 3 x 5 grid with f0 = 1 starts its run at byte 45: the byte-store path."""
import pytest
import torch

import isolation as iso
from isolation import Operand

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("Cz,kcols", [(16, 160), (5, 64)])
def test_isolation_first_im2col_nc(Cz, kcols):
    from videosys_amd import ops

    F, H, W = 2, 3, 5
    z = torch.randn(F, Cz, H, W, generator=torch.Generator().manual_seed(Cz)).to(dev())
    o = {"z": Operand(z), "out": Operand(torch.zeros(F * H * W, kcols, dtype=torch.bfloat16, device=dev()))}

    def fn(t):
        ops._call("vsys_vae_first_im2col_nc", ops._p(t["z"]), F, Cz, H, W, kcols, 1.5305, 0.0609, ops._p(t["out"]))

    iso.check_isolated(fn, o, ["out"], what=f"vae_first_im2col_nc Cz={Cz} kcols={kcols}")


@pytest.mark.parametrize("N,H,W,f0,Ftot", [(2, 4, 6, 1, 4), (2, 3, 5, 1, 3)], ids=["dword-stores", "byte-stores"])
def test_isolation_pixels_to_u8(N, H, W, f0, Ftot):
    from videosys_amd import vchitect_ops as vops
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
        vops.pixels_to_u8(t["x"], g, t["out"], f0)

    iso.check_isolated(fn, o, ["out"], inplace=["out"], what=f"pixels_to_u8 {N}x{H}x{W} f0={f0}")
