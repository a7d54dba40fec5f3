"""-m gpu: guard-band tests (tests/isolation.py) of the two kernels of the Open-Sora-Plan v1.1 pipeline (csrc/vae_osp.hip):
vsys_upsample_time2x and vsys_cfg_pndm_step.  Exact assertions only, under both guard fills: same bits as the call on tight operands,
every guard byte untouched, every input unchanged.

Operand forms, as tests/test_gpu_isolation_osp_pipeline.py.  upsample_time2x: the source rows over a conv-output grid (pad 1) with an
INTERIOR guard on its border pixels — a clamped frame tap never leaves a pixel, a wrong row index would — the destination over the
padded input grid of the conv that follows (pad 1, two front frames) and the residual destination over that conv's output grid (pad 1),
both pure outputs with INTERIOR guards on their border pixels and front frames, which belong to the host.  cfg_pndm_step: the
learned-sigma half of model_out an interior guard, model_in and the history slot pure outputs; the warm-up forms with the sample read
from one buffer and written to another and the accumulator updated in place, the multistep form in place on the sample with three
history sources; sources whose weights are zero are not passed at all."""
import pytest
import torch

import isolation as iso
from isolation import Operand

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def border_mask(g, C):
    """True on every element of the rows of grid ``g`` that is not an interior voxel (border pixels, front frames)."""
    m = torch.ones(g.n, g.T + g.tf, g.Hp, g.Wp, C, dtype=torch.bool, device=dev())
    m[:, g.tf:, g.pad:g.pad + g.H, g.pad:g.pad + g.W] = False
    return m.view(g.rows, C)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("C,T,H,W", [(32, 1, 3, 5), (128, 2, 2, 2), (32, 4, 5, 3)])
def test_isolation_upsample_time2x(C, T, H, W, with_res):
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd.ops import VaeGrid

    gs = VaeGrid(1, T, H, W, 1, 0)
    T2 = 1 if T == 1 else 2 * T - 1
    gd, gr = VaeGrid(1, T2, H, W, 1, 2), VaeGrid(1, T2, H, W, 1, 0)
    x = torch.randn(gs.rows, C, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16).to(dev())
    o = {"x": Operand(x, interior=border_mask(gs, C)),
         "y": Operand(torch.zeros(gd.rows, C, dtype=torch.bfloat16, device=dev()), interior=border_mask(gd, C))}
    if with_res:
        o["y2"] = Operand(torch.zeros(gr.rows, C, dtype=torch.bfloat16, device=dev()), interior=border_mask(gr, C))

    def fn(t):
        vops.upsample_time2x(t["x"], gs, t["y"], gd, C, t.get("y2"), gr if with_res else None, 0.8125)

    iso.check_isolated(fn, o, ["y", "y2"] if with_res else ["y"], what=f"upsample_time2x C={C} T={T} {H}x{W} res={with_res}")


@pytest.mark.parametrize("Bz,thw", [(1, 7), (2, 4096 + 3)])
@pytest.mark.parametrize("call", [0, 1, 3, 12], ids=["prk0", "prk1", "prk3", "plms"])
def test_isolation_cfg_pndm_step(Bz, thw, call):
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    s = PNDMScheduler()
    s.set_timesteps(50)
    k = s.step_coeffs(call)
    kind = k["kind"]
    Cin = 4
    g = torch.Generator().manual_seed(thw + call)
    r = lambda: torch.randn(Bz, Cin, thw, generator=g).to(dev())
    mo = torch.randn(2 * Bz, 2 * Cin, thw, generator=g).to(dev())
    sigma = torch.zeros(2 * Bz, 2 * Cin, thw, dtype=torch.bool, device=dev())
    sigma[:, Cin:] = True
    o = {"mo": Operand(mo, interior=sigma), "mi": Operand(torch.zeros(2 * Bz, Cin, thw, dtype=torch.bfloat16, device=dev()))}
    outs, inplace = ["mi"], []
    if kind == "plms":
        o.update(z=Operand(r()), h1=Operand(r()), h2=Operand(r()), h3=Operand(r()), e=Operand(torch.zeros(Bz, Cin, thw, device=dev())))
        outs += ["z", "e"]
        inplace += ["z"]

        def fn(t):
            vops.cfg_pndm_step(t["mo"], t["mi"], t["z"], 7.5, k["c_base"], k["cz"], k["ca"], base=t["z"], srcs=(t["h1"], t["h2"], t["h3"]),
                               e_out=t["e"])
    else:
        o.update(cur=Operand(r()), z=Operand(torch.zeros(Bz, Cin, thw, device=dev())))
        outs += ["z"]
        if kind == "prk0":                               # the accumulator and the history slot are pure outputs
            o.update(acc=Operand(torch.zeros(Bz, Cin, thw, device=dev())), e=Operand(torch.zeros(Bz, Cin, thw, device=dev())))
            outs += ["acc", "e"]
        else:
            o.update(acc=Operand(r()))
            if kind != "prk3":
                outs += ["acc"]
                inplace += ["acc"]

        def fn(t):
            vops.cfg_pndm_step(t["mo"], t["mi"], t["z"], 7.5, k["c_base"], k["cz"], k["ca"], base=t["cur"], srcs=(t["acc"],),
                               e_out=t.get("e"), aux_out=None if kind == "prk3" else t["acc"])

    iso.check_isolated(fn, o, outs, inplace=inplace, what=f"cfg_pndm_step {kind} Bz={Bz} thw={thw}")
