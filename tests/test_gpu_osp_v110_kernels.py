"""-m gpu: the two kernels the Open-Sora-Plan v1.1 pipeline adds to csrc/vae_osp.hip against their contracts (include/videosys_amd.h).

  * vsys_upsample_time2x: element-wise against float64 F.interpolate(scale_factor=(2, 1, 1), mode="trilinear") of frames 1.. with
    frame 0 copied.  Bound: ONE rounding of the exact value to bf16, rnd(ref), as tests/test_gpu_osp_vae_kernels.py::
    test_upsample_trilinear2x (check_elementwise adds numerics.FLOOR).  The second destination against alpha * v in float64 with the same
    bound of ITS value.  Both destinations are interiors of padded grids whose border and front frames must keep their bits.
  * vsys_cfg_pndm_step: the five call kinds of PNDMScheduler (Runge-Kutta 0, 1, 2, 3 and the multistep) with the coefficients of
    n = 50 at those positions, against float64 on the fp32 operands; |out - ref| <= 4 2^-24 (sum of |terms|) per element for z_out,
    aux_out and e_out (the bound of test_cfg_ancestral_step), model_in within half a bf16 ulp plus that slack, the two CFG halves
    bit-equal, NaN in the learned-sigma channels and in every operand whose weight is zero without influence.  The warm-up calls run
    in the ping-pong form (base and z_out two buffers, aux_out the accumulator source itself), the multistep in place."""
import pytest
import torch
import torch.nn.functional as F

import numerics as nm

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def time2x_ref(x):
    """x [1, C, T, H, W] float64 -> TimeUpsample2x.forward (autoencoder_kl_open_sora_plan_v110.py:1549-1554)."""
    if x.size(2) > 1:
        return torch.cat([x[:, :, :1], F.interpolate(x[:, :, 1:], scale_factor=(2, 1, 1), mode="trilinear")], dim=2)
    return x


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("C,T,H,W", [(32, 1, 3, 5), (128, 2, 2, 2), (32, 4, 5, 3), (256, 3, 2, 2)])
def test_upsample_time2x(C, T, H, W, with_res):
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd.ops import VaeGrid

    x = torch.randn(T * H * W, C, generator=torch.Generator().manual_seed(C + T)).to(torch.bfloat16)
    gs = VaeGrid(1, T, H, W, 1, 0)                      # a conv-output grid, as the decoder hands it over
    T2 = 1 if T == 1 else 2 * T - 1
    gd = VaeGrid(1, T2, H, W, 1, 2)                     # the padded input grid of the causal conv that follows
    gr = VaeGrid(1, T2, H, W, 1, 0)                     # the residual operand: rows of that conv's output grid
    xs = torch.full((gs.rows, C), float("nan"), dtype=torch.bfloat16)
    nm.grid_interior(xs, gs)[:] = x.view(1, T, H, W, C)   # (a NaN border: a tap that left the interior would show)
    sentinel, alpha = 123.0, nm.f32(0.8807970779778823)   # sigmoid(2.0), the reference's initial mix_factor
    y = torch.full((gd.rows, C), sentinel, dtype=torch.bfloat16, device=dev())
    y2 = torch.full((gr.rows, C), sentinel, dtype=torch.bfloat16, device=dev()) if with_res else None
    vops.upsample_time2x(xs.to(dev()), gs, y, gd, C, y2, gr if with_res else None, alpha)
    torch.cuda.synchronize()
    x5 = x.double().view(1, T, H, W, C).permute(0, 4, 1, 2, 3)
    ref = time2x_ref(x5).permute(0, 2, 3, 4, 1)                             # [1, T2, H, W, C]
    what = f"upsample_time2x C={C} T={T} {H}x{W}"
    for out, g, want, name in ((y, gd, ref, "y"),) + (((y2, gr, alpha * ref, "y_res"),) if with_res else ()):
        out = out.cpu()
        got = nm.grid_interior(out, g)
        nm.check_elementwise(got.reshape(-1, C), want.reshape(-1, C), nm.rnd(want).reshape(-1, C), f"{what} {name}")
        # border pixels and the front frames are the conv's padding: never written
        full = nm.grid_view(out.clone(), g)
        nm.grid_interior(full.reshape(g.rows, C), g)[:] = sentinel
        assert torch.equal(full, torch.full_like(full, sentinel)), f"{name}: the kernel wrote outside the interior of its grid"
    if T <= 2:     # frame 0, and both frames of a one-frame range, are the source's bits
        got = nm.grid_interior(y.cpu(), gd)
        for t in range(T2):
            assert torch.equal(got[0, t].view(torch.int16), x.view(T, H, W, C)[min(t, T - 1)].view(torch.int16)), f"{what}: frame {t} is no copy"


def _pndm_calls():
    """(kind, coefficients) of calls 0, 1, 2, 3 (Runge-Kutta) and 12 (multistep) of PNDMScheduler at n = 50."""
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    s = PNDMScheduler()
    s.set_timesteps(50)
    return [s.step_coeffs(i) for i in (0, 1, 2, 3, 12)]


@pytest.mark.parametrize("Bz,thw", [(1, 7), (2, 4096 + 3)])
@pytest.mark.parametrize("call", range(5), ids=["prk0", "prk1", "prk2", "prk3", "plms"])
def test_cfg_pndm_step(Bz, thw, call):
    from videosys_amd import open_sora_plan_v110_ops as vops

    k = _pndm_calls()[call]
    kind = k["kind"]
    Cin, guidance = 4, 7.5
    g = torch.Generator().manual_seed(Bz * 100 + thw + call)
    shape = (Bz, Cin, thw, 1, 1)
    mo = torch.randn(2 * Bz, 2 * Cin, thw, 1, 1, generator=g)
    base = torch.randn(shape, generator=g)
    src = [torch.randn(shape, generator=g) for _ in range(4)]
    u, c = mo[:Bz, :Cin].double(), mo[Bz:, :Cin].double()
    e = u + guidance * (c - u)
    e_abs = u.abs() + guidance * (c.abs() + u.abs())
    S = [e] + [t.double() for t in src]
    Sa = [e_abs] + [t.double().abs() for t in src]
    used = [j for j in range(5) if k["cz"][j] != 0.0 or k["ca"][j] != 0.0]
    z_ref = k["c_base"] * base.double() + sum(k["cz"][j] * S[j] for j in range(5) if k["cz"][j] != 0.0)
    z_abs = abs(k["c_base"]) * base.double().abs() + sum(abs(k["cz"][j]) * Sa[j] for j in range(5))
    stores_aux, stores_e = any(k["ca"]), kind in ("prk0", "plms")
    mo[:, Cin:] = float("nan")                           # the learned-sigma half must have no influence
    for j in range(1, 5):
        if j not in used:
            src[j - 1].fill_(float("nan"))               # an operand whose weights are zero is never read
    d = dev()
    srcs = [t.clone().to(d) for t in src]
    mi = torch.full((2 * Bz, Cin, thw, 1, 1), 9.0, dtype=torch.bfloat16, device=d)
    e_out = torch.full(shape, 5.0, device=d) if stores_e else None
    if kind == "plms":                                   # in place on the sample
        zb = base.clone().to(d)
        base_t, z_out, aux = zb, zb, None
    else:                                                # ping-pong: the other buffer; the accumulator is its own source
        base_t, z_out = base.clone().to(d), torch.full(shape, float("nan"), device=d)
        aux = (srcs[0] if kind != "prk0" else torch.full(shape, float("nan"), device=d)) if stores_aux else None
        if kind == "prk0":
            srcs[0] = aux                                # (weight zero: the accumulator's old content, NaN here, is not read)
    vops.cfg_pndm_step(mo.to(d), mi, z_out, guidance, k["c_base"], k["cz"], k["ca"], base=base_t, srcs=srcs, e_out=e_out, aux_out=aux)
    torch.cuda.synchronize()
    what = f"cfg_pndm_step {kind} Bz={Bz} thw={thw}"
    flat = lambda t: t.reshape(Bz, -1)
    slack = 4 * 2.0**-24 * z_abs
    zo = z_out.cpu()
    nm.check_elementwise(flat(zo), flat(z_ref), flat(slack), what + " z_out")
    if kind != "plms":
        assert torch.equal(base_t.cpu(), base), "the ping-pong form changed the sample the group started from"
    if stores_e:
        nm.check_elementwise(flat(e_out.cpu()), flat(e), flat(4 * 2.0**-24 * e_abs), what + " e_out")
    if stores_aux:
        a_ref = sum(k["ca"][j] * S[j] for j in range(5) if k["ca"][j] != 0.0)
        a_abs = sum(abs(k["ca"][j]) * Sa[j] for j in range(5) if k["ca"][j] != 0.0)
        nm.check_elementwise(flat(aux.cpu()), flat(a_ref), flat(4 * 2.0**-24 * a_abs), what + " aux_out")
    mi = mi.cpu()
    half_ulp = torch.exp2(torch.floor(torch.log2(z_ref.abs().clamp_min(2.0**-120))) - 8)   # bf16: 8 significant bits
    nm.check_elementwise(flat(mi[:Bz]), flat(z_ref), flat(half_ulp + slack), what + " model_in")
    assert torch.equal(mi[:Bz].view(torch.int16), mi[Bz:].view(torch.int16)), "the two CFG halves of model_in differ"
