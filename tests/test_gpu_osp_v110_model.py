"""-m gpu: the HIP Open-Sora-Plan v1.1 transformer (videosys_amd/open_sora_plan_v110.py) on the cases, inputs and weights recipe of
tests/golden/osp_v110_fwd_small.pt at 8 heads instead of 2 (fx["wide_heads"]: the HIP GEMMs take hidden sizes that are multiples of 192
and 64, so 576 is the smallest 72-per-head model they run; the restatement is pinned to the class at both head counts): every fixture case within 1.5 x the bf16 floor of tests/osp_v110_ref.py (its bf16 run against its
float64 run, max abs — the rule of tests/test_gpu_osp_model.py; the restatement is pinned to the reference's own class by
tests/test_osp_v110_cpu.py), the three-step PAB sequence, use_rope=False against latte.py's un-roped path on the same weights, and
bit-equal repeated calls.  The reference (float64 and bf16 runs of every case) is computed once per session."""
import pytest
import torch

import test_osp_v110_cpu as C
from test_osp_v110_cpu import fx  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu
HEADS = 8


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return "cuda:0"


@pytest.fixture(scope="module")
def refs(fx):  # noqa: F811
    sd = C.state_dict(fx, heads=HEADS)
    return {name: (C.run_case(fx, name, torch.float64, sd, HEADS), C.run_case(fx, name, torch.bfloat16, sd, HEADS).double()) for name in C.CASES}


def hip_model(fx, kwargs=None, **over):  # noqa: F811
    from videosys_amd import open_sora_plan_v110 as m

    model = m.LatteT2V(**{**(kwargs or fx["kwargs"]), **fx["wide_heads"], **over}, device=dev())
    return model.load_state_dict(C.state_dict(fx, heads=HEADS))


def run_hip(fx, model, name):  # noqa: F811
    xk, masked, _, _ = C.CASES[name]
    t = torch.tensor([fx["timestep"]] * 2)
    out = model(fx[xk].float(), timestep=t, encoder_hidden_states=fx["encoder_hidden_states"].float(),
                encoder_attention_mask=fx["encoder_attention_mask"] if masked else None, return_dict=False)
    assert isinstance(out, tuple) and len(out) == 1
    torch.cuda.synchronize()
    return out[0].double().cpu()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_hip_model_within_the_bf16_floor(fx, refs, name):  # noqa: F811
    _, _, kwk, over = C.CASES[name]
    out = run_hip(fx, hip_model(fx, fx[kwk] if kwk else None, **over), name)
    f64, bf = refs[name]
    floor, err = (bf - f64).abs().max().item(), (out - f64).abs().max().item()
    print(f"{name}: err {err:.4f}, bf16 floor {floor:.4f}, output max {f64.abs().max().item():.3f}")
    assert out.shape == f64.shape and err <= 1.5 * floor


def test_hip_model_at_1024_tokens_per_frame(fx):  # noqa: F811
    """The production grid: sample_size (64, 64) at patch 2 = 32 x 32 = 1 024 tokens per frame, where the spatial attention runs the
    three-workgroup roped flash kernel (whole tiles, >= 512 keys) that the fixture's 16- to 256-token frames never reach.  Two
    frames, the fixture's text and weight recipe, a seeded input; same rule: 1.5 x the restatement's bf16 floor."""
    over = dict(sample_size=(64, 64), video_length=2)
    g = torch.Generator().manual_seed(fx["seed"] + 64)
    x = torch.randn(2, 4, 2, 64, 64, generator=g).to(torch.bfloat16).float()
    t = torch.tensor([fx["timestep"]] * 2)
    enc, mask = fx["encoder_hidden_states"].float(), fx["encoder_attention_mask"]
    sd = C.state_dict(fx, heads=HEADS)
    with torch.no_grad():
        f64, bf = (C.ref_model(fx, sd, dt, num_attention_heads=HEADS, **over)(x, t, enc, mask).double() for dt in (torch.float64, torch.bfloat16))
    out = hip_model(fx, **over)(x, timestep=t, encoder_hidden_states=enc, encoder_attention_mask=mask, return_dict=False)[0]
    torch.cuda.synchronize()
    floor, err = (bf - f64).abs().max().item(), (out.double().cpu() - f64).abs().max().item()
    print(f"1024 tokens per frame: err {err:.4f}, bf16 floor {floor:.4f}, output max {f64.abs().max().item():.3f}")
    assert err <= 1.5 * floor


def test_hip_model_pab_sequence(fx):  # noqa: F811
    from videosys_amd import pab

    sd = C.state_dict(fx, heads=HEADS)
    ts = fx["pab_timesteps"]
    enc, mask, ats = fx["encoder_hidden_states"].float(), fx["encoder_attention_mask"], torch.tensor(ts)

    def sequence(run):
        pab.set_pab_manager(pab.PABConfig(**fx["pab"]))
        try:
            pab.update_steps(len(ts))
            return [run(i, t) for i, t in enumerate(ts)]
        finally:
            pab.set_pab_manager(None)

    outs = {}
    for dtype in (torch.float64, torch.bfloat16):
        m = C.ref_model(fx, sd, dtype, num_attention_heads=HEADS)
        with torch.no_grad():
            outs[dtype] = sequence(lambda i, t: m(fx["pab_x"][i].float(), torch.tensor([t, t]), enc, mask, all_timesteps=ats).double())
    model = hip_model(fx)
    model.reset_pab_state()

    def hip(i, t):
        o = model(fx["pab_x"][i].float(), timestep=torch.tensor([t, t]), all_timesteps=ats, encoder_hidden_states=enc,
                  encoder_attention_mask=mask, return_dict=False)[0]
        torch.cuda.synchronize()
        return o.double().cpu()

    got = sequence(hip)
    for i in range(len(ts)):
        floor, err = (outs[torch.bfloat16][i] - outs[torch.float64][i]).abs().max().item(), (got[i] - outs[torch.float64][i]).abs().max().item()
        print(f"PAB step {i}: err {err:.4f}, bf16 floor {floor:.4f}")
        assert err <= 1.5 * floor, f"PAB step {i}"


def test_use_rope_false_is_the_unroped_latte_path(fx):  # noqa: F811
    """Same weights through latte.LatteT2V (plain kernels, no permutation): the same bits."""
    from videosys_amd import latte

    k = fx["kwargs"]
    out = run_hip(fx, hip_model(fx, use_rope=False), "norope")
    plain = latte.LatteT2V(num_attention_heads=HEADS, attention_head_dim=72, in_channels=k["in_channels"],
                           out_channels=k["out_channels"], num_layers=k["num_layers"], cross_attention_dim=HEADS * 72,
                           sample_size=k["sample_size"][0], patch_size=k["patch_size"], caption_channels=k["caption_channels"],
                           video_length=k["video_length"], device=dev())
    sd = {n: v for n, v in C.state_dict(fx, heads=HEADS).items() if n != "caption_projection.y_embedding"}
    plain.load_state_dict(sd)
    want = plain(fx["x"].float(), timestep=torch.tensor([fx["timestep"]] * 2), encoder_hidden_states=fx["encoder_hidden_states"][:, 0].float(),
                 encoder_attention_mask=fx["encoder_attention_mask"], return_dict=False)[0]
    torch.cuda.synchronize()
    assert torch.equal(out, want.double().cpu())


def test_two_calls_give_the_same_bits(fx):  # noqa: F811
    model = hip_model(fx)
    assert torch.equal(run_hip(fx, model, "rope"), run_hip(fx, model, "rope"))
