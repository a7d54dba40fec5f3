"""-m gpu: the Open-Sora-Plan v1.2 CausalVAE decode on HIP (videosys_amd/vae_open_sora_plan.py) against the float64 outputs of the
reference's own CausalVAEModel (tests/golden/osp_vae_small*.pt, tools/mint_osp_vae.py), hidden_size 32, the fixture's weights.

Bound (the project's): the RMS error of the HIP decode against the fixture stays within 1.5 x the bf16 floor — the restatement
(tests/osp_vae_ref.py, held to the fixture at 1e-9 by tests/test_osp_pipeline_cpu.py) run in bf16 on the CPU against the same float64
output, computed here.  Cases: (a) [1, 4, 3, 6, 8] untiled, (b) the same latent tiled (two temporal chunks, 2 x 3 spatial tiles with
smaller edge tiles), (c) T = 1, (d) T = 2.  The tiled output must also differ from the untiled one: tiling changes the result, and a
decoder that ignored ``use_tiling`` would pass (a) twice."""
import functools
import os

import pytest
import torch

import osp_vae_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture():
    fx = dict(torch.load(os.path.join(GOLDEN, "osp_vae_small.pt"), weights_only=True))
    fx["a"] = torch.load(os.path.join(GOLDEN, "osp_vae_small_a.pt"), weights_only=True)["a"]
    fx["b"] = torch.load(os.path.join(GOLDEN, "osp_vae_small_b.pt"), weights_only=True)["b"]
    return fx


@functools.lru_cache(maxsize=None)
def weights():
    from videosys_amd.vae_open_sora_plan import synth_state_dict

    fx = fixture()
    return synth_state_dict(fx["seed"], fx["hidden_size"])


def case(name):
    fx = fixture()
    z = fx["z"]
    return {"a": (z, None), "b": (z, fx["tiling"]), "c": (z[:, :, :1], None), "d": (z[:, :, :2], None)}[name]


@functools.lru_cache(maxsize=None)
def hip_decode(name):
    from videosys_amd.vae_open_sora_plan import CausalVAEModelWrapper

    z, tiling = case(name)
    w = CausalVAEModelWrapper(weights(), device=dev())
    if tiling:
        for k, v in tiling.items():
            setattr(w.vae, k, v)
        w.vae.enable_tiling()
    out = w.decode(z.to(dev()))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16
    return out.float().cpu()


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_decode_within_bf16_floor(name):
    z, tiling = case(name)
    ref = fixture()[name]
    out = hip_decode(name)
    assert tuple(out.shape) == tuple(ref.shape) == (1, 4 * (z.shape[2] - 1) + 1, 3, 8 * z.shape[3], 8 * z.shape[4])
    floor = rms(R.wrapper_decode(z, weights(), tiling, dtype=torch.bfloat16).double() - ref)
    err = rms(out.double() - ref)
    print(f"case {name}: HIP rms error {err:.4e}, bf16 floor {floor:.4e} (ratio {err / floor:.3f}), output rms {rms(ref):.3f}")
    assert floor < 0.05 * rms(ref), "the floor is vacuous"
    assert err <= 1.5 * floor, f"case {name}: HIP rms error {err:.4e} > 1.5 x the bf16 floor {floor:.4e}"


def test_tiling_changes_the_result():
    a, b = hip_decode("a"), hip_decode("b")
    assert not torch.equal(a, b), "the tiled decode equals the untiled one bit for bit: use_tiling was ignored"
    fx = fixture()
    # ... and it moves the way the reference's tiling moves it: the tiled HIP output is nearer the tiled reference than the untiled one
    assert rms(b.double() - fx["b"]) < rms(b.double() - fx["a"])


def test_wrapper_surface():
    from videosys_amd.vae_open_sora_plan import CausalVAEModelWrapper

    w = CausalVAEModelWrapper(weights(), device=dev())
    v = w.vae
    assert (v.use_tiling, v.tile_overlap_factor, v.tile_sample_min_size, v.tile_latent_min_size, v.tile_sample_min_size_t,
            v.tile_latent_min_size_t) == (False, 0.125, 256, 32, 33, 16)
    v.enable_tiling()
    assert v.use_tiling
    v.disable_tiling()
    assert not v.use_tiling
