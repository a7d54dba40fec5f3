"""-m gpu: the Open-Sora-Plan v1.1 CausalVAE decode on HIP (videosys_amd/vae_open_sora_plan_v110.py) against the float64 outputs of the
reference's own v1.1 CausalVAEModel (tests/golden/osp_v110_vae_small*.pt, tools/mint_osp_v110_vae.py), hidden_size 32, the fixture's
weights.

Bound (the project's, as tests/test_gpu_osp_vae.py): the RMS error of the HIP decode against the fixture stays within 1.5 x the bf16
floor — the restatement (tests/osp_v110_vae_ref.py, held to the fixture at 1e-9 by tests/test_osp_v110_vae_cpu.py) run in bf16 on the
CPU against the same float64 output, computed here; the floor itself must be below 5 % of the output's RMS, or it would bound nothing.
Cases: (a) [1, 4, 3, 6, 8] untiled, (b) the same latent tiled (two temporal chunks, 2 x 3 spatial tiles with smaller edge tiles),
(c) T = 1, (d) T = 2, all with TimeUpsampleRes2x; (e) [1, 4, 2, 4, 4] with TimeUpsample2x.  The tiled output must differ from the untiled
one, and the uint8 frames of the pipeline's post-process are exact against the truncating contract on the decoder's own bf16 output."""
import functools

import pytest
import torch

import osp_v110_vae_ref as R
from test_osp_v110_vae_cpu import PLAIN, case, fixture, weights

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def hip_decode(name):
    from videosys_amd.vae_open_sora_plan_v110 import CausalVAEModelWrapper

    z, tiling, plain = case(name)
    w = CausalVAEModelWrapper(weights(plain), device=dev(), **(dict(decoder_temporal_upsample=PLAIN) if plain else {}))
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


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_decode_within_bf16_floor(name):
    z, tiling, plain = case(name)
    ref = fixture()[name]
    out = hip_decode(name)
    assert tuple(out.shape) == tuple(ref.shape) == (1, 4 * (z.shape[2] - 1) + 1, 3, 8 * z.shape[3], 8 * z.shape[4])
    floor = rms(R.wrapper_decode(z, weights(plain), tiling, dtype=torch.bfloat16).double() - ref)
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


def test_uint8_frames_are_exact_against_the_truncating_contract():
    """OpenSoraPlanV110Pipeline.decode_latents on the fixture's weights: the bytes are ((v / 2 + 0.5).clamp(0, 1) * 255).to(uint8) of the
    decoder's own bf16 video, evaluated with torch's bf16 tensor ops (pipeline_open_sora_plan.py:1184-1190)."""
    from videosys_amd.pipeline_open_sora_plan_v110 import OpenSoraPlanV110Pipeline
    from videosys_amd.vae_open_sora_plan_v110 import CausalVAEModelWrapper

    z = case("d")[0]
    p = OpenSoraPlanV110Pipeline.__new__(OpenSoraPlanV110Pipeline)
    p.vae = CausalVAEModelWrapper(weights(), device=dev())
    p._config = None
    got = p.decode_latents(z.to(dev()))
    video = hip_decode("d").to(torch.bfloat16)                                   # [1, T, 3, H, W]
    want = ((video / 2.0 + 0.5).clamp(0, 1) * 255).to(dtype=torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 5, 48, 64, 3) and torch.equal(got, want)
    assert len(torch.unique(got)) > 16, "a degenerate video: the check would say little"


def test_wrapper_surface():
    from videosys_amd.vae_open_sora_plan_v110 import CausalVAEModelWrapper

    w = CausalVAEModelWrapper("synthetic:3", device=dev(), hidden_size=32)
    v = w.vae
    assert (v.use_tiling, v.tile_overlap_factor, v.tile_sample_min_size, v.tile_latent_min_size, v.tile_sample_min_size_t,
            v.tile_latent_min_size_t) == (False, 0.25, 256, 32, 65, 17)
    assert v.temporal == ("", "", "TimeUpsampleRes2x", "TimeUpsampleRes2x") and sorted(v.time_ups) == [2, 3]
    assert abs(v.time_ups[2].alpha - v.time_ups[3].alpha) > 1e-3
    v.enable_tiling()
    assert v.use_tiling
    v.disable_tiling()
    assert not v.use_tiling
    out = w.decode(torch.zeros(1, 4, 1, 2, 2, device=dev()), group=None)
    assert tuple(out.shape) == (1, 1, 3, 16, 16)
