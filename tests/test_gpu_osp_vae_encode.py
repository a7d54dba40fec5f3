"""-m gpu: the Open-Sora-Plan v1.2 CausalVAE ENCODE on HIP against the float64 posterior moments of the reference's own CausalVAEModel
(tests/golden/osp_vae_encode_small.pt, tools/mint_osp_vae_encode.py; hidden_size 32, T = 5 and T = 1).  Bound (the decoder test's,
computed the same way): the RMS error of the HIP mean and logvar stays within 1.5 x the bf16 floor — the restatement
(tests/test_osp_vae_encode_cpu.py ``moments``, held to the fixture at 1e-9 there) run in bf16 on the CPU, computed here."""
import functools

import pytest
import torch

import test_osp_vae_encode_cpu as E

pytestmark = pytest.mark.gpu
fixture = functools.lru_cache(maxsize=None)(E.fixture)


DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def weights():
    from videosys_amd.vae_open_sora_plan import synth_state_dict

    return synth_state_dict(fixture()["seed"], fixture()["hidden_size"], encoder=True)


@functools.lru_cache(maxsize=None)
def wrapper():
    from videosys_amd.vae_open_sora_plan import CausalVAEModelWrapper

    return CausalVAEModelWrapper(weights(), device=DEV, **fixture()["kwargs"])


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("name", ["x5", "x1"])
def test_posterior_within_bf16_floor(name):
    fx = fixture()
    post = wrapper().vae.encode(fx[name].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(post.mode(), post.mean) and post.mean.dtype == torch.float32
    low = E.moments(fx[name], weights(), dtype=torch.bfloat16)
    for part, out, floor_of in (("mean", post.mean, low[0]), ("logvar", post.logvar, low[1])):
        ref = fx[f"{name}_{part}"]
        assert tuple(out.shape) == tuple(ref.shape)
        floor, err = rms(floor_of - ref), rms(out.cpu().double() - ref)
        print(f"{name} {part}: HIP rms error {err:.4e}, bf16 floor {floor:.4e} (ratio {err / floor:.3f}), reference rms {rms(ref):.3f}")
        assert floor < 0.05 * rms(ref), "the floor is vacuous"
        assert err <= 1.5 * floor, f"{name} {part}: HIP rms error {err:.4e} > 1.5 x the bf16 floor {floor:.4e}"


def test_wrapper_encode_samples_its_own_posterior():
    x = fixture()["x5"].to(DEV)
    z = wrapper().encode(x, generator=torch.Generator().manual_seed(11))
    post = wrapper().vae.encode(x)
    noise = torch.randn(post.mean.shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    assert z.shape == post.mean.shape and torch.equal(z, (post.mean + torch.exp(0.5 * post.logvar) * noise) * 0.18215)


def test_recorded_encode_replays_the_eager_bits():
    from videosys_amd import program

    enc, x = wrapper().vae.encoder, fixture()["x5"].to(DEV)
    eager = enc.moments(x).clone()            # (also leaves the staging buffers of this geometry resident)
    with program.Recorder() as rec:
        out = enc.moments(x)
    prog = rec.finish()
    assert prog is not None, rec.invalid
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    for _ in range(2):
        out.fill_(float("nan"))
        prog.run()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "the replayed encode differs from the eager one"
