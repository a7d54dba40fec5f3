"""-m gpu: the CogVideoX VAE ENCODE on HIP against the float64 posterior moments of the reference's own AutoencoderKLCogVideoX
(tests/golden/cogvideox_vae_encode_small.pt, tools/mint_cogvideox_vae_encode.py; 16 x 16 pixels, T = 9, 8 and 1).  Bound: the RMS error
of the HIP mean and logvar stays within 1.5 x the bf16 floor — the restatement (tests/test_cogvideox_vae_encode_cpu.py ``moments``, held
to the fixture at 1e-9 there) run in bf16 on the CPU, computed here."""
import functools

import pytest
import torch

import test_cogvideox_vae_encode_cpu as E

pytestmark = pytest.mark.gpu
fixture = functools.lru_cache(maxsize=None)(E.fixture)
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def weights():
    from videosys_amd.vae_cogvideox import synth_state_dict

    return synth_state_dict(fixture()["seed"], encoder=True)


@functools.lru_cache(maxsize=None)
def vae():
    from videosys.models.autoencoders.autoencoder_kl_cogvideox import AutoencoderKLCogVideoX

    return AutoencoderKLCogVideoX(weights(), device=DEV)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("name", E.INPUTS)
def test_posterior_within_bf16_floor(name):
    fx, x = fixture(), fixture()[name].to(DEV)
    post = vae().encode(x).latent_dist
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
    again, = vae().encode(x, return_dict=False)                  # a 1-tuple, and a fresh state: the second encode gives the same bits
    assert torch.equal(again.parameters, post.parameters), "a second encode of the same clip differs from the first"


def test_recorded_encode_replays_the_eager_bits():
    from videosys_amd import program

    x = fixture()["x9"].to(DEV)
    eager = vae().moments(x).clone()          # (also leaves the staging buffers of this geometry resident)
    with program.Recorder() as rec:
        out = vae().moments(x)
    prog = rec.finish()
    assert prog is not None, rec.invalid
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    for _ in range(2):
        out.fill_(float("nan"))
        prog.run()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "the replayed encode differs from the eager one"


def test_decoder_only_state_dict_cannot_encode():
    from videosys_amd.vae_cogvideox import CogVideoXVAE, synth_state_dict

    with pytest.raises(RuntimeError, match="encoder.conv_in.conv"):
        CogVideoXVAE(synth_state_dict(fixture()["seed"]), device=DEV).encode(fixture()["x1"].to(DEV))
