"""-m gpu: the Open-Sora-Plan v1.1 CausalVAE ENCODE on HIP against the float64 posterior moments of the reference's own v1.1 CausalVAEModel
(tests/golden/osp_v110_vae_encode_small.pt, tools/mint_osp_v110_vae_encode.py; hidden_size 32, 32 x 32 pixels, T = 9, 8 and 1, temporal
downsamplers (Res, Res) and (Res, pool-only)).  Bound: the RMS error of the HIP mean and logvar stays within 1.5 x the bf16 floor — the
restatement (tests/test_osp_v110_vae_encode_cpu.py ``moments``, held to the fixture at 1e-9 there) run in bf16 on the CPU, computed here."""
import functools

import pytest
import torch

import test_osp_v110_vae_encode_cpu as E

pytestmark = pytest.mark.gpu
fixture = E.fixture
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def wrapper(cfg):
    from videosys.models.autoencoders.autoencoder_kl_open_sora_plan_v110 import CausalVAEModelWrapper

    return CausalVAEModelWrapper(E.weights(cfg), device=DEV, **dict(fixture()["kwargs"], encoder_temporal_downsample=fixture()["configs"][cfg]))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("cfg", ["res", "mix"])
@pytest.mark.parametrize("name", list(E.INPUTS))
def test_posterior_within_bf16_floor(name, cfg):
    fx, x = fixture(), fixture()[name].to(DEV)
    post = wrapper(cfg).vae.encode(x)
    torch.cuda.synchronize()
    assert torch.equal(post.mode(), post.mean) and post.mean.dtype == torch.float32
    low = E.moments(fx[name], E.weights(cfg), fx["configs"][cfg], dtype=torch.bfloat16)
    for part, out, floor_of in (("mean", post.mean, low[0]), ("logvar", post.logvar, low[1])):
        ref = fx[f"{name}_{cfg}_{part}"]
        assert tuple(out.shape) == tuple(ref.shape) == E.INPUTS[name]
        floor, err = rms(floor_of - ref), rms(out.cpu().double() - ref)
        print(f"{name} {cfg} {part}: HIP rms error {err:.4e}, bf16 floor {floor:.4e} (ratio {err / floor:.3f}), reference rms {rms(ref):.3f}")
        assert floor < 0.05 * rms(ref), "the floor is vacuous"
        assert err <= 1.5 * floor, f"{name} {cfg} {part}: HIP rms error {err:.4e} > 1.5 x the bf16 floor {floor:.4e}"
    again = wrapper(cfg).vae.encode(x)
    assert torch.equal(again.parameters, post.parameters), "a second encode of the same clip differs from the first"


def test_wrapper_encode_samples_its_own_posterior():
    x = fixture()["x9"].to(DEV)
    z = wrapper("res").encode(x, generator=torch.Generator().manual_seed(11))
    post = wrapper("res").vae.encode(x)
    noise = torch.randn(post.mean.shape, generator=torch.Generator().manual_seed(11)).to(DEV)
    assert z.shape == post.mean.shape and torch.equal(z, (post.mean + torch.exp(0.5 * post.logvar) * noise) * 0.18215)


@pytest.mark.parametrize("cfg", ["res", "mix"])
def test_recorded_encode_replays_the_eager_bits(cfg):
    from videosys_amd import program

    enc, x = wrapper(cfg).vae.encoder, fixture()["x9"].to(DEV)
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


def test_decoder_only_state_dict_cannot_encode():
    from videosys_amd.vae_open_sora_plan_v110 import CausalVAEModel, synth_state_dict

    vae = CausalVAEModel(synth_state_dict(fixture()["seed"], 32), device=DEV)
    assert vae.encoder is None
    with pytest.raises(RuntimeError, match="decode only"):
        vae.encode(fixture()["x1"].to(DEV))
    with pytest.raises(NotImplementedError, match="encode"):
        wrapper("res").vae.tiled_encode(fixture()["x1"].to(DEV))
