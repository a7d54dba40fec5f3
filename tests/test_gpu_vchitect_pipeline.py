"""-m gpu: VchitectXLPipeline.generate (videosys_amd/pipeline_vchitect.py) end to end on the tiny synthetic model of
tests/test_gpu_vchitect_model.py (dim 192, depth 2, latent 16 x 16, L = 8) with precomputed embeddings and the synthetic SD3 VAE.

End to end.  The final latent (taken through callback_on_step_end) of a 3-step run against a float64 restatement of the loop: the
model of tests/vchitect_ref.py called twice per step (uncond, text), the flow-match schedule from its closed form (numpy, checked
bit for bit against the scheduler's), the per-step guidance of pipeline_vchitect.py:942-944 and the Euler update.  Bound (the project's):
the same loop with the model in bf16 on the CPU against the float64 loop is the floor; the HIP latent's RMS error against float64
must stay within 1.5 x that floor.  Output: F PIL images of the requested size.  F = 2 and F = 1.

PAB.  Four steps with thresholds that cover all four timesteps: the (temporal, cross, spatial) decisions of the 8 model calls equal the
ones counters restated here give — the counters advance twice per step and wrap at num_inference_steps, so the second call of a step
broadcasts what the first computed.

Replay.  With PAB off the steps after the first replay a recorded program; the final latent equals the forced-eager run bit for bit.

Engine.  VideoSysEngine(VchitectConfig(<synthetic>)).generate(...) once."""
import math

import numpy as np
import pytest
import torch

import vchitect_ref as vr

pytestmark = pytest.mark.gpu

CFG = dict(num_layers=2, heads=3, patch=2, out_channels=16, sample_size=32, pos_embed_max_size=24)
TCFG = dict(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=3, joint_attention_dim=64,
            caption_projection_dim=192, pooled_projection_dim=64, out_channels=16, pos_embed_max_size=24)
SEED, L, JD, PD, HW, GS = 11, 8, 64, 64, 16, 7.5


def config(**kw):
    from videosys_amd import VchitectConfig

    return VchitectConfig(f"synthetic:{SEED}", transformer_config=dict(TCFG), **kw)


def inputs(F):
    g = torch.Generator().manual_seed(100 + F)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    return dict(prompt_embeds=bf(1, L, JD), pooled_prompt_embeds=bf(1, PD), negative_prompt_embeds=bf(1, L, JD),
                negative_pooled_prompt_embeds=bf(1, PD)), bf(1, F, 16, HW, HW)


def schedule(n, shift=1.0, N=1000):
    """(timesteps fp32, sigmas fp32 with the trailing 0) from the closed form, in numpy."""
    sh = lambda s: shift * s / (1 + (shift - 1) * s)
    s0 = sh(np.linspace(1, N, N, dtype=np.float32)[::-1] / np.float32(N)).astype(np.float32)
    s = sh(np.linspace(float(s0[0]) * N, float(s0[-1]) * N, n) / N).astype(np.float32)
    return s * np.float32(N), np.concatenate([s, np.zeros(1, np.float32)])


def restated_loop(emb, z0, steps, dtype):
    """The denoise loop of pipeline_vchitect.py:917-952 with the model in ``dtype`` and the latents in float64."""
    from videosys_amd.vchitect import synth_state_dict

    sd = {k: v.to(torch.bfloat16).float() for k, v in synth_state_dict(2, 3, 16, 16, 2, JD, PD, seed=SEED).items()}
    F = z0.shape[1]
    ts, sig = schedule(steps)
    z = z0.double().clone()
    cast = (lambda t: t.to(dtype)) if dtype != torch.float64 else (lambda t: t)
    for i in range(steps):
        t = float(ts[i])
        tt = torch.tensor([t])
        call = lambda e, p: vr.model_forward(sd, CFG, cast(z.float()), cast(emb[e].expand(F, L, JD)), cast(emb[p]), tt, dtype).double()
        unc = call("negative_prompt_embeds", "negative_pooled_prompt_embeds")
        txt = call("prompt_embeds", "pooled_prompt_embeds")
        gi = 1 + GS * (1 - math.cos(math.pi * ((steps - t) / steps) ** 5.0)) / 2
        z = z + float(sig[i + 1] - sig[i]) * (unc + gi * (txt - unc)).view_as(z)
    return z


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def run(pipe, F, steps, **kw):
    emb, z0 = inputs(F)
    seen = []

    def cb(p, i, t, kwargs):
        seen.append((i, t, kwargs["latents"].clone()))
        return {}

    out = pipe.generate(height=8 * HW, width=8 * HW, frames=F, num_inference_steps=steps, guidance_scale=GS, seed=0, latents=z0,
                        callback_on_step_end=cb, **emb, **kw)
    torch.cuda.synchronize()
    return out, seen


_PIPE = {}


def pipeline():
    if "p" not in _PIPE:
        from videosys_amd import VchitectXLPipeline

        _PIPE["p"] = VchitectXLPipeline(config())
    return _PIPE["p"]


@pytest.mark.parametrize("F", [2, 1])
def test_generate_end_to_end(F):
    from PIL import Image

    from videosys_amd import pab
    from videosys_amd.pipeline import VideoSysPipelineOutput

    pipe = pipeline()
    pab.set_pab_manager(None)
    steps = 3
    ts, sig = schedule(steps)
    out, seen = run(pipe, F, steps)
    assert np.array_equal(pipe.scheduler.timesteps.numpy(), ts) and np.array_equal(pipe.scheduler.sigmas.numpy(), sig)
    assert [s[0] for s in seen] == [0, 1, 2] and [s[1] for s in seen] == [float(t) for t in ts] and pipe.num_timesteps == steps
    emb, z0 = inputs(F)
    want = restated_loop(emb, z0, steps, torch.float64)
    floor = rms(restated_loop(emb, z0, steps, torch.bfloat16), want)
    got = seen[-1][2].cpu()
    err = rms(got, want)
    print(f"[vchitect generate F={F}] HIP rms error {err:.4e}, bf16 floor {floor:.4e}, ratio {err / floor:.3f}, latent rms {float(want.pow(2).mean().sqrt()):.3f}")
    assert got.shape == (1, F, 16, HW, HW) and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert err <= 1.5 * floor, f"generate F={F}: HIP rms error {err:.4e} vs float64 > 1.5 x bf16 floor {floor:.4e}"
    assert isinstance(out, VideoSysPipelineOutput) and len(out.video) == 1 and len(out.video[0]) == F
    for im in out.video[0]:
        assert isinstance(im, Image.Image) and im.size == (8 * HW, 8 * HW) and im.mode == "RGB"
    # the frames are the decoder's bytes of the final latent; "np" gives the same picture as floats in [0, 1]
    u8 = pipe.vae.decode_u8(seen[-1][2]).cpu().numpy()
    assert all(np.array_equal(np.asarray(im), u8[f]) for f, im in enumerate(out.video[0]))
    arr = pipe.decode_frames(seen[-1][2], "np")
    assert len(arr) == F and arr[0].shape == (8 * HW, 8 * HW, 3) and arr[0].dtype == np.float32 and 0.0 <= arr[0].min() <= arr[0].max() <= 1.0
    assert np.array_equal(np.round(arr[0] * 255).astype(np.uint8), u8[0])
    assert pipe.guidance_scale == 1 + GS * (1 - math.cos(math.pi * ((steps - float(ts[-1])) / steps) ** 5.0)) / 2
    lat = pipe.generate(height=8 * HW, width=8 * HW, frames=F, num_inference_steps=steps, guidance_scale=GS, seed=0, latents=z0,
                        output_type="latent", **emb).video
    assert torch.equal(lat.cpu(), got)


def test_replayed_steps_equal_eager_steps_bit_for_bit():
    from videosys_amd import pab

    pipe = pipeline()
    pab.set_pab_manager(None)
    pipe._steps.entries = {}
    before = dict(pipe.step_stats)
    _, seen = run(pipe, 2, 3, output_type="latent")
    assert pipe.step_stats["recorded"] - before["recorded"] == 1 and pipe.step_stats["replayed"] - before["replayed"] == 2
    _, again = run(pipe, 2, 3, output_type="latent")                 # same geometry and embeddings: the program is reused
    assert pipe.step_stats["recorded"] - before["recorded"] == 1 and pipe.step_stats["replayed"] - before["replayed"] == 5
    pipe.transformer.use_programs = False
    try:
        _, eager = run(pipe, 2, 3, output_type="latent")
    finally:
        pipe.transformer.use_programs = True
    assert pipe.step_stats["eager"] - before["eager"] == 3
    for a, b, c in zip(seen, again, eager):
        assert torch.equal(a[2], c[2]) and torch.equal(b[2], c[2]), f"step {a[0]}: replayed and eager latents differ"
    # an interrupt set by the callback skips the remaining steps
    emb, z0 = inputs(2)
    calls = []

    def stop(p, i, t, kw):
        calls.append(i)
        p._interrupt = True
        return {}

    out = pipe.generate(height=8 * HW, width=8 * HW, frames=2, num_inference_steps=3, guidance_scale=GS, seed=0, latents=z0,
                        output_type="latent", callback_on_step_end=stop, **emb).video
    assert calls == [0] and pipe.interrupt and torch.equal(out, seen[0][2])


def test_new_embeddings_of_the_same_shape_drop_the_recorded_pair():
    """The rule of ``_step_buffers`` (program.StepCache's table): a recorded pair holds the addresses of its resident buffers, and
    embeddings that differ get new buffers, so the pair is recorded again — also when the first embeddings come back.  Expected from
    the rule, per generate() of 3 steps: 1 recorded (the first step) + 2 replayed, three times over; nothing eager.  Every output
    equals what a freshly built pipeline gives for those embeddings."""
    from videosys_amd import VchitectXLPipeline, pab

    pipe = pipeline()
    pab.set_pab_manager(None)
    emb_a, z0 = inputs(2)
    emb_b = {k: v.flip(-1).contiguous() for k, v in emb_a.items()}
    assert all(emb_b[k].shape == emb_a[k].shape and not torch.equal(emb_b[k], emb_a[k]) for k in emb_a)

    def latents(p, emb):
        out = p.generate(height=8 * HW, width=8 * HW, frames=2, num_inference_steps=3, guidance_scale=GS, seed=0, latents=z0,
                         output_type="latent", **emb).video.clone()
        torch.cuda.synchronize()
        return out

    def fresh():
        return VchitectXLPipeline(config(), text_encoder=pipe.text_encoder, text_encoder_2=pipe.text_encoder_2,
                                  text_encoder_3=pipe.text_encoder_3, tokenizer=pipe.tokenizer, tokenizer_2=pipe.tokenizer_2)

    want = {"a": latents(fresh(), emb_a), "b": latents(fresh(), emb_b)}
    assert not torch.equal(want["a"], want["b"])
    pipe._steps.entries = {}
    for name, emb in (("a", emb_a), ("b", emb_b), ("a", emb_a)):
        before = dict(pipe.step_stats)
        got = latents(pipe, emb)
        delta = {k: pipe.step_stats[k] - before[k] for k in before}
        assert delta == {"recorded": 1, "replayed": 2, "eager": 0}, (name, delta)
        assert len(pipe._steps) == 1 and torch.equal(got, want[name]), f"embeddings {name}: not the fresh pipeline's latents"


def test_pab_decisions_of_the_eight_calls():
    from videosys_amd import VchitectPABConfig, VchitectXLPipeline, pab

    rule = dict(spatial=2, temporal=3, cross=4)
    pc = VchitectPABConfig(spatial_threshold=[0, 1001], spatial_range=2, temporal_threshold=[0, 1001], temporal_range=3,
                           cross_threshold=[0, 1001], cross_range=4)
    steps = 4
    free = run(pipeline_free(), 2, steps, output_type="latent")[1]
    try:
        pipe = VchitectXLPipeline(config(enable_pab=True, pab_config=pc))      # installs the PAB manager
        out, seen = run(pipe, 2, steps, output_type="latent")
        assert pipe.step_stats == {"recorded": 0, "replayed": 0, "eager": steps}
        ts, _ = schedule(steps)
        count, want = dict(spatial=0, temporal=0, cross=0), []
        for t in ts:
            for _ in range(2):                                       # uncond, then text: one module, two calls
                d = {}
                for kind in ("temporal", "cross", "spatial"):
                    d[kind] = count[kind] % rule[kind] != 0 and 0 < int(t) < 1001
                    count[kind] = (count[kind] + 1) % steps
                want.append((d["temporal"], d["cross"], d["spatial"]))
        assert len(pipe.pab_trace) == 8
        assert pipe.pab_trace == [[w, w] for w in want], (pipe.pab_trace, want)
        assert want[0] == (False, False, False) and want[1] == (True, True, True)      # the text call of step 0 reuses the uncond call's branches
        assert all(any(w[k] for w in want) for k in range(3))
        assert torch.isfinite(seen[-1][2]).all() and not torch.equal(seen[-1][2], free[-1][2])
    finally:
        pab.set_pab_manager(None)


def pipeline_free():
    from videosys_amd import pab

    p = pipeline()
    pab.set_pab_manager(None)
    return p


def test_engine_generates_once():
    from PIL import Image

    from videosys import VideoSysEngine
    from videosys_amd import pab

    emb, z0 = inputs(2)
    engine = VideoSysEngine(config())
    try:
        out = engine.generate(height=8 * HW, width=8 * HW, frames=2, num_inference_steps=2, guidance_scale=GS, seed=0, latents=z0, **emb)
        frames = out.video[0]
        assert len(frames) == 2 and all(isinstance(f, Image.Image) and f.size == (8 * HW, 8 * HW) for f in frames)
    finally:
        engine.shutdown()
        pab.set_pab_manager(None)
