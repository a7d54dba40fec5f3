"""-m gpu: OpenSoraPlanPipeline (videosys_amd/pipeline_open_sora_plan.py) end to end at a small geometry — OpenSoraT2V with 2 layers,
2 heads x 96, caption_channels 32, out_channels 8, latent [1, 4, 3, 8, 12], a 2-layer synthetic text encoder over the mT5 vocabulary,
the hidden_size-32 CausalVAE, 3 steps.

Sampler.  The HIP loop against a float64 restatement — tests/osp_ref.py for the model, the Euler-ancestral closed form for the step —
fed the identical per-step noise (drawn on the device from an identically seeded generator, in the pipeline's order).  Bound (the
project's): RMS error of the final latents within 1.5 x the bf16 FLOOR, the same restatement run the way the reference runs it in bf16
(bf16 latents and model, the step in fp32, :1109-1161) against its float64 self.  Replay equals eager bit for bit; the PAB decision
sequence equals the pab module's; masked text positions have no influence.

Output.  ``output_type="latents"``; uint8 frames equal the reference's post-process (:1186-1188) restated with torch bf16 ops on the
pipeline's own bf16 decode, exactly; frames are cropped to ``num_frames``; one VideoSysEngine round trip; the synthetic encoder at
the mT5 vocabulary and 512 tokens against oracle/t5_oracle.py inside the bound tests/test_gpu_t5.py uses."""
import math

import pytest
import torch
import torch.nn.functional as F

import osp_ref

pytestmark = pytest.mark.gpu

TCFG = dict(num_attention_heads=2, attention_head_dim=96, in_channels=4, out_channels=8, num_layers=2, cross_attention_dim=192,
            attention_bias=True, sample_size=(8, 12), sample_size_t=3, patch_size=2, patch_size_t=1, activation_fn="gelu-approximate",
            norm_type="ada_norm_single", norm_elementwise_affine=False, norm_eps=1e-6, caption_channels=32, use_rope=True,
            interpolation_scale_h=1.0, interpolation_scale_w=1.0, interpolation_scale_t=1.0)
SEED, STEPS, GS, LMAX = 1204, 3, 4.5, 24
ZSHAPE = (1, 4, 3, 8, 12)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def config(**over):
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanConfig

    kw = dict(transformer=f"synthetic:{SEED}", text_encoder="synthetic:3", transformer_config=dict(TCFG), vae_config=dict(hidden_size=32),
              num_frames=9)
    kw.update(over)
    return OpenSoraPlanConfig(**kw)


_PIPE = {}


def pipeline(**over):
    """One pipeline per configuration for the whole module (construction draws the mT5-sized embedding table)."""
    from videosys_amd import pab
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanPipeline

    key = tuple(sorted((k, repr(v)) for k, v in over.items()))
    if key not in _PIPE:
        _PIPE[key] = OpenSoraPlanPipeline(config(**over), device=dev())
    p = _PIPE[key]
    c = p._config
    pab.set_pab_manager(c.pab_config if c.enable_pab else None)
    return p


def rms(a, b):
    return float(((a.double() - b.double()) ** 2).mean().sqrt())


def state_dict():
    from videosys_amd.open_sora_plan import synth_state_dict

    return synth_state_dict(num_layers=2, num_heads=2, caption_channels=32, in_channels=4, out_channels=8, patch_size=2, seed=SEED)


def embeds(pipe, prompts):
    """(prompt_embeds, mask, negative_prompt_embeds, negative mask) of the pipeline's own text encoder at LMAX tokens, on the CPU."""
    e = pipe.encode_prompt_v120(prompts, True, negative_prompt="", max_sequence_length=LMAX)
    return tuple(t.float().cpu() if t.is_floating_point() else t.cpu() for t in e)


def start(batch=1, seed=5):
    return torch.randn((batch,) + ZSHAPE[1:], generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float()


def device_noise(shape, seed, n):
    """The pipeline's per-step draws: torch.randn on the device from a generator seeded ``seed``, one per step that has sigma_up > 0."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    return [torch.randn(shape, generator=g, dtype=torch.float32, device=dev()).cpu() for _ in range(n)]


def restated_loop(e, z0, noises, dtype, steps=STEPS):
    """pipeline_open_sora_plan.py:1104-1161 with osp_ref.forward as the transformer, in ``dtype`` (float64: every operation; bf16: the
    latents and the model in bf16, the scheduler step in fp32 with its result cast back, as diffusers does)."""
    from videosys_amd.pipeline_open_sora_plan import EulerAncestralDiscreteScheduler

    pe, pm, ne, nm = e
    sch = EulerAncestralDiscreteScheduler()
    sch.set_timesteps(steps)
    enc = torch.cat([ne, pe], 0)[:, None]
    mask = torch.cat([nm, pm], 0)[:, None]
    sd = state_dict()
    cos, sin = osp_ref.rope_tables(3, 4, 6, 96, torch.bfloat16)
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    z = (z0.to(wide) * sch.init_noise_sigma).to(dtype)
    B = z.shape[0]
    for i, t in enumerate(sch.timesteps.tolist()):
        x = torch.cat([z, z], 0)
        # scale_model_input: in float64 the exact factor; in bf16 diffusers' own expression on the bf16 sample and the fp32 sigma
        x = x * sch.in_scale(i) if dtype == torch.float64 else x / ((sch.sigmas[i] ** 2 + 1) ** 0.5)
        assert x.dtype == dtype
        out = osp_ref.forward(sd, TCFG, x, torch.full((2 * B,), t), enc, mask, cos, sin, dtype)
        u, c = out[:B], out[B:]
        eps = (u + GS * (c - u))[:, :4]
        dt, up = sch.step_coeffs(i)
        nz = noises[i].to(wide) if up > 0 else 0.0
        z = (z.to(wide) + eps.to(wide) * dt + nz * up).to(dtype)
    return z


def hip_latents(pipe, e, z0, seed=77, steps=STEPS, **kw):
    pe, pm, ne, nm = e
    g = torch.Generator(device=dev()).manual_seed(seed)
    out = pipe.generate(prompt_embeds=pe, prompt_attention_mask=pm, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm,
                        negative_prompt=None, num_inference_steps=steps, guidance_scale=GS, latents=z0.clone(), generator=g,
                        output_type="latents", verbose=False, **kw)
    torch.cuda.synchronize()
    return out


def test_sampler_within_bf16_floor_of_the_float64_restatement():
    pipe = pipeline()
    e = embeds(pipe, ["a red fox runs over the snow"])
    z0 = start()
    noises = device_noise(ZSHAPE, 77, STEPS - 1)
    want = restated_loop(e, z0, noises, torch.float64)
    floor = rms(restated_loop(e, z0, noises, torch.bfloat16), want)
    out = hip_latents(pipe, e, z0)
    lat = out.video
    assert lat.dtype == torch.float32 and tuple(lat.shape) == ZSHAPE and bool(torch.isfinite(lat).all())
    err = rms(lat.cpu(), want)
    print(f"[osp pipeline] final latents: HIP rms error {err:.4e}, bf16 floor {floor:.4e} (ratio {err / floor:.3f}), rms {float(want.pow(2).mean().sqrt()):.3f}")
    assert floor < 0.05 * float(want.pow(2).mean().sqrt()), "the floor is vacuous"
    assert err <= 1.5 * floor, f"final latents: HIP rms error {err:.4e} > 1.5 x the bf16 floor {floor:.4e}"
    tup = hip_latents(pipe, e, z0, return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 1 and torch.equal(tup[0], lat)


def test_replayed_steps_equal_eager_steps_bit_for_bit():
    pipe = pipeline()
    e = embeds(pipe, ["a red fox runs over the snow"])
    z0 = start()
    pipe._steps.entries, pipe._step_bufs = {}, None
    pipe.step_stats = {"recorded": 0, "replayed": 0, "eager": 0}
    a = hip_latents(pipe, e, z0).video.clone()
    assert pipe.step_stats == {"recorded": 1, "replayed": STEPS - 1, "eager": 0}
    b = hip_latents(pipe, e, z0).video.clone()          # a second video of the same geometry replays every step
    assert pipe.step_stats == {"recorded": 1, "replayed": 2 * STEPS - 1, "eager": 0} and torch.equal(a, b)
    pipe.transformer.use_programs = False
    try:
        c = hip_latents(pipe, e, z0).video.clone()
    finally:
        del pipe.transformer.use_programs
    assert pipe.step_stats["eager"] == STEPS and torch.equal(a, c), "the replayed steps differ from the eager ones"
    # the recorded step is ONE command array: the d96 attention launches are commands of it, and nothing is a host action
    from videosys_amd._opcodes import OPCODES

    (prog, _), = pipe._steps.entries.values()
    assert len(prog.segments) == 1 and isinstance(prog.segments[0], tuple), "a recorded single-rank step holds a host action"
    ops = [c.op for c in prog.segments[0][0]]
    layers = TCFG["num_layers"]
    assert len(ops) == prog.n_launches and ops.count(OPCODES["vsys_attn_prep_kv96"]) >= layers
    assert ops.count(OPCODES["vsys_flash_attn_d96"]) == 2 * layers                                  # self- and cross-attention


def test_new_prompt_of_the_same_shape_keeps_the_recorded_step():
    """The rule of ``_buffers`` (program.StepCache's table): a prompt of the shape of the last one is copied into the resident text
    buffers and its K / V are refilled in place, so the recorded step stays valid.  Expected from the rule: the first generate()
    records its first step and replays STEPS - 1, the two after it replay every step; nothing is recorded again and nothing runs
    eagerly.  Every output equals what a freshly built pipeline gives for that prompt."""
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanPipeline

    pipe = pipeline()
    ea, eb = embeds(pipe, ["a red fox runs over the snow"]), embeds(pipe, ["two boats leave the harbour at dawn"])
    assert all(a.shape == b.shape for a, b in zip(ea, eb)) and not torch.equal(ea[0], eb[0])
    z0 = start()
    fresh = lambda: OpenSoraPlanPipeline(config(), text_encoder=pipe.text_encoder, device=dev())
    want = {"a": hip_latents(fresh(), ea, z0).video.clone(), "b": hip_latents(fresh(), eb, z0).video.clone()}
    assert not torch.equal(want["a"], want["b"])
    pipe._steps.entries, pipe._step_bufs = {}, None
    expect = [{"recorded": 1, "replayed": STEPS - 1, "eager": 0}, {"recorded": 0, "replayed": STEPS, "eager": 0},
              {"recorded": 0, "replayed": STEPS, "eager": 0}]
    for (name, e), exp in zip((("a", ea), ("b", eb), ("a", ea)), expect):
        before = dict(pipe.step_stats)
        got = hip_latents(pipe, e, z0).video.clone()
        delta = {k: pipe.step_stats[k] - before[k] for k in before}
        assert delta == exp, (name, delta)
        assert len(pipe._steps) == 1 and torch.equal(got, want[name]), f"prompt {name}: not the fresh pipeline's latents"


def test_pab_decision_sequence_and_programs():
    from videosys_amd import pab
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanV120PABConfig

    pcfg = OpenSoraPlanV120PABConfig(spatial_threshold=[100, 850], spatial_range=2, cross_threshold=[100, 850], cross_range=3)
    pipe = pipeline(enable_pab=True, pab_config=pcfg)
    try:
        e = embeds(pipe, ["a red fox runs over the snow"])
        z0 = start()
        steps = 5
        a = hip_latents(pipe, e, z0, steps=steps).video.clone()
        trace = [list(s) for s in pipe.pab_trace]
        stats = dict(pipe.step_stats)
        pipe.transformer.use_programs = False
        try:
            b = hip_latents(pipe, e, z0, steps=steps).video.clone()
        finally:
            del pipe.transformer.use_programs
        assert [list(s) for s in pipe.pab_trace] == trace
        # the pab module's own decisions for the schedule, one counter pair per block
        from videosys_amd.pipeline_open_sora_plan import EulerAncestralDiscreteScheduler

        sch = EulerAncestralDiscreteScheduler()
        sch.set_timesteps(steps)
        mgr = pab.PABManager(pcfg)
        pcfg.steps = steps
        sc = cc = 0
        want = []
        for t in sch.timesteps.tolist():
            s, sc = mgr.if_broadcast_spatial(int(t), sc)
            c, cc = mgr.if_broadcast_cross(int(t), cc)
            want.append([(s, c)] * TCFG["num_layers"])
        assert trace == want and any(s for step in want for s, _ in step) and any(c for step in want for _, c in step)
        patterns = len({tuple(step) for step in want})
        assert stats["recorded"] == patterns and stats["replayed"] == steps - patterns and stats["eager"] == 0
        assert torch.equal(a, b), "PAB: the replayed steps differ from the eager ones"
    finally:
        pab.set_pab_manager(None)


def test_two_prompts_of_different_length_and_masks_honoured():
    pipe = pipeline()
    pe, pm, ne, nm = embeds(pipe, ["a cat", "a much longer prompt about a red fox that runs over the snow"])
    n1, n2 = int(pm[0].sum()), int(pm[1].sum())
    assert n1 < n2 <= LMAX and int(nm[0].sum()) == 1 and tuple(pe.shape) == (2, LMAX, 32)
    z0 = start(batch=2)
    a = hip_latents(pipe, (pe, pm, ne, nm), z0).video.clone()
    assert tuple(a.shape) == (2,) + ZSHAPE[1:] and not torch.equal(a[0], a[1])
    # every embedding row behind a mask is poisoned: masked keys must have no influence, bit for bit
    pe2, ne2 = pe.clone(), ne.clone()
    pe2[~pm.bool()] = 50.0
    ne2[~nm.bool()] = -50.0
    b = hip_latents(pipe, (pe2, pm, ne2, nm), z0).video.clone()
    assert torch.equal(a, b), "embeddings behind the attention mask changed the result"
    # ... and the restatement with the reference's additive mask agrees within the sampler's bound
    noises = device_noise((2,) + ZSHAPE[1:], 77, STEPS - 1)
    want = restated_loop((pe, pm, ne, nm), z0, noises, torch.float64)
    floor = rms(restated_loop((pe, pm, ne, nm), z0, noises, torch.bfloat16), want)
    assert rms(a.cpu(), want) <= 1.5 * floor, (rms(a.cpu(), want), floor)
    # text prompts go the same way as their embeddings
    g = torch.Generator(device=dev()).manual_seed(77)
    c = pipe.generate(prompt=["a cat", "a much longer prompt about a red fox that runs over the snow"], num_inference_steps=STEPS,
                      guidance_scale=GS, latents=z0.clone(), generator=g, output_type="latents", verbose=False, clean_caption=False,
                      max_sequence_length=LMAX).video
    assert torch.equal(a, c)


def u8_contract(video_bf16):
    """pipeline_open_sora_plan.py:1186-1188 on the bf16 video [B, T, 3, H, W] -> uint8 [B, T, H, W, 3]."""
    return ((video_bf16 / 2.0 + 0.5).clamp(0, 1) * 255).to(dtype=torch.uint8).permute(0, 1, 3, 4, 2).contiguous()


def test_uint8_frames_and_cropping():
    pipe = pipeline(num_frames=7)            # 3 latent frames decode to 9 frames: the video is cropped to 7
    e = embeds(pipe, ["a red fox runs over the snow"])
    z0 = start()
    lat = hip_latents(pipe, e, z0).video
    dec = pipe.vae.decode(lat.to(torch.bfloat16))
    assert dec.dtype == torch.bfloat16 and tuple(dec.shape) == (1, 9, 3, 64, 96)
    want = u8_contract(dec.cpu())
    got = pipe.decode_latents(lat)
    assert got.dtype == torch.uint8 and got.device.type == "cpu" and torch.equal(got, want), f"{int((got != want).sum())} bytes differ"
    assert 20 < float(want.float().mean()) < 235 and int(want.min()) == 0 and int(want.max()) == 255      # a real picture, clamped at both ends
    pe, pm, ne, nm = e
    g = torch.Generator(device=dev()).manual_seed(77)
    out = pipe.generate(prompt_embeds=pe, prompt_attention_mask=pm, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm,
                        negative_prompt=None, num_inference_steps=STEPS, guidance_scale=GS, latents=z0.clone(), generator=g, verbose=False)
    assert tuple(out.video.shape) == (1, 7, 64, 96, 3) and torch.equal(out.video, want[:, :7])


def test_engine_round_trip(tmp_path):
    from videosys import VideoSysEngine
    from videosys_amd import pab

    engine = VideoSysEngine(config())
    try:
        out = engine.generate(prompt="a red fox runs over the snow", num_inference_steps=2, guidance_scale=GS, seed=3, verbose=False,
                              clean_caption=False, max_sequence_length=LMAX)
        video = out.video
        assert video.dtype == torch.uint8 and tuple(video.shape) == (1, 9, 64, 96, 3)
        engine.save_video(video[0], str(tmp_path / "osp.mp4"))
    finally:
        engine.shutdown()
        pab.set_pab_manager(None)


def test_mt5_geometry_against_the_oracle():
    """The synthetic encoder at the mT5 vocabulary (250112) and the pipeline's 512 tokens, 2 layers of width 128, against
    oracle/t5_oracle.py in fp32; floor = the oracle in bf16; the bound of tests/test_gpu_t5.py."""
    from oracle import t5_oracle
    from videosys_amd.pipeline_open_sora_plan import MT5_VOCAB
    from videosys_amd.t5 import ByteTokenizer, T5Encoder, synth_state_dict

    geo = dict(d_model=128, d_ff=256, num_layers=2, num_heads=2)
    sd = synth_state_dict(vocab_size=MT5_VOCAB, seed=9, **geo)
    enc = T5Encoder(device=dev(), vocab_size=MT5_VOCAB, **geo).load_state_dict(sd)
    tok = ByteTokenizer(MT5_VOCAB)(["a red fox runs over the snow " * 30, "short"], max_length=512)
    ids, mask = tok["input_ids"], tok["attention_mask"]
    ids[0, 5], ids[1, 2] = MT5_VOCAB - 1, 200000          # rows of the table far beyond the T5 vocabulary
    assert int(mask[0].sum()) == 512 and int(mask[1].sum()) == 6
    out = enc(ids, mask).last_hidden_state.float().cpu()
    assert tuple(out.shape) == (2, 512, 128)
    ref = t5_oracle.encode(sd, ids, mask, 2, 2)
    low = t5_oracle.encode({k: v.to(torch.bfloat16) for k, v in sd.items()}, ids, mask, 2, 2).float()
    keep = mask.bool()
    r = lambda t: t.pow(2).mean().sqrt().item()
    floor = r((low - ref)[keep]) / r(ref[keep])
    mine = r((out - ref)[keep]) / r(ref[keep])
    cos = F.cosine_similarity(out[keep].flatten(), ref[keep].flatten(), dim=0).item()
    assert mine <= 1.5 * floor + 1e-3, f"rel rms {mine:.4f} vs bf16 floor {floor:.4f}"
    assert cos >= 0.999, cos
