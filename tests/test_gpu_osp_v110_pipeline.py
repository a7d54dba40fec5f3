"""-m gpu: OpenSoraPlanV110Pipeline (videosys_amd/pipeline_open_sora_plan_v110.py) end to end at the small geometry of
tests/test_gpu_osp_v110_model.py — LatteT2V with 2 layers, 8 heads x 72, caption_channels 32, latent [1, 4, 3, 8, 8] (num_frames 9,
64 x 64 pixels), a 2-layer synthetic T5 over the T5 v1.1 vocabulary, the hidden_size-32 v1.1 CausalVAE — with num_inference_steps = 5:
14 model calls, twelve Runge-Kutta warm-up calls and two multistep calls.

Sampler.  The HIP loop against a float64 restatement — tests/osp_v110_ref.py for the model, PNDMScheduler.step in float64 for the
scheduler — fed the same start latents and the same embeddings.  Bound (the project's): RMS error of the final latents within 1.5 x
the bf16 FLOOR, the same restatement run the way the reference runs it in bf16 (bf16 latents, model and scheduler arithmetic,
:1109-1161) against its float64 self.  Replayed equals eager bit for bit; ``step_stats`` counts the calls; the PAB decision sequence
runs with OpenSoraPlanV110PABConfig(); a prompt of k tokens reaches the transformer as k keys with the negative cut to k, a batch of
two at 300 keys with the masked rows zero; one VideoSysEngine round trip to uint8 frames; ``cpu_offload``."""
import pytest
import torch

import osp_v110_ref
import test_osp_v110_cpu as C

pytestmark = pytest.mark.gpu

HEADS, SEED, STEPS, GS = 8, 1101, 5, 4.5
ZSHAPE = (1, 4, 3, 8, 8)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return torch.load(C.FIXTURE, weights_only=True)


def tcfg(fx):
    return {**fx["kwargs"], **fx["wide_heads"], "video_length": 3, "model_max_length": 300}


def config(fx, **over):
    from videosys_amd.pipeline_open_sora_plan_v110 import OpenSoraPlanV110Config

    kw = dict(transformer=f"synthetic:{SEED}", text_encoder="synthetic:3", transformer_config=tcfg(fx), vae_config=dict(hidden_size=32),
              num_frames=9)
    kw.update(over)
    return OpenSoraPlanV110Config(**kw)


_PIPE = {}


def pipeline(fx, **over):
    """One pipeline per configuration for the whole module."""
    from videosys_amd import pab
    from videosys_amd.pipeline_open_sora_plan_v110 import OpenSoraPlanV110Pipeline

    key = tuple(sorted((k, repr(v)) for k, v in over.items()))
    if key not in _PIPE:
        _PIPE[key] = OpenSoraPlanV110Pipeline(config(fx, **over), device=dev())
    p = _PIPE[key]
    c = p._config
    pab.set_pab_manager(c.pab_config if c.enable_pab else None)
    return p


def rms(a, b):
    return float(((a.double() - b.double()) ** 2).mean().sqrt())


def start(batch=1, seed=5):
    return torch.randn((batch,) + ZSHAPE[1:], generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float()


def state_dict(fx):
    from videosys_amd.open_sora_plan_v110 import synth_state_dict

    k = tcfg(fx)
    return synth_state_dict(num_layers=k["num_layers"], num_heads=HEADS, caption_channels=k["caption_channels"], in_channels=4,
                            out_channels=8, patch_size=2, seed=SEED)


def restated_loop(fx, pe, ne, z0, dtype, steps=STEPS):
    """pipeline_open_sora_plan.py:1104-1161 at version v110 with tests/osp_v110_ref.py as the transformer, in ``dtype``."""
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    k = tcfg(fx)
    model = osp_v110_ref.LatteT2VRef(state_dict(fx), k["num_layers"], HEADS, sample_size=k["sample_size"], out_channels=8,
                                     video_length=k["video_length"], use_rope=True, dtype=dtype)
    sch = PNDMScheduler()
    sch.set_timesteps(steps)
    enc = torch.cat([ne, pe], 0)[:, None].to(dtype)
    z = z0.to(dtype)
    B = z.shape[0]
    with torch.no_grad():
        for t in sch.timesteps.tolist():
            out = model.forward(torch.cat([z, z], 0), torch.full((2 * B,), t), enc, None, all_timesteps=sch.timesteps)
            u, c = out[:B, :4], out[B:, :4]
            z = sch.step(u + GS * (c - u), t, z, return_dict=False)[0].to(dtype)
    return z


@pytest.fixture(scope="module")
def embeds(fx):
    pe, ne = pipeline(fx).encode_prompt("a small red boat on a lake", True, negative_prompt="")
    return pe.float().cpu(), ne.float().cpu()


def run(pipe, pe, ne, z0, **kw):
    out = pipe.generate(prompt_embeds=pe.to(dev()), negative_prompt_embeds=ne.to(dev()), num_inference_steps=STEPS, guidance_scale=GS,
                        latents=z0.clone(), output_type="latents", verbose=False, **kw).video
    torch.cuda.synchronize()
    return out.float().cpu()


def test_latents_within_the_bf16_floor_and_replay_equals_eager(fx, embeds):
    pe, ne = embeds
    assert pe.shape == ne.shape and pe.shape[1] < 300          # one prompt: both cut to its token count
    z0 = start()
    pipe = pipeline(fx)
    pipe.step_stats = {"recorded": 0, "replayed": 0, "eager": 0}
    pipe._steps.entries = {}
    out = run(pipe, pe, ne, z0)
    assert pipe.step_stats == {"recorded": 1, "replayed": STEPS + 8, "eager": 0}, pipe.step_stats
    # the recorded step holds no text path: as many launches as a recording made while the text K / V are resident, and fewer than one
    # made with the transformer's text cache cold (caption projection + a K / V GEMM and a prep launch per layer)
    from videosys_amd import program

    (prog, _), = pipe._steps.entries.values()
    bufs, ts = pipe._step_bufs, pipe.scheduler.timesteps

    def recorded_launches():
        with program.Recorder() as rec:
            pipe._model(bufs["xin"], 500, bufs["enc"], ts)
        return rec.finish().n_launches

    warm = recorded_launches()
    pipe.transformer.reset_text_cache()
    cold = recorded_launches()
    pipe._prepare_text(bufs["enc"])
    layers = tcfg(fx)["num_layers"]
    print(f"recorded launches: program {prog.n_launches}, text resident {warm}, text cache cold {cold}")
    assert prog.n_launches == warm and cold >= warm + 2 * layers
    pipe._steps.entries = {}                                  # (the cold recording made new text K / V: record again on the next call)
    out2 = run(pipe, pe, ne, z0)
    assert torch.equal(out, out2)
    pipe.step_stats = {"recorded": 1, "replayed": STEPS + 8, "eager": 0}
    again = run(pipe, pe, ne, z0)
    assert pipe.step_stats["replayed"] == 2 * (STEPS + 9) - 1 and torch.equal(out, again)
    pipe.transformer.use_programs = False
    try:
        eager = run(pipe, pe, ne, z0)
    finally:
        pipe.transformer.use_programs = True
    assert pipe.step_stats["eager"] == STEPS + 9
    assert torch.equal(out, eager), "the replayed sampler differs from the eager one"
    # the recorded call is ONE command array: the roped d72 attention launches are commands of it, and nothing is a host action
    from videosys_amd._opcodes import OPCODES

    (prog, _), = pipe._steps.entries.values()
    assert len(prog.segments) == 1 and isinstance(prog.segments[0], tuple), "a recorded single-rank call holds a host action"
    ops = [c.op for c in prog.segments[0][0]]
    assert len(ops) == prog.n_launches
    assert ops.count(OPCODES["vsys_attn_prep_kv_rope"]) >= 1 and ops.count(OPCODES["vsys_attn_prep_kv_rope"]) == ops.count(OPCODES["vsys_flash_attn_d72_rope"])
    f64 = restated_loop(fx, pe, ne, z0, torch.float64)
    floor = rms(restated_loop(fx, pe, ne, z0, torch.bfloat16), f64)
    err = rms(out, f64)
    print(f"latents after {STEPS + 9} calls: HIP rms error {err:.4e}, bf16 floor {floor:.4e} (ratio {err / floor:.3f}), rms {rms(f64, 0 * f64):.3f}")
    assert tuple(out.shape) == ZSHAPE and floor < 0.05 * rms(f64, 0 * f64), "the floor is vacuous"
    assert err <= 1.5 * floor


def test_new_prompt_of_the_same_shape_drops_the_recorded_call(fx, embeds):
    """The rule of ``_buffers`` (program.StepCache's table): the recorded call reads the text K / V that ``_prepare_text`` made for
    one text, and another text gets new ones, so the call is recorded again — also when the first prompt comes back.  Expected from
    the rule, per generate() of STEPS + 9 calls: 1 recorded (the first call) + STEPS + 8 replayed, three times over; nothing eager.
    Every output equals what a freshly built pipeline gives for that prompt."""
    from videosys_amd.pipeline_open_sora_plan_v110 import OpenSoraPlanV110Pipeline

    pipe = pipeline(fx)
    pb, nb = (t.float().cpu() for t in pipe.encode_prompt("a large red ship on a lake", True, negative_prompt=""))
    ea, eb = embeds, (pb, nb)
    assert eb[0].shape == ea[0].shape and eb[1].shape == ea[1].shape and not torch.equal(eb[0], ea[0])
    z0 = start()
    fresh = lambda: OpenSoraPlanV110Pipeline(config(fx), text_encoder=pipe.text_encoder, device=dev())
    want = {"a": run(fresh(), *ea, z0), "b": run(fresh(), *eb, z0)}
    assert not torch.equal(want["a"], want["b"])
    pipe._steps.entries, pipe._step_bufs = {}, None
    for name, e in (("a", ea), ("b", eb), ("a", ea)):
        before = dict(pipe.step_stats)
        got = run(pipe, *e, z0)
        delta = {k: pipe.step_stats[k] - before[k] for k in before}
        assert delta == {"recorded": 1, "replayed": STEPS + 8, "eager": 0}, (name, delta)
        assert len(pipe._steps) == 1 and torch.equal(got, want[name]), f"prompt {name}: not the fresh pipeline's latents"


def test_callbacks_follow_the_reference_rule(fx, embeds):
    pe, ne = embeds
    seen = []
    run(pipeline(fx), pe, ne, start(), callback=lambda i, t, z: seen.append((i, t, tuple(z.shape))))
    # num_warmup_steps = len(timesteps) - n = 9: calls 9 .. 13 report
    assert [s[0] for s in seen] == list(range(9, STEPS + 9)) and all(s[2] == ZSHAPE for s in seen)


def test_pab_sequence_runs(fx, embeds):
    from videosys_amd.pipeline_open_sora_plan_v110 import OpenSoraPlanV110PABConfig

    pe, ne = embeds
    pipe = pipeline(fx, enable_pab=True)
    assert isinstance(pipe._config.pab_config, OpenSoraPlanV110PABConfig)
    before = dict(pipe.step_stats)
    out = run(pipe, pe, ne, start())
    assert pipe.step_stats["eager"] - before["eager"] == STEPS + 9 and len(pipe.pab_trace) == STEPS + 9
    assert bool(torch.isfinite(out).all())
    # pab_trace: per call, per block in execution order (spatial, temporal, ...), the (attention, cross, mlp) decisions — those of the
    # pab module replayed here on counters of our own: n = 5 gives the calls 800, 700, 700, 600, ... 200, 200, 0, all but the first
    # and the last inside (100, 850), so the spatial attention is broadcast on odd counters (range 2), the temporal one on 3 of 4, the cross one on 5 of 6
    from videosys_amd import pab
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    sch = PNDMScheduler()
    sch.set_timesteps(STEPS)
    ts = sch.timesteps.tolist()
    nblk = 2 * tcfg(fx)["num_layers"]
    counts = [[0, 0] for _ in range(nblk)]
    mgr = pab.PAB_MANAGER
    for call, (t, row) in enumerate(zip(ts, pipe.pab_trace)):
        assert len(row) == nblk
        for i, (attn, cross, mlp) in enumerate(row):
            temporal = bool(i % 2)
            want_attn, counts[i][0] = (mgr.if_broadcast_temporal if temporal else mgr.if_broadcast_spatial)(t, counts[i][0])
            assert attn == want_attn, (call, i)
            if temporal:
                assert cross is None
            else:
                want_cross, counts[i][1] = mgr.if_broadcast_cross(t, counts[i][1])
                assert cross == want_cross, (call, i)
            assert mlp is False                  # none of these timesteps opens or lies in an MLP window (738 ... 426 in steps of 24)
    for st, (a, c) in zip(pipe.transformer.states, counts):      # ... and the blocks themselves counted the same calls
        assert (st.attn_count, st.cross_count) == (a, c)
    spatial = [row[0][0] for row in pipe.pab_trace]
    # (the counters wrap at update_steps(5), as the reference's do: F T F T F | F T F T F | F T F, and the last call, t = 0, is outside)
    assert spatial == [False, True, False, True, False] * 2 + [False, True, False, False], spatial
    assert any(r[1][0] for r in pipe.pab_trace) and any(r[0][1] for r in pipe.pab_trace), "no temporal / cross block ever broadcast"
    plain = run(pipeline(fx), pe, ne, start())
    assert not torch.equal(out, plain), "PAB on gives the bits of PAB off: nothing was broadcast"


def test_text_masking_reaches_the_transformer(fx):
    pipe = pipeline(fx)
    seen = []
    orig = pipe._issue_model

    def spy(xin, t, enc, *a, **k):
        seen.append(enc.clone())
        return orig(xin, t, enc, *a, **k)

    pipe._issue_model = spy
    try:
        pipe.generate("red boat", num_inference_steps=4, guidance_scale=GS, output_type="latents", verbose=False, seed=1, clean_caption=False)
        one = seen[0]
        seen.clear()
        pipe.generate(["red boat", "a much longer prompt about a lake"], num_inference_steps=4, guidance_scale=GS, output_type="latents",
                      verbose=False, seed=1, clean_caption=False)
        two = seen[0]
    finally:
        pipe._issue_model = orig
    k = int(pipe.text_encoder(["red boat"])[1].sum())
    assert tuple(one.shape) == (2, 1, k, 32) and 0 < k < 300        # [negative | prompt], both at the prompt's k keys
    assert tuple(two.shape) == (4, 1, 300, 32)
    m = pipe.text_encoder(["red boat", "a much longer prompt about a lake"])[1].bool().to(two.device)
    assert float(two[2:, 0][~m].abs().max()) == 0.0 and float(two[2:, 0][m].abs().max()) > 0.0       # masked rows of the prompts are zero
    assert float(two[:2, 0, 299].abs().max()) > 0.0                                                    # the negative ones are as encoded


def test_engine_round_trip_and_cpu_offload(fx):
    from videosys import VideoSysEngine
    from videosys_amd import pab

    engine = VideoSysEngine(config(fx))
    try:
        video = engine.generate(prompt="a small red boat", num_inference_steps=4, guidance_scale=GS, seed=3, verbose=False,
                                clean_caption=False).video
    finally:
        engine.shutdown()
        pab.set_pab_manager(None)
    assert video.dtype == torch.uint8 and tuple(video.shape) == (1, 9, 64, 64, 3) and len(torch.unique(video)) > 8
    off = pipeline(fx, cpu_offload=True)
    v2 = off.generate("a small red boat", num_inference_steps=4, guidance_scale=GS, seed=3, verbose=False, clean_caption=False).video
    assert torch.equal(video, v2), "cpu_offload changed the video"
