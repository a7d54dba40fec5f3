"""-m gpu: the HIP OpenSoraT2V (videosys_amd/open_sora_plan.py) at the small geometry of tests/golden/osp_v120_fwd_small.pt — 2 heads x
96, 2 layers, latent [2, 4, 3, 8, 12] at patch 2 = 72 tokens (one full 64-key tile + 8), 8 text keys with visible counts [8, 5].

The yardstick is the bf16 FLOOR: tests/osp_ref.py (pinned to the reference's own class by tests/test_osp_cpu.py) run in bf16 against
its float64 self, same weights, inputs and RoPE tables.  The HIP model's RMS error against the float64 run must stay within 1.5 x
that floor (the project's standing bound: the HIP path rounds in fewer places than a bf16 torch run, in other places, never more
coarsely).  Both numbers are in every failure message."""
import os

import pytest
import torch

import osp_ref

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "osp_v120_fwd_small.pt")
THW = (3, 4, 6)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=True)


def state_dict(fx, out_channels=None):
    from videosys_amd.open_sora_plan import synth_state_dict

    kw = fx["kwargs"]
    return synth_state_dict(num_layers=kw["num_layers"], num_heads=kw["num_attention_heads"], caption_channels=kw["caption_channels"],
                            in_channels=kw["in_channels"], out_channels=out_channels or kw["out_channels"], patch_size=kw["patch_size"],
                            seed=fx["seed"])


def make(fx, rope_dtype=torch.bfloat16, out_channels=None):
    from videosys_amd.open_sora_plan import OpenSoraT2V

    kw = dict(fx["kwargs"])
    if out_channels:
        kw["out_channels"] = out_channels
    return OpenSoraT2V(**kw, device=dev(), rope_dtype=rope_dtype).load_state_dict(state_dict(fx, out_channels))


def rms(a, b):
    return float(((a.double() - b.double())**2).mean().sqrt())


_REF = {}


def reference(fx, key, x, t, broadcast=(False, False), cache_from=None):
    """(float64 run, bf16 floor) of osp_ref with the bf16-made tables, computed once per key; ``cache_from``: the key of the run whose
    PAB caches a broadcasting step reads (per dtype)."""
    if key not in _REF:
        sd, kw = state_dict(fx), fx["kwargs"]
        res = {}
        for dt in (torch.float64, torch.bfloat16):
            cos, sin = osp_ref.rope_tables(*THW, 96, torch.bfloat16)
            cache = {} if cache_from is None else dict(_REF[cache_from][2][dt])
            res[dt] = (osp_ref.forward(sd, kw, x, torch.tensor([t, t]), fx["encoder_hidden_states"], fx["encoder_attention_mask"], cos, sin, dt,
                                       cache=cache, broadcast=broadcast), cache)
        w = res[torch.float64][0]
        _REF[key] = (w, rms(res[torch.bfloat16][0], w), {dt: r[1] for dt, r in res.items()})
    return _REF[key][:2]


def within_floor(out, want, floor, what):
    err = rms(out.cpu(), want)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    assert err <= 1.5 * floor, f"{what}: RMS error {err:.4e} against the float64 run exceeds 1.5 x the bf16 floor {floor:.4e}"
    return err


def run(model, fx, x, t):
    return model(x, timestep=torch.tensor([t, t]), encoder_hidden_states=fx["encoder_hidden_states"], attention_mask=fx["attention_mask"],
                 encoder_attention_mask=fx["encoder_attention_mask"]).video


def test_model_within_bf16_floor(fx):
    from videosys_amd import pab

    pab.set_pab_manager(None)
    t1 = fx["pab_timesteps"][0]
    want, floor = reference(fx, "plain", fx["x"], t1)
    model = make(fx)
    out = run(model, fx, fx["x"], t1)
    assert out.shape == want.shape and out.dtype == torch.float32
    err = within_floor(out, want, floor, "OpenSoraT2V small geometry")
    print(f"[osp] HIP RMS error {err:.4e}, bf16 floor {floor:.4e}")
    tup = model(fx["x"], timestep=torch.tensor([t1, t1]), encoder_hidden_states=fx["encoder_hidden_states"],
                encoder_attention_mask=fx["encoder_attention_mask"], return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 1 and torch.equal(tup[0], out)


def test_model_against_the_reference_class(fx):
    """The fixture's float64 output is the reference class itself, whose float64 run makes its tables in float64: the HIP model with
    rope_dtype as minted meets the same bound against it (floor: the reference class's own bf16 run against its float64 run)."""
    from videosys_amd import pab

    pab.set_pab_manager(None)
    want = fx["ref_f64"]
    floor = rms(fx["ref_bf16"], want)
    out = run(make(fx, rope_dtype=torch.float64), fx, fx["x"], fx["pab_timesteps"][0])
    within_floor(out, want, floor, "OpenSoraT2V against the reference class's float64 output")


def test_model_at_non_unit_scales_against_the_reference_class(fx):
    """The fixture's second geometry (T = H/p = 4, scales (2, 1.5, 2): 96 tokens): the reference class's float64 output, whose rows are
    rotated with the frames' table (its table cache is keyed by length, not scale).  Same bound, floor = the class's own bf16 run."""
    from videosys_amd import pab
    from videosys_amd.open_sora_plan import OpenSoraT2V

    pab.set_pab_manager(None)
    model = OpenSoraT2V(**fx["scaled_kwargs"], device=dev(), rope_dtype=torch.float64).load_state_dict(state_dict(fx))
    t = fx["pab_timesteps"][0]
    out = model(fx["scaled_x"], timestep=torch.tensor([t, t]), encoder_hidden_states=fx["encoder_hidden_states"],
                encoder_attention_mask=fx["encoder_attention_mask"]).video
    want = fx["scaled_ref_f64"]
    within_floor(out, want, rms(fx["scaled_ref_bf16"], want), "OpenSoraT2V at scales (2, 1.5, 2) against the reference class")


def test_model_out_channels_8_has_the_reference_shape(fx):
    from videosys_amd import pab

    pab.set_pab_manager(None)
    out = run(make(fx, out_channels=8), fx, fx["x"], 500)
    assert tuple(out.shape) == (2, 8, 3, 8, 12) and torch.isfinite(out).all()


def test_model_pab_decisions_and_broadcast_bits(fx):
    """Four timesteps, ranges 2 (spatial) and 3 (cross): both branches broadcast at some step.  The decisions equal pab.if_broadcast_*
    driven with the same counters; a broadcasting step on unchanged inputs gives the bits of the computing step before it (the cached
    tensors are what the reference caches: un-gated attn1 output, attn2 output); every step stays within the floor of the restatement
    taking the same decisions."""
    from videosys_amd import pab

    steps = [800, 700, 600, 500]
    cfg = dict(spatial_broadcast=True, spatial_threshold=[100, 900], spatial_range=2, cross_broadcast=True, cross_threshold=[100, 900],
               cross_range=3)
    try:
        pab.set_pab_manager(pab.PABConfig(**cfg))
        pab.update_steps(len(steps))
        model = make(fx)
        model.reset_pab_state()
        outs, got = [], []
        for t in steps:
            outs.append(run(model, fx, fx["x"], t).clone())
            got.append(list(model.last_decisions))
        cs = cc = 0
        want = []
        for t in steps:
            bs, cs = pab.if_broadcast_spatial(t, cs)
            bc, cc = pab.if_broadcast_cross(t, cc)
            want.append((bs, bc))
        assert got == [[w, w] for w in want], (got, want)
        assert want[0] == (False, False) and any(w[0] for w in want) and any(w[1] for w in want)
        prev = None
        for i, (t, w) in enumerate(zip(steps, want)):
            ref, floor = reference(fx, ("pab", i), fx["x"], t, broadcast=w, cache_from=prev)
            within_floor(outs[i], ref, floor, f"PAB step {i} (t = {t}, broadcast spatial / cross = {w})")
            prev = ("pab", i)
        # a step that broadcasts BOTH branches on unchanged inputs and timestep: the bits of the computing step
        pab.update_steps(2)
        cfg2 = dict(cfg, cross_range=2)
        pab.set_pab_manager(pab.PABConfig(**cfg2))
        pab.update_steps(2)
        model.reset_pab_state()
        a = run(model, fx, fx["x"], 500).clone()
        b = run(model, fx, fx["x"], 500).clone()
        assert model.last_decisions == [(True, True)] * 2
        assert torch.equal(a, b), "a broadcasting step on unchanged inputs differs from the computing step"
    finally:
        pab.set_pab_manager(None)


def test_model_pab_against_the_reference_class(fx):
    """The fixture's PAB pair: computed at t1 on x, both branches broadcast at t2 on x2 — the reference class's own float64 output."""
    from videosys_amd import pab

    t1, t2 = fx["pab_timesteps"]
    try:
        pab.set_pab_manager(pab.PABConfig(**fx["pab"]))
        pab.update_steps(2)
        model = make(fx, rope_dtype=torch.float64)
        model.reset_pab_state()
        first = run(model, fx, fx["x"], t1)
        within_floor(first, fx["ref_f64"], rms(fx["ref_bf16"], fx["ref_f64"]), "PAB computing step against the reference class")
        second = run(model, fx, fx["x2"], t2)
        assert model.last_decisions == [(True, True)] * 2
        within_floor(second, fx["pab_f64"], rms(fx["pab_bf16"], fx["pab_f64"]), "PAB broadcasting step against the reference class")
    finally:
        pab.set_pab_manager(None)


def test_model_recorded_step_replays_and_takes_a_second_prompt(fx):
    """A recorded forward replayed equals the eager bits; a second prompt with another visible count refills the resident text
    buffers (no launch carries a count) and the SAME program gives that prompt's eager bits."""
    from videosys_amd import pab, program

    pab.set_pab_manager(None)
    model = make(fx)
    args = dict(timestep=torch.tensor([500, 500]), encoder_hidden_states=fx["encoder_hidden_states"],
                encoder_attention_mask=fx["encoder_attention_mask"])
    model(fx["x"], **args)                       # warm: text K / V, tables and workspace resident
    with program.Recorder() as rec:
        out = model(fx["x"], **args).video
    prog = rec.finish()
    assert prog is not None, rec.invalid
    # the d96 launches (one prep and two flash per layer) are recorded as commands with their op codes, none as a host closure
    from videosys_amd._opcodes import OPCODES

    d96 = [it for it in rec.items if isinstance(it, tuple) and it[1] in (OPCODES["vsys_attn_prep_kv96"], OPCODES["vsys_flash_attn_d96"])]
    assert len(d96) >= 3 * fx["kwargs"]["num_layers"], "the d96 launches were not recorded"
    assert all(isinstance(it, tuple) for it in rec.items), "a single-rank step recorded a host closure"
    torch.cuda.synchronize()
    want = out.clone()
    out.fill_(float("nan"))
    model._ws["qkv"].fill_(float("nan"))
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(out, want), "the replayed step differs from the eager one"
    # second prompt: other text, visible counts [3, 8]
    g = torch.Generator().manual_seed(99)
    enc2 = torch.randn(fx["encoder_hidden_states"].shape, generator=g).to(torch.bfloat16).float()
    mask2 = torch.ones(2, 1, 8)
    mask2[0, 0, 3:] = 0
    eager = make(fx)(fx["x"], timestep=args["timestep"], encoder_hidden_states=enc2, encoder_attention_mask=mask2).video.clone()
    assert not torch.equal(eager, want)
    model._encode_text(enc2, mask2)              # what a sampler does between prompts: refill the resident text state
    out.fill_(float("nan"))
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(out, eager), "the program replayed for a second prompt differs from that prompt's eager step"
