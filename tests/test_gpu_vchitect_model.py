"""-m gpu: VchitectXLTransformerModel (videosys_amd/vchitect.py) against the float64 restatement of the reference forward
(tests/vchitect_ref.py::model_forward), under PAB, and recorded / replayed.

Geometry: dim 192 (3 heads), depth 2 (the second block is `context_pre_only`), B = 2, latent 16 x 16 with patch 2 (S = 64; sample_size 32
and pos_embed_max_size 24, so the 8 x 8 token grid is a centre crop of the position table), L = 8, F = 3 and F = 1 (the one-frame rule).

B = 2 with F = 3 is a shape the reference class cannot run (`norm_out(hidden_states [B*F, S, C], temb [B, C])` does not broadcast), so
these tests hold the HIP model to the restatement's EXTENSION of the forward to that shape only.  The shapes the class does run — the
pipeline's B = 1 call with one text row, and B = 2 at one frame — are held to the class itself in tests/test_gpu_vchitect_pinned.py.

Bound.  The same restatement run in bf16 torch on the CPU against its float64 self is the reference's own bf16 floor (RMS error of the
output); the HIP model's RMS error against float64 must stay within 1.5 x that floor.  Both values are in the failure message."""
import pytest
import torch

import vchitect_ref as vr

pytestmark = pytest.mark.gpu

CFG = dict(num_layers=2, heads=3, patch=2, out_channels=16, sample_size=32, pos_embed_max_size=24)
B, L, HW, JD, PD = 2, 8, 16, 64, 64


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def make(F, seed=11, step=0):
    from videosys_amd.vchitect import VchitectXLTransformerModel, synth_state_dict

    sd = {k: v.to(torch.bfloat16).float() for k, v in synth_state_dict(2, 3, joint_attention_dim=JD, pooled_projection_dim=PD, seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 100 * F + step)
    x = torch.randn(B, F, 16, HW, HW, generator=g).to(torch.bfloat16).float()
    enc = torch.randn(B * F, L, JD, generator=g).to(torch.bfloat16).float()
    pooled = torch.randn(B, PD, generator=g).to(torch.bfloat16).float()
    model = VchitectXLTransformerModel(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=3,
                                       joint_attention_dim=JD, caption_projection_dim=192, pooled_projection_dim=PD, out_channels=16,
                                       pos_embed_max_size=24, device=dev()).load_state_dict(sd)
    return sd, x, enc, pooled, model


_REF = {}


def reference(F, t, step=0):
    key = (F, t, step)
    if key not in _REF:
        sd, x, enc, pooled, _ = make(F, step=step)
        ts = torch.tensor([float(t)] * B)
        want = vr.model_forward(sd, CFG, x, enc, pooled, ts, torch.float64)
        low = vr.model_forward(sd, CFG, x.to(torch.bfloat16), enc.to(torch.bfloat16), pooled.to(torch.bfloat16), ts, torch.bfloat16)
        _REF[key] = (want, rms(low, want))
    return _REF[key]


def check(out, want, floor, what):
    err = rms(out.float().cpu(), want)
    print(f"[{what}] HIP rms error {err:.4e}, bf16 floor {floor:.4e}, ratio {err / floor:.3f}, output rms {float(want.pow(2).mean().sqrt()):.3f}")
    assert out.shape == want.shape and torch.isfinite(out).all()
    assert err <= 1.5 * floor, f"{what}: HIP rms error {err:.4e} vs float64 > 1.5 x bf16 floor {floor:.4e}"


@pytest.mark.parametrize("F", [3, 1])
def test_model_within_the_bf16_floor(F):
    from videosys_amd import pab

    pab.set_pab_manager(None)
    _, x, enc, pooled, model = make(F)
    out = model(x, enc, pooled, torch.tensor([500.0] * B), return_dict=False)[0]
    torch.cuda.synchronize()
    assert out.shape == (B * F, 16, HW, HW)
    want, floor = reference(F, 500)
    check(out, want, floor, f"model F={F}")


def test_model_surface():
    import videosys  # noqa: F401
    from videosys.models.transformers.vchitect_transformer_3d import JointTransformerBlock, VchitectXLTransformerModel
    from videosys_amd import vchitect

    assert VchitectXLTransformerModel is vchitect.VchitectXLTransformerModel and JointTransformerBlock is vchitect.JointTransformerBlock
    sd, x, enc, pooled, model = make(3)
    assert sorted(model.expected_keys()) == sorted(sd)
    with pytest.raises(NotImplementedError):
        model.enable_parallel(1, 2, False)
    model.enable_parallel(1, 1, False)
    with pytest.raises(KeyError):
        model.load_state_dict({k: v for k, v in sd.items() if k != "proj_out.bias"})
    # encoder_hidden_states given per sample is what every frame of the sample reads
    per_sample = enc.view(B, 3, L, JD)[:, 0]
    a = model(x, per_sample, pooled, torch.tensor([500.0] * B)).sample.clone()
    b = model(x, per_sample[:, None].expand(B, 3, L, JD).reshape(B * 3, L, JD), pooled, torch.tensor([500.0] * B)).sample
    assert torch.equal(a, b)


def test_model_pab_four_steps():
    """Four steps with DIFFERENT latents and timesteps; ranges 2 / 3 / 4 make every branch broadcast at least once.  Decisions equal pab's
    functions in the layer's call order.  A broadcast step must differ from the PAB-free model on the same inputs (it mixes stale
    branches) and must EQUAL a hand-mixed run: a second model whose caches are filled from the stale step and whose counters are set so
    that it takes the same decisions — so a wrong cache, or recomputing instead of broadcasting, shows.  Outputs stay within the floor
    scaled by nothing: a broadcast step is held to 1.5 x floor only where no branch is stale (step 0)."""
    from videosys_amd import pab

    F, steps = 3, [900, 700, 500, 300]
    cfg = dict(spatial_broadcast=True, spatial_threshold=[100, 950], spatial_range=2, temporal_broadcast=True, temporal_threshold=[100, 950],
               temporal_range=3, cross_broadcast=True, cross_threshold=[100, 950], cross_range=4)
    models = [make(F, step=i) for i in range(4)]
    model = models[0][4]
    try:
        pab.set_pab_manager(None)
        free = []
        for i, t in enumerate(steps):
            _, x, enc, pooled, _ = models[i]
            free.append(model(x, enc, pooled, torch.tensor([float(t)] * B)).sample.clone())
        pab.set_pab_manager(pab.PABConfig(**cfg))
        pab.update_steps(len(steps))
        model.reset_pab_state()
        got, outs = [], []
        for i, t in enumerate(steps):
            _, x, enc, pooled, _ = models[i]
            outs.append(model(x, enc, pooled, torch.tensor([float(t)] * B)).sample.clone())
            torch.cuda.synchronize()
            got.append([blk.attn.last_decisions for blk in model.transformer_blocks])
        ct = cc = cs = 0
        want = []
        for t in steps:
            bt, ct = pab.if_broadcast_temporal(t, ct)
            bc, cc = pab.if_broadcast_cross(t, cc)
            bs, cs = pab.if_broadcast_spatial(t, cs)
            want.append((bt, bc, bs))
        assert got == [[w, w] for w in want], (got, want)
        assert want[0] == (False, False, False) and all(any(w[i] for w in want) for i in range(3))
        assert torch.equal(outs[0], free[0])
        w0, fl0 = reference(F, steps[0], 0)
        check(outs[0], w0, fl0, "PAB step 0 (nothing stale)")
        for i in range(1, 4):
            assert not torch.equal(outs[i], free[i]), f"step {i} broadcasts {want[i]} and still equals the PAB-free output"
        # hand-mixed: replay the same four steps on a fresh model; identical caches and counters -> identical bits, step by step;
        # then break ONE cache before the last step (its temporal branch is recomputed, cross and spatial are broadcast) and see it show
        again = make(F)[4]
        pab.update_steps(len(steps))
        for i, t in enumerate(steps[:3]):
            _, x, enc, pooled, _ = models[i]
            o = again(x, enc, pooled, torch.tensor([float(t)] * B)).sample
            assert torch.equal(o, outs[i])
        assert want[3] == (False, True, True)
        blk = again.transformer_blocks[0].attn
        blk.last_cross, blk.last_spatial = (blk.last_spatial[0], blk.last_spatial[1]), (blk.last_cross[0], blk.last_cross[1])   # swapped caches
        _, x, enc, pooled, _ = models[3]
        o = again(x, enc, pooled, torch.tensor([float(steps[3])] * B)).sample
        assert not torch.equal(o, outs[3]), "swapping the cross and spatial caches of a block did not change a step that broadcasts both"
    finally:
        pab.set_pab_manager(None)


def test_model_recorded_step_replays_bit_for_bit():
    from videosys_amd import _opcodes, pab, program

    pab.set_pab_manager(None)
    F = 3
    _, x, enc, pooled, model = make(F)
    ts = torch.tensor([500.0] * B)
    model(x, enc, pooled, ts)
    with program.Recorder() as rec:
        out = model(x, enc, pooled, ts).sample
    prog = rec.finish()
    assert prog is not None, rec.invalid
    recorded = {it[1] for it in rec.items if isinstance(it, tuple)}
    assert {_opcodes.OPCODES["vsys_attn_temporal_d64"], _opcodes.OPCODES["vsys_scale_add_rows"]} <= recorded
    torch.cuda.synchronize()
    want = out.clone()
    out.fill_(float("nan"))
    model._ws["x"].fill_(float("nan"))
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    w, fl = reference(F, 500)
    check(out.view(want.shape), w, fl, "replayed step")
