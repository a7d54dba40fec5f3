"""-m gpu: the HIP VchitectXLTransformerModel and JointTransformerBlock held to the reference's OWN classes through the fixtures of
tools/mint_vchitect.py (tests/golden/vchitect_{fwd,pab,layer}_small.pt) — not to the restatement; tests/test_vchitect_pinned_cpu.py
holds the restatement to the same files, so a failure here that is none there is the HIP code's.

The model is called as pipeline_vchitect.py calls it: B = 1 with ONE text row [1, L, D] (all L keys go to cross attention, the text
rows broadcast to the F frames in the first block), plus b2f1, the only B = 2 shape the class executes.  Weights: bf16-rounded
synth_state_dict(seed of the fixture), as tests/test_gpu_vchitect_model.py::make builds them.

Bound: rms(HIP - class float64) <= 1.5 x rms(class bfloat16 - class float64), both tensors from the fixture (the 1.5 of
test_gpu_vchitect_model.check; the floor is the class's own).  Error, floor and ratio are printed.  Under PAB every call is held to
its own floor; the mint asserted that a stale branch moves the class's output by >= 6 floors, so recomputing instead of broadcasting,
or mixing in the wrong cache, cannot pass.  Every output buffer is NaN before the call."""
import os

import pytest
import torch

import vchitect_ref as vr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_FX = {}


def fixture(name):
    if name not in _FX:
        _FX[name] = torch.load(os.path.join(GOLDEN, f"vchitect_{name}_small.pt"), weights_only=True)
    return _FX[name]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def weights():
    from videosys_amd.vchitect import synth_state_dict

    meta = fixture("fwd")["meta"]
    kw = meta["kwargs"]
    return {k: v.to(torch.bfloat16).float() for k, v in synth_state_dict(kw["num_layers"], kw["num_attention_heads"],
            joint_attention_dim=kw["joint_attention_dim"], pooled_projection_dim=kw["pooled_projection_dim"], seed=meta["seed"]).items()}


def make():
    from videosys_amd.vchitect import VchitectXLTransformerModel

    return VchitectXLTransformerModel(**fixture("fwd")["meta"]["kwargs"], device=dev()).load_state_dict(weights())


def run(model, x, enc, pooled, t):
    """One call in the pipeline's form into a NaN-filled buffer of the test's own."""
    B, F, co, Hh, Ww = x.shape[0], x.shape[1], model.out_channels, x.shape[3], x.shape[4]
    buf = torch.full((B * F * co * Hh * Ww,), float("nan"), dtype=torch.float32, device=dev())
    out = model(x.float(), enc.float(), pooled.float(), torch.tensor([float(t)] * B), out=buf).sample
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and out.shape == (B * F, co, Hh, Ww)
    return out


def check(out, want, low, what):
    floor = rms(low, want)
    err = rms(out.float().cpu(), want)
    print(f"[{what}] HIP rms error {err:.4e}, reference bf16 floor {floor:.4e}, ratio {err / floor:.3f}, output rms {float(want.pow(2).mean().sqrt()):.3f}")
    assert out.shape == want.shape and torch.isfinite(out).all()
    assert err <= 1.5 * floor, f"{what}: HIP rms error {err:.4e} vs the class's float64 > 1.5 x the class's bf16 floor {floor:.4e}"


@pytest.mark.parametrize("case", ["f3", "f1", "rect", "b2f1"])
def test_model_in_the_pipelines_call_form(case):
    from videosys_amd import pab

    pab.set_pab_manager(None)
    c = fixture("fwd")["cases"][case]
    out = run(make(), c["x"], c["encoder_hidden_states"], c["pooled"], c["t"])
    check(out, c["ref_f64"], c["ref_bf16"], f"model {case}")


def test_model_pab_eight_calls():
    """Four steps of two calls (row 0, then row 1 of a CFG pair: the same latents, another prompt) on ONE model: the counters advance
    once per call, so call 1 broadcasts all three branches of call 0 — computed for the other prompt — as the reference does."""
    from videosys_amd import pab

    p = fixture("pab")
    model = make()
    calls = [(s, r) for s in range(len(p["timesteps"])) for r in range(2)]
    one = lambda s, r: run(model, p["x"][s:s + 1], p["encoder_hidden_states"][r:r + 1], p["pooled"][r:r + 1], p["timesteps"][s])
    try:
        pab.set_pab_manager(None)
        free0 = one(0, 0).clone()
        pab.set_pab_manager(pab.PABConfig(**p["config"]))
        pab.update_steps(len(p["timesteps"]))
        ct = cc = cs = 0
        want = []
        for s, _ in calls:        # once per CALL: twice per sampler step
            t = p["timesteps"][s]
            bt, ct = pab.if_broadcast_temporal(t, ct)
            bc, cc = pab.if_broadcast_cross(t, cc)
            bs, cs = pab.if_broadcast_spatial(t, cs)
            want.append((bt, bc, bs))
        assert want == [tuple(d) for d in p["decisions"]]
        assert want[0] == (False, False, False) and all(any(w[i] for w in want) for i in range(3))
        model.reset_pab_state()
        for i, (s, r) in enumerate(calls):
            out = one(s, r)
            got = [blk.attn.last_decisions for blk in model.transformer_blocks]
            assert got == [want[i]] * len(model.transformer_blocks), (i, got, want[i])
            if i == 0:
                assert torch.equal(out, free0), "the first PAB call differs from the same model's PAB-free output"
            check(out, p["pab_f64"][i], p["pab_bf16"][i], f"pab call {i} {want[i]}")
        a = model.transformer_blocks[0].attn
        assert (a.temporal_count, a.cross_count, a.spatial_count) == (ct, cc, cs)
    finally:
        pab.set_pab_manager(None)


def test_recorded_step_replays_bit_for_bit_inside_the_bound():
    from videosys_amd import pab, program

    pab.set_pab_manager(None)
    c = fixture("fwd")["cases"]["f3"]
    model = make()
    args = (c["x"].float(), c["encoder_hidden_states"].float(), c["pooled"].float(), torch.tensor([float(c["t"])]))
    buf = torch.full((c["ref_f64"].numel(),), float("nan"), dtype=torch.float32, device=dev())
    model(*args, out=buf)                    # buffers allocated, tables resident
    with program.Recorder() as rec:
        out = model(*args, out=buf).sample
    prog = rec.finish()
    assert prog is not None, rec.invalid
    torch.cuda.synchronize()
    eager = out.clone()
    check(eager, c["ref_f64"], c["ref_bf16"], "eager step")
    buf.fill_(float("nan"))
    model._ws["x"].fill_(float("nan"))
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    check(out, c["ref_f64"], c["ref_bf16"], "replayed step")


@pytest.mark.parametrize("which", ["joint", "context_pre_only"])
def test_block_against_the_reference_block(which):
    """vchitect.JointTransformerBlock on the inputs of the stand-alone reference block (B = 1, F = 3, S = 16, L = 4): the modulation
    table is linear(silu(temb)) of norm1 | norm1_context in one launch, as the model makes it."""
    from videosys_amd import ops, pab
    from videosys_amd.vchitect import JointTransformerBlock
    from videosys_amd.workspace import Workspace

    pab.set_pab_manager(None)
    fx = fixture("layer")
    ref, last = fx[which], which == "context_pre_only"
    hs, enc, temb = vr.layer_inputs(fx["meta"]["seed"])
    F, S, C = hs.shape
    L = enc.shape[1]
    pre = f"transformer_blocks.{int(last)}."
    sd = weights()
    blk = JointTransformerBlock(C, 3, C, last, device=dev()).load_state_dict(sd, pre)
    on = lambda t: t.to(device=dev(), dtype=torch.bfloat16).contiguous()
    mod = ops.linear_small(on(temb), on(torch.cat([sd[pre + "norm1.linear.weight"], sd[pre + "norm1_context.linear.weight"]], 0)),
                           on(torch.cat([sd[pre + "norm1.linear.bias"], sd[pre + "norm1_context.linear.bias"]], 0)), act_in=ops.ACT_SILU)
    x, y = on(hs.reshape(F * S, C)), on(enc.reshape(F * L, C))
    y0 = y.clone()
    blk.forward(x, y, mod[0], mod[0, 6 * C:], mod.shape[1], 1, F, Workspace(dev(), torch.bfloat16).buf)
    torch.cuda.synchronize()
    check(x.view(F, S, C), ref["x_f64"], ref["x_bf16"], f"block video, {which}")
    if last:
        assert torch.equal(y, y0)          # the class returns None for the text stream
    else:
        check(y.view(F, L, C), ref["y_f64"], ref["y_bf16"], f"block text, {which}")
