"""-m gpu: the Vchitect-2.0 attention layer (videosys_amd.vchitect.VchitectAttention) against the float64 restatement of
VchitectAttnProcessor.__call__ (tests/vchitect_ref.py::attention_layer), under PAB, and recorded / replayed.

Geometry: dim 192 (3 heads), B = 2, S = 64 (latent 16 x 16, patch 2), L = 8 (72 keys per frame: ragged), F = 3 and F = 1 (the
`cur_frame == 1` rule: the temporal contributions are multiplied by 0), with and without `context_pre_only`.

Bound.  Not a constant: the same restatement run in bf16 torch on the CPU against its float64 self is the reference's own bf16 floor
(RMS error over an output); the HIP layer's RMS error against float64 must stay within 1.5 x that floor.  Both are in the failure
message."""
import pytest
import torch

import vchitect_ref as vr

pytestmark = pytest.mark.gpu

DIM, H, B, S, L = 192, 3, 2, 64, 8


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def make(F, pre_only, seed=5):
    from videosys_amd.vchitect import VchitectAttention, synth_attention_state_dict

    sd = {k: v.to(torch.bfloat16).float() for k, v in synth_attention_state_dict(DIM, pre_only, seed=seed).items()}
    g = torch.Generator().manual_seed(seed + F)
    hs = torch.randn(B * F, S, DIM, generator=g).to(torch.bfloat16)
    enc = torch.randn(B * F, L, DIM, generator=g).to(torch.bfloat16)
    layer = VchitectAttention(DIM, H, context_pre_only=pre_only, device=dev()).load_state_dict(sd)
    return sd, hs, enc, layer


_REF = {}


def reference(F, pre_only):
    """(float64 outputs, bf16 floor per output), computed once per case and shared."""
    key = (F, pre_only)
    if key not in _REF:
        sd, hs, enc, _ = make(F, pre_only)
        want = vr.attention_layer(sd, hs, enc, B, F, H, pre_only, torch.float64)
        low = vr.attention_layer(sd, hs, enc, B, F, H, pre_only, torch.bfloat16)
        _REF[key] = (want, tuple(rms(a, b) for a, b in zip(low, want)))
    return _REF[key]


def check(out, F, pre_only, what):
    want, floor = reference(F, pre_only)
    for name, o, w, fl in zip(("hidden_states", "encoder_hidden_states"), out, want, floor):
        err = rms(o.float().cpu().reshape(w.shape), w)
        print(f"[{what}] {name}: HIP rms error {err:.4e}, bf16 floor {fl:.4e}, ratio {err / fl:.3f}")
        assert torch.isfinite(o).all() and err <= 1.5 * fl, f"{what} {name}: HIP rms error {err:.4e} vs float64 > 1.5 x bf16 floor {fl:.4e}"


@pytest.mark.parametrize("pre_only", [False, True], ids=["joint", "context_pre_only"])
@pytest.mark.parametrize("F", [3, 1])
def test_layer_within_the_bf16_floor(F, pre_only):
    from videosys_amd import pab

    pab.set_pab_manager(None)
    _, hs, enc, layer = make(F, pre_only)
    out = layer(hs.reshape(-1, DIM).to(dev()), enc.reshape(-1, DIM).to(dev()), B, F)
    torch.cuda.synchronize()
    check(out, F, pre_only, f"layer F={F} pre_only={pre_only}")
    if F == 1:      # the temporal branch contributes nothing: the output is the one of a layer whose temporal weights are zero
        sd, _, _, _ = make(F, pre_only)
        from videosys_amd.vchitect import VchitectAttention

        sd0 = {k: (torch.zeros_like(v) if "temp" in k else v) for k, v in sd.items()}
        o0 = VchitectAttention(DIM, H, context_pre_only=pre_only, device=dev()).load_state_dict(sd0)(
            hs.reshape(-1, DIM).to(dev()), enc.reshape(-1, DIM).to(dev()), B, F)
        assert torch.equal(o0[0], out[0]) and torch.equal(o0[1], out[1])


def test_layer_refuses_what_it_does_not_build():
    from videosys_amd.vchitect import VchitectAttention

    _, hs, enc, layer = make(3, False)
    with pytest.raises(NotImplementedError):
        layer.enable_parallel(1, 2, False)
    layer.enable_parallel(1, 1, False)
    with pytest.raises(ValueError):       # 7 text keys cannot be dealt out over 2 samples
        layer(hs.reshape(-1, DIM).to(dev()), enc[:, :7].reshape(-1, DIM).contiguous().to(dev()), B, 3)


def test_layer_pab_decisions_and_outputs():
    """Four steps; ranges 2 / 3 / 4 inside the threshold window make every branch broadcast at least once.  The decisions equal those
    of pab's functions called with the same timesteps and counters (pinned against the reference in tests/test_pab_cpu.py); a step
    that broadcasts on the SAME inputs gives the bits of the step that computed; every output stays within the floor."""
    from videosys_amd import pab

    F, steps = 3, [900, 700, 500, 300]
    cfg = dict(spatial_broadcast=True, spatial_threshold=[100, 950], spatial_range=2, temporal_broadcast=True, temporal_threshold=[100, 950],
               temporal_range=3, cross_broadcast=True, cross_threshold=[100, 950], cross_range=4)
    _, hs, enc, layer = make(F, False)
    h, e = hs.reshape(-1, DIM).to(dev()), enc.reshape(-1, DIM).to(dev())
    pab.set_pab_manager(None)
    base = [t.clone() for t in layer(h, e, B, F)]
    try:
        pab.set_pab_manager(pab.PABConfig(**cfg))
        pab.update_steps(len(steps))
        layer.reset_pab_state()
        got = []
        for t in steps:
            out = layer(h, e, B, F, timestep=t)
            torch.cuda.synchronize()
            got.append(layer.last_decisions)
            assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1]), f"t={t}: broadcast on unchanged inputs changed bits"
            check(out, F, False, f"PAB t={t} decisions={layer.last_decisions}")
        ct = cc = cs = 0
        want = []
        for t in steps:       # the same calls, in the layer's order: temporal, cross, spatial
            bt, ct = pab.if_broadcast_temporal(t, ct)
            bc, cc = pab.if_broadcast_cross(t, cc)
            bs, cs = pab.if_broadcast_spatial(t, cs)
            want.append((bt, bc, bs))
        assert got == want, (got, want)
        assert want[0] == (False, False, False)
        for i, name in enumerate(("temporal", "cross", "spatial")):
            assert any(w[i] for w in want), f"{name} never broadcast"
        assert (layer.temporal_count, layer.cross_count, layer.spatial_count) == (ct, cc, cs)
    finally:
        pab.set_pab_manager(None)


def test_layer_recorded_step_replays_bit_for_bit():
    from videosys_amd import _opcodes, pab, program

    pab.set_pab_manager(None)
    F = 3
    _, hs, enc, layer = make(F, False)
    h, e = hs.reshape(-1, DIM).to(dev()), enc.reshape(-1, DIM).to(dev())
    layer(h, e, B, F)                       # buffers allocated, RoPE tables resident
    with program.Recorder() as rec:
        out = layer(h, e, B, F)
    prog = rec.finish()
    assert prog is not None, rec.invalid
    recorded = {it[1] for it in rec.items if isinstance(it, tuple)}
    assert {_opcodes.OPCODES["vsys_attn_temporal_d64"], _opcodes.OPCODES["vsys_scale_add_rows"]} <= recorded
    torch.cuda.synchronize()
    want = [t.clone() for t in out]
    for t in out:
        t.fill_(float("nan"))
    prog.run()
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    check(out, F, False, "replayed step")
