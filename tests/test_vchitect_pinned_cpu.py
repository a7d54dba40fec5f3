"""No GPU, no reference tree: the Vchitect-2.0 restatements (tests/vchitect_ref.py, tests/vchitect_sp_ref.py) and the HIP model's state
dict held to fixtures minted from the reference's OWN VchitectXLTransformerModel / JointTransformerBlock (tools/mint_vchitect.py):

  tests/golden/vchitect_fwd_small.pt     the model in the pipeline's call form (B = 1, one text row [1, L, D]): f3, f1, rect, b2f1
  tests/golden/vchitect_pab_small.pt     eight calls (four steps x the two rows of a CFG pair) under PAB, and the same calls without
  tests/golden/vchitect_layer_small.pt   one JointTransformerBlock (context_pre_only False / True) and the outputs of its attn module
  tests/golden/vchitect_sp_small.pt      the model with sp_size = 2 in two gloo processes

Bound.  The restatement computes every step as the class does except the temporal rotation, which it does in float64 where the class
uses fp32 (`xq.float()`, complex64) whatever the dtype.  So rms(restatement - class float64) must stay within the class's own
rms(float32 run - float64 run) of the same tensor — a number of the reference alone, stored in the fixture — and where the rotated
branch is multiplied by 0 (one frame: f1, b2f1) within 1e-12 of the output's magnitude.  Both sides are printed."""
import os
import subprocess
import sys

import pytest
import torch

import vchitect_ref as vr
import vchitect_sp_ref as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = {n: os.path.join(GOLDEN, f"vchitect_{n}_small.pt") for n in ("fwd", "pab", "layer", "sp")}
CFG = dict(num_layers=2, heads=3, patch=2, out_channels=16, sample_size=32, pos_embed_max_size=24)


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def fx():
    return {n: torch.load(p, weights_only=True) for n, p in FILES.items()}


@pytest.fixture(scope="module")
def sd(fx):
    from videosys_amd.vchitect import synth_state_dict

    kw = fx["fwd"]["meta"]["kwargs"]
    assert all(fx[n]["meta"]["seed"] == fx["fwd"]["meta"]["seed"] for n in FILES)
    return {k: v.to(torch.bfloat16).float() for k, v in synth_state_dict(kw["num_layers"], kw["num_attention_heads"],
            joint_attention_dim=kw["joint_attention_dim"], pooled_projection_dim=kw["pooled_projection_dim"], seed=fx["fwd"]["meta"]["seed"]).items()}


def hold(got, want, floor, what, exact=False):
    """rms(got - want) <= floor (the class's fp32-vs-float64 rms), or max|got - want| <= 1e-12 max|want| where nothing is rotated."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float64
    err, worst, mag = rms(got, want), float((got - want).abs().max()), float(want.abs().max())
    print(f"[{what}] restatement rms error {err:.4e} (max {worst:.4e}), reference fp32 floor {floor:.4e}, max |ref| {mag:.3f}")
    if exact:
        assert worst <= 1e-12 * mag, f"{what}: max error {worst:.4e} > 1e-12 x {mag:.3f}"
    else:
        assert err <= floor, f"{what}: rms error {err:.4e} > the reference's own fp32 floor {floor:.4e}"


def test_fixtures_are_small_and_hold_data_only(fx):
    sizes = [os.path.getsize(p) for p in FILES.values()]
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("vchitect_"))
    assert all(s < 1 << 20 for s in sizes) and sum(sizes) < largest
    meta = fx["fwd"]["meta"]
    assert meta["kwargs"] == dict(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=3,
                                  joint_attention_dim=64, caption_projection_dim=192, pooled_projection_dim=64, out_channels=16,
                                  pos_embed_max_size=24)
    shapes = {n: (tuple(c["x"].shape), tuple(c["encoder_hidden_states"].shape), tuple(c["pooled"].shape)) for n, c in fx["fwd"]["cases"].items()}
    assert shapes == {"f3": ((1, 3, 16, 16, 16), (1, 8, 64), (1, 64)), "f1": ((1, 1, 16, 16, 16), (1, 8, 64), (1, 64)),
                      "rect": ((1, 2, 16, 16, 12), (1, 8, 64), (1, 64)), "b2f1": ((2, 1, 16, 16, 16), (2, 8, 64), (2, 64))}
    for c in fx["fwd"]["cases"].values():        # bf16-exact inputs; float64, float32 and bfloat16 outputs of the class
        assert c["x"].dtype == torch.bfloat16
        assert [c["ref_" + t].dtype for t in ("f64", "f32", "bf16")] == [torch.float64, torch.float32, torch.bfloat16]
    p = fx["pab"]
    assert p["timesteps"] == [900, 700, 500, 300] and tuple(p["encoder_hidden_states"].shape) == (2, 8, 64)
    assert all(len(p[k + t]) == 8 for k in ("pab_", "free_") for t in ("f64", "f32", "bf16"))
    assert not torch.equal(p["encoder_hidden_states"][0], p["encoder_hidden_states"][1])


@pytest.mark.parametrize("case", ["f3", "f1", "rect", "b2f1"])
def test_model_forward_is_pinned_to_the_reference_class(fx, sd, case):
    """vr.model_forward in float64, handed the [B, L, D] text rows as videosys_amd/vchitect.py accepts them."""
    c = fx["fwd"]["cases"][case]
    B = c["x"].shape[0]
    out = vr.model_forward(sd, CFG, c["x"].float(), c["encoder_hidden_states"].float(), c["pooled"].float(), torch.tensor([float(c["t"])] * B))
    hold(out, c["ref_f64"], fx["fwd"]["meta"]["floor_f32"][case], f"model {case}", exact=case in ("f1", "b2f1"))


@pytest.mark.parametrize("which", ["joint", "context_pre_only"])
def test_block_and_attention_layer_are_pinned_to_the_reference_block(fx, sd, which):
    """block_forward (the block of model_forward) and the attention_layer inside it against a stand-alone reference JointTransformerBlock
    and its attn module (forward hook), B = 1, F = 3, S = 16, L = 4."""
    ref = fx["layer"][which]
    last = which == "context_pre_only"
    hs, enc, temb = (t.double() for t in vr.layer_inputs(fx["layer"]["meta"]["seed"]))
    x, y, (av, at) = vr.block_forward(sd, f"transformer_blocks.{int(last)}.", hs, enc, temb, 1, 3, 3, last)
    hold(av, ref["attn_x_f64"], ref["attn_x_f32_floor"], f"attention_layer video, {which}")
    hold(at, ref["attn_y_f64"], ref["attn_y_f32_floor"], f"attention_layer text, {which}")
    hold(x, ref["x_f64"], ref["x_f32_floor"], f"block video, {which}")
    if last:
        assert "y_f64" not in ref and torch.equal(y, enc)          # the class returns None for the text stream
    else:
        hold(y, ref["y_f64"], ref["y_f32_floor"], f"block text, {which}")


def pab_decisions(p):
    """(temporal, cross, spatial) of the eight calls from videosys_amd.pab, counters advancing once per CALL (twice per step)."""
    from videosys_amd import pab

    ct = cc = cs = 0
    want = []
    for t in p["timesteps"]:
        for _ in range(2):
            bt, ct = pab.if_broadcast_temporal(t, ct)
            bc, cc = pab.if_broadcast_cross(t, cc)
            bs, cs = pab.if_broadcast_spatial(t, cs)
            want.append((bt, bc, bs))
    return want


def test_pab_run_is_pinned_to_the_reference_class(fx, sd):
    """The restatement with a PabState (three counters and the three caches, cached where attentions.py:839-896 caches them; the
    decisions from videosys_amd.pab) over the eight calls: every output within the floor of the class's PAB run, so a GPU failure
    against the fixture can be told from a restatement failure.  The fixture itself shows what a wrong cache costs: on every call with
    a stale branch the class's PAB output is >= 6 x its bf16 floor away from its PAB-free output."""
    from videosys_amd import pab

    p = fx["pab"]
    try:
        pab.set_pab_manager(pab.PABConfig(**p["config"]))
        pab.update_steps(len(p["timesteps"]))
        want = pab_decisions(p)
        assert want == [tuple(d) for d in p["decisions"]]       # videosys_amd.pab decides as the reference's pab_mgr did at mint time
        assert want[0] == (False, False, False) and all(any(w[i] for w in want) for i in range(3))
        state = vr.PabState(CFG["num_layers"])
        for i in range(8):
            s, r = divmod(i, 2)
            out = vr.model_forward(sd, CFG, p["x"][s:s + 1].float(), p["encoder_hidden_states"][r:r + 1].float(), p["pooled"][r:r + 1].float(),
                                   torch.tensor([float(p["timesteps"][s])]), pab_state=state)
            assert [b.last_decisions for b in state.blocks] == [want[i]] * 2
            hold(out, p["pab_f64"][i], p["meta"]["floor_f32"][i], f"pab call {i} {want[i]}")
            gap, floor = rms(p["pab_f64"][i], p["free_f64"][i]), p["meta"]["floor_bf16"][i]
            assert floor == pytest.approx(rms(p["pab_bf16"][i], p["pab_f64"][i]), rel=1e-9)
            if any(want[i]):
                assert gap >= 4 * 1.5 * floor
            else:
                assert torch.equal(p["pab_f64"][i], p["free_f64"][i])
    finally:
        pab.set_pab_manager(None)


def test_sharded_restatement_is_pinned_to_the_two_process_reference(fx, sd):
    """vchitect_sp_ref.model_forward(P = 2) against the reference run with sp_size = 2 over gloo: F = 3 (temporal pad 1), S + L = 71
    (spatial pad 1).  The sharded class does NOT compute what the single-rank class computes (a rank's cross keys are row 0 of its own
    shard), which the fixture shows, so this pin can only be met by restating the sharded forward."""
    f = fx["sp"]
    meta = f["meta"]
    assert (meta["P"], meta["F"], meta["L"]) == (2, 3, 7) and tuple(f["x"].shape) == (1, 3, 16, 16, 16)
    enc = f["encoder_hidden_states"].float().repeat_interleave(meta["F"], dim=0)
    out = vs.model_forward(sd, CFG, f["x"].float(), enc, f["pooled"].float(), torch.tensor([float(f["t"])]), meta["P"])
    hold(out, f["ref_f64"], meta["floor_f32"], "sharded model, P = 2")
    assert rms(f["single_f64"], f["ref_f64"]) > 100 * meta["floor_f32"]
    single = vr.model_forward(sd, CFG, f["x"].float(), f["encoder_hidden_states"].float(), f["pooled"].float(), torch.tensor([float(f["t"])]))
    hold(single, f["single_f64"], meta["floor_f32"], "the same call, one rank")


def test_state_dict_names_shapes_and_position_buffer(fx, sd):
    from videosys_amd import vchitect

    meta = fx["fwd"]["meta"]
    model = vchitect.VchitectXLTransformerModel(**meta["kwargs"], device="cpu")
    ref = {k: tuple(s) for k, s in meta["state_dict_shapes"]}
    assert set(model.expected_keys()) | {"pos_embed.pos_embed"} == set(ref) and len(set(model.expected_keys())) == len(model.expected_keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: s for k, s in ref.items() if k != "pos_embed.pos_embed"}
    buf = fx["fwd"]["pos_embed"]
    assert tuple(buf.shape) == ref["pos_embed.pos_embed"] == (1, 24 * 24, 192) and buf.dtype == torch.float32
    # the table the model computes is the class's buffer bit for bit (w-first grid, base_size = sample_size // patch)
    assert torch.equal(model.pos_embed, buf[0])
    computed = model.load_state_dict(sd).cropped_pos_embed(8, 6).clone()
    m = 24
    assert torch.equal(computed, buf.reshape(m, m, 192)[8:16, 9:15].reshape(48, 192).to(torch.bfloat16))      # top 8, left 9: H != W
    # a checkpoint's buffer is taken when present: the same table from the class's buffer, another table from another buffer
    assert torch.equal(model.load_state_dict({**sd, "pos_embed.pos_embed": buf}).cropped_pos_embed(8, 6), computed)
    other = model.load_state_dict({**sd, "pos_embed.pos_embed": buf.flip(1)}).cropped_pos_embed(8, 6)
    assert torch.equal(other, buf.flip(1).reshape(m, m, 192)[8:16, 9:15].reshape(48, 192).to(torch.bfloat16)) and not torch.equal(other, computed)


def test_committed_fixtures_are_what_the_mint_makes():
    """Where the reference tree is present: tools/mint_vchitect.py --check rebuilds the four fixtures in memory (the two-process run
    included) and compares them with the committed files."""
    from oracle import ref_loader

    if not ref_loader.reference_available():
        pytest.skip("no reference tree: the fixtures cannot be rebuilt here")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mint_vchitect.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fixture matches" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
