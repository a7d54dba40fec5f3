"""CPU: Open-Sora-Plan v1.1 without a device.  tests/osp_v110_ref.py (the plain-torch restatement the GPU tests measure against) is held
to the float64 outputs of the reference's OWN LatteT2V v110 class (tests/golden/osp_v110_fwd_small.pt, tools/mint_osp_v110.py) to 1e-9
of the output's magnitude on every case; the HIP class's state-dict names, tables, permutations and refusals are checked on the host."""
import os
import re

import pytest
import torch

import osp_v110_ref as R
from conftest import ROOT
from op_table import assert_coded

FIXTURE = os.path.join(ROOT, "tests", "golden", "osp_v110_fwd_small.pt")


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=True)


def state_dict(fx, gain=None, heads=None):
    from videosys_amd.open_sora_plan_v110 import synth_state_dict

    k = fx["kwargs"]
    return synth_state_dict(num_layers=k["num_layers"], num_heads=heads or k["num_attention_heads"], caption_channels=k["caption_channels"],
                            in_channels=k["in_channels"], out_channels=k["out_channels"], patch_size=k["patch_size"], seed=fx["seed"],
                            qk_gain=fx["qk_gain"] if gain is None else gain)


def ref_model(fx, sd, dtype, kwargs=None, **over):
    k = {**(kwargs or fx["kwargs"]), **over}
    return R.LatteT2VRef(sd, k["num_layers"], k["num_attention_heads"], sample_size=k["sample_size"], out_channels=k["out_channels"],
                         video_length=k["video_length"], use_rope=k["use_rope"], interpolation_scale_1d=k.get("interpolation_scale_1d"),
                         dtype=dtype)


CASES = {"rope": ("x", True, None, {}), "norope": ("x", True, None, {"use_rope": False}), "wide": ("x_wide", True, None, {}),
         "nomask": ("x", False, None, {}), "scaled": ("x_scaled", True, "scaled_kwargs", {})}


def run_case(fx, name, dtype, sd=None, heads=None):
    """``heads``: the same case at another head count (the GPU tests: fx["wide_heads"], the smallest model the HIP GEMMs take)."""
    xk, masked, kwk, over = CASES[name]
    over = dict(over, num_attention_heads=heads) if heads else over
    sd = state_dict(fx, heads=heads) if sd is None else sd
    t = torch.tensor([fx["timestep"]] * 2)
    with torch.no_grad():
        x = fx[xk].float()
        return ref_model(fx, sd, dtype, fx[kwk] if kwk else None, **over)(
            x, t, fx["encoder_hidden_states"].float(), fx["encoder_attention_mask"] if masked else None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_class_in_float64(fx, name):
    out, want = run_case(fx, name, torch.float64), fx[name + "_f64"]
    assert out.shape == want.shape
    assert (out - want).abs().max().item() <= 1e-9 * want.abs().max().item()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_class_in_bf16(fx, name):
    """The same operations in the same order on the CPU: the restatement's bf16 run IS the class's, bit for bit.  This is what holds the
    bf16-only steps (angles cast to bf16 before cos / sin, the position tables' dtype) that no float64 run makes."""
    out, want = run_case(fx, name, torch.bfloat16), fx[name + "_bf16"]
    assert out.dtype == want.dtype == torch.bfloat16 and torch.equal(out, want)


def test_rotation_restatements_equal_the_reference_modules_in_bf16(fx):
    """LinearScalingRoPE2D / 1D of the reference applied in bf16 at scale 2 (fixture ``rope_module``) against rope_tokens_2d / 1d, bit for
    bit; and the HIP class's fp32 tables against the same module outputs through the permutation (rotation in fp32 on the widened
    bf16 tables, compared after the modules' own bf16 rounding of each product and of the sum)."""
    rm = fx["rope_module"]
    tok, (gh, gw), sc = rm["tokens"], rm["grid"], rm["scale"]
    assert torch.equal(R.rope_tokens_2d(tok, gh, gw, sc), rm["out_2d"])
    assert torch.equal(R.rope_tokens_1d(tok, gh * gw, sc), rm["out_1d"])
    from videosys_amd import open_sora_plan_v110 as m

    def interleaved_bf16(x, cos, sin):          # the modules round every product and the sum to bf16
        a, b = x[..., 0::2], x[..., 1::2]
        c, s = cos.to(torch.bfloat16), sin.to(torch.bfloat16)
        return torch.stack([a * c + (-b) * s, b * c + a * s], dim=-1).flatten(-2)

    cos, sin = m.rope_tables_2d(gh, gw, sc)
    perm = m.head_permutation_2d()
    assert torch.equal(interleaved_bf16(tok[..., perm], cos, sin), rm["out_2d"][..., perm])
    cos, sin = m.rope_tables_1d(gh * gw, sc)
    perm = m.head_permutation_1d()
    assert torch.equal(interleaved_bf16(tok[..., perm], cos[:, 0::2], sin[:, 0::2]), rm["out_1d"][..., perm])


def test_restatement_equals_the_reference_class_at_the_gpu_tests_head_count(fx):
    out, want = run_case(fx, "rope", torch.float64, heads=fx["wide_heads"]["num_attention_heads"]), fx["rope_heads8_f64"]
    assert (out - want).abs().max().item() <= 1e-9 * want.abs().max().item()


def test_restatement_equals_the_reference_class_under_pab(fx):
    from videosys_amd import pab

    m = ref_model(fx, state_dict(fx), torch.float64)
    pab.set_pab_manager(pab.PABConfig(**fx["pab"]))
    try:
        pab.update_steps(len(fx["pab_timesteps"]))
        with torch.no_grad():
            for i, t in enumerate(fx["pab_timesteps"]):
                out = m(fx["pab_x"][i].float(), torch.tensor([t, t]), fx["encoder_hidden_states"].float(), fx["encoder_attention_mask"],
                        all_timesteps=torch.tensor(fx["pab_timesteps"]))
                want = fx["pab_f64"][i]
                assert (out - want).abs().max().item() <= 1e-9 * want.abs().max().item(), f"PAB step {i}"
    finally:
        pab.set_pab_manager(None)


@pytest.mark.parametrize("heads", [None, 8], ids=["fixture", "gpu-heads"])
def test_rotation_shows_at_the_fixture_weights(fx, heads):
    """Sensitivity: RoPE off differs from RoPE on by at least 10 x the bf16 floor (restatement in bf16 against its own float64 run),
    max abs.  The q / k gain of the fixture exists for this: at gain 1 the effect is a few floors and a missing rotation could pass."""
    on, off = run_case(fx, "rope", torch.float64, heads=heads), run_case(fx, "norope", torch.float64, heads=heads)
    floor = (run_case(fx, "rope", torch.bfloat16, heads=heads).double() - on).abs().max().item()
    effect = (on - off).abs().max().item()
    print(f"rope effect {effect:.4f}, bf16 floor {floor:.4f} (output max {on.abs().max().item():.3f})")
    assert effect >= 10 * floor


def test_hip_class_state_dict_names_and_shapes(fx, monkeypatch):
    from videosys_amd import _lib, open_sora_plan_v110 as m

    monkeypatch.setattr(_lib, "load", lambda: None)
    model = m.LatteT2V(**fx["kwargs"], device="cpu")
    want = dict(fx["state_dict_shapes"])
    sd = state_dict(fx)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert set(model.expected_keys()) | {"caption_projection.y_embedding"} == set(want)
    model.load_state_dict(sd, strict=True)
    for gone in ("proj_out.bias", "transformer_blocks.1.attn1.to_q.weight", "temporal_transformer_blocks.0.attn1.to_k.bias"):
        with pytest.raises(KeyError, match="missing keys.*" + re.escape(gone)):      # the strict check names the key
            model.load_state_dict({k: v for k, v in sd.items() if k != gone}, strict=True)
    # the permuted rows: q of head 1, new column 2p / 2p + 1 of a spatial block = old p / p + 18
    p = "transformer_blocks.0.attn1"
    w = model.w[p + ".qkv.weight"].float()
    old = sd[p + ".to_q.weight"].to(torch.bfloat16).float()
    assert torch.equal(w[72 + 2], old[72 + 1]) and torch.equal(w[72 + 3], old[72 + 19]) and torch.equal(w[72 + 36], old[72 + 36])
    p = "temporal_transformer_blocks.1.attn1"
    w, old = model.w[p + ".qkv.weight"].float(), sd[p + ".to_k.weight"].to(torch.bfloat16).float()
    assert torch.equal(w[144 + 3], old[37]) and torch.equal(w[144 + 72 + 70], old[72 + 35])
    v_old = sd[p + ".to_v.weight"].to(torch.bfloat16).float()
    assert torch.equal(w[288:], v_old), "v is not permuted"
    plain = m.LatteT2V(**{**fx["kwargs"], "use_rope": False}, device="cpu").load_state_dict(sd)
    assert torch.equal(plain.w["transformer_blocks.0.attn1.qkv.weight"][:144].float(), sd["transformer_blocks.0.attn1.to_q.weight"].to(torch.bfloat16).float())


@pytest.mark.parametrize("gh,gw,T,s2,s1", [(4, 4, 5, 1.0, 1.0), (4, 6, 5, 1.0, 1.0), (64, 4, 3, 2.0, 2.0), (5, 7, 17, 1.0, 3.0)])
def test_tables_equal_the_restatements_bit_for_bit(gh, gw, T, s2, s1):
    from videosys_amd import open_sora_plan_v110 as m

    for mine, ref in zip(m.rope_tables_2d(gh, gw, s2) + m.rope_tables_1d(T, s1), R.tables_2d(gh, gw, s2) + R.tables_1d(T, s1)):
        assert mine.dtype == torch.float32 and mine.shape == ref.shape and torch.equal(mine, ref)
    if s1 > 1:      # the truncation: frames 0 .. s1 - 1 share position 0
        c, _ = m.rope_tables_1d(T, s1)
        assert torch.equal(c[0], c[int(s1) - 1]) and not torch.equal(c[0], c[int(s1)])


def test_permutation_identity_in_float64():
    """Interleaved rotation on permuted q, k gives the logits of rotate-half on the originals (to 1e-12), for both permutations."""
    from videosys_amd import open_sora_plan_v110 as m

    g = torch.Generator().manual_seed(3)
    q, k = torch.randn(2, 35, 72, generator=g, dtype=torch.float64), torch.randn(2, 35, 72, generator=g, dtype=torch.float64)

    def interleaved(x, cos, sin):
        a, b = x[..., 0::2], x[..., 1::2]
        return torch.stack([a * cos - b * sin, b * cos + a * sin], dim=-1).flatten(-2)

    want = R.rope_tokens_2d(q[:, None], 5, 7, 1.0)[:, 0] @ R.rope_tokens_2d(k[:, None], 5, 7, 1.0)[:, 0].transpose(-1, -2)
    # (float64 angles in the tables' pair order: the model's own tables are widened to fp32 only, which would cost 1e-7 here)
    y, x = torch.arange(5).repeat_interleave(7), torch.arange(7).repeat(5)
    (cy, sy), (cx, sx) = R.cos_sin(36, y, 1.0, torch.float64), R.cos_sin(36, x, 1.0, torch.float64)
    cos, sin = torch.cat([cy[:, :18], cx[:, :18]], 1), torch.cat([sy[:, :18], sx[:, :18]], 1)
    perm = m.head_permutation_2d()
    got = interleaved(q[..., perm], cos, sin) @ interleaved(k[..., perm], cos, sin).transpose(-1, -2)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    want = R.rope_tokens_1d(q[:, None], 35, 2.0)[:, 0] @ R.rope_tokens_1d(k[:, None], 35, 2.0)[:, 0].transpose(-1, -2)
    cos, sin = (t[:, :36] for t in R.cos_sin(72, torch.arange(35), 2.0, torch.float64))
    perm = m.head_permutation_1d()
    got = interleaved(q[..., perm], cos, sin) @ interleaved(k[..., perm], cos, sin).transpose(-1, -2)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert sorted(m.head_permutation_2d().tolist()) == sorted(m.head_permutation_1d().tolist()) == list(range(72))


@pytest.mark.parametrize("over", [{"compress_kv_factor": 2}, {"norm_type": "layer_norm"}, {"norm_type": "ada_norm"}, {"activation_fn": "geglu"},
                                  {"attention_bias": False}, {"norm_elementwise_affine": True}, {"patch_size_t": 2},
                                  {"rope_scaling_type": "dynamic"}, {"sample_size": (8, 12)}], ids=lambda o: next(iter(o)) + "=" + str(next(iter(o.values()))))
def test_unbuilt_configurations_raise(fx, monkeypatch, over):
    from videosys_amd import _lib, open_sora_plan_v110 as m

    monkeypatch.setattr(_lib, "load", lambda: None)
    with pytest.raises(NotImplementedError):
        m.LatteT2V(**{**fx["kwargs"], **over}, device="cpu")


def test_forward_refuses_what_is_not_built(fx, monkeypatch):
    from videosys_amd import _lib, open_sora_plan_v110 as m

    monkeypatch.setattr(_lib, "load", lambda: None)
    model = m.LatteT2V(**fx["kwargs"], attention_mode="xformers", device="cpu")       # attention_mode: accepted and ignored
    x, enc = fx["x"].float(), fx["encoder_hidden_states"].float()
    with pytest.raises(NotImplementedError):
        model(x, timestep=torch.tensor([1, 1]), encoder_hidden_states=enc, use_image_num=2)
    holes = torch.ones(2, 5, 8, 8)
    holes[0, 0, 0, 0] = 0
    with pytest.raises(NotImplementedError):
        model(x, timestep=torch.tensor([1, 1]), encoder_hidden_states=enc, attention_mask=holes)
    with pytest.raises(NotImplementedError):
        model.enable_parallel(dp_size=1, sp_size=2, enable_cp=False)
    with pytest.raises(NotImplementedError, match="single frame"):       # (the reference's temporal block fails on one frame too)
        model(x[:, :, :1], timestep=torch.tensor([1, 1]), encoder_hidden_states=enc)


def test_new_entry_points_are_bound_with_op_codes():
    from videosys_amd import _opcodes

    names = ("vsys_attn_prep_kv_rope", "vsys_flash_attn_d72_rope")
    for name in names:
        assert name in _opcodes.ENTRY_POINTS
    assert_coded(names)
