"""No GPU: the Open-Sora-Plan v1.2 transformer's host side.

* tests/osp_ref.py (the plain-torch restatement every GPU test of the model is measured against) is PINNED to the reference's own
  OpenSoraT2V class through tests/golden/osp_v120_fwd_small.pt (tools/mint_osp_v120.py): its float64 run equals the class's float64
  output to 1e-9 of the output's magnitude — float64 round-off over a few thousand operations — without and with PAB.
* videosys_amd.open_sora_plan.rope3d_tables equals the restatement of PositionGetter3D + RoPE3D.get_cos_sin bit for bit.
* The HIP model's state-dict names and shapes are the reference class's; unbuilt configurations raise NotImplementedError at
  construction; masks that are no prefix of ones raise ValueError; the two new entry points are declared, exported, bound, and
  outside the (pinned) op table; their host-side argument checks refuse bad shapes before any launch."""
import os
import re

import pytest
import torch

import osp_ref
from op_table import assert_coded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "osp_v120_fwd_small.pt")
NEW = ("vsys_attn_prep_kv96", "vsys_flash_attn_d96")
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3


@pytest.fixture(scope="module")
def fx():
    return torch.load(FIXTURE, weights_only=True)


def synth(fx):
    from videosys_amd.open_sora_plan import synth_state_dict

    kw = fx["kwargs"]
    return synth_state_dict(num_layers=kw["num_layers"], num_heads=kw["num_attention_heads"], caption_channels=kw["caption_channels"],
                            in_channels=kw["in_channels"], out_channels=kw["out_channels"], patch_size=kw["patch_size"], seed=fx["seed"])


def test_fixture_is_small_and_holds_data_only(fx):
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")))
    assert os.path.getsize(FIXTURE) < min(largest, 1 << 20) and os.path.getsize(FIXTURE) < 256 * 1024
    assert tuple(fx["x"].shape) == (2, 4, 3, 8, 12) and tuple(fx["encoder_hidden_states"].shape) == (2, 1, 8, 32)
    assert fx["encoder_attention_mask"].sum(dim=-1).flatten().tolist() == [8.0, 5.0]
    for tag in ("f64", "f32", "bf16"):
        assert tuple(fx["ref_" + tag].shape) == tuple(fx["pab_" + tag].shape) == (2, 4, 3, 8, 12)
    assert fx["ref_f64"].dtype == torch.float64 and fx["ref_bf16"].dtype == torch.bfloat16


def test_restatement_is_pinned_to_the_reference_class(fx):
    sd, kw = synth(fx), fx["kwargs"]
    t1, t2 = fx["pab_timesteps"]
    cos, sin = osp_ref.rope_tables(3, 4, 6, 96, torch.float64, (1.0, 1.0, 1.0))     # a float64 run of the class makes float64 tables
    cache = {}
    args = (fx["encoder_hidden_states"], fx["encoder_attention_mask"], cos, sin, torch.float64)
    out = osp_ref.forward(sd, kw, fx["x"], torch.tensor([t1, t1]), *args, cache=cache)
    ref = fx["ref_f64"]
    assert float((out - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    assert len(cache) == 2 * kw["num_layers"]
    out2 = osp_ref.forward(sd, kw, fx["x2"], torch.tensor([t2, t2]), *args, cache=cache, broadcast=(True, True))
    ref2 = fx["pab_f64"]
    assert float((out2 - ref2).abs().max()) <= 1e-9 * float(ref2.abs().max())
    # the PAB step is not the plain forward of x2: the caches matter
    plain2 = osp_ref.forward(sd, kw, fx["x2"], torch.tensor([t2, t2]), *args)
    assert float((plain2 - ref2).abs().max()) > 1e-3 * float(ref2.abs().max())


def test_restatement_is_pinned_at_non_unit_scales_and_equal_axis_lengths(fx):
    """The fixture's second geometry: T = H/p = 4 tokens with scales (2, 1.5, 2).  The reference's table cache is keyed by length, not
    scale (:74), so its rows are rotated with the FRAMES' table: the restatement with that property equals the class's float64 output
    to round-off; tables made per axis with the axis's own scale do not."""
    from videosys_amd.open_sora_plan import OpenSoraT2V, rope3d_tables

    sd, kw = synth(fx), fx["scaled_kwargs"]
    scales = (kw["interpolation_scale_t"], kw["interpolation_scale_h"], kw["interpolation_scale_w"])
    assert scales == (2.0, 1.5, 2.0) and tuple(fx["scaled_x"].shape) == (2, 4, 4, 8, 12)
    t = torch.tensor([fx["pab_timesteps"][0]] * 2)
    ref = fx["scaled_ref_f64"]
    run = lambda cos, sin: osp_ref.forward(sd, kw, fx["scaled_x"], t, fx["encoder_hidden_states"], fx["encoder_attention_mask"], cos, sin,
                                           torch.float64)
    cos, sin = osp_ref.rope_tables(4, 4, 6, 96, torch.float64, scales)
    assert float((run(cos, sin) - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    own = [osp_ref.cos_sin_1d(32, n, torch.float64, s) for n, s in zip((4, 4, 6), scales)]         # every axis at its own scale
    pos = torch.cartesian_prod(torch.arange(4), torch.arange(4), torch.arange(6))
    cos_own, sin_own = (torch.cat([own[a][i][pos[:, a]] for a in range(3)], dim=-1) for i in (0, 1))
    assert float((run(cos_own, sin_own) - ref).abs().max()) > 1e-4 * float(ref.abs().max())
    # the model's builder has the property too, and derives the same scales from the constructor arguments
    model = OpenSoraT2V(**kw, device="cpu")
    assert model.interpolation_scale_thw == scales
    for dt in (torch.float64, torch.bfloat16):
        got, want = rope3d_tables(4, 4, 6, scales, dt), osp_ref.rope_tables(4, 4, 6, 96, dt, scales)
        assert torch.equal(got[0], want[0].float()) and torch.equal(got[1], want[1].float())
        assert torch.equal(got[0][:, 32:64].view(4, 4, 6, 32)[0, :, 0], got[0][:, :32].view(4, 4, 6, 32)[:, 0, 0])   # rows use the frames' table


def test_hard_mask_equals_the_reference_bias(fx):
    """What the HIP model does with the mask (sample b sees its first count keys) against what the reference does (-10000 on hidden
    keys): the same float64 output to round-off."""
    sd, kw = synth(fx), fx["kwargs"]
    cos, sin = osp_ref.rope_tables(3, 4, 6, 96, torch.float64)
    t = torch.tensor([500, 500])
    b = 1
    enc, mask = fx["encoder_hidden_states"][b:b + 1], fx["encoder_attention_mask"][b:b + 1]
    with_bias = osp_ref.forward(sd, kw, fx["x"][b:b + 1], t[:1], enc, mask, cos, sin, torch.float64)
    hard = osp_ref.forward(sd, kw, fx["x"][b:b + 1], t[:1], enc[:, :, :5], None, cos, sin, torch.float64)
    assert float((with_bias - hard).abs().max()) <= 1e-12 * float(hard.abs().max())


@pytest.mark.parametrize("scales", [(1.0, 1.0, 1.0), (2.0, 1.5, 2.0)])
@pytest.mark.parametrize("thw", [(3, 4, 6), (8, 30, 40)])
@pytest.mark.parametrize("rope_dtype", [torch.bfloat16, torch.float32])
def test_rope_table_builder_bit_for_bit(thw, scales, rope_dtype):
    from videosys_amd.open_sora_plan import rope3d_tables

    cos, sin = rope3d_tables(*thw, scales, rope_dtype)
    rc, rs = osp_ref.rope_tables(*thw, 96, rope_dtype, scales)
    n = thw[0] * thw[1] * thw[2]
    assert cos.dtype == sin.dtype == torch.float32 and tuple(cos.shape) == tuple(sin.shape) == (n, 96)
    assert torch.equal(cos, rc.float()) and torch.equal(sin, rs.float())
    # the tables are rotations chunk by chunk: columns i and i + 16 of a chunk share their angle
    c = cos.view(n, 3, 2, 16)
    assert torch.equal(c[:, :, 0], c[:, :, 1])


def test_state_dict_names_and_shapes_are_the_reference_classes(fx):
    from videosys_amd.open_sora_plan import OpenSoraT2V

    model = OpenSoraT2V(**fx["kwargs"], device="cpu")
    want = {k: tuple(s) for k, s in fx["state_dict_shapes"]}
    assert model.expected_shapes() == want
    assert {k: tuple(v.shape) for k, v in synth(fx).items()} == want
    sd = synth(fx)
    assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values()), "synthetic weights are not bf16-exact"
    model.enable_parallel(1, 1, False)
    with pytest.raises(NotImplementedError):
        model.enable_parallel(1, 2, False)
    with pytest.raises(NotImplementedError):
        model.enable_parallel(1, 1, True)
    model.reset_pab_state()


def test_rope_l_122_geometry():
    from videosys_amd.open_sora_plan import OpenSoraT2V_ROPE_L_122

    m = OpenSoraT2V_ROPE_L_122(in_channels=4, out_channels=8, attention_bias=True, sample_size=(60, 80), sample_size_t=8,
                               activation_fn="gelu-approximate", norm_elementwise_affine=False, norm_eps=1e-6, use_rope=True,
                               interpolation_scale_t=1.0, device="cpu")
    assert (m.L, m.H, m.C, m.config.cross_attention_dim, m.config.caption_channels) == (32, 24, 2304, 2304, 4096)
    assert m.interpolation_scale_thw == (1.0, 2.0, 2.0)            # sample_size / (30, 40) (:1610-1617)


@pytest.mark.parametrize("change", [dict(norm_type="layer_norm"), dict(use_rope=False), dict(downsampler="k33_s22"), dict(patch_size_t=2),
                                    dict(activation_fn="geglu"), dict(attention_head_dim=72, cross_attention_dim=144),
                                    dict(out_channels=12), dict(norm_elementwise_affine=True), dict(attention_bias=False),
                                    dict(cross_attention_dim=1152), dict(caption_channels=None)],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_unbuilt_configurations_are_refused(fx, change):
    from videosys_amd.open_sora_plan import OpenSoraT2V

    with pytest.raises(NotImplementedError):
        OpenSoraT2V(**{**fx["kwargs"], **change}, device="cpu")


def test_masks(fx):
    from videosys_amd.open_sora_plan import OpenSoraT2V

    model = OpenSoraT2V(**fx["kwargs"], device="cpu")
    assert model._check_mask(fx["encoder_attention_mask"], 2, 8) == [8, 5]
    assert model._check_mask(None, 2, 8) == [8, 8]
    hole = torch.ones(2, 1, 8)
    hole[0, 0, 2] = 0
    empty = torch.ones(2, 1, 8)
    empty[1] = 0
    for bad in (hole, empty, torch.ones(2, 1, 7)):
        with pytest.raises(ValueError):
            model._check_mask(bad, 2, 8)
    # a video mask that hides a token, and image joint training, are refused before anything is launched
    vm = torch.ones(2, 3, 8, 12)
    vm[0, 0, 0, 0] = 0
    with pytest.raises(NotImplementedError):
        model.forward(fx["x"], torch.tensor([500]), fx["encoder_hidden_states"], attention_mask=vm)
    with pytest.raises(NotImplementedError):
        model.forward(fx["x"], torch.tensor([500]), fx["encoder_hidden_states"], use_image_num=1)


def test_alias_and_top_level_names():
    import importlib

    import videosys

    m = importlib.import_module("videosys.models.transformers.open_sora_plan_v120_transformer_3d")
    from videosys_amd import open_sora_plan

    assert m is open_sora_plan and hasattr(m, "OpenSoraT2V") and hasattr(m, "OpenSoraT2V_ROPE_L_122")
    with pytest.raises(ImportError):
        videosys.OpenSoraPlanConfig


def test_entry_points_declared_exported_bound_and_in_the_op_table():
    from videosys_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    lib = _lib.load()
    for n in NEW:
        assert re.search(rf"\nint {n}\(", hdr) and n in _lib.SIGNATURES and hasattr(lib, n)
    assert_coded(NEW)                                 # in the launch-program table, with the prototype's arity
    assert "open_sora_plan_v120_transformer_3d.py:" in hdr


def test_host_side_argument_checks():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # an aligned address that is never dereferenced: every call below is refused before any launch

    def prep(k=P, ks=192, v=P, vs=192, cos=None, sin=None, kp=P, vt=P, batch=2, heads=2, kv_len=72, kv_pad=128):
        return lib.vsys_attn_prep_kv96(k, ks, v, vs, cos, sin, kp, vt, batch, heads, kv_len, kv_pad, None)

    def flash(q=P, qs=192, cos=None, sin=None, kp=P, vt=P, lens=None, out=P, os_=192, batch=2, heads=2, q_len=72, kv_len=72, kv_pad=128):
        return lib.vsys_flash_attn_d96(q, qs, cos, sin, kp, vt, lens, out, os_, batch, heads, q_len, kv_len, kv_pad, None)

    assert prep(kv_pad=100) == VSYS_ERR_SHAPE and prep(kv_pad=64) == VSYS_ERR_SHAPE          # not a multiple of 64 / shorter than kv_len
    assert prep(ks=190) == VSYS_ERR_SHAPE and prep(vs=96) == VSYS_ERR_SHAPE                  # unaligned / narrower than heads * 96
    assert prep(cos=P) == VSYS_ERR_ARG and prep(k=None) == VSYS_ERR_ARG and prep(vt=None) == VSYS_ERR_ARG
    assert prep(batch=1 << 40) == VSYS_ERR_SHAPE and prep(batch=40000, heads=2) == VSYS_ERR_SHAPE
    assert flash(kv_pad=96) == VSYS_ERR_SHAPE and flash(kv_len=0) == VSYS_ERR_SHAPE and flash(kv_len=200) == VSYS_ERR_SHAPE
    assert flash(qs=100) == VSYS_ERR_SHAPE and flash(os_=190) == VSYS_ERR_SHAPE and flash(os_=96) == VSYS_ERR_SHAPE
    assert flash(sin=P) == VSYS_ERR_ARG and flash(out=None) == VSYS_ERR_ARG and flash(q_len=-1) == VSYS_ERR_SHAPE
    # base pointers: 16-byte loads of q / k / v / tables / images, 8-byte stores to out, 4-byte loads of the counts
    assert prep(k=P + 8) == VSYS_ERR_ALIGN and prep(vt=P + 2) == VSYS_ERR_ALIGN and prep(cos=P + 4, sin=P) == VSYS_ERR_ALIGN
    assert flash(q=P + 8) == VSYS_ERR_ALIGN and flash(out=P + 4) == VSYS_ERR_ALIGN and flash(lens=P + 2) == VSYS_ERR_ALIGN
    assert flash(cos=P, sin=P + 8) == VSYS_ERR_ALIGN and flash(kp=P + 8) == VSYS_ERR_ALIGN
    assert prep(batch=0) == 0 and flash(q_len=0) == 0                                          # nothing to do: nothing is launched
