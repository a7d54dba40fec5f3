"""CPU tests of the Open-Sora-Plan v1.2 pipeline pieces (no GPU):

  * tests/osp_vae_ref.py (the torch restatement of the CausalVAE decoder, tiling included) against the float64 outputs of the
    reference's own CausalVAEModel (tests/golden/osp_vae_small*.pt, tools/mint_osp_vae.py) to 1e-9 on all four cases, and its
    state-dict names and shapes against the fixture's and ``decoder_param_shapes(32)``;
  * EulerAncestralDiscreteScheduler (an UNPINNED restatement of diffusers' class) against its closed form in float64;
  * the three entry points of csrc/vae_osp.hip: in the header, the library and the ctypes table, outside the op table, and their
    host-side argument refusals on a never-dereferenced pointer;
  * config defaults, the v110 refusal, the signatures against tests/golden/osp_pipeline_surface.json (tools/mint_osp_surface.py);
  * the ``videosys`` aliases resolve and the top-level names still raise."""
import ctypes
import functools
import inspect
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import osp_vae_ref as R
from op_table import assert_coded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3


# ---------------------------------------------------------------------------------------------------- decoder restatement
@functools.lru_cache(maxsize=None)
def fixture():
    fx = dict(torch.load(os.path.join(GOLDEN, "osp_vae_small.pt"), weights_only=True))
    fx["a"] = torch.load(os.path.join(GOLDEN, "osp_vae_small_a.pt"), weights_only=True)["a"]
    fx["b"] = torch.load(os.path.join(GOLDEN, "osp_vae_small_b.pt"), weights_only=True)["b"]
    return fx


@functools.lru_cache(maxsize=None)
def weights():
    from videosys_amd.vae_open_sora_plan import synth_state_dict

    fx = fixture()
    return synth_state_dict(fx["seed"], fx["hidden_size"])


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_restatement_equals_the_reference_class(name):
    fx = fixture()
    z = fx["z"]
    zz, tiling = {"a": (z, None), "b": (z, fx["tiling"]), "c": (z[:, :, :1], None), "d": (z[:, :, :2], None)}[name]
    out = R.wrapper_decode(zz, weights(), tiling)
    ref = fx[name]
    assert out.dtype == torch.float64 and tuple(out.shape) == tuple(ref.shape) == (1, 4 * (zz.shape[2] - 1) + 1, 3, 48, 64)
    assert float((out - ref).abs().max()) <= 1e-9
    if name == "b":      # two temporal chunks, 2 x 3 spatial tiles, edge tiles smaller than the interior ones
        t = fx["tiling"]
        assert R.t_chunks(3, t["tile_latent_min_size_t"]) == [[0, 2], [1, 3]]
        step = int(t["tile_latent_min_size"] * (1 - t["tile_overlap_factor"]))
        assert (len(range(0, 6, step)), len(range(0, 8, step))) == (2, 3) and 6 - step < t["tile_latent_min_size"]
        assert float((fx["a"] - fx["b"]).abs().max()) > 1e-3        # tiling changes the result


def test_state_dict_names_and_shapes():
    from videosys_amd.vae_open_sora_plan import decoder_param_shapes

    fx = fixture()
    want = decoder_param_shapes(32)
    assert dict(fx["state_dict_shapes"]) == want and set(weights()) == set(want)
    assert want["decoder.conv_in.conv.weight"] == (128, 4, 3, 3, 3) and want["decoder.mid.block_1.norm1.weight"] == (128,)
    assert want["post_quant_conv.conv.weight"] == (4, 4, 1, 1, 1) and want["decoder.up.1.upsample.conv.conv.weight"] == (64, 64, 1, 3, 3)
    assert want["decoder.up.3.upsample.conv.conv.weight"] == (128, 128, 3, 3, 3) and "decoder.up.0.upsample.conv.conv.weight" not in want
    big = decoder_param_shapes(128)
    assert big["decoder.conv_out.conv.weight"] == (3, 128, 3, 3, 3) and big["decoder.mid.attn_1.q.conv.weight"] == (512, 512, 1, 1, 1)
    sd = weights()
    assert float((sd["decoder.norm_out.weight"] - 1).abs().max()) > 0.01 and float(sd["decoder.norm_out.bias"].abs().max()) > 0.01
    assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())


def test_unsupported_configurations_and_key_count_refusal():
    from videosys_amd import vae_open_sora_plan as V

    for kw in (dict(decoder_attention="AttnBlock3D"), dict(decoder_temporal_upsample=("", "", "TimeUpsample2x", "TimeUpsample2x")),
               dict(hidden_size_mult=(1, 2, 4)), dict(z_channels=8), dict(attn_resolutions=[16]), dict(bogus=1),
               dict(decoder_spatial_upsample=("", "SpatialUpsample2x", "SpatialUpsample2x", "SpatialUpsample2x"))):
        with pytest.raises(NotImplementedError):
            V._check_config(kw)
    V._check_config(dict(hidden_size=32, decoder_attention="AttnBlock3DFix", attn_resolutions=[], encoder_attention="whatever"))
    with pytest.raises(NotImplementedError):
        V._ChanMap(96)
    assert V.check_attention_keys(90, 90) == 8192 and V.check_attention_keys(3, 2) == 128
    with pytest.raises(ValueError, match="enable tiling"):
        V.check_attention_keys(96, 96)                  # 9216 keys per frame
    with pytest.raises(RuntimeError, match="HIP device"):
        V.CausalVAEDecoder(weights(), device="cpu")


def test_channel_map_keeps_group_statistics():
    """The 128-column layout of a 32- / 64-channel activation: a GroupNorm over 32 groups of 4 columns sees each group's channels
    repeated, so its statistics — and with the repeated affine its output — are those of the 32-group norm over the channels."""
    from videosys_amd.vae_open_sora_plan import _ChanMap

    for C in (32, 64, 128):
        cm = _ChanMap(C)
        g = torch.Generator().manual_seed(C)
        x = torch.randn(2, C, 5, generator=g, dtype=torch.float64)
        w, b = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
        want = torch.nn.functional.group_norm(x, 32, w, b, 1e-6)
        got = torch.nn.functional.group_norm(x[:, cm.src], 32, cm.out_rows(w), cm.out_rows(b), 1e-6)
        assert cm.P == max(C, 128) and float((got - want[:, cm.src]).abs().max()) < 1e-12
        wt = torch.randn(7, C, generator=g, dtype=torch.float64)          # a consumer reads each channel once
        assert float((cm.in_cols(wt) @ x[0, cm.src] - wt @ x[0]).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------- scheduler
def closed_form(n):
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float32)
    ac = torch.cumprod(1.0 - betas, dim=0).double().numpy()
    import numpy as np

    sig = ((1 - ac) / ac) ** 0.5
    t = np.linspace(0, 999, n, dtype=np.float32)[::-1]
    return t, np.concatenate([np.interp(t, np.arange(1000), sig), [0.0]])


@pytest.mark.parametrize("n", [1, 2, 50])
def test_scheduler_properties(n):
    from videosys_amd.pipeline_open_sora_plan import EulerAncestralDiscreteScheduler, retrieve_timesteps

    s = EulerAncestralDiscreteScheduler()
    ts, steps = retrieve_timesteps(s, n, "cpu", None)
    t, sig = closed_form(n)
    assert steps == n and s.order == 1 and ts.dtype == torch.float32 and tuple(ts.shape) == (n,) and tuple(s.sigmas.shape) == (n + 1,)
    assert ts.tolist() == [float(v) for v in t] and s.sigmas.dtype == torch.float32
    assert torch.allclose(s.sigmas.double(), torch.from_numpy(sig), rtol=1e-6, atol=0)
    sg = s.sigmas.double()
    assert bool((sg[:-1] > sg[1:]).all()) and float(sg[-1]) == 0.0 and s.init_noise_sigma == float(sg.max())
    for i in range(n):
        dt, up = s.step_coeffs(i)
        s_from, s_to = float(sg[i]), float(sg[i + 1])
        down = dt + s_from
        assert up ** 2 + down ** 2 == pytest.approx(s_to ** 2, rel=1e-12, abs=1e-300)
        assert up == pytest.approx(math.sqrt(s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2), rel=1e-14)
        assert s.in_scale(i) == pytest.approx(1 / math.sqrt(s_from ** 2 + 1), rel=1e-15)
    assert s.step_coeffs(n - 1)[1] == 0.0 and s.in_scale(n) == 1.0            # the last step is noise-free and lands on sigma = 0
    with pytest.raises(ValueError):                                            # no custom schedules (diffusers' class takes none)
        retrieve_timesteps(s, None, "cpu", [10, 5])


def test_scheduler_step_equals_the_closed_form():
    from videosys_amd.pipeline_open_sora_plan import EulerAncestralDiscreteScheduler

    s = EulerAncestralDiscreteScheduler()
    s.set_timesteps(5)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 3, 2, 2, dtype=torch.float64, generator=g) * s.init_noise_sigma
    x0 = x.clone()
    gen, gen2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    for i, t in enumerate(s.timesteps):
        scaled = s.scale_model_input(x, t)
        assert torch.allclose(scaled, x / math.sqrt(float(s.sigmas[i]) ** 2 + 1), rtol=1e-6)     # (sigma^2 + 1 in fp32, as diffusers)
        eps = torch.randn(x.shape, dtype=torch.float64, generator=g)
        (nxt,) = s.step(eps, t, x, generator=gen, return_dict=False)
        s_from, s_to = float(s.sigmas[i]), float(s.sigmas[i + 1])
        up = math.sqrt(s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2)
        down = math.sqrt(s_to ** 2 - up ** 2)
        noise = torch.randn(x.shape, dtype=torch.float64, generator=gen2)
        # diffusers' own form: x0-prediction, derivative, Euler step to sigma_down, then the fresh noise
        pred = x - s_from * eps
        want = x + (x - pred) / s_from * (down - s_from) + noise * up
        assert nxt.dtype == torch.float64 and float((nxt - want).abs().max()) <= 1e-9 * float(x0.abs().max())
        assert s.step_index == i + 1
        x = nxt
    assert "generator" in inspect.signature(s.step).parameters and "eta" not in inspect.signature(s.step).parameters


# ---------------------------------------------------------------------------------------------------- C ABI
NEW = ("vsys_upsample_trilinear2x", "vsys_cfg_ancestral_step", "vsys_pixels_to_u8_trunc")


def test_new_entry_points_in_header_library_and_ctypes_table():
    from videosys_amd import _lib, _opcodes

    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    gen = open(os.path.join(ROOT, "videosys_amd", "csrc", "gen", "program_gen.py")).read()
    no_op = re.search(r"\nNO_OP = \{(.*?)\}", gen, flags=re.S).group(1)
    assert_coded(NEW)                                 # in the launch-program table, with the prototype's arity
    lib = _lib.load()
    for n in NEW:
        assert re.search(rf"\nint {n}\(", hdr), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
        assert f'"{n}"' not in no_op, n
        proto = re.search(rf"\nint {n}\(([^;]*?)\);", hdr, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[n]), n
    assert len(_opcodes.OPCODES) == 74 and "#define VSYS_OP_COUNT 75" in hdr
    assert "autoencoder_kl_open_sora_plan_v120.py:349-357" in hdr and "pipeline_open_sora_plan.py:1186-1188" in hdr
    import __graft_entry__ as G

    assert "vae_osp.hip" in G.SOURCES
    src = open(os.path.join(ROOT, "videosys_amd", "csrc", "vae_osp.hip")).read()
    assert "asm" not in src.replace("namespace", "")  # plain HIP C++


def test_host_side_argument_checks_of_the_new_kernels():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # an aligned address that is never dereferenced: every call below is refused before any launch

    def grid(T=1, H=4, W=6, pad=1, tf=0, rows=None):
        return (ctypes.c_int64 * 6)(T, H, W, pad, tf, (T + tf) * (H + 2 * pad) * (W + 2 * pad) if rows is None else rows)

    def up(gs=None, gd=None, N=1, C=128, x=P, y=P):
        return lib.vsys_upsample_trilinear2x(x, grid(3, 2, 2) if gs is None else gs, y, grid(5, 4, 4, 1, 2) if gd is None else gd, N, C, None)

    assert up(x=None) == VSYS_ERR_ARG and up(y=None) == VSYS_ERR_ARG
    assert lib.vsys_upsample_trilinear2x(P, None, P, grid(), 1, 128, None) == VSYS_ERR_ARG
    assert up(gd=grid(6, 4, 4, 1, 2)) == VSYS_ERR_SHAPE                 # 3 frames -> 5, not 6
    assert up(gs=grid(1, 2, 2), gd=grid(2, 4, 4, 1, 2)) == VSYS_ERR_SHAPE   # one frame stays one frame
    assert up(gd=grid(5, 4, 5, 1, 2)) == VSYS_ERR_SHAPE and up(gd=grid(5, 3, 4, 1, 2)) == VSYS_ERR_SHAPE
    assert up(C=12) == VSYS_ERR_SHAPE and up(C=0) == VSYS_ERR_SHAPE and up(C=4096) == VSYS_ERR_SHAPE
    assert up(gd=grid(5, 4, 4, 1, 2, rows=10)) == VSYS_ERR_SHAPE        # a sample stride smaller than the sample
    assert up(gs=grid(3, 2, 2, pad=2)) == VSYS_ERR_SHAPE and up(N=-1) == VSYS_ERR_SHAPE
    assert up(x=P + 8) == VSYS_ERR_ALIGN and up(y=P + 2) == VSYS_ERR_ALIGN
    assert up(N=0) == 0

    def step(z=P, mo=P, noise=P, mi=P, Bz=1, Cin=4, Cout=8, thw=7, su=0.5):
        return lib.vsys_cfg_ancestral_step(z, mo, noise, mi, Bz, Cin, Cout, thw, 7.5, -0.5, su, 0.4, None)

    assert step(z=None) == VSYS_ERR_ARG and step(mo=None) == VSYS_ERR_ARG and step(mi=None) == VSYS_ERR_ARG
    assert step(noise=None) == VSYS_ERR_ARG                              # sigma_up != 0 needs its noise
    assert step(Cout=4) == VSYS_ERR_SHAPE and step(Cin=0, Cout=0) == VSYS_ERR_SHAPE and step(Bz=-1) == VSYS_ERR_SHAPE
    assert step(thw=-1) == VSYS_ERR_SHAPE and step(Bz=1 << 31) == VSYS_ERR_SHAPE
    assert step(thw=0) == 0 and step(Bz=0) == 0 and step(noise=None, su=0.0, thw=0) == 0

    def u8(g=None, N=2, ldx=128, x=P, out=P, Ftot=3, f0=1):
        return lib.vsys_pixels_to_u8_trunc(x, grid() if g is None else g, N, ldx, out, Ftot, f0, None)

    assert u8(x=None) == VSYS_ERR_ARG and u8(out=None) == VSYS_ERR_ARG
    assert lib.vsys_pixels_to_u8_trunc(P, None, 2, 128, P, 3, 1, None) == VSYS_ERR_ARG
    assert u8(f0=2) == VSYS_ERR_SHAPE and u8(f0=-1) == VSYS_ERR_SHAPE and u8(Ftot=0) == VSYS_ERR_SHAPE and u8(N=-1) == VSYS_ERR_SHAPE
    assert u8(ldx=2) == VSYS_ERR_SHAPE and u8(g=grid(pad=2)) == VSYS_ERR_SHAPE and u8(g=grid(H=0)) == VSYS_ERR_SHAPE
    assert u8(g=grid(rows=10)) == VSYS_ERR_SHAPE
    assert u8(ldx=130) == VSYS_ERR_ALIGN and u8(x=P + 4) == VSYS_ERR_ALIGN
    assert u8(N=0) == 0


# ---------------------------------------------------------------------------------------------------- surface
_SOURCE_DEFAULTS = {"torch.device('cuda')": lambda v: v == torch.device("cuda"),
                    "torch.float16": lambda v: v is torch.bfloat16}      # the family runs in bf16 like the rest of this build


def _assert_signature(fn, want, what):
    ps = [p for p in list(inspect.signature(fn).parameters.values())[1:] if p.kind is not inspect.Parameter.VAR_KEYWORD]
    assert [p.name for p in ps] == [w["name"] for w in want], what
    for p, w in zip(ps, want):
        assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, (what, p.name)
        if w.get("required"):
            assert p.default is inspect.Parameter.empty, (what, p.name)
        elif "default" in w:
            assert p.default == w["default"] and type(p.default) is type(w["default"]), (what, p.name, p.default, w["default"])
        else:
            assert _SOURCE_DEFAULTS[w["default_source"]](p.default), (what, p.name, p.default, w["default_source"])


def test_surface_matches_the_reference_fixture():
    from videosys_amd.pab import PABConfig
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanConfig, OpenSoraPlanPipeline, OpenSoraPlanV120PABConfig

    with open(os.path.join(GOLDEN, "osp_pipeline_surface.json")) as fh:
        fx = json.load(fh)
    _assert_signature(OpenSoraPlanV120PABConfig.__init__, fx["OpenSoraPlanV120PABConfig.__init__"], "OpenSoraPlanV120PABConfig")
    _assert_signature(OpenSoraPlanConfig.__init__, fx["OpenSoraPlanConfig.__init__"], "OpenSoraPlanConfig")
    _assert_signature(OpenSoraPlanPipeline.__init__, fx["OpenSoraPlanPipeline.__init__"], "OpenSoraPlanPipeline")
    _assert_signature(OpenSoraPlanPipeline.generate, fx["OpenSoraPlanPipeline.generate"], "generate")
    _assert_signature(OpenSoraPlanPipeline.encode_prompt_v120, fx["OpenSoraPlanPipeline.encode_prompt_v120"], "encode_prompt_v120")
    _assert_signature(OpenSoraPlanPipeline.prepare_latents, fx["OpenSoraPlanPipeline.prepare_latents"], "prepare_latents")
    for name in fx["OpenSoraPlanPipeline.methods"]:
        assert callable(getattr(OpenSoraPlanPipeline, name)), name
    c = OpenSoraPlanConfig()
    assert (c.version, c.transformer_type, c.num_frames, c.num_gpus, c.cpu_offload, c.enable_tiling, c.tile_overlap_factor,
            c.enable_pab, c.pab_config) == ("v120", "29x480p", 29, 1, False, True, 0.25, False, None)
    assert (c.transformer, c.text_encoder, c.pipeline_cls) == ("LanguageBind/Open-Sora-Plan-v1.2.0", "google/mt5-xxl", OpenSoraPlanPipeline)
    for tt, nf in (("93x480p", 93), ("93x720p", 93), ("29x480p", 29), ("29x720p", 29)):
        assert OpenSoraPlanConfig(transformer_type=tt).num_frames == nf
    p = OpenSoraPlanConfig(enable_pab=True).pab_config
    assert isinstance(p, OpenSoraPlanV120PABConfig) and isinstance(p, PABConfig)
    assert (p.spatial_broadcast, p.spatial_threshold, p.spatial_range) == (True, [100, 850], 2)
    assert (p.cross_broadcast, p.cross_threshold, p.cross_range) == (True, [100, 850], 6) and not p.temporal_broadcast
    with pytest.raises(NotImplementedError, match="v1.1"):
        OpenSoraPlanConfig(version="v110", transformer_type="65x512x512")
    with pytest.raises(AssertionError):
        OpenSoraPlanConfig(version="v130")
    with pytest.raises(AssertionError):
        OpenSoraPlanConfig(transformer_type="65x512x512")
    with pytest.raises(TypeError):
        OpenSoraPlanConfig(bogus=1)
    with pytest.raises(NotImplementedError, match="num_gpus"):
        OpenSoraPlanPipeline(OpenSoraPlanConfig(num_gpus=2))


def test_latent_shape_and_input_checks():
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanPipeline

    p = OpenSoraPlanPipeline.__new__(OpenSoraPlanPipeline)
    p.vae_scale_factor = [4, 8, 8]
    assert p.latent_shape(1, 4, 29, 480, 640) == (1, 4, 8, 60, 80) and p.latent_shape(2, 4, 93, 720, 1280) == (2, 4, 24, 90, 160)
    assert p.latent_shape(1, 4, 9, 64, 96) == (1, 4, 3, 8, 12) and p.latent_shape(1, 4, 8, 64, 96)[2] == 2
    with pytest.raises(ValueError, match="divisible by 8"):
        p.check_inputs("a", 60, 64, "", 1)
    with pytest.raises(ValueError, match="callback_steps"):
        p.check_inputs("a", 64, 64, "", 0)
    with pytest.raises(ValueError, match="Provide either"):
        p.check_inputs(None, 64, 64, None, 1)
    with pytest.raises(ValueError, match="Cannot forward both"):
        p.check_inputs("a", 64, 64, None, 1, prompt_embeds=torch.zeros(1, 2, 3))
    e, m = torch.zeros(1, 4, 8), torch.ones(1, 4)
    with pytest.raises(ValueError, match="same shape"):
        p.check_inputs(None, 64, 64, None, 1, e, torch.zeros(1, 5, 8), m, torch.ones(1, 5))
    p.check_inputs(None, 64, 64, None, 1, e, e, m, m)
    with pytest.raises(NotImplementedError, match="v1.1"):
        p.encode_prompt("a")


def test_aliases_resolve_and_the_top_level_names_still_raise():
    code = ("import videosys, videosys_amd\n"
            "from videosys.pipelines.open_sora_plan import OpenSoraPlanConfig, OpenSoraPlanPipeline, OpenSoraPlanV120PABConfig\n"
            "from videosys.pipelines.open_sora_plan.pipeline_open_sora_plan import EulerAncestralDiscreteScheduler, retrieve_timesteps\n"
            "from videosys.models.autoencoders.autoencoder_kl_open_sora_plan_v120 import CausalVAEModelWrapper, CausalVAEModel, CausalVAEDecoder\n"
            "import videosys_amd.pipeline_open_sora_plan as m\n"
            "assert OpenSoraPlanConfig is m.OpenSoraPlanConfig and CausalVAEModel is CausalVAEDecoder\n"
            "for n in ('OpenSoraPlanConfig', 'OpenSoraPlanPipeline', 'OpenSoraPlanV120PABConfig'):\n"
            "    try:\n        getattr(videosys, n)\n        raise SystemExit(3)\n    except ImportError as e:\n        assert 'outside' in str(e)\n"
            "assert OpenSoraPlanConfig().pipeline_cls is OpenSoraPlanPipeline\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-800:]
