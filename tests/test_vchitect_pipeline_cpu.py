"""No GPU: the host side of the Vchitect-2.0 pipeline (videosys_amd/pipeline_vchitect.py) and the C ABI of its two decode kernels.

  * FlowMatchEulerDiscreteScheduler against its closed form, computed here independently in numpy float64 (the class is an UNPINNED
    restatement of diffusers': no fixture of the third-party class exists offline);
  * the per-step guidance schedule against the formula of pipeline_vchitect.py:942-944;
  * constructor / generate() parameter names and defaults against tests/golden/vchitect_pipeline_surface.json (minted from the
    reference's source by tools/mint_vchitect_surface.py);
  * every check_inputs error branch, the three batch ValueErrors and the "CLIP encoders are not built" error;
  * the videosys aliases, and the top-level name that keeps raising;
  * vsys_vae_first_im2col_nc / vsys_pixels_to_u8: in the header, the library and the ctypes table, outside the op table, and their
    error codes for bad arguments (a refused call launches nothing, so no device is needed)."""
import ctypes
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from op_table import assert_coded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3


# ---------------------------------------------------------------------------------------------------- scheduler
def closed_form(n, shift, N=1000):
    """(timesteps, sigmas) in float64: the arithmetic of the class docstring with fp32 only where diffusers holds fp32 arrays."""
    sh = lambda s: shift * s / (1 + (shift - 1) * s)
    s0 = sh(np.linspace(1, N, N, dtype=np.float32)[::-1] / np.float32(N)).astype(np.float32)
    smax, smin = float(s0[0]), float(s0[-1])
    s = sh(np.linspace(smax * N, smin * N, n) / N)
    return s * N, np.concatenate([s, [0.0]])


@pytest.mark.parametrize("shift", [1.0, 3.0])
@pytest.mark.parametrize("n", [1, 4, 100])
def test_scheduler_matches_the_closed_form(n, shift):
    from videosys_amd.pipeline_vchitect import FlowMatchEulerDiscreteScheduler, retrieve_timesteps

    sch = FlowMatchEulerDiscreteScheduler(num_train_timesteps=1000, shift=shift)
    assert sch.order == 1
    ts, steps = retrieve_timesteps(sch, n, "cpu", None)
    assert steps == n and ts is sch.timesteps
    want_t, want_s = closed_form(n, shift)
    assert sch.timesteps.dtype == torch.float32 and sch.sigmas.dtype == torch.float32
    assert sch.timesteps.shape == (n,) and sch.sigmas.shape == (n + 1,)
    # fp32 storage of float64 values: half an ulp of the largest magnitude (1000 for timesteps, 1 for sigmas), and one more for s * N
    assert np.abs(sch.sigmas.double().numpy() - want_s).max() <= 2.0 ** -24
    assert np.abs(sch.timesteps.double().numpy() - want_t).max() <= 2 * 1000 * 2.0 ** -24
    assert float(sch.sigmas[-1]) == 0.0
    assert bool((sch.sigmas[1:] < sch.sigmas[:-1]).all()), "sigmas must strictly decrease"
    assert torch.equal(sch.timesteps, sch.sigmas[:-1] * 1000)
    if shift == 1.0:
        assert float(sch.timesteps[0]) == 1000.0 and (n == 1 or abs(float(sch.timesteps[-1]) - 1.0) < 1e-3)
    # step: prev = float32(sample) + (sigma_next - sigma) * model_output, the index advances by one
    x = torch.arange(6, dtype=torch.float32).reshape(2, 3).to(torch.bfloat16)
    v = torch.full((2, 3), 0.5)
    assert sch.step_index is None
    for i in range(n):
        out = sch.step(v, sch.timesteps[i], x, return_dict=False)[0]
        assert sch.step_index == i + 1
        assert out.dtype == torch.float32 and torch.equal(out, x.float() + (sch.sigmas[i + 1] - sch.sigmas[i]) * v)
        assert sch.step_dt(i) == float(sch.sigmas[i + 1] - sch.sigmas[i]) < 0


def test_scheduler_refuses_custom_timesteps_and_reads_its_config(tmp_path):
    from videosys_amd.pipeline_vchitect import FlowMatchEulerDiscreteScheduler, retrieve_timesteps
    from videosys_amd.utils import ctor_kwargs, read_component

    sch = FlowMatchEulerDiscreteScheduler()
    with pytest.raises(ValueError, match="does not support custom"):
        retrieve_timesteps(sch, None, "cpu", [900, 500, 100])
    with pytest.raises(ValueError, match="does not support custom"):
        retrieve_timesteps(sch, None, "cpu", None, sigmas=[0.9, 0.5])
    with pytest.raises(ValueError, match="Only one of"):
        retrieve_timesteps(sch, None, "cpu", [1], sigmas=[0.5])
    assert "unpinned" in FlowMatchEulerDiscreteScheduler.__doc__.lower()
    os.makedirs(tmp_path / "scheduler")
    with open(tmp_path / "scheduler" / "scheduler_config.json", "w") as fh:
        json.dump({"_class_name": "FlowMatchEulerDiscreteScheduler", "num_train_timesteps": 500, "shift": 3.0}, fh)
    kw = ctor_kwargs(FlowMatchEulerDiscreteScheduler.__init__, read_component(str(tmp_path), "scheduler")[0])
    assert kw == {"num_train_timesteps": 500, "shift": 3.0}
    s2 = FlowMatchEulerDiscreteScheduler(**kw)
    assert (s2.num_train_timesteps, s2.shift) == (500, 3.0) and s2.sigma_max == 1.0


def test_guidance_schedule():
    from videosys_amd.pipeline_vchitect import FlowMatchEulerDiscreteScheduler, guidance_at

    N, g = 100, 7.5
    sch = FlowMatchEulerDiscreteScheduler()
    sch.set_timesteps(N)
    for i in (0, N // 2, N - 1):
        t = sch.timesteps[i].item()
        want = 1 + g * (1 - math.cos(math.pi * ((N - t) / N) ** 5.0)) / 2
        assert guidance_at(g, N, t) == pytest.approx(want, rel=1e-15, abs=0)
        assert isinstance(guidance_at(g, N, t), float) and 1 <= guidance_at(g, N, t) <= 1 + g
    # the base is negative while t > N: the 5th power keeps it real, and the last step (t = 1) sees cos(pi * 0.99 ** 5)
    assert guidance_at(g, N, 1000.0) == pytest.approx(1 + g * (1 - math.cos(math.pi * (-9.0) ** 5.0)) / 2, rel=1e-15)
    assert guidance_at(g, N, 1.0) == pytest.approx(1 + g * (1 - math.cos(math.pi * 0.99 ** 5)) / 2, rel=1e-15)


# ---------------------------------------------------------------------------------------------------- surface
_SOURCE_DEFAULTS = {"torch.device('cuda')": lambda v: v == torch.device("cuda"), "torch.bfloat16": lambda v: v is torch.bfloat16,
                    "VchitectPABConfig()": lambda v: type(v).__name__ == "VchitectPABConfig"}


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
    from videosys_amd import VchitectConfig, VchitectPABConfig, VchitectXLPipeline
    from videosys_amd.pab import PABConfig

    with open(os.path.join(ROOT, "tests", "golden", "vchitect_pipeline_surface.json")) as fh:
        fx = json.load(fh)
    _assert_signature(VchitectPABConfig.__init__, fx["VchitectPABConfig.__init__"], "VchitectPABConfig")
    _assert_signature(VchitectConfig.__init__, fx["VchitectConfig.__init__"], "VchitectConfig")
    _assert_signature(VchitectXLPipeline.__init__, fx["VchitectXLPipeline.__init__"], "VchitectXLPipeline")
    _assert_signature(VchitectXLPipeline.generate, fx["VchitectXLPipeline.generate"], "generate")
    c = VchitectConfig()
    assert (c.model_path, c.num_gpus, c.cpu_offload, c.enable_pab) == ("Vchitect/Vchitect-2.0-2B", 1, False, False)
    assert c.pipeline_cls is VchitectXLPipeline and isinstance(c.pab_config, VchitectPABConfig) and isinstance(c.pab_config, PABConfig)
    p = c.pab_config
    assert (p.spatial_broadcast, p.spatial_threshold, p.spatial_range) == (True, [100, 800], 2)
    assert (p.temporal_broadcast, p.temporal_threshold, p.temporal_range) == (True, [100, 800], 4)
    assert (p.cross_broadcast, p.cross_threshold, p.cross_range) == (True, [100, 800], 6)
    with pytest.raises(TypeError):
        VchitectConfig(bogus=1)
    # the literal methods and properties of the reference class
    for name in ("check_inputs", "prepare_latents", "encode_prompt", "_get_clip_prompt_embeds", "_get_t5_prompt_embeds", "save_video",
                 "_set_parallel", "_set_seed", "generate"):
        assert callable(getattr(VchitectXLPipeline, name)), name
    for name in ("guidance_scale", "clip_skip", "do_classifier_free_guidance", "joint_attention_kwargs", "num_timesteps", "interrupt"):
        assert isinstance(getattr(VchitectXLPipeline, name), property), name
    assert list(inspect.signature(VchitectXLPipeline.prepare_latents).parameters)[1:] == [
        "batch_size", "num_channels_latents", "height", "width", "frames", "dtype", "device", "generator", "latents"]
    assert VchitectXLPipeline._callback_tensor_inputs == ["latents", "prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds"]


# ---------------------------------------------------------------------------------------------------- input checks
def bare_pipeline():
    """A pipeline object without its constructor (which needs a device): what check_inputs and the early errors of generate() read."""
    from videosys_amd import VchitectXLPipeline

    p = VchitectXLPipeline.__new__(VchitectXLPipeline)
    p.text_encoder = p.text_encoder_2 = p.text_encoder_3 = p.tokenizer = p.tokenizer_2 = None
    return p


def test_check_inputs_raises_on_every_branch():
    p = bare_pipeline()
    e, pe = torch.zeros(1, 4, 8), torch.zeros(1, 8)
    ok = dict(prompt="a", prompt_2=None, prompt_3=None, height=64, width=64)
    p.check_inputs(**ok)
    p.check_inputs(None, None, None, 64, 64, prompt_embeds=e, pooled_prompt_embeds=pe, negative_prompt_embeds=e,
                   negative_pooled_prompt_embeds=pe, callback_on_step_end_tensor_inputs=["latents"])
    bad = [
        (dict(ok, height=65), "divisible by 8"),
        (dict(ok, width=12), "divisible by 8"),
        (dict(ok, callback_on_step_end_tensor_inputs=["latents", "nope"]), "callback_on_step_end_tensor_inputs"),
        (dict(ok, prompt_embeds=e, pooled_prompt_embeds=pe), "both `prompt`"),
        (dict(ok, prompt=None, prompt_2="b", prompt_embeds=e, pooled_prompt_embeds=pe), "both `prompt_2`"),
        (dict(ok, prompt=None, prompt_3="c", prompt_embeds=e, pooled_prompt_embeds=pe), "both `prompt_3`"),
        (dict(ok, prompt=None), "Provide either"),
        (dict(ok, prompt=3), "`prompt` has to be of type"),
        (dict(ok, prompt_2=3), "`prompt_2` has to be of type"),
        (dict(ok, prompt_3=3), "`prompt_3` has to be of type"),
        (dict(ok, negative_prompt="n", negative_prompt_embeds=e, negative_pooled_prompt_embeds=pe), "both `negative_prompt`"),
        (dict(ok, negative_prompt_2="n", negative_prompt_embeds=e, negative_pooled_prompt_embeds=pe), "both `negative_prompt_2`"),
        (dict(ok, negative_prompt_3="n", negative_prompt_embeds=e, negative_pooled_prompt_embeds=pe), "both `negative_prompt_3`"),
        (dict(ok, prompt=None, prompt_embeds=e, pooled_prompt_embeds=pe, negative_prompt_embeds=torch.zeros(1, 5, 8),
              negative_pooled_prompt_embeds=pe), "must have the same shape"),
        (dict(ok, prompt=None, prompt_embeds=e), "`pooled_prompt_embeds` also have to be passed"),
        (dict(ok, negative_prompt_embeds=e), "`negative_pooled_prompt_embeds` also have to be passed"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            p.check_inputs(**kw)


def test_generate_refuses_what_the_reference_loop_cannot_run():
    p = bare_pipeline()
    e, pe = torch.zeros(1, 4, 8), torch.zeros(1, 8)
    emb = dict(prompt_embeds=e, pooled_prompt_embeds=pe, negative_prompt_embeds=e, negative_pooled_prompt_embeds=pe)
    with pytest.raises(ValueError, match="one prompt per call"):
        p.generate(prompt=["a", "b"], height=64, width=64, seed=0)
    with pytest.raises(ValueError, match="num_images_per_prompt"):
        p.generate(height=64, width=64, seed=0, num_images_per_prompt=2, **emb)
    for g in (1.0, 0.5):
        with pytest.raises(ValueError, match="guidance_scale"):
            p.generate(height=64, width=64, seed=0, guidance_scale=g, **emb)
    for kw in (dict(prompt="a sunset"), dict(prompt_embeds=e, pooled_prompt_embeds=pe)):
        with pytest.raises(RuntimeError, match="CLIP encoders .* are not built") as ei:
            p.generate(height=64, width=64, seed=0, **kw)
        assert "text_encoder_2=" in str(ei.value) and "pooled_prompt_embeds" in str(ei.value) and "negative_pooled_prompt_embeds" in str(ei.value)
    with pytest.raises(ValueError, match="does not support custom"):
        from videosys_amd.pipeline_vchitect import FlowMatchEulerDiscreteScheduler

        p.scheduler, p._device = FlowMatchEulerDiscreteScheduler(), "cpu"
        p.encode_prompt = lambda **kw: (e, e, pe, pe)
        p._enter_stage = lambda name: None
        p.generate(height=64, width=64, seed=0, timesteps=[900, 100], **emb)


def test_clip_objects_are_called_as_the_reference_calls_them():
    """_get_clip_prompt_embeds on injected stand-ins: element 0 is the pooled embedding, hidden_states[-2] / [-(clip_skip + 2)] the
    prompt embedding; encode_prompt pads [CLIP-L | CLIP-bigG] to the T5 width and puts the T5 states (zeros without an encoder) behind."""
    from types import SimpleNamespace

    p = bare_pipeline()
    p._device, p._dtype, p.tokenizer_max_length, p.max_sequence_length_t5 = torch.device("cpu"), torch.bfloat16, 7, 5
    p.transformer = SimpleNamespace(config=SimpleNamespace(joint_attention_dim=16))
    calls = []

    class Tok:
        def __call__(self, prompt, padding=None, max_length=None, truncation=None, return_tensors=None):
            n = max_length or 3
            return SimpleNamespace(input_ids=torch.arange(len(prompt) * n).reshape(len(prompt), n))

    class Clip:
        def __init__(self, d):
            self.d = d

        def __call__(self, ids, output_hidden_states=False):
            calls.append((self.d, tuple(ids.shape), output_hidden_states))
            hs = [torch.full((ids.shape[0], ids.shape[1], self.d), float(k)) for k in range(4)]
            out = SimpleNamespace(hidden_states=hs)
            return type("Out", (), {"hidden_states": hs, "__getitem__": lambda s, i: torch.full((ids.shape[0], 2 * self.d), 9.0)})()

    p.tokenizer, p.tokenizer_2, p.text_encoder, p.text_encoder_2 = Tok(), Tok(), Clip(4), Clip(6)
    e, pooled = p._get_clip_prompt_embeds("x", clip_model_index=1)
    assert e.shape == (1, 7, 6) and float(e[0, 0, 0]) == 2.0 and pooled.shape == (1, 12) and calls[-1] == (6, (1, 7), True)
    e, _ = p._get_clip_prompt_embeds("x", clip_skip=1, clip_model_index=0)
    assert e.shape == (1, 7, 4) and float(e[0, 0, 0]) == 1.0
    pe, ne, pp, npp = p.encode_prompt("x", None, None, negative_prompt=None)
    assert pe.shape == ne.shape == (1, 7 + 5, 16) and pp.shape == npp.shape == (1, 8 + 12)
    assert float(pe[0, 0, 3]) == 2.0 and float(pe[0, 0, 9]) == 2.0 and float(pe[0, 0, 10]) == 0.0 and float(pe[0, 7:].abs().max()) == 0.0


def test_aliases_import_and_the_top_level_name_still_raises():
    import subprocess
    import sys

    code = ("import videosys, videosys_amd\n"
            "from videosys.pipelines.vchitect import VchitectConfig, VchitectPABConfig, VchitectXLPipeline\n"
            "from videosys.pipelines.vchitect.pipeline_vchitect import VchitectXLPipeline as P2, FlowMatchEulerDiscreteScheduler, retrieve_timesteps\n"
            "assert VchitectConfig is videosys_amd.VchitectConfig and P2 is VchitectXLPipeline is videosys_amd.VchitectXLPipeline\n"
            "assert VchitectPABConfig is videosys_amd.VchitectPABConfig and VchitectConfig().pipeline_cls is VchitectXLPipeline\n"
            "assert set(('VchitectXLPipeline', 'VchitectConfig', 'VchitectPABConfig')) <= set(videosys_amd.__all__)\n"
            "try:\n    from videosys import VchitectConfig\n    raise SystemExit(3)\nexcept ImportError as e:\n    assert 'outside' in str(e)\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-800:]


# ---------------------------------------------------------------------------------------------------- C ABI
NEW = ("vsys_vae_first_im2col_nc", "vsys_pixels_to_u8")


def test_new_entry_points_in_header_library_and_ctypes_table():
    from videosys_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    lib = _lib.load()
    assert_coded(NEW)                                 # in the launch-program table, with the prototype's arity
    for n in NEW:
        assert re.search(rf"\nint {n}\(", hdr), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
        proto = re.search(rf"\nint {n}\(([^;]*?)\);", hdr, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[n]), n
    import __graft_entry__ as G

    assert "vae_sd3.hip" in G.SOURCES
    src = open(os.path.join(ROOT, "videosys_amd", "csrc", "vae_sd3.hip")).read()
    assert "asm" not in src.replace("namespace", "")  # plain HIP C++: no inline assembly in the new kernels


def test_host_side_argument_checks_of_the_decode_kernels():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # an aligned address that is never dereferenced: every call below is refused before any launch

    def first(F=2, Cz=16, H=3, W=5, kcols=160, z=P, out=P, sf=1.5305):
        return lib.vsys_vae_first_im2col_nc(z, F, Cz, H, W, kcols, sf, 0.0609, out, None)

    assert first(z=None) == VSYS_ERR_ARG and first(out=None) == VSYS_ERR_ARG
    assert first(Cz=0) == VSYS_ERR_SHAPE and first(Cz=33, kcols=320) == VSYS_ERR_SHAPE
    assert first(kcols=144) == VSYS_ERR_SHAPE          # not a multiple of 32
    assert first(kcols=128) == VSYS_ERR_SHAPE          # below 9 * Cz
    assert first(Cz=5, kcols=32) == VSYS_ERR_SHAPE
    assert first(H=0) == VSYS_ERR_SHAPE and first(W=-1) == VSYS_ERR_SHAPE and first(F=-1) == VSYS_ERR_SHAPE
    assert first(F=1 << 31) == VSYS_ERR_SHAPE
    assert first(sf=0.0) == VSYS_ERR_ARG
    assert first(out=P + 8) == VSYS_ERR_ALIGN
    assert first(F=0) == 0                             # nothing to do, nothing launched

    grid = lambda T=1, H=4, W=6, pad=1, tf=0, rows=None: (ctypes.c_int64 * 6)(T, H, W, pad, tf, (T + tf) * (H + 2 * pad) * (W + 2 * pad) if rows is None else rows)

    def u8(g=None, N=2, ldx=128, x=P, out=P, Ftot=3, f0=1):
        return lib.vsys_pixels_to_u8(x, grid() if g is None else g, N, ldx, out, Ftot, f0, None)

    assert u8(x=None) == VSYS_ERR_ARG and u8(out=None) == VSYS_ERR_ARG
    assert lib.vsys_pixels_to_u8(P, None, 2, 128, P, 3, 1, None) == VSYS_ERR_ARG
    assert u8(f0=2) == VSYS_ERR_SHAPE                  # frames f0 .. f0 + N - 1 must fit Ftot
    assert u8(f0=-1) == VSYS_ERR_SHAPE and u8(Ftot=0) == VSYS_ERR_SHAPE and u8(N=-1) == VSYS_ERR_SHAPE
    assert u8(ldx=2) == VSYS_ERR_SHAPE
    assert u8(g=grid(pad=2)) == VSYS_ERR_SHAPE and u8(g=grid(H=0)) == VSYS_ERR_SHAPE
    assert u8(g=grid(rows=10)) == VSYS_ERR_SHAPE       # a sample stride smaller than the sample
    assert u8(ldx=130) == VSYS_ERR_ALIGN
    assert u8(x=P + 4) == VSYS_ERR_ALIGN
    assert u8(N=0) == 0


def test_sd3_decoder_rejects_quant_convs_and_names_its_parameters():
    from videosys_amd import vae_sd3

    shapes = vae_sd3.decoder_param_shapes()
    assert shapes["decoder.conv_in.weight"] == (512, 16, 3, 3) and shapes["decoder.conv_out.weight"] == (3, 128, 3, 3)
    assert not any("quant" in k for k in shapes) and all(k.startswith("decoder.") for k in shapes)
    assert shapes["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert "decoder.up_blocks.3.upsamplers.0.conv.weight" not in shapes and "decoder.up_blocks.2.upsamplers.0.conv.weight" in shapes
    sd = vae_sd3.synth_state_dict(3)
    assert sorted(sd) == sorted(shapes) and all(tuple(sd[k].shape) == shapes[k] for k in sd)
    assert torch.equal(sd["decoder.conv_in.weight"], vae_sd3.synth_state_dict(3)["decoder.conv_in.weight"])
    bad = dict(sd)
    bad["post_quant_conv.weight"], bad["post_quant_conv.bias"] = torch.zeros(16, 16, 1, 1), torch.zeros(16)
    with pytest.raises(ValueError, match="no quant convs"):
        vae_sd3.AutoencoderKLSD3Decoder(bad, device="cuda")
    with pytest.raises(RuntimeError, match="HIP device"):
        vae_sd3.AutoencoderKLSD3Decoder(sd, device="cpu")
