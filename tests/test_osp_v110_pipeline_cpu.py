"""CPU tests of the Open-Sora-Plan v1.1 pipeline pieces (no GPU):

  * PNDMScheduler (an UNPINNED restatement of diffusers' class) against the algorithm in its docstring: the timestep lists, the refusal
    of fewer than four steps, and the analytic path — a model that returns the TRUE epsilon of a fixed x0 is carried by the transfer
    formula exactly, so the float64 loop must end at sqrt(acp[0]) x0 + sqrt(1 - acp[0]) eps to 1e-12 for every n, which pins the
    formula, the Runge-Kutta bookkeeping and the multistep weights without the library; ``step_coeffs`` (the linear form the step
    kernel evaluates) against ``step`` on random tensors;
  * the two entry points the pipeline adds to csrc/vae_osp.hip: in the header, the library and the ctypes table, outside the op table,
    and their host-side argument refusals on a never-dereferenced pointer;
  * config defaults, the PAB defaults and the signatures against tests/golden/osp_v110_pipeline_surface.json
    (tools/mint_osp_v110_surface.py), the refusals that stay, the text masking rule of ``encode_prompt`` on an injected encoder;
  * the ``videosys`` aliases resolve in a fresh interpreter."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from op_table import assert_coded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3


# ---------------------------------------------------------------------------------------------------- PNDM
def test_pndm_timesteps():
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    s = PNDMScheduler()
    assert (s.order, s.init_noise_sigma) == (1, 1.0)
    x = torch.randn(3)
    assert s.scale_model_input(x, 5) is x
    for n in (4, 10, 50, 150):
        s.set_timesteps(n)
        assert len(s.timesteps) == n + 9 and len(s.prk_timesteps) == 12 and len(s.plms_timesteps) == n - 3
    s.set_timesteps(50)
    assert s.timesteps.tolist() == [980, 970, 970, 960, 960, 950, 950, 940, 940, 930, 930, 920] + list(range(920, -1, -20))
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [750, 625, 625, 500, 500, 375, 375, 250, 250, 125, 125, 0, 0]
    with pytest.raises(ValueError, match="at least 4"):
        s.set_timesteps(3)
    assert float(s.alphas_cumprod[0]) == float(torch.tensor(1.0 - 1e-4, dtype=torch.float32)) and s.alphas_cumprod.dtype == torch.float32
    for kw in (dict(skip_prk_steps=True), dict(set_alpha_to_one=True), dict(prediction_type="v_prediction"), dict(beta_schedule="scaled_linear"),
               dict(timestep_spacing="trailing"), dict(steps_offset=1)):
        with pytest.raises(NotImplementedError):
            PNDMScheduler(**kw)


@pytest.mark.parametrize("n", [4, 10, 50, 100, 150])
def test_pndm_carries_an_exact_epsilon_to_the_closed_form(n):
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    s = PNDMScheduler()
    s.set_timesteps(n)
    acp = s.alphas_cumprod.double()
    g = torch.Generator().manual_seed(n)
    x0, eps = torch.randn(256, generator=g, dtype=torch.float64), torch.randn(256, generator=g, dtype=torch.float64)
    t0 = int(s.timesteps[0])
    z = acp[t0].sqrt() * x0 + (1 - acp[t0]).sqrt() * eps
    for t in s.timesteps.tolist():
        z = s.step((z - acp[t].sqrt() * x0) / (1 - acp[t]).sqrt(), t, z, return_dict=False)[0]
    assert s.counter == n + 9 and z.dtype == torch.float64
    err = float((z - (acp[0].sqrt() * x0 + (1 - acp[0]).sqrt() * eps)).abs().max())
    print(f"n={n}: |end - closed form| = {err:.3e}")
    assert err <= 1e-12


def pndm_linear_form(k, e, base, srcs):
    """(z_out, aux_out or None) of one call from its coefficients, in the dtype of the operands: vsys_cfg_pndm_step's contract."""
    S = [e] + list(srcs)
    z = k["c_base"] * base + sum(k["cz"][j] * S[j] for j in range(len(S)) if k["cz"][j] != 0.0)
    assert all(c == 0.0 for c in k["cz"][len(S):]) and all(c == 0.0 for c in k["ca"][len(S):]), "a weight on a source that is not there"
    aux = sum(k["ca"][j] * S[j] for j in range(len(S)) if k["ca"][j] != 0.0) if any(k["ca"]) else None
    return z, aux


@pytest.mark.parametrize("n", [4, 7, 50])
def test_step_coeffs_reproduce_step(n):
    """The host bookkeeping the pipeline does around the kernel (ping-pong sample, accumulator, history) on float64 tensors."""
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    s = PNDMScheduler()
    s.set_timesteps(n)
    g = torch.Generator().manual_seed(n)
    z = torch.randn(64, generator=g, dtype=torch.float64)
    mine, cur, acc, hist = z.clone(), None, None, []
    kinds = []
    for i, t in enumerate(s.timesteps.tolist()):
        e = torch.randn(64, generator=g, dtype=torch.float64)
        want = s.step(e, t, z, return_dict=False)[0]
        k = s.step_coeffs(i)
        kinds.append(k["kind"])
        assert k["t"] == t and all(isinstance(c, float) for c in [k["c_base"]] + k["cz"] + k["ca"])
        if k["kind"] == "prk0":
            cur = mine
        if k["kind"].startswith("prk"):
            out, aux = pndm_linear_form(k, e, cur, [] if k["kind"] == "prk0" else [acc])
            acc = aux
        else:
            out, aux = pndm_linear_form(k, e, mine, hist[-3:][::-1])
            assert aux is None
        if k["kind"] in ("prk0", "plms"):
            hist.append(e)
        assert float((out - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (i, k["kind"])
        z, mine = want, out
    assert kinds == ["prk0", "prk1", "prk2", "prk3"] * 3 + ["plms"] * (n - 3)


# ---------------------------------------------------------------------------------------------------- C ABI
NEW = ("vsys_upsample_time2x", "vsys_cfg_pndm_step")


def test_new_entry_points_in_header_library_and_ctypes_table():
    from videosys_amd import _lib

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
    assert "autoencoder_kl_open_sora_plan_v110.py:1549-1554" in hdr and "PNDMScheduler" in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "videosys_amd", "csrc", "gen", "program_gen.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_host_side_argument_checks_of_the_new_kernels():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # an aligned address that is never dereferenced: every call below is refused before any launch

    def grid(T=1, H=4, W=6, pad=1, tf=0, rows=None):
        return (ctypes.c_int64 * 6)(T, H, W, pad, tf, (T + tf) * (H + 2 * pad) * (W + 2 * pad) if rows is None else rows)

    def up(gs=None, gd=None, N=1, C=128, x=P, y=P, y2=None, gr=None):
        return lib.vsys_upsample_time2x(x, grid(3, 2, 2) if gs is None else gs, y, grid(5, 2, 2, 1, 2) if gd is None else gd, y2, gr, 0.5, N, C, None)

    assert up(x=None) == VSYS_ERR_ARG and up(y=None) == VSYS_ERR_ARG
    assert lib.vsys_upsample_time2x(P, None, P, grid(), None, None, 0.5, 1, 128, None) == VSYS_ERR_ARG
    assert up(y2=P, gr=None) == VSYS_ERR_ARG                            # a second destination needs its grid
    assert up(gd=grid(6, 2, 2, 1, 2)) == VSYS_ERR_SHAPE                 # 3 frames -> 5, not 6
    assert up(gs=grid(1, 2, 2), gd=grid(2, 2, 2, 1, 2)) == VSYS_ERR_SHAPE   # one frame stays one frame
    assert up(gd=grid(5, 4, 4, 1, 2)) == VSYS_ERR_SHAPE and up(gd=grid(5, 2, 3, 1, 2)) == VSYS_ERR_SHAPE   # H and W stay
    assert up(C=12) == VSYS_ERR_SHAPE and up(C=0) == VSYS_ERR_SHAPE and up(C=4096) == VSYS_ERR_SHAPE
    assert up(gd=grid(5, 2, 2, 1, 2, rows=10)) == VSYS_ERR_SHAPE        # a sample stride smaller than the sample
    assert up(gs=grid(3, 2, 2, pad=2)) == VSYS_ERR_SHAPE and up(N=-1) == VSYS_ERR_SHAPE
    assert up(y2=P, gr=grid(4, 2, 2, 1, 0)) == VSYS_ERR_SHAPE and up(y2=P, gr=grid(5, 2, 3, 1, 0)) == VSYS_ERR_SHAPE
    assert up(x=P + 8) == VSYS_ERR_ALIGN and up(y=P + 2) == VSYS_ERR_ALIGN and up(y2=P + 4, gr=grid(5, 2, 2, 1, 0)) == VSYS_ERR_ALIGN
    assert up(N=0) == 0 and up(N=0, y2=P, gr=grid(5, 2, 2, 1, 0)) == 0

    def step(mo=P, e=None, src=(None,) * 4, base=P, z=P, aux=None, mi=P, Bz=1, Cin=4, Cout=8, thw=7, cb=1.0, cz=(1.0, 0, 0, 0, 0),
             ca=(0.0,) * 5, coef=True):
        c = (ctypes.c_double * 12)(7.5, cb, *cz, *ca) if coef else None
        return lib.vsys_cfg_pndm_step(mo, e, *src, base, z, aux, mi, Bz, Cin, Cout, thw, c, None)

    assert step(mo=None) == VSYS_ERR_ARG and step(z=None) == VSYS_ERR_ARG and step(mi=None) == VSYS_ERR_ARG and step(coef=False) == VSYS_ERR_ARG
    assert step(cz=(1.0, 0, 0.5, 0, 0)) == VSYS_ERR_ARG                 # a non-zero weight on a NULL source
    assert step(aux=P, ca=(0.0, 1.0, 0, 0, 0)) == VSYS_ERR_ARG          # the same through the accumulator's weights
    assert step(base=None) == VSYS_ERR_ARG                              # c_base != 0 needs its base
    assert step(Cout=4) == VSYS_ERR_SHAPE and step(Cin=0, Cout=0) == VSYS_ERR_SHAPE and step(Bz=-1) == VSYS_ERR_SHAPE
    assert step(thw=-1) == VSYS_ERR_SHAPE and step(Bz=1 << 31) == VSYS_ERR_SHAPE and step(Bz=1 << 16) == VSYS_ERR_SHAPE
    assert step(thw=0) == 0 and step(Bz=0) == 0 and step(base=None, cb=0.0, thw=0) == 0
    assert step(ca=(0.0, 1.0, 0, 0, 0), thw=0) == 0                     # no aux_out: its weights are ignored
    assert step(src=(P, None, None, None), cz=(1.0, 0.5, 0, 0, 0), thw=0) == 0


# ---------------------------------------------------------------------------------------------------- surface
_SOURCE_DEFAULTS = {"torch.device('cuda')": lambda v: v == torch.device("cuda"),
                    "torch.float16": lambda v: v is torch.bfloat16}      # the family runs in bf16 like the rest of this build


def _jsonable(v):
    return json.loads(json.dumps(v))          # (the timesteps of the MLP tables are strings in the fixture, as JSON holds dict keys)


def _assert_signature(fn, want, what, drop=()):
    ps = [p for p in list(inspect.signature(fn).parameters.values())[1:] if p.kind is not inspect.Parameter.VAR_KEYWORD]
    want = [w for w in want if w["name"] not in drop]
    assert [p.name for p in ps] == [w["name"] for w in want], what
    for p, w in zip(ps, want):
        assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, (what, p.name)
        if w.get("required"):
            assert p.default is inspect.Parameter.empty, (what, p.name)
        elif "default" in w:
            assert _jsonable(p.default) == w["default"] and type(p.default) is type(w["default"]), (what, p.name, p.default, w["default"])
        else:
            assert _SOURCE_DEFAULTS[w["default_source"]](p.default), (what, p.name, p.default, w["default_source"])


def test_surface_matches_the_reference_fixture():
    from videosys_amd.pab import PABConfig
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanConfig, OpenSoraPlanPipeline
    from videosys_amd.pipeline_open_sora_plan_v110 import (OpenSoraPlanV110Config, OpenSoraPlanV110PABConfig, OpenSoraPlanV110Pipeline,
                                                            PNDMScheduler)

    with open(os.path.join(GOLDEN, "osp_v110_pipeline_surface.json")) as fh:
        fx = json.load(fh)
    _assert_signature(OpenSoraPlanV110PABConfig.__init__, fx["OpenSoraPlanV110PABConfig.__init__"], "OpenSoraPlanV110PABConfig")
    _assert_signature(OpenSoraPlanV110Config.__init__, [w if w["name"] != "transformer_type" else dict(w, default="65x512x512")
                                                        for w in fx["OpenSoraPlanConfig.__init__"]], "OpenSoraPlanV110Config", drop=("version",))
    _assert_signature(OpenSoraPlanV110Pipeline.__init__, fx["OpenSoraPlanPipeline.__init__"], "OpenSoraPlanV110Pipeline")
    _assert_signature(OpenSoraPlanV110Pipeline.generate, fx["OpenSoraPlanPipeline.generate"], "generate")
    _assert_signature(OpenSoraPlanV110Pipeline.encode_prompt, fx["OpenSoraPlanPipeline.encode_prompt"], "encode_prompt")
    c = OpenSoraPlanV110Config()
    assert (c.version, c.transformer_type, c.num_frames, c.num_gpus, c.cpu_offload, c.enable_tiling, c.tile_overlap_factor, c.enable_pab,
            c.pab_config) == ("v110", "65x512x512", 65, 1, False, True, 0.25, False, None)
    assert (c.transformer, c.text_encoder, c.pipeline_cls) == ("LanguageBind/Open-Sora-Plan-v1.1.0", "DeepFloyd/t5-v1_1-xxl", OpenSoraPlanV110Pipeline)
    assert OpenSoraPlanV110Config(transformer_type="221x512x512").num_frames == 221
    p = OpenSoraPlanV110Config(enable_pab=True).pab_config
    assert isinstance(p, OpenSoraPlanV110PABConfig) and isinstance(p, PABConfig)
    assert (p.spatial_broadcast, p.spatial_threshold, p.spatial_range) == (True, [100, 850], 2)
    assert (p.temporal_broadcast, p.temporal_threshold, p.temporal_range) == (True, [100, 850], 4)
    assert (p.cross_broadcast, p.cross_threshold, p.cross_range, p.mlp_broadcast) == (True, [100, 850], 6, True)
    for tab in (p.mlp_spatial_broadcast_config, p.mlp_temporal_broadcast_config):
        assert sorted(tab) == list(range(426, 739, 24)) and all(v == {"block": [0, 1, 2, 3, 4, 5, 6], "skip_count": 2} for v in tab.values())
    with pytest.raises(AssertionError):
        OpenSoraPlanV110Config(transformer_type="29x480p")
    with pytest.raises(TypeError):
        OpenSoraPlanV110Config(bogus=1)
    with pytest.raises(TypeError):
        OpenSoraPlanV110Config(version="v110")                         # the keywords of the reference MINUS version
    with pytest.raises(NotImplementedError, match="num_gpus"):
        OpenSoraPlanV110Pipeline(OpenSoraPlanV110Config(num_gpus=2))
    # the refusals of the v1.2 classes stay, and name where the v1.1 route lives
    with pytest.raises(NotImplementedError, match="v1.1.*OpenSoraPlanV110Config"):
        OpenSoraPlanConfig(version="v110", transformer_type="65x512x512")
    with pytest.raises(NotImplementedError, match="v1.1"):
        OpenSoraPlanPipeline.__new__(OpenSoraPlanPipeline).encode_prompt("a")
    with pytest.raises(TypeError, match="step_coeffs|PNDMScheduler"):
        OpenSoraPlanV110Pipeline._check_scheduler(object(), "step_coeffs", "videosys_amd.pipeline_open_sora_plan_v110.PNDMScheduler")
    assert OpenSoraPlanV110Pipeline._check_scheduler(PNDMScheduler(), "step_coeffs", "x") is not None


class _FakeEncoder:
    """prompts -> (embeddings [B, 1, L, d], mask [B, L]): row l of prompt b holds 1000 b + l + 1 (pad positions included, as T5 gives
    pad positions outputs too); the prompt's token count is its number of words."""
    max_length = 300

    def __call__(self, prompts):
        B, L = len(prompts), self.max_length
        emb = (torch.arange(L)[None, :, None] + 1 + 1000.0 * torch.arange(B)[:, None, None]).expand(B, L, 8).clone()
        mask = torch.zeros(B, L, dtype=torch.int64)
        for b, p in enumerate(prompts):
            mask[b, :max(len(p.split()), 1)] = 1
        return emb[:, None], mask


def _bare_pipeline():
    from videosys_amd.pipeline_open_sora_plan_v110 import OpenSoraPlanV110Pipeline

    p = OpenSoraPlanV110Pipeline.__new__(OpenSoraPlanV110Pipeline)
    p.text_encoder, p._dtype, p._device = _FakeEncoder(), torch.float32, torch.device("cpu")
    p._enter_stage = lambda *a, **k: None
    return p


def test_encode_prompt_masks_as_the_reference_does():
    p = _bare_pipeline()
    pe, ne = p.encode_prompt("one two three", True, negative_prompt="")
    # a batch of one: both cut to keep_index = 3; the negative one is SLICED (its rows 1 and 2 are pad-position outputs)
    assert tuple(pe.shape) == tuple(ne.shape) == (1, 3, 8) and pe[0, :, 0].tolist() == [1.0, 2.0, 3.0] and ne[0, :, 0].tolist() == [1.0, 2.0, 3.0]
    pe, ne = p.encode_prompt(["one two", "a b c d e"], True, negative_prompt="")
    # a batch of several: 300 positions, the prompt embeddings multiplied by the mask, the negative ones as encoded
    assert tuple(pe.shape) == tuple(ne.shape) == (2, 300, 8)
    assert pe[0, :3, 0].tolist() == [1.0, 2.0, 0.0] and pe[1, 3:6, 0].tolist() == [1004.0, 1005.0, 0.0] and float(pe[0, 2:].abs().max()) == 0.0
    assert float(ne[1, 299, 0]) == 1300.0
    pe, ne = p.encode_prompt("one two three", False)
    assert ne is None and tuple(pe.shape) == (1, 3, 8)
    pe, ne = p.encode_prompt("one two three", True, mask_feature=False)
    assert tuple(pe.shape) == tuple(ne.shape) == (1, 300, 8)
    e = torch.randn(2, 5, 8)
    pe, ne = p.encode_prompt(None, True, prompt_embeds=e, negative_prompt_embeds=-e)      # embeddings passed in are not masked
    assert torch.equal(pe, e) and torch.equal(ne, -e)
    pe, ne = p.encode_prompt("a b", True, num_images_per_prompt=2)
    assert tuple(pe.shape) == tuple(ne.shape) == (2, 300, 8) and float(pe[1, 1, 0]) == 2.0 and float(pe[1, 2, 0]) == 0.0


def test_aliases_resolve_in_a_fresh_interpreter():
    code = ("import videosys, videosys_amd\n"
            "from videosys.pipelines.open_sora_plan import OpenSoraPlanV110PABConfig, OpenSoraPlanV110Config, OpenSoraPlanV110Pipeline\n"
            "from videosys.pipelines.open_sora_plan.pipeline_open_sora_plan import OpenSoraPlanV110PABConfig as P2, PNDMScheduler\n"
            "from videosys.models.autoencoders.autoencoder_kl_open_sora_plan_v110 import CausalVAEModelWrapper, CausalVAEModel\n"
            "from videosys.models.autoencoders.autoencoder_kl_open_sora_plan_v120 import CausalVAEModel as V120\n"
            "from videosys_amd import pipeline_open_sora_plan_v110 as m, vae_open_sora_plan_v110 as v\n"
            "assert OpenSoraPlanV110PABConfig is P2 is m.OpenSoraPlanV110PABConfig and PNDMScheduler is m.PNDMScheduler\n"
            "assert CausalVAEModel is v.CausalVAEModel and CausalVAEModel is not V120 and issubclass(CausalVAEModel, V120)\n"
            "assert OpenSoraPlanV110Config().pipeline_cls is OpenSoraPlanV110Pipeline\n"
            "for n in ('OpenSoraPlanPipeline', 'OpenSoraPlanConfig', 'OpenSoraPlanV110PABConfig'):\n"
            "    try:\n"
            "        getattr(videosys, n)\n"
            "    except ImportError:\n"
            "        continue\n"
            "    raise SystemExit(n + ' resolved at the top level')\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------- Python wrappers
def test_wrapper_argument_checks_raise_before_any_launch(monkeypatch):
    """The refusals of open_sora_plan_v110_ops.upsample_time2x / cfg_pndm_step on CPU tensors: every wrong call is an AssertionError
    naming the fault, a right call on the wrong device the library's VsysError — and the entry points are never reached."""
    from videosys_amd import _lib
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd.ops import VaeGrid

    def no_launch(name, *a):
        raise RuntimeError(f"{name} was launched")

    monkeypatch.setattr(vops, "_call", no_launch)
    bf = lambda g, C: torch.zeros(g.rows, C, dtype=torch.bfloat16)
    gs, gd, gr = VaeGrid(1, 3, 2, 2, 1, 0), VaeGrid(1, 5, 2, 2, 1, 2), VaeGrid(1, 5, 2, 2, 1, 0)
    ok = dict(x=bf(gs, 32), gs=gs, y=bf(gd, 32), gd=gd, C=32)
    with pytest.raises(AssertionError, match="multiple of 8"):
        vops.upsample_time2x(**dict(ok, x=bf(gs, 12), y=bf(gd, 12), C=12))
    for bad in (VaeGrid(1, 6, 2, 2, 1, 2), VaeGrid(1, 5, 2, 3, 1, 2), VaeGrid(2, 5, 2, 2, 1, 2)):
        with pytest.raises(AssertionError, match="grid_dst does not match"):
            vops.upsample_time2x(**dict(ok, y=bf(bad, 32), gd=bad))
    with pytest.raises(AssertionError, match="grid_dst does not match"):       # one frame stays one frame
        vops.upsample_time2x(bf(VaeGrid(1, 1, 2, 2, 1, 0), 32), VaeGrid(1, 1, 2, 2, 1, 0), bf(VaeGrid(1, 2, 2, 2, 1, 2), 32), VaeGrid(1, 2, 2, 2, 1, 2), 32)
    with pytest.raises(AssertionError):                                        # rows of another grid
        vops.upsample_time2x(**dict(ok, y=bf(gr, 32)))
    with pytest.raises(AssertionError, match="grid_res does not match"):
        vops.upsample_time2x(**ok, y_res=bf(gr, 32), g_res=VaeGrid(1, 4, 2, 2, 1, 0))
    with pytest.raises(AssertionError, match="grid_res"):
        vops.upsample_time2x(**ok, y_res=bf(gr, 32), g_res=None)
    with pytest.raises(_lib.VsysError, match="HIP device"):
        vops.upsample_time2x(**ok, y_res=bf(gr, 32), g_res=gr, alpha=0.5)

    Bz, Cin, thw = 1, 4, 7
    f = lambda: torch.zeros(Bz, Cin, thw)
    good = dict(model_out=torch.zeros(2 * Bz, 2 * Cin, thw), model_in=torch.zeros(2 * Bz, Cin, thw, dtype=torch.bfloat16), z_out=f(),
                guidance=7.5, c_base=1.0, cz=[1.0], base=f())
    with pytest.raises(AssertionError, match="learned sigma"):
        vops.cfg_pndm_step(**dict(good, model_out=torch.zeros(2 * Bz, Cin, thw)))             # Cout != 2 Cin
    with pytest.raises(AssertionError):
        vops.cfg_pndm_step(**dict(good, model_out=torch.zeros(Bz, 2 * Cin, thw)))             # one CFG half
    with pytest.raises(AssertionError, match="weight on source 1"):
        vops.cfg_pndm_step(**dict(good, cz=[1.0, 0.0, 0.5], srcs=(f(),)))
    with pytest.raises(AssertionError, match="weight on source 0"):
        vops.cfg_pndm_step(**dict(good, ca=[0.0, 1.0]), aux_out=f())
    vops_ok_without_aux = dict(good, ca=[0.0, 1.0])                                            # no aux_out: its weights are ignored
    with pytest.raises(_lib.VsysError, match="HIP device"):
        vops.cfg_pndm_step(**vops_ok_without_aux)
    with pytest.raises(AssertionError, match="no base"):
        vops.cfg_pndm_step(**dict(good, base=None))
    z = f()
    with pytest.raises(AssertionError, match="distinct"):
        vops.cfg_pndm_step(**dict(good, z_out=z), e_out=z)
    with pytest.raises(AssertionError, match="at most four"):
        vops.cfg_pndm_step(**good, srcs=[f() for _ in range(5)])
    with pytest.raises(AssertionError):
        vops.cfg_pndm_step(**good, srcs=(torch.zeros(Bz, Cin, thw + 1),))
    with pytest.raises(AssertionError):
        vops.cfg_pndm_step(**dict(good, model_in=torch.zeros(2 * Bz, Cin, thw)[:, :, ::1].float().to(torch.bfloat16)[:1]))
    with pytest.raises(_lib.VsysError, match="HIP device"):                    # in place and accumulator forms are legal arguments
        vops.cfg_pndm_step(**dict(good, z_out=z, base=z), srcs=(f(),))
