"""No GPU: the host side of the CLIP text encoders (videosys_amd/clip.py) and the C ABI of their two kernels (csrc/clip_ops.hip).

  * vsys_clip_attention_d64 / vsys_splitk_reduce_bias_act: in the header, the library and the ctypes table, outside the op table; their
    error codes for bad arguments (a refused call launches nothing, so no device is needed);
  * clip_ops.hip cross-compiles for gfx950 and the attention kernel uses no scratch and spills no VGPR;
  * load_state_dict reads exactly the keys transformers.CLIPTextModelWithProjection has, and refuses a dict that lacks one;
  * ClipByteTokenizer: round trip, truncation at 77, its end token under both pooling rules;
  * pooled_positions against transformers' own pooling on ids where pad equals eos and where the prompt fills all 77 positions;
  * a checkpoint directory written with safetensors + config.json is parsed into the constructor's keywords and state dict."""
import json
import os
import re
from types import SimpleNamespace

import pytest
import torch

from op_table import assert_coded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3
NEW = ("vsys_clip_attention_d64", "vsys_splitk_reduce_bias_act")
TINY = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, vocab_size=300,
            max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=96, eos_token_id=2)


# ---------------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_in_header_library_and_ctypes_table():
    import __graft_entry__ as G
    from videosys_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    lib = _lib.load()
    assert_coded(NEW)                                 # in the launch-program table, with the prototype's arity
    for n in NEW:
        assert re.search(rf"\nint {n}\(", hdr), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
        proto = re.search(rf"\nint {n}\(([^;]*?)\);", hdr, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[n]), n
        comment = hdr[:hdr.index(f"\nint {n}(")].rsplit("/*", 1)[1]
        assert "modeling_clip.py" in comment and "pipeline_vchitect.py:368" in comment, n   # names the third-party code it replaces
    assert re.search(r"#define VSYS_OP_COUNT 75\b", hdr) and re.search(r"#define VSYS_ABI_VERSION 1\b", hdr)
    assert "clip_ops.hip" in G.SOURCES
    src = open(os.path.join(ROOT, "videosys_amd", "csrc", "clip_ops.hip")).read()
    assert "asm" not in src.replace("namespace", "")  # plain HIP C++: no inline assembly in the new kernels
    assert src.count("__builtin_amdgcn_mfma_f32_16x16x32_bf16") >= 3   # both products of the attention on the 16x16x32 form


def test_host_side_argument_checks():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # a 16-byte aligned address that is never dereferenced: every call below is refused before any launch

    def attn(B=2, L=77, inner=128, ld=384, ldo=128, qkv=P, out=P):
        return lib.vsys_clip_attention_d64(qkv, ld, inner, out, ldo, B, L, None)

    assert attn(L=0) == VSYS_ERR_SHAPE and attn(L=129) == VSYS_ERR_SHAPE and attn(L=-1) == VSYS_ERR_SHAPE
    assert attn(inner=96, ld=288, ldo=96) == VSYS_ERR_SHAPE and attn(inner=0) == VSYS_ERR_SHAPE
    assert attn(qkv=None) == VSYS_ERR_ARG and attn(out=None) == VSYS_ERR_ARG
    assert attn(B=0) == VSYS_ERR_SHAPE and attn(B=1 << 31) == VSYS_ERR_SHAPE
    assert attn(ld=256) == VSYS_ERR_SHAPE and attn(ldo=64) == VSYS_ERR_SHAPE       # rows narrower than 3 inner / inner
    assert attn(ld=388) == VSYS_ERR_ALIGN and attn(ldo=132) == VSYS_ERR_ALIGN      # strides off the 8-element grid
    assert attn(qkv=P + 2) == VSYS_ERR_ALIGN and attn(out=P + 8) == VSYS_ERR_ALIGN

    def red(M=77, N=128, S=3, slab=None, ldp=128, ldr=128, ldo=128, part=P, res=P, out=P, bias=P, act=1):
        return lib.vsys_splitk_reduce_bias_act(part, S, 384 * N if slab is None else slab, ldp, res, ldr, out, ldo, M, N, bias, act, None)

    assert red(act=3) == VSYS_ERR_ARG and red(act=-1) == VSYS_ERR_ARG
    assert red(part=None) == VSYS_ERR_ARG and red(out=None) == VSYS_ERR_ARG
    assert red(N=124, ldp=124) == VSYS_ERR_SHAPE                                    # not whole 16-byte chunks
    assert red(S=0) == VSYS_ERR_SHAPE and red(S=65) == VSYS_ERR_SHAPE
    assert red(ldp=64) == VSYS_ERR_SHAPE and red(slab=128) == VSYS_ERR_SHAPE and red(ldo=132) == VSYS_ERR_SHAPE
    assert red(ldr=132) == VSYS_ERR_SHAPE and red(ldo=64) == VSYS_ERR_SHAPE
    assert red(bias=P + 2) == VSYS_ERR_ALIGN and red(out=P + 8) == VSYS_ERR_ALIGN
    assert red(M=0) == 0                                                            # nothing to do, nothing launched


def test_clip_kernels_compile_without_scratch():
    from test_build_resources import HIPCC, _usage

    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    u = _usage("clip_ops.hip")
    attn = {k: v for k, v in u.items() if "clip_attention_d64_kernel" in k}
    red = {k: v for k, v in u.items() if "splitk_reduce_bias_act_kernel" in k}
    assert len(attn) == 1 and len(red) == 3, list(u)
    for name, res in {**attn, **red}.items():
        assert res.get("ScratchSize", 0) == 0, f"{name} uses scratch: {res}"
        assert res.get("VGPRs Spill", 0) == 0 and res.get("SGPRs Spill", 0) == 0, f"{name} spills: {res}"
    (res,) = attn.values()
    assert res.get("VGPRs", 0) <= 128 and res.get("LDS Size", 0) <= 64 * 1024, res   # two workgroups of 4 waves per CU at least


# ---------------------------------------------------------------------------------------------------- weights
def test_state_dict_keys_are_those_of_transformers():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection

    from videosys_amd import clip

    m = CLIPTextModelWithProjection(CLIPTextConfig(**TINY, bos_token_id=1, pad_token_id=0))
    theirs = {k for k in m.state_dict() if not k.endswith("position_ids")}      # (a buffer in older transformers, no weight)
    assert set(clip.state_dict_keys(TINY["num_hidden_layers"])) == theirs
    sd = clip.synth_state_dict(TINY["hidden_size"], TINY["intermediate_size"], TINY["num_hidden_layers"], TINY["vocab_size"], 77,
                               TINY["projection_dim"], seed=3)
    assert set(sd) == theirs and all(sd[k].shape == v.shape for k, v in m.state_dict().items() if k in sd)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing)


def _bare_encoder(**cfg):
    """A CLIPTextEncoder without its constructor's device check: what load_state_dict reads, weights kept on the CPU."""
    from videosys_amd.clip import CLIPTextEncoder

    e = CLIPTextEncoder.__new__(CLIPTextEncoder)
    e.config, e.device, e.dtype, e.w = SimpleNamespace(**cfg, layer_norm_eps=1e-5), torch.device("cpu"), torch.bfloat16, {}
    return e


def test_load_state_dict_fuses_qkv_and_refuses_a_missing_key():
    from videosys_amd import clip

    sd = clip.synth_state_dict(128, 256, 2, 300, 77, 96, seed=4)
    e = _bare_encoder(**TINY).load_state_dict(sd)
    p = "text_model.encoder.layers.1.self_attn."
    assert e.w["1.qkv.weight"].shape == (384, 128) and e.w["1.qkv.bias"].shape == (384,)
    assert torch.equal(e.w["1.qkv.weight"][128:256].float(), sd[p + "k_proj.weight"])
    assert torch.equal(e.w["1.qkv.bias"][256:].float(), sd[p + "v_proj.bias"])
    assert torch.equal(e.w["proj"].float(), sd["text_projection.weight"]) and e.w["proj"].shape == (96, 128)
    for k in ("text_projection.weight", p + "q_proj.bias", "text_model.final_layer_norm.bias",
              "text_model.embeddings.position_embedding.weight"):
        with pytest.raises(KeyError, match=re.escape(k)):
            _bare_encoder(**TINY).load_state_dict({a: b for a, b in sd.items() if a != k})
    with pytest.raises(ValueError, match="shape"):
        _bare_encoder(**dict(TINY, projection_dim=128)).load_state_dict(sd)


def test_constructor_refuses_what_the_kernels_do_not_cover():
    from videosys_amd.clip import CLIPTextEncoder

    with pytest.raises(RuntimeError, match="HIP device"):
        CLIPTextEncoder(device="cpu")
    # (the checks below come before any device work, but after the device check: a cuda device STRING is enough to reach them)
    with pytest.raises(ValueError, match="64 \\* num_attention_heads"):
        CLIPTextEncoder(hidden_size=768, num_attention_heads=8, device="cuda:0")
    with pytest.raises(ValueError, match="hidden_act"):
        CLIPTextEncoder(hidden_act="gelu_new", device="cuda:0")


# ---------------------------------------------------------------------------------------------------- tokenizer and pooling
def test_byte_tokenizer_round_trip_truncation_and_end_token():
    from videosys_amd.clip import ClipByteTokenizer, pooled_positions

    tok = ClipByteTokenizer(400)
    assert tok.model_max_length == 77 and tok.eos_token_id == 399
    prompts = ["a sunset", "grüße, 世界", ""]
    enc = tok(prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt")
    ids = enc.input_ids
    assert ids is enc["input_ids"] and ids.shape == (3, 77) and ids.dtype == torch.int64
    assert tok.batch_decode(ids) == prompts
    n = [len(p.encode("utf-8")) for p in prompts]
    for b in range(3):
        assert int(ids[b, 0]) == tok.bos_token_id and int(ids[b, n[b] + 1]) == tok.eos_token_id
        assert bool((ids[b, n[b] + 2:] == tok.pad_token_id).all()) and int(ids[b].max()) == tok.eos_token_id
        assert int(enc.attention_mask[b].sum()) == n[b] + 2
    # both pooling rules of CLIPTextTransformer land on the end token
    want = torch.tensor([v + 1 for v in n])
    assert torch.equal(pooled_positions(ids, 2), want) and torch.equal(pooled_positions(ids, tok.eos_token_id), want)
    # truncation at 77 keeps begin and end; "longest" pads to the longest prompt and does not truncate
    long = "x" * 200
    t = tok([long, "ab"], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert t.shape == (2, 77) and int(t[0, -1]) == tok.eos_token_id and tok.batch_decode(t)[0] == "x" * 75
    u = tok([long, "ab"], padding="longest", return_tensors="pt").input_ids
    assert u.shape == (2, 202) and tok.batch_decode(u) == [long, "ab"]
    assert tok.batch_decode(u[:, 76:-1])[0] == "x" * 125          # what the pipeline's truncation warning prints
    with pytest.raises(ValueError):
        ClipByteTokenizer(200)


@pytest.mark.parametrize("eos", [2, 299])
def test_pooled_positions_agree_with_transformers(eos):
    """ids where the pad token EQUALS the end token (CLIP-L's tokenizer) and a row that fills all 77 positions: the row this build
    gathers is the one CLIPTextModelWithProjection pools — text_embeds equals text_projection of that row of last_hidden_state."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection

    from videosys_amd.clip import pooled_positions

    torch.manual_seed(0)
    m = CLIPTextModelWithProjection(CLIPTextConfig(**dict(TINY, eos_token_id=eos), bos_token_id=1, pad_token_id=0)).eval()
    end = 299                                             # the largest id: what the legacy argmax rule looks for
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, 290, (3, 77), generator=g)
    ids[:, 0] = 1
    ids[0, 9:] = end                                      # pad == eos: the FIRST of the run is the end of the prompt
    ids[1, 76] = end                                      # the prompt fills all 77 positions
    ids[2, 30], ids[2, 31:] = end, 0                      # pad id 0 behind the end token
    pos = pooled_positions(ids, eos)
    assert pos.tolist() == [9, 76, 30]
    with torch.no_grad():
        out = m(ids)
        want = m.text_projection(out.last_hidden_state[torch.arange(3), pos])
    assert torch.equal(out.text_embeds, want)
    assert not torch.equal(out.text_embeds[0], m.text_projection(out.last_hidden_state[0, 10]))   # (a neighbour row differs)


# ---------------------------------------------------------------------------------------------------- checkpoint directory
def test_checkpoint_directory_is_parsed(tmp_path, monkeypatch):
    """<dir>/config.json + model.safetensors (the transformers file name) -> constructor keywords + state dict; through
    pipeline.build_clip_encoder with the device part replaced, so nothing here needs a GPU."""
    from safetensors.torch import save_file

    from videosys_amd import clip, pipeline
    from videosys_amd.utils import ctor_kwargs, read_component

    d = tmp_path / "text_encoder_2"
    d.mkdir()
    sd = clip.synth_state_dict(128, 256, 2, 300, 77, 96, seed=6)
    save_file({k: v.to(torch.bfloat16) for k, v in sd.items()}, str(d / "model.safetensors"))
    hf = dict(TINY, architectures=["CLIPTextModelWithProjection"], model_type="clip_text_model", torch_dtype="bfloat16", bos_token_id=0,
              pad_token_id=1, attention_dropout=0.0, initializer_range=0.02)
    (d / "config.json").write_text(json.dumps(hf))
    cfg, got = read_component(str(tmp_path), "text_encoder_2")
    assert set(got) == set(sd) and all(torch.equal(got[k].float(), sd[k]) for k in sd)
    kw = ctor_kwargs(clip.CLIPTextEncoder.__init__, cfg)
    assert kw == TINY                                       # every constructor field, none of the bookkeeping keys
    seen = {}

    def fake(cfg, sd, device):
        seen.update(cfg=cfg, sd=sd, device=device)
        return _bare_encoder(**ctor_kwargs(clip.CLIPTextEncoder.__init__, cfg)).load_state_dict(sd)

    monkeypatch.setattr(pipeline, "clip_encoder_from", fake)
    tok = object()
    enc, tok2 = pipeline.build_clip_encoder(str(d), tok, device="cuda:0", geometry={})
    assert tok2 is tok and seen["device"] == "cuda:0" and enc.w["0.qkv.weight"].shape == (384, 128)
    assert pipeline.build_clip_encoder(None, tok, device="cuda:0", geometry={}) == (None, tok)
    inj = lambda ids, output_hidden_states=False: None     # an injected object stays what it is
    assert pipeline.build_clip_encoder(inj, None, device="cuda:0", geometry={}) == (inj, None)
    with pytest.raises(FileNotFoundError):
        pipeline.build_clip_encoder(str(tmp_path / "nope"), None, device="cuda:0", geometry={})
