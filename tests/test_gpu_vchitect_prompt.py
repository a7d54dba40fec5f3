"""-m gpu: VchitectXLPipeline from a PROMPT — the two CLIP encoders of this build (videosys_amd/clip.py) wired into
videosys_amd/pipeline_vchitect.py.  The transformer is the tiny synthetic model of tests/test_gpu_vchitect_pipeline.py (dim 192, depth
2, latent 16 x 16) with ``pooled_projection_dim = 2048`` (the published 768 + 1280, which fixes the two projection_dims) and
``joint_attention_dim = 384``; the CLIP geometries are reduced through ``clip_config`` (2 layers, hidden 128, byte vocabulary) so that
the file runs in seconds; no T5 (``text_encoder_3=None``: the zeros of pipeline_vchitect.py:295-300).

  * generate(prompt=...) returns frames (without the encoders it raises "the CLIP encoders ... are not built");
  * encode_prompt: [1, 77 + 256, joint_attention_dim] and [1, 2048]; the CLIP columns equal _get_clip_prompt_embeds on the same
    encoder called directly, the columns behind them and the T5 rows are zero; clip_skip = 1 selects hidden_states[-3];
  * two generate calls with the same seed and prompt give identical bytes;
  * cpu_offload=True: the same bytes, and the CLIP weights are off the device when generate returns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, JD, PD, HW = 11, 384, 2048, 16
TCFG = dict(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=3, joint_attention_dim=JD,
            caption_projection_dim=192, pooled_projection_dim=PD, out_channels=16, pos_embed_max_size=24)
SMALL = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, vocab_size=320)
PROMPT = "a sunset"


def build(**kw):
    from videosys_amd import VchitectConfig, VchitectXLPipeline

    cfg = VchitectConfig(f"synthetic:{SEED}", transformer_config=dict(TCFG), clip_config={"text_encoder": SMALL, "text_encoder_2": SMALL},
                         **kw)
    return VchitectXLPipeline(cfg, text_encoder="synthetic:1", text_encoder_2="synthetic:2", text_encoder_3=None)


_PIPE = {}


def pipeline():
    if "p" not in _PIPE:
        _PIPE["p"] = build()
    return _PIPE["p"]


def frames(pipe):
    out = pipe.generate(prompt=PROMPT, negative_prompt="", height=8 * HW, width=8 * HW, frames=2, num_inference_steps=2, seed=3)
    torch.cuda.synchronize()
    return [np.asarray(f) for f in out.video[0]]


_FRAMES = {}


def reference_frames():
    if "f" not in _FRAMES:
        _FRAMES["f"] = frames(pipeline())
    return _FRAMES["f"]


def test_generate_from_a_prompt_returns_frames():
    from videosys_amd.clip import CLIPTextEncoder, ClipByteTokenizer

    pipe = pipeline()
    assert isinstance(pipe.text_encoder, CLIPTextEncoder) and isinstance(pipe.text_encoder_2, CLIPTextEncoder)
    assert isinstance(pipe.tokenizer, ClipByteTokenizer) and pipe.tokenizer_max_length == 77
    c1, c2 = pipe.text_encoder.config, pipe.text_encoder_2.config
    assert (c1.projection_dim, c2.projection_dim) == (768, 1280) and (c1.hidden_act, c2.hidden_act) == ("quick_gelu", "gelu")
    f = reference_frames()
    assert len(f) == 2 and all(a.shape == (8 * HW, 8 * HW, 3) and a.dtype == np.uint8 for a in f)
    assert len({a.tobytes() for a in f}) == 2 and all(a.std() > 0 for a in f)


def test_encode_prompt_shapes_and_clip_columns():
    pipe = pipeline()
    pe, ne, pp, npp = pipe.encode_prompt(PROMPT, None, None, negative_prompt="")
    assert pe.shape == ne.shape == (1, 77 + 256, JD) and pp.shape == npp.shape == (1, PD)
    e1, p1 = pipe._get_clip_prompt_embeds(PROMPT, clip_model_index=0)
    e2, p2 = pipe._get_clip_prompt_embeds(PROMPT, clip_model_index=1)
    assert e1.shape == e2.shape == (1, 77, 128) and p1.shape == (1, 768) and p2.shape == (1, 1280)
    assert torch.equal(pe[:, :77, :128], e1) and torch.equal(pe[:, :77, 128:256], e2)
    assert float(pe[:, :77, 256:].abs().max()) == 0.0 and float(pe[:, 77:].abs().max()) == 0.0
    assert torch.equal(pp, torch.cat([p1, p2], dim=-1)) and float(pp.float().abs().max()) > 0
    assert not torch.equal(pe, ne) and not torch.equal(pp, npp)
    # the encoder called directly, as pipeline_vchitect.py:368 calls it
    ids = pipe.tokenizer(PROMPT, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    out = pipe.text_encoder(ids.to(pipe._device), output_hidden_states=True)
    assert len(out.hidden_states) == 3
    assert torch.equal(e1, out.hidden_states[-2]) and torch.equal(p1, out[0])
    skipped, _ = pipe._get_clip_prompt_embeds(PROMPT, clip_skip=1, clip_model_index=0)
    assert torch.equal(skipped, out.hidden_states[-3]) and not torch.equal(skipped, e1)


def test_generate_is_deterministic():
    a, b = reference_frames(), frames(pipeline())
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_cpu_offload_gives_the_same_frames_and_parks_the_clip_weights():
    pipe = build(cpu_offload=True)
    on_device = lambda enc: [k for k, v in enc.w.items() if v.is_cuda]
    assert not on_device(pipe.text_encoder) and not on_device(pipe.text_encoder_2)       # parked from the start
    got = frames(pipe)
    assert all(np.array_equal(x, y) for x, y in zip(reference_frames(), got))
    assert not on_device(pipe.text_encoder) and not on_device(pipe.text_encoder_2)
    assert list(pipe._stages)[:2] == ["text_encoder", "text_encoder_2"]                  # the reference's model_cpu_offload_seq order
