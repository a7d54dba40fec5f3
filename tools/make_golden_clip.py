"""TEST INFRASTRUCTURE ONLY — mints tests/golden/clip_l_small.pt and clip_g_small.pt from the REAL
transformers.CLIPTextModelWithProjection (the third-party class Vchitect-2.0 instantiates twice, pipeline_vchitect.py:194-201), on
the CPU, with random weights from videosys_amd.clip.synth_state_dict.

Two tiny configs, 3 layers, L = 77, B = 2 (one short prompt, one that fills all 77 positions):
  clip_l_small   2 heads, quick_gelu, eos_token_id = 2 (the legacy pooling rule: argmax of the ids), projection_dim = hidden
  clip_g_small   3 heads, gelu, the tokenizer's real eos_token_id (first-match rule), projection_dim != hidden
Each file holds the ids, the fp32 model's hidden_states and text_embeds, and the bf16 model's (stored as bf16).  The weights are NOT in
the file — a committed file stays below 1 MiB — but come from ``synth_state_dict(seed=...)`` as tests/golden/t5_small.pt's do; the file
carries a float64 checksum of them so that a test can tell a changed generator from a wrong encoder.  Attention runs as
``attn_implementation="eager"``: softmax(..., dtype=float32).to(bf16), the formula vsys_clip_attention_d64 is written against.

    python tools/make_golden_clip.py
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from videosys_amd.clip import ClipByteTokenizer, synth_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
VOCAB = 320
CASES = {
    "clip_l_small.pt": dict(seed=31, cfg=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                                              vocab_size=VOCAB, max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=128,
                                              eos_token_id=2)),
    "clip_g_small.pt": dict(seed=32, cfg=dict(hidden_size=192, intermediate_size=384, num_hidden_layers=3, num_attention_heads=3,
                                              vocab_size=VOCAB, max_position_embeddings=77, hidden_act="gelu", projection_dim=96,
                                              eos_token_id=VOCAB - 1)),
}
PROMPTS = ["a sunset over the sea", "a very long prompt that fills every position of the window, " * 3]


def weights(cfg, seed):
    return synth_state_dict(cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["vocab_size"],
                            cfg["max_position_embeddings"], cfg["projection_dim"], seed=seed)


def checksum(sd) -> float:
    return float(sum(v.double().abs().sum() * (1 + i % 7) for i, (k, v) in enumerate(sorted(sd.items()))))


def hf_model(cfg, sd, dtype):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection

    c = CLIPTextConfig(**cfg, bos_token_id=1, pad_token_id=0, attention_dropout=0.0, attn_implementation="eager")
    m = CLIPTextModelWithProjection(c).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m.to(dtype)


def main():
    tok = ClipByteTokenizer(VOCAB)
    ids = tok(PROMPTS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert ids.shape == (2, 77) and int(ids[1, -1]) == tok.eos_token_id and int(ids[0, -1]) == tok.pad_token_id
    rel = lambda a, b: ((a.float() - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    for name, case in CASES.items():
        cfg, seed = case["cfg"], case["seed"]
        sd = weights(cfg, seed)
        with torch.no_grad():
            o32 = hf_model(cfg, sd, torch.float32)(ids, output_hidden_states=True)
            o16 = hf_model(cfg, sd, torch.bfloat16)(ids, output_hidden_states=True)
        assert len(o32.hidden_states) == cfg["num_hidden_layers"] + 1
        print(name, "bf16 vs fp32 rel rms per hidden state:", [round(rel(a, b), 5) for a, b in zip(o16.hidden_states, o32.hidden_states)],
              "text_embeds:", round(rel(o16.text_embeds, o32.text_embeds), 5))
        path = os.path.join(OUT, name)
        torch.save({"cfg": cfg, "seed": seed, "weights_checksum": checksum(sd), "ids": ids,
                    "hidden_states_fp32": [h.clone() for h in o32.hidden_states], "text_embeds_fp32": o32.text_embeds.clone(),
                    "last_hidden_state_fp32": o32.last_hidden_state.clone(),
                    "hidden_states_bf16": [h.clone() for h in o16.hidden_states], "text_embeds_bf16": o16.text_embeds.clone()}, path)
        print("wrote", name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
