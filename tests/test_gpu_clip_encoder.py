"""-m gpu: clip.CLIPTextEncoder against transformers.CLIPTextModelWithProjection — tests/golden/clip_l_small.pt and clip_g_small.pt,
minted on the CPU by tools/make_golden_clip.py (2 heads / quick_gelu / eos_token_id 2 / projection = hidden, and 3 heads / gelu / a
real eos_token_id / projection != hidden; 3 layers, L = 77, B = 2, one prompt that fills all 77 positions).

Per hidden_states[k] and for text_embeds: rel-rms error against the fp32 model <= 1.5 x (the bf16 transformers run's error) + 1e-3 —
the margin of tests/test_gpu_t5.py for an implementation that rounds differently from, but no worse than, the bf16 reference.  The
weights come from clip.synth_state_dict at the golden's seed; the golden carries their checksum, so a generator that changed shows
as that, not as an encoder error."""
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_RUN = {}


def run(name):
    """(golden, encoder, output with hidden states) — one encode per golden, shared by the tests."""
    if name not in _RUN:
        import os
        import sys

        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from make_golden_clip import checksum, weights   # (the recipe the golden was minted with: same weights, same checksum)

        from videosys_amd.clip import CLIPTextEncoder

        gold = load_golden(name)
        sd = weights(gold["cfg"], gold["seed"])
        assert checksum(sd) == gold["weights_checksum"], "synth_state_dict no longer draws the weights the golden was minted from"
        enc = CLIPTextEncoder(device=dev(), **gold["cfg"]).load_state_dict(sd)
        out = enc(gold["ids"], output_hidden_states=True)
        torch.cuda.synchronize()
        _RUN[name] = (gold, enc, out)
    return _RUN[name]


def rel_rms(a, ref):
    return ((a.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("name", ["clip_l_small.pt", "clip_g_small.pt"])
def test_encoder_matches_transformers_golden(name):
    gold, enc, out = run(name)
    cfg = gold["cfg"]
    B, L = gold["ids"].shape
    assert out[0] is out.text_embeds and out.text_embeds.shape == (B, cfg["projection_dim"])
    assert len(out.hidden_states) == cfg["num_hidden_layers"] + 1 == len(gold["hidden_states_fp32"])
    assert out.last_hidden_state.shape == (B, L, cfg["hidden_size"]) and out.text_embeds.dtype == torch.bfloat16
    report = []
    for k, (h, h32, h16) in enumerate(zip(out.hidden_states, gold["hidden_states_fp32"], gold["hidden_states_bf16"])):
        assert h.shape == (B, L, cfg["hidden_size"])
        report.append((f"hidden_states[{k}]", rel_rms(h.cpu(), h32), rel_rms(h16, h32)))
    report.append(("text_embeds", rel_rms(out.text_embeds.cpu(), gold["text_embeds_fp32"]),
                   rel_rms(gold["text_embeds_bf16"], gold["text_embeds_fp32"])))
    for what, mine, floor in report:
        print(f"{name} {what}: rel rms {mine:.5f}, transformers-bf16 floor {floor:.5f}")
    for what, mine, floor in report:
        assert mine <= 1.5 * floor + 1e-3, f"{what}: rel rms {mine:.5f} vs transformers-bf16 floor {floor:.5f}"


@pytest.mark.parametrize("name", ["clip_l_small.pt", "clip_g_small.pt"])
def test_last_hidden_state_is_normed_and_hidden_states_are_not(name):
    """hidden_states[-1] is taken BEFORE final_layer_norm, last_hidden_state after it (transformers' convention)."""
    gold, enc, out = run(name)
    last32 = gold["last_hidden_state_fp32"]
    floor = rel_rms(torch.nn.functional.layer_norm(gold["hidden_states_bf16"][-1], last32.shape[-1:],
                                                   enc.w["ln_f.weight"].float().cpu(), enc.w["ln_f.bias"].float().cpu(), 1e-5), last32)
    assert rel_rms(out.last_hidden_state.cpu(), last32) <= 1.5 * floor + 1e-3
    assert rel_rms(out.hidden_states[-1].cpu(), gold["hidden_states_fp32"][-1]) < 0.05
    assert rel_rms(out.hidden_states[-1].cpu(), last32) > 0.2          # the two differ by the norm: neither stands in for the other
    plain = enc(gold["ids"])
    assert plain.hidden_states is None and torch.equal(plain.text_embeds, out.text_embeds)
    assert torch.equal(plain.last_hidden_state, out.last_hidden_state)
    assert enc.dtype == torch.bfloat16 and enc.device == dev() and enc.config.projection_dim == gold["cfg"]["projection_dim"]


def test_pooled_row_is_the_end_token_under_both_rules():
    """text_embeds is the projection of the END-token row of last_hidden_state: position 22 of the short prompt, 76 of the full one
    (clip_l_small: argmax rule; clip_g_small: first-match rule)."""
    from videosys_amd import clip_ops

    for name in ("clip_l_small.pt", "clip_g_small.pt"):
        gold, enc, out = run(name)
        ids = gold["ids"]
        pos = [int((ids[b] == ids.max()).nonzero()[0]) for b in range(ids.shape[0])]
        assert pos[1] == 76 and pos[0] < 76
        rows = torch.stack([out.last_hidden_state[b, p] for b, p in enumerate(pos)])
        x = torch.zeros(384, rows.shape[1], dtype=torch.bfloat16, device=dev())
        x[:len(pos)] = rows
        want = clip_ops.linear_skinny_bias_act(x, len(pos), enc.w["proj"])[:len(pos)]
        assert torch.equal(want, out.text_embeds)
