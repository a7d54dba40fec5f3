"""-m gpu: ops.attn_temporal past 64 frames (csrc/attention_tlong.hip: 32 x 32 frame blocks on the matrix pipe, running maximum).
Element-wise against float64 softmax attention with the bounds, families and non-vacuity conditions of
tests/test_gpu_numerics_attention.py, at the block edges (65, 96 / 97, 129), the Open-Sora 16 s length (120) and past the 284 frames
the VALU kernel stops at (285, 300: refused before this kernel existed); then through a one-block STDiT3 at T = 120."""
import pytest
import torch

import attn_families as fam
import numerics as nm
from test_gpu_numerics_attention import FREQS, HD, LOG2E, check_stack, dev, temporal_chain, temporal_inputs, vacuous_rows

pytestmark = pytest.mark.gpu

LONG_CASES = [  # (B, T, S, H, norm, rope): H = 3 is one partial head group, 16 four full ones
    (1, 65, 9, 3, True, True), (1, 65, 70, 3, False, True), (1, 96, 70, 3, False, False), (1, 96, 9, 16, True, True),
    (1, 97, 9, 16, False, True), (2, 120, 9, 16, True, True), (1, 120, 70, 3, False, False), (1, 129, 9, 3, True, True),
    (1, 285, 9, 3, True, True), (1, 285, 9, 16, False, False), (1, 300, 9, 16, False, True), (1, 300, 70, 3, True, True),
]


def long_reference(family, B, T, S, H, norm, rope, device):
    """Inputs and the float64 reference of one case on ``device`` (the GPU in the test; the CPU when the cases are screened)."""
    q, k, v, qw, kw, pi = temporal_inputs(family, B, T, S, H, norm, rope, 100 * T + S + H)
    cos = sin = cosd = sind = None
    if rope:
        ang = (torch.arange(T, dtype=torch.float32)[:, None] * FREQS).repeat_interleave(2, dim=-1)
        cos, sin = ang.cos().contiguous().to(device), ang.sin().contiguous().to(device)
        cosd, sind = cos.double(), sin.double()
    qwd, kwd = (None if w is None else w.to(device).double() for w in (qw, kw))
    qh, eq = temporal_chain(q.to(device).double(), qwd, cosd, sind, HD**-0.5)
    kh, ek = temporal_chain(k.to(device).double(), kwd, cosd, sind, None)
    N = B * S * H
    targets = None if pi is None else pi.reshape(N, T, 1).to(device)
    vd = v.to(device).double().reshape(N, T, HD)
    ref = nm.attention_ref(qh.reshape(N, T, HD), kh.reshape(N, T, HD), vd, eq=eq.reshape(N, T, HD), ek=ek.reshape(N, T, HD),
                           log2_scale=LOG2E, denominator="fp32", targets=targets)
    what = f"{family} B{B} T{T} S{S} H{H} norm={norm} rope={rope}"
    vacuous_rows(ref, what, family == "retrieval" and norm)      # (the rule of test_gpu_numerics_attention.py's docstring)
    vt = None
    if targets is not None:
        vt = torch.gather(vd.view(B, S, H, T, HD), 3, pi.to(device)[..., None].expand(B, S, H, T, HD)).reshape(N, T, HD)
        fam.check_targets(ref, dict(expect=vt), what)
    return (q, k, v, qw, kw, cos, sin), ref, vt, vd, what


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("B,T,S,H,norm,rope", LONG_CASES)
def test_attn_temporal_long_elementwise(B, T, S, H, norm, rope, family):
    from videosys_amd import _lib, ops

    lib, C, N = _lib.load(), H * HD, B * S * H
    (q, k, v, qw, kw, cos, sin), ref, vt, vd, what = long_reference(family, B, T, S, H, norm, rope, dev())
    qkv = torch.stack([q, k, v], dim=3).permute(0, 4, 1, 3, 2, 5).reshape(B * T * S, 3 * C).contiguous().to(dev())
    qwg, kwg = (None if w is None else w.to(dev()) for w in (qw, kw))
    for variant in (0, 9) if T <= 284 else (0,):      # 9 = the VALU kernel, which holds 284 frames at the most
        out = torch.full((B * T * S, C), float("nan"), dtype=torch.bfloat16, device=dev())
        assert lib.vsys_tune_flash_variant(variant) == 0
        try:
            ops.attn_temporal(qkv, C, qwg, kwg, cos, sin, out, B, T, S, H)
            torch.cuda.synchronize()
        finally:
            lib.vsys_tune_flash_variant(0)
        o = out.view(B, T, S, H, HD).permute(0, 2, 3, 1, 4).reshape(N, T, HD)
        check_stack(o, ref, f"attn_temporal [variant {variant}] {what}", vt, vd)


def test_stdit3_block_at_the_16s_length():
    """One STDiT3 block (hidden 576 = 8 x 72, 2 x 2 tokens per frame) at the 120 latent frames of the 16 s preset: within 1.5 x the
    bf16 floor of the oracle (the oracle in bf16 against itself in fp32) on the block-loop kernel and on the VALU kernel (variant 9),
    and the two within the floor of each other."""
    from fulldepth_util import bf16_round, stats
    from oracle import stdit3_oracle as O
    from videosys_amd import _lib
    from videosys_amd.stdit3 import STDiT3, STDiT3Config

    lib = _lib.load()
    cfg = dict(depth=1, hidden_size=576, num_heads=8, caption_channels=64, model_max_length=16)
    sd = bf16_round(O.synth_state_dict(**cfg, seed=77))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 120, 4, 4, generator=g).to(torch.bfloat16).float()
    y = torch.randn(2, 1, 16, 64, generator=g).to(torch.bfloat16).float()
    mask = torch.zeros(1, 16, dtype=torch.long)
    mask[:, :11] = 1
    kw = dict(mask=mask, fps=torch.tensor([24.0, 24.0]), height=torch.tensor([32.0, 32.0]), width=torch.tensor([32.0, 32.0]))
    t = torch.tensor([500.0, 500.0])
    ref, floor = (O.STDiT3Oracle(sd, cfg["depth"], cfg["hidden_size"], cfg["num_heads"], device="cuda:0", dtype=d).forward(x, t, y, **kw)
                  for d in (torch.float32, torch.bfloat16))
    floor_rms = stats(floor, ref)["rel_rms"]
    model = STDiT3(STDiT3Config(**cfg), device="cuda:0")
    model.load_state_dict(sd)
    outs = {}
    for variant in (0, 9):
        assert lib.vsys_tune_flash_variant(variant) == 0
        try:
            outs[variant] = model(x, t, y, **kw).float()
            torch.cuda.synchronize()
        finally:
            lib.vsys_tune_flash_variant(0)
        rms = stats(outs[variant], ref)["rel_rms"]
        print(f"[stdit3 T=120] variant {variant}: rel-rms {rms:.3e}, bf16 floor {floor_rms:.3e}")
        assert rms <= 1.5 * floor_rms, (variant, rms, floor_rms)
    between = stats(outs[0], outs[9])["rel_rms"]
    print(f"[stdit3 T=120] variant 0 against 9: rel-rms {between:.3e}")
    assert between <= floor_rms, (between, floor_rms)
