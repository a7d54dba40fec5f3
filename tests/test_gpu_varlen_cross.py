"""-m gpu: varlen cross-attention — a prompt batch whose samples have DIFFERENT token counts, the reference's
``flash_attn_varlen_func`` path (modules/attentions.py:240-258 over the packed text of open_sora_transformer_3d.py:526-537):
sample i attends to the y_lens[i] packed text rows that start at sum(y_lens[:i]).

Kernels: vsys_attn_prep_kv_varlen against what vsys_attn_prep_kv writes for every sample alone (bit for bit), and
vsys_flash_attn_d72_varlen against torch fp32 SDPA per (sample, head) (``check(..., tol=2.0**-6)``, the tolerance of
test_flash_keys_exact_promise) and against the per-sample launches it replaces (bit for bit).  Model: STDiT3.forward on a ragged CFG
batch against the oracle run PER PROMPT (an equal-length CFG pair, which it supports) under the project's stated tolerance
(fulldepth_util.verdict, factor 1.15), recorded launch programs, the pipeline / engine surface, PAB, and the batch split (enable_cp).
"""
import os

import pytest
import torch

import fulldepth_util as fu
from oracle import stdit3_oracle as O
from test_gpu_parity import check          # the project's tolerance helper: max|err| / max|ref| <= tol

pytestmark = pytest.mark.gpu

HD = 72


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


def _nan_kv(ops, batch, heads, kv_len):
    """Kp / Vt full of NaN except the Vt rows the prep contract leaves to the caller (73-75, 77-95: zero)."""
    kp, vt = ops.alloc_kv_buffers(batch, heads, kv_len, dev())
    kp.fill_(float("nan"))
    vt.fill_(float("nan"))
    vt[:, :, 73:76] = 0
    vt[:, :, 77:] = 0
    return kp, vt


def _packed(lens, heads, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    C = heads * HD
    k = (torch.randn(sum(lens), C, generator=g) * scale).to(torch.bfloat16).to(dev())
    v = torch.randn(sum(lens), C, generator=g).to(torch.bfloat16).to(dev())
    return k, v


def _prep_varlen(ops, k, v, lens, heads, w=None):
    keys = ops.VarlenKeys(lens, dev())
    kp, vt = ops.alloc_kv_buffers(len(lens), heads, max(lens), dev())
    ops.attn_prep_kv_varlen(k, v, w, keys, kp, vt, heads)
    return keys, kp, vt


# ------------------------------------------------------------------------------------------------ prep
@pytest.mark.parametrize("norm", [False, True])
def test_attn_prep_kv_varlen_equals_per_sample_prep(ops, norm):
    """Every kp[b], vt[b] is bit for bit what attn_prep_kv writes for that sample ALONE at kv_len = lens[b] into a buffer of the same
    kv_pad; behind lens[b] exactly zero.  Both sides start from NaN-poisoned buffers (zero only where the contract says the caller
    zeroes), so an element either kernel leaves unwritten fails the comparison.  k, v are column slices of a wider kv buffer."""
    lens, heads = [300, 1, 64, 65, 127, 17], 16
    C = heads * HD
    g = torch.Generator().manual_seed(3)
    kv = (torch.randn(sum(lens), 2 * C, generator=g) + 0.3).to(torch.bfloat16).to(dev())
    k, v = kv[:, :C], kv[:, C:]
    w = (1 + 0.5 * torch.randn(HD, generator=g)).to(torch.bfloat16).to(dev()) if norm else None
    keys = ops.VarlenKeys(lens, dev())
    assert keys.cu_seqlens.tolist() == [0, 300, 301, 365, 430, 557, 574] and keys.kv_lens.tolist() == lens
    kp, vt = _nan_kv(ops, len(lens), heads, max(lens))
    kv_pad = kp.shape[2]
    assert kv_pad == 320
    ops.attn_prep_kv_varlen(k, v, w, keys, kp, vt, heads)
    torch.cuda.synchronize()
    assert not torch.isnan(kp.float()).any() and not torch.isnan(vt.float()).any()
    row = 0
    for b, n in enumerate(lens):
        kp1, vt1 = _nan_kv(ops, 1, heads, kv_pad)
        ops.attn_prep_kv(k[row:row + n], v[row:row + n], w, kp1, vt1, 1, heads, n)
        torch.cuda.synchronize()
        assert torch.equal(kp[b], kp1[0]), f"Kp of sample {b} ({n} keys)"
        assert torch.equal(vt[b], vt1[0]), f"Vt of sample {b} ({n} keys)"
        assert not kp[b, :, n:].any() and not vt[b, :, :, n:].any(), f"sample {b}: something behind its {n} keys is not zero"
        ones = torch.zeros(kv_pad, dtype=torch.bfloat16, device=dev())
        ones[:n] = 1.0
        assert torch.equal(vt[b, :, 72], ones.expand(heads, -1)) and torch.equal(vt[b, :, 76], ones.expand(heads, -1))
        assert torch.equal(vt[b, :, :HD, :n], v[row:row + n].reshape(n, heads, HD).permute(1, 2, 0))
        row += n


# ------------------------------------------------------------------------------------------------ flash
def _sdpa_check(out, q, k, v, lens, heads, q_len, samples, head_ids, rows=2048):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    for b in samples:
        for h in head_ids:
            sl = slice(b * q_len, b * q_len + min(q_len, rows))
            qq = q[sl, h * HD:(h + 1) * HD].float()
            kk = k[cu[b]:cu[b + 1], h * HD:(h + 1) * HD].float()
            vv = v[cu[b]:cu[b + 1], h * HD:(h + 1) * HD].float()
            ref = O.sdpa(qq[None], kk[None], vv[None])[0]
            check(out[sl, h * HD:(h + 1) * HD], ref, tol=2.0 ** -6, what=f"varlen flash b{b} ({lens[b]} keys) h{h}")
            tail = slice(b * q_len + max(0, q_len - 64), (b + 1) * q_len)      # the last (ragged) workgroup's rows too
            ref = O.sdpa(q[tail, h * HD:(h + 1) * HD].float()[None], kk[None], vv[None])[0]
            check(out[tail, h * HD:(h + 1) * HD], ref, tol=2.0 ** -6, what=f"varlen flash b{b} h{h}, last rows")


@pytest.mark.parametrize("q_len,heads,lens", [
    (19456, 16, [300, 41, 128, 7]),      # the cross attention of config 2, CFG batch 4
    (700, 2, [300, 41, 7]),              # ragged last workgroup (700 = 2 x 256 + 188), one- to five-tile samples in one launch
    (300, 3, [65, 128]),                 # second workgroup has 44 rows; a whole-tile sample beside a ragged one
])
def test_flash_attn_varlen_vs_fp32_and_per_sample_launches(ops, q_len, heads, lens):
    """(a) fp32 SDPA per (sample, head), first / last sample and head (every one at the small shapes); (b) at the production shape
    torch.equal per sample to flash_attn(batch=1, kv_len=lens[b], keys_exact=True) on the slice kp[b:b+1], vt[b:b+1]: the same
    kernel walks the same tile sequence.  At the small shapes the per-sample launch is not the resident-K/V kernel (its launcher takes
    that kernel only where a workgroup walks several query blocks, the one-launch entry point always), and the streaming kernel it
    runs masks the last tile where the EXACT form lets the padding keys' logit 0 take part in the running max — P may be rounded at
    another scale there (test_flash_keys_exact_promise), so (a) alone applies."""
    batch, C = len(lens), heads * HD
    g = torch.Generator().manual_seed(q_len + sum(lens))
    q = torch.randn(batch * q_len, C, generator=g).to(torch.bfloat16).to(dev())
    k, v = _packed(lens, heads, q_len + 1)
    keys, kp, vt = _prep_varlen(ops, k, v, lens, heads)
    out = torch.full((batch * q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.flash_attn_varlen(q, None, kp, vt, keys, out, heads, q_len)
    out2 = torch.full_like(out, float("nan"))
    ops.flash_attn_varlen(q, None, kp, vt, keys, out2, heads, q_len)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, out2), "two launches differ (a race)"
    small = q_len < 4096
    _sdpa_check(out, q, k, v, lens, heads, q_len, range(batch) if small else (0, batch - 1),
                range(heads) if small else (0, heads - 1))
    if not small:
        for b, n in enumerate(lens):
            one = torch.full((q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
            ops.flash_attn(q[b * q_len:(b + 1) * q_len], None, kp[b:b + 1], vt[b:b + 1], one, 1, heads, q_len, n, keys_exact=True)
            torch.cuda.synchronize()
            assert torch.equal(out[b * q_len:(b + 1) * q_len], one), f"sample {b} ({n} keys) differs from its own launch"


def test_flash_attn_varlen_equal_lengths_is_the_exact_entry_point(ops):
    """All lengths equal: the buffers are bit for bit those of attn_prep_kv, the output that of vsys_flash_attn_d72_exact."""
    q_len, heads, batch, n = 19456, 16, 4, 300
    C = heads * HD
    g = torch.Generator().manual_seed(11)
    q = torch.randn(batch * q_len, C, generator=g).to(torch.bfloat16).to(dev())
    k, v = _packed([n] * batch, heads, 12)
    keys, kp, vt = _prep_varlen(ops, k, v, [n] * batch, heads)
    kp0, vt0 = ops.alloc_kv_buffers(batch, heads, n, dev())
    ops.attn_prep_kv(k, v, None, kp0, vt0, batch, heads, n)
    out = torch.full((batch * q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
    base = torch.full_like(out, float("nan"))
    ops.flash_attn_varlen(q, None, kp, vt, keys, out, heads, q_len)
    ops.flash_attn(q, None, kp0, vt0, base, batch, heads, q_len, n, keys_exact=True)
    torch.cuda.synchronize()
    assert torch.equal(kp, kp0) and torch.equal(vt, vt0)
    assert torch.equal(out, base)


def test_flash_attn_varlen_guard_answers_with_the_masked_kernels_bits(ops):
    """The all_far_negative construction of test_flash_keys_exact_promise on ONE sample of the batch (every real logit ~ -300 in the
    exp2 domain, so the padding keys' logit 0 would own the softmax): the per-block guard recomputes with the mask, and that sample
    comes out with the masked kernel's bits; its neighbours keep the bits of their own exact launch... of the masked kernel too where
    no padding key raised a max, which is not asserted — only that they are finite and inside the fp32 tolerance."""
    q_len, heads, lens = 2000, 16, [300, 300, 41]
    batch, C = len(lens), heads * HD
    g = torch.Generator().manual_seed(2300)
    q = torch.randn(batch * q_len, C, generator=g).to(torch.bfloat16)
    k = torch.randn(sum(lens), C, generator=g).to(torch.bfloat16)
    u = torch.randn(1, HD, generator=g)
    u = u / u.norm() * (300.0 * 72 ** 0.5 / 1.4427) ** 0.5
    q[q_len:2 * q_len] = (u.repeat(1, heads) + 0.1 * torch.randn(q_len, C, generator=g)).to(torch.bfloat16)
    k[300:600] = (-u.repeat(1, heads) + 0.1 * torch.randn(300, C, generator=g)).to(torch.bfloat16)
    v = torch.randn(sum(lens), C, generator=g).to(torch.bfloat16)
    q, k, v = q.to(dev()), k.to(dev()), v.to(dev())
    keys, kp, vt = _prep_varlen(ops, k, v, lens, heads)
    out = torch.full((batch * q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.flash_attn_varlen(q, None, kp, vt, keys, out, heads, q_len)
    masked = torch.full((q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.flash_attn(q[q_len:2 * q_len], None, kp[1:2], vt[1:2], masked, 1, heads, q_len, 300)     # no promise: the masked kernel
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out[q_len:2 * q_len], masked), float((out[q_len:2 * q_len].float() - masked.float()).abs().max())
    _sdpa_check(out, q, k, v, lens, heads, q_len, (0, 2), (0, heads - 1))


def test_varlen_error_returns_without_a_launch(ops):
    """A count of 0, or one past kv_pad: 'unsupported shape' from the entry point's host-side check; the output buffers keep their NaN
    poison, i.e. nothing was launched.  (No device array disagrees with its host copy here: nothing faulty reaches a kernel.)"""
    from videosys_amd._lib import VsysError

    heads, q_len = 4, 256
    C = heads * HD
    k, v = _packed([64, 64, 64], heads, 5)
    q = torch.zeros(3 * q_len, C, dtype=torch.bfloat16, device=dev())
    for lens, pad_for in (([64, 0, 64], 64), ([64, 65, 63], 64)):
        keys = ops.VarlenKeys(lens, dev())
        kp, vt = _nan_kv(ops, 3, heads, pad_for)
        out = torch.full((3 * q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
        with pytest.raises(VsysError, match="unsupported shape"):
            ops.attn_prep_kv_varlen(k, v, None, keys, kp, vt, heads)
        with pytest.raises(VsysError, match="unsupported shape"):
            ops.flash_attn_varlen(q, None, kp, vt, keys, out, heads, q_len)
        torch.cuda.synchronize()
        assert torch.isnan(kp.float()).all() and torch.isnan(out.float()).all() and torch.isnan(vt[:, :, :73].float()).all()


def test_flash_attn_varlen_falls_back_to_per_sample_launches(ops):
    """What the resident-K/V kernel does not take (here: a sample of 400 keys, more than its 320) is answered inside the entry point
    by one exact launch per sample with the host copy of the lengths: same bits as issuing those launches by hand."""
    q_len, heads, lens = 600, 2, [400, 33]
    batch, C = len(lens), heads * HD
    g = torch.Generator().manual_seed(77)
    q = torch.randn(batch * q_len, C, generator=g).to(torch.bfloat16).to(dev())
    k, v = _packed(lens, heads, 78)
    keys, kp, vt = _prep_varlen(ops, k, v, lens, heads)
    assert kp.shape[2] == 448
    out = torch.full((batch * q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.flash_attn_varlen(q, None, kp, vt, keys, out, heads, q_len)
    for b, n in enumerate(lens):
        one = torch.full((q_len, C), float("nan"), dtype=torch.bfloat16, device=dev())
        ops.flash_attn(q[b * q_len:(b + 1) * q_len], None, kp[b:b + 1], vt[b:b + 1], one, 1, heads, q_len, n, keys_exact=True)
        torch.cuda.synchronize()
        assert torch.equal(out[b * q_len:(b + 1) * q_len], one)
    _sdpa_check(out, q, k, v, lens, heads, q_len, range(batch), range(heads))


# ------------------------------------------------------------------------------------------------ STDiT3
LENS = (300, 41)


@pytest.fixture(scope="module")
def models():
    return fu.opensora_models(depth=2, seed=1234)


def _ragged_inputs(lens=LENS, seed=0, T=5, HW=16):
    """Two prompts of different length + their null halves: x [4, 4, T, HW, HW], y [4, 1, 300, 4096] without the null rows (the
    caller appends them), mask [2, 300] (the sampler hands ONE mask over for both halves)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2, 4, T, HW, HW, generator=g).to(torch.bfloat16).float()
    y = (torch.randn(2, 1, 300, 4096, generator=g) * 0.1).to(torch.bfloat16).float()
    mask = torch.zeros(2, 300, dtype=torch.long)
    for i, n in enumerate(lens):
        mask[i, :n] = 1
    px = float(HW * 8)
    geom = dict(fps=torch.tensor([24.0] * 4), height=torch.tensor([px] * 4), width=torch.tensor([px] * 4))
    return z, y, mask, geom


def _batch4(z, y, y_null):
    return torch.cat([z, z], 0), torch.cat([y, y_null.expand(2, -1, -1, -1)], 0)


T700 = torch.tensor([700.0] * 4).to(torch.bfloat16).float()


def test_stdit3_ragged_cfg_batch_vs_oracle_per_prompt(models):
    """The oracle keeps the reference's equal-length view, so it runs each prompt as its own CFG pair (fp32 = ref, torch bf16 kernels
    = floor); the product runs all four samples in one forward.  Stated tolerance per prompt — a short prompt cannot hide behind a
    long one.  Then the second prompt is swapped for another of the same token count: the first prompt's two rows must not move by a
    bit (identical launch shapes, so a difference would mean sample 0 read sample 1's keys)."""
    hip, ref, floor, y_null = models
    z, y, mask, geom = _ragged_inputs()
    x4, y4 = _batch4(z, y, y_null)
    hip.reset_text_cache()
    out = hip(x4, T700, y4, mask=mask, **geom).float()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert hip._text_cache["varlen"] is not None and hip._text_cache["varlen"].lens == LENS * 2
    for i in range(2):
        xi = torch.cat([z[i:i + 1], z[i:i + 1]], 0)
        yi = torch.cat([y[i:i + 1], y_null], 0)
        kw = dict(mask=mask[i:i + 1], fps=geom["fps"][:2], height=geom["height"][:2], width=geom["width"][:2])
        r = ref.forward(xi, T700[:2], yi, **kw)
        f = floor.forward(xi, T700[:2], yi, **kw)
        mine = out[[i, i + 2]]
        sh, sf = fu.stats(mine, r), fu.stats(f, r)
        print(f"prompt {i} ({LENS[i]} tokens): hip rel-rms {sh['rel_rms']:.4e} cos {sh['cosine']:.6f} | "
              f"floor rel-rms {sf['rel_rms']:.4e} cos {sf['cosine']:.6f}", flush=True)
        why = fu.verdict(sh, sf)
        assert why == "", f"prompt {i} ({LENS[i]} tokens): {why}"
    g = torch.Generator().manual_seed(99)
    y_b = y.clone()
    y_b[1] = (torch.randn(1, 300, 4096, generator=g) * 0.1).to(torch.bfloat16).float()
    x4b, y4b = _batch4(z, y_b, y_null)
    out_b = hip(x4b, T700, y4b, mask=mask.clone(), **geom).float()
    torch.cuda.synchronize()
    assert torch.equal(out_b[[0, 2]], out[[0, 2]]), "prompt 0's rows changed when prompt 1's text changed"
    assert not torch.equal(out_b[1], out[1])


def test_stdit3_ragged_batch_records_replays_and_is_not_served_stale(models):
    hip, _, _, y_null = models
    z, y, mask, geom = _ragged_inputs(seed=1)
    x4, y4 = _batch4(z, y, y_null)
    assert hip.use_programs
    hip.reset_text_cache()
    s0 = dict(hip.program_stats)
    a = hip(x4, T700, y4, mask=mask, **geom).float()
    b = hip(x4, T700, y4, mask=mask, **geom).float()
    s1 = dict(hip.program_stats)
    assert s1["recorded"] == s0["recorded"] + 1 and s1["replayed"] == s0["replayed"] + 1 and s1["eager"] == s0["eager"]
    hip.use_programs = False
    try:
        hip.reset_text_cache()
        e = hip(x4, T700, y4, mask=mask, **geom).float()
    finally:
        hip.use_programs = True
    torch.cuda.synchronize()
    assert torch.equal(a, e) and torch.equal(b, e), "recorded / replayed step differs from the eager forward"
    # a following ragged batch with other lengths (same tensor shapes): neither the text cache nor a recorded program may answer it
    hip.reset_text_cache()
    first = hip(x4, T700, y4, mask=mask, **geom).float()
    mask2 = torch.zeros_like(mask)
    mask2[0, :120] = 1
    mask2[1, :77] = 1
    got = hip(x4, T700, y4, mask=mask2, **geom).float()
    got2 = hip(x4, T700, y4, mask=mask2, **geom).float()
    assert hip._text_cache["varlen"].lens == (120, 77, 120, 77)
    hip.use_programs = False
    try:
        hip.reset_text_cache()
        want = hip(x4, T700, y4, mask=mask2.clone(), **geom).float()
    finally:
        hip.use_programs = True
    torch.cuda.synchronize()
    assert torch.equal(first, e)
    assert torch.equal(got, want) and torch.equal(got2, want) and not torch.equal(got, first)
    # the mask edited IN PLACE between two steps is a new prompt too (version counter)
    mask2[1, 77:90] = 1
    again = hip(x4, T700, y4, mask=mask2, **geom).float()
    torch.cuda.synchronize()
    assert hip._text_cache["varlen"].lens == (120, 90, 120, 90) and not torch.equal(again[1], got[1])
    assert torch.equal(again[[0, 2]], got[[0, 2]])


def test_stdit3_ragged_inputs_that_stay_rejected(models):
    hip, _, _, y_null = models
    z, y, mask, geom = _ragged_inputs(seed=2)
    x4, y4 = _batch4(z, y, y_null)
    hole = mask.clone()
    hole[1, 10] = 0
    hip.reset_text_cache()
    with pytest.raises(ValueError, match="prefix"):
        hip(x4, T700, y4, mask=hole, **geom)
    empty = mask.clone()
    empty[1] = 0
    with pytest.raises(ValueError, match="at least one"):
        hip(x4, T700, y4, mask=empty, **geom)
    hip.reset_text_cache()


def test_stdit3_packed_text_form_ragged(models):
    """skip_y_embedder: y is the y_embedder's output already packed [1, sum(y_lens), C] and ``mask`` carries the lengths.  Same
    result as the mask form fed with the same embedded tokens is not available without the embedder's output, so the check is the
    property the form must have: a ragged list is accepted, sample rows depend on their own text only, a wrong row count is refused."""
    hip, _, _, _ = models
    C = hip.hidden_size
    lens = [41, 300, 41, 300]
    g = torch.Generator().manual_seed(6)
    z = torch.randn(2, 4, 5, 16, 16, generator=g).to(torch.bfloat16).float()
    x4 = torch.cat([z, z], 0)
    yp = (torch.randn(1, sum(lens), C, generator=g) * 0.5).to(torch.bfloat16)
    geom = dict(fps=torch.tensor([24.0] * 4), height=torch.tensor([128.0] * 4), width=torch.tensor([128.0] * 4))
    hip.config.skip_y_embedder = True
    try:
        hip.reset_text_cache()
        a = hip(x4, T700, yp, mask=lens, **geom).float()
        yq = yp.clone()
        yq[0, 41:341] = (torch.randn(300, C, generator=g) * 0.5).to(torch.bfloat16)      # sample 1's rows only
        b = hip(x4, T700, yq, mask=lens, **geom).float()
        torch.cuda.synchronize()
        assert torch.isfinite(a).all()
        assert torch.equal(a[[0, 2, 3]], b[[0, 2, 3]]) and not torch.equal(a[1], b[1])
        with pytest.raises(ValueError, match="sum to"):
            hip(x4, T700, yp[:, :-1], mask=lens, **geom)
        with pytest.raises(ValueError, match="at least one"):
            hip(x4, T700, yp, mask=[41, 300, 0, 341], **geom)
    finally:
        hip.config.skip_y_embedder = False
        hip.reset_text_cache()


# ------------------------------------------------------------------------------------------------ pipeline / engine
P0, P1, P1B, P0B = "a cat", "big dog", "red fox", "a cow"
GEN = dict(height=128, width=128, num_frames=17, seed=5)


def _config(**kw):
    from test_gpu_pipeline import _config as base      # the SMALL synthetic geometry of the pipeline tests

    return base(**kw)


def _tokens(pipe, prompt):
    text = pipe.prepare_prompt(prompt, aes=6.5, flow=None, camera_motion=None, loop_i=0)
    _, mask = pipe.text_encoder([text])
    return int(mask.sum())


def test_pipeline_generate_ragged_prompt_batch():
    from videosys import OpenSoraPipeline, VideoSysEngine

    pipe = OpenSoraPipeline(_config())
    n0, n1, n1b, n0b = (_tokens(pipe, p) for p in (P0, P1, P1B, P0B))
    assert n0 != n1 and n1 == n1b and n0 == n0b and max(n0, n1) < 32, (n0, n1, n1b, n0b)
    lat = lambda prompts, p=pipe: p.generate(prompts, output_type="latent", **GEN).video
    a = lat([P0, P1])
    assert a.shape[0] == 2 and torch.isfinite(a.float()).all()
    assert pipe.transformer._text_cache is None or pipe.transformer._text_cache.get("varlen") is not None
    assert torch.equal(lat([P0, P1]), a), "two calls differ"
    b = lat([P0, P1B])
    assert torch.equal(b[0], a[0]), "latent 0 moved when prompt 1 was swapped for another of the same token count"
    assert not torch.equal(b[1], a[1])
    c = lat([P0B, P1])
    assert not torch.equal(c[0], a[0])
    video = pipe.generate([P0, P1], **GEN).video
    assert video.dtype == torch.uint8 and video.shape[0] == 2 and tuple(video.shape[2:]) == (128, 128, 3)
    engine = VideoSysEngine(_config())
    try:
        ev = engine.generate([P0, P1], **GEN).video
        assert torch.equal(ev, video)
        el = engine.generate(prompt=[P0, P1], output_type="latent", **GEN).video
        assert torch.equal(el, a)
    finally:
        engine.shutdown()


@pytest.mark.parametrize("mlp", [False, True])
def test_pipeline_ragged_batch_with_pab(mlp):
    """PAB keeps one cross-attention slab per BLOCK (not per sample), so a ragged batch needs nothing new: attention-only broadcast
    and the default config (MLP broadcast included), 30 steps; window of test_pab_default_config_runs_with_mlp_broadcast."""
    from videosys import OpenSoraPABConfig, OpenSoraPipeline
    from videosys_amd import pab

    kw = dict(output_type="latent", **GEN)
    try:
        extra = {} if mlp else dict(pab_config=OpenSoraPABConfig(mlp_broadcast=False))
        pipe = OpenSoraPipeline(_config(enable_pab=True, num_sampling_steps=30, **extra))
        assert pab.PAB_MANAGER.config.mlp_broadcast == mlp
        z = pipe.generate([P0, P1], **kw).video
        assert torch.isfinite(z.float()).all()
        pab.set_pab_manager(None)
        z0 = OpenSoraPipeline(_config(num_sampling_steps=30)).generate([P0, P1], **kw).video
        for i in range(2):
            cos = torch.nn.functional.cosine_similarity(z[i].flatten().float(), z0[i].flatten().float(), dim=0).item()
            assert 0.9 < cos < 1.0 - 1e-6, (i, cos)
    finally:
        pab.set_pab_manager(None)


# ------------------------------------------------------------------------------------------------ batch split (enable_cp)
def _cp_worker(rank, world, port, outdir):
    import traceback

    import torch.distributed as dist

    try:
        from videosys_amd.stdit3 import STDiT3, STDiT3Config

        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
        cfg = dict(depth=2, hidden_size=576, num_heads=8, caption_channels=64, model_max_length=16)
        sd = O.synth_state_dict(**cfg, seed=31)
        sd = {k: (v if k == "rope.freqs" else v.to(torch.bfloat16).float()) for k, v in sd.items()}
        g = torch.Generator().manual_seed(9)
        z = torch.randn(2, 4, 5, 16, 16, generator=g).to(torch.bfloat16).float()
        x = torch.cat([z, z], 0)
        y = torch.randn(4, 1, 16, 64, generator=g).to(torch.bfloat16).float()
        mask = torch.zeros(2, 16, dtype=torch.long)      # cond and null halves: equal lengths per prompt, the two prompts differ
        mask[0, :11] = 1
        mask[1, :4] = 1
        kw = dict(mask=mask, fps=torch.tensor([24.0] * 4), height=torch.tensor([128.0] * 4), width=torch.tensor([128.0] * 4))
        t = torch.tensor([500.0] * 4)
        model = STDiT3(STDiT3Config(**cfg), device="cuda:0")
        model.load_state_dict(sd)
        ref = model(x, t, y, **kw).float().cpu()
        assert model._text_cache["varlen"].lens == (11, 4, 11, 4)
        model.enable_parallel(1, world, True)
        assert model.parallel_manager.cp_size == 2 and model.parallel_manager.sp_size == 1
        out = model(x, t, y, **kw).float().cpu()
        assert model._text_cache["varlen"].lens == (11, 4), "a rank keeps its own rows of the batch, hence its own lengths"
        out2 = model(x, t, y, **kw).float().cpu()         # the replayed launch program
        torch.cuda.synchronize()
        ok = torch.equal(out, ref) and torch.equal(out2, ref)
        with open(os.path.join(outdir, f"r{rank}.txt"), "w") as f:
            f.write("ok" if ok else f"mismatch max|diff| {(out - ref).abs().max().item()} of {ref.abs().max().item()}")
    except Exception:
        with open(os.path.join(outdir, f"r{rank}.txt"), "w") as f:
            f.write(traceback.format_exc())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_stdit3_ragged_batch_split_two_processes_equals_single():
    from test_gpu_sp import _run      # the worker harness of the sequence-parallel tests (spawn, per-process timeout, result files)

    _run(_cp_worker, (), world=2, timeout=300)
