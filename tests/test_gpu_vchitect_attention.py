"""-m gpu: the three attentions of VchitectAttnProcessor and the `* 1.1 +` combine, every output element against float64 softmax
attention (tests/vchitect_ref.py, the restatement of attentions.py:641-949) with the per-element bound of tests/numerics.py
(attention_ref), unchanged.  Output buffers are NaN before every launch.

Temporal (vchitect_ops.attn_temporal64, attention_t64.hip).  q^ / k^ = the interleaved-pair rotation in fp32 rounded to bf16 (eq / ek
= acc(2) + one rounding, as q_chain64 of tests/test_gpu_numerics_attention.py), natural-domain logits times 1/8, P unrounded, one
division: the "fp32" form of the bound with tile = 4 (the kernel adopts its running maximum once per 4 keys).  B = 2, heads = 3 (one
wave of the workgroup has no head), S + L = 16 + 5 = 21, video rows a column slice of a fused qkv buffer (stride 3 C), text rows
slices of three separate buffers (stride C + 16), outputs with strides of their own.  T crosses every boundary of the kernel:
  1   one key: a 4-key group with three masked keys, one query lane         3   a partial group
  19  five groups, the last partial                                          32  exactly one K / V chunk (8 full groups)
  33  a second chunk of ONE key: the rescale across chunks                   41  second chunk with a partial group
  64  two full chunks, all 64 query lanes of a pass                          65  a second query pass of one query, three chunks
each with RoPE (theta = 1e6 tables of the reference) and with NULL tables.

Joint spatial and cross attention run on the EXISTING head-dim-64 kernels (ops.attn_prep_kv64 + ops.flash_attn64) with no qk-norm and
no RoPE, at S = 64, L = 8 (72 keys: one ragged 64-key tile), T = 3, heads = 3, B = 2.  K^ = bf16(k log2(e) / 8) (ek = one rounding).
Cross: the keys are cross_keys() of the restatement — frame 0 of sample 0, dealt out over the B samples as the reference's view does
(L / B = 4 keys per sample) — and the `(S T)` query order needs no pass: attention is row-wise in the queries, so the video rows
(batch B, q_len T S) and the text rows (batch B, q_len T L) are two launches over the same prepared keys.
The combine is compared bit for bit with the two bf16 torch ops."""
import math

import pytest
import torch

import numerics as nm
import vchitect_ref as vr
from test_gpu_numerics_attention import check_stack, vacuous_rows

pytestmark = pytest.mark.gpu

HD = 64
LOG2E = math.log2(math.e)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


@pytest.fixture(scope="module")
def vops():
    from videosys_amd import vchitect_ops as o

    return o


def rand_bf16(g, *shape, offset=0.0):
    return (torch.randn(*shape, generator=g) + offset).to(torch.bfloat16)


def heads_major(x, H):
    """[N, L, H, 64] -> [N * H, L, 64]"""
    return x.transpose(1, 2).reshape(-1, x.shape[1], HD)


TEMPORAL_T = [1, 3, 19, 32, 33, 41, 64, 65]


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("T", TEMPORAL_T)
def test_attn_temporal64_elementwise(vops, T, rope):
    B, H, S, L = 2, 3, 16, 5
    C, SL = H * HD, S + L
    g = torch.Generator().manual_seed(1000 + T)
    qkv = rand_bf16(g, B * T * S, 3 * C)
    qkv[:, 2 * C:] += 0.5
    txt = [torch.zeros(B * T * L, C + 16, dtype=torch.bfloat16) for _ in range(3)]
    for i, t in enumerate(txt):
        t[:, 8:8 + C] = rand_bf16(g, B * T * L, C, offset=0.5 if i == 2 else 0.0)
    qkv_d, txt_d = qkv.to(dev()), [t.to(dev()) for t in txt]
    vid = [qkv_d[:, i * C:(i + 1) * C] for i in range(3)]
    tx = [t[:, 8:8 + C] for t in txt_d]
    cos = sin = None
    if rope:
        cos, sin = (t.to(dev()) for t in vr.rope_tables(T))
    # ---- float64 reference on the device from the bf16-exact operands
    d3 = lambda x, n: x.double().reshape(B * T, n, C)
    q, k, v = (vr.temporal_tokens(d3(a, S), d3(b, L), B, T, H) for a, b in zip(vid, tx))       # [B * SL, T, H, 64]
    eq = ek = None
    qh, kh = q, k
    if rope:
        cd, sd = cos.double(), sin.double()               # the fp32 tables the kernel reads, exactly
        qh, kh = vr.apply_rotary(q, cd, sd), vr.apply_rotary(k, cd, sd)
        eq, ek = heads_major(vr.rotary_error(q, cd, sd), H), heads_major(vr.rotary_error(k, cd, sd), H)
    ref = nm.attention_ref(heads_major(qh, H), heads_major(kh, H), heads_major(v, H), eq=eq, ek=ek, log2_scale=LOG2E / 8,
                           denominator="fp32", tile=4)
    what = f"attn_temporal64 B{B} T{T} S{S}+L{L} H{H} rope={rope}"
    vacuous_rows(ref, what)
    # the restatement's own temporal_attention (rotation left unrounded) is the same function: ties attention_ref to the line-by-line text
    rv, rt = vr.temporal_attention(d3(vid[0], S), d3(vid[1], S), d3(vid[2], S), d3(tx[0], L), d3(tx[1], L), d3(tx[2], L),
                                   cos.double() if rope else None, sin.double() if rope else None, B, T, H, round_rope=False)
    rs = heads_major(vr.temporal_tokens(rv, rt, B, T, H), H)
    assert (rs - ref.out).abs().max().item() < 1e-12
    # ---- the kernel
    out_vid_buf = torch.full((B * T * S, C + 8), float("nan"), dtype=torch.bfloat16, device=dev())
    out_vid = out_vid_buf[:, :C]
    out_txt = torch.full((B * T * L, C), float("nan"), dtype=torch.bfloat16, device=dev())
    vops.attn_temporal64(vid[0], vid[1], vid[2], tx[0], tx[1], tx[2], cos, sin, out_vid, out_txt, B, T, S, L, H)
    torch.cuda.synchronize()
    assert torch.isnan(out_vid_buf[:, C:]).all(), "columns behind the video output were written"
    o = heads_major(vr.temporal_tokens(out_vid.reshape(B * T, S, C), out_txt.reshape(B * T, L, C), B, T, H), H)
    check_stack(o, ref, what)
    if T == 1:      # one key: the output is v, bit for bit
        assert torch.equal(out_vid, vid[2]) and torch.equal(out_txt, tx[2])


def test_attn_temporal64_video_only_and_text_only(vops):
    """S = 0 or L = 0: that side's pointers are NULL and are not read; the other side's result is the one of the joint call."""
    B, H, S, L, T = 1, 2, 7, 3, 5
    C = H * HD
    g = torch.Generator().manual_seed(7)
    vid = [rand_bf16(g, B * T * S, C).to(dev()) for _ in range(3)]
    tx = [rand_bf16(g, B * T * L, C).to(dev()) for _ in range(3)]
    cos, sin = (t.to(dev()) for t in vr.rope_tables(T))
    new = lambda n: torch.full((B * T * n, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ov, ot, ov2, ot2 = new(S), new(L), new(S), new(L)
    vops.attn_temporal64(*vid, *tx, cos, sin, ov, ot, B, T, S, L, H)
    vops.attn_temporal64(*vid, None, None, None, cos, sin, ov2, None, B, T, S, 0, H)
    vops.attn_temporal64(None, None, None, *tx, cos, sin, None, ot2, B, T, 0, L, H)
    torch.cuda.synchronize()
    assert not torch.isnan(ov).any() and not torch.isnan(ot).any()
    assert torch.equal(ov, ov2) and torch.equal(ot, ot2)


# ------------------------------------------------------------------------------------------------ joint spatial, cross, combine
@pytest.fixture(scope="module")
def joint_case():
    B, T, S, L, H = 2, 3, 64, 8, 3
    C = H * HD
    g = torch.Generator().manual_seed(64 + 8)
    t = {n: rand_bf16(g, B * T * (S if n.endswith("vid") else L), C, offset=0.5 if n[0] == "v" else 0.0).to(dev())
         for n in ("q_vid", "k_vid", "v_vid", "q_txt", "k_txt", "v_txt")}
    return dict(B=B, T=T, S=S, L=L, H=H, C=C, **t)


def d3(x, n):
    return x.double().reshape(-1, n, x.shape[-1])


def run_spatial(ops, c):
    B, T, S, L, H, C = (c[k] for k in "BTSLHC")
    SL = S + L
    joint = lambda a, b: torch.cat([a.view(B * T, S, C), b.view(B * T, L, C)], dim=1).reshape(B * T * SL, C)
    q2, k2, v2 = joint(c["q_vid"], c["q_txt"]), joint(c["k_vid"], c["k_txt"]), joint(c["v_vid"], c["v_txt"])
    kp, vt = ops.alloc_kv_buffers64(B * T, H, SL, dev())
    ops.attn_prep_kv64(k2, v2, None, None, None, None, 0, kp, vt, B * T, H, SL)
    out = torch.full((B * T * SL, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.flash_attn64(q2, None, None, None, None, 0, kp, vt, out, B * T, H, SL, SL)
    torch.cuda.synchronize()
    return out, (q2, k2, v2)


def run_cross(ops, c):
    B, T, S, L, H, C = (c[k] for k in "BTSLHC")
    Lk = L // B
    kp, vt = ops.alloc_kv_buffers64(B, H, Lk, dev())
    ops.attn_prep_kv64(c["k_txt"][:L], c["v_txt"][:L], None, None, None, None, 0, kp, vt, B, H, Lk)      # frame 0 of sample 0, B runs of L / B
    ov = torch.full((B * T * S, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ot = torch.full((B * T * L, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.flash_attn64(c["q_vid"], None, None, None, None, 0, kp, vt, ov, B, H, T * S, Lk)
    ops.flash_attn64(c["q_txt"], None, None, None, None, 0, kp, vt, ot, B, H, T * L, Lk)
    torch.cuda.synchronize()
    return ov, ot


def kp_operand(k):
    """(K^, ek) of attn_prep_kv64 without norm and RoPE: k log2(e) / 8 rounded to bf16 once."""
    kh = k * (LOG2E / 8)
    return kh, nm.rnd(kh)


def test_joint_spatial_attention_elementwise(ops, joint_case):
    c = joint_case
    B, T, S, L, H, C = (c[k] for k in "BTSLHC")
    SL = S + L
    out, (q2, k2, v2) = run_spatial(ops, c)
    hm = lambda x: heads_major(x.double().view(B * T, SL, H, HD), H)
    kh, ek = kp_operand(hm(k2))
    ref = nm.attention_ref(hm(q2), kh, hm(v2), ek=ek, denominator="fp32")
    what = f"joint spatial attention B{B} T{T} S{S}+L{L} H{H}"
    vacuous_rows(ref, what)
    want = vr.spatial_attention(*(d3(c[n], S if n.endswith("vid") else L) for n in ("q_vid", "k_vid", "v_vid", "q_txt", "k_txt", "v_txt")), H)
    assert (hm(want) - ref.out).abs().max().item() < 1e-12         # attention_ref computes the restatement's function
    check_stack(hm(out), ref, what)


def test_cross_attention_elementwise(ops, joint_case):
    c = joint_case
    B, T, S, L, H, C = (c[k] for k in "BTSLHC")
    ov, ot = run_cross(ops, c)
    ky, vy = vr.cross_keys(d3(c["k_txt"], L), d3(c["v_txt"], L), B, H)           # [B, L / B, H, 64]
    want = vr.cross_attention(d3(c["q_vid"], S), d3(c["q_txt"], L), d3(c["k_txt"], L), d3(c["v_txt"], L), B, T, H)   # [B*T, S+L, C]
    for name, o, n, w in (("video", ov, S, want[:, :S]), ("text", ot, L, want[:, S:])):
        q = heads_major(c["q_" + ("vid" if name == "video" else "txt")].double().view(B, T * n, H, HD), H)
        kh, ek = kp_operand(heads_major(ky, H))
        ref = nm.attention_ref(q, kh, heads_major(vy, H), ek=ek, denominator="fp32")
        what = f"cross attention ({name} queries) B{B} T{T} S{S} L{L} H{H}"
        vacuous_rows(ref, what)
        assert (heads_major(w.reshape(B, T * n, H, HD), H) - ref.out).abs().max().item() < 1e-12
        check_stack(heads_major(o.view(B, T * n, H, HD), H), ref, what)


def test_combine_is_the_two_bf16_ops(ops, vops, joint_case):
    """hidden = spatial * 1.1 + cross on the kernels' own outputs, bit for bit the two bf16 tensor ops of the reference — on tight
    tensors, on row-strided views, and in place."""
    c = joint_case
    B, T, S, L, H, C = (c[k] for k in "BTSLHC")
    spatial, _ = run_spatial(ops, c)
    ov, ot = run_cross(ops, c)
    sp3 = spatial.view(B * T, S + L, C)
    a = sp3[:, :S].reshape(-1, C)                                       # the video rows of the joint spatial output
    want = a * 1.1 + ov                                                  # two bf16 ops (torch rounds after each)
    assert torch.equal(want, vr.combine_bf16(a, ov))
    got = vops.scale_add_rows(a, ov, 1.1)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the joint spatial buffer read in place through row-strided views (frame f: rows f (S + L) .. + S), text rows likewise
    flat = spatial.clone()
    for f in range(B * T):
        rows = flat[f * (S + L): f * (S + L) + S]
        vops.scale_add_rows(rows, ov[f * S:(f + 1) * S], 1.1, out=rows)
        trow = flat[f * (S + L) + S:(f + 1) * (S + L)]
        vops.scale_add_rows(trow, ot[f * L:(f + 1) * L], 1.1, out=trow)
    wide = torch.full((B * T * S, C + 24), float("nan"), dtype=torch.bfloat16, device=dev())
    vops.scale_add_rows(a, ov, 1.1, out=wide[:, 8:8 + C])
    torch.cuda.synchronize()
    f3 = flat.view(B * T, S + L, C)
    assert torch.equal(f3[:, :S].reshape(-1, C).view(torch.int16), want.view(torch.int16))
    want_t = sp3[:, S:].reshape(-1, C) * 1.1 + ot
    assert torch.equal(f3[:, S:].reshape(-1, C).view(torch.int16), want_t.view(torch.int16))
    assert torch.equal(wide[:, 8:8 + C].view(torch.int16), want.view(torch.int16))
    assert torch.isnan(wide[:, :8]).all() and torch.isnan(wide[:, 8 + C:]).all()
