"""-m gpu: the head-dim-96 attention kernels of Open-Sora-Plan v1.2 (csrc/attention96.hip: ops attn_prep_kv96 + flash_attn96)
element-wise against a float64 softmax (tests/numerics.py: attention_ref, one bound per output element), and the prep kernel bit for
bit against its fp32 restatement.

Contract (include/videosys_amd.h, attention96.hip).  Per-token fp32 tables [tokens, 96]; inside each 32-column chunk
out = x cos + rotate_half(x) sin, rotate_half = (-x[16:32], x[0:16]):
    q^ = bf16(fp32(q cos) + fp32(rot(q) sin))                       eq = acc(2, |q cos| + |rot(q) sin|) + rnd(q^)
    k^ = bf16((fp32(k cos) + fp32(rot(k) sin)) * KSCALE)            ek = KSCALE acc(2, |k cos| + |rot(k) sin|) + acc(1, |k^|) + rnd(k^)
(two products, one sum, the softmax scale KSCALE = fp32(96^-0.5) * fp32(log2 e) on K, ONE rounding; without tables q is the operand
bit for bit and k^ = bf16(k KSCALE)).  Logits in the exp2 domain with a running maximum adopted every 64-key tile, P rounded to bf16
for P V, the row sum from the fp32 p ("fp32" form of attention_ref), one division, one rounding.

Families (d96 copies of tests/attn_families.py): diffuse — every key matters a little; retrieval — query i is 3.5 times key t(i) as
the kernel will see it (un-rotated by the query's own position), t walking the tile edges first: asserted on the float64 reference
(weight >= 1 - 2^-12 on the target) before the case is trusted, then the output must be v[t(i)].  Cross-attention cases put large
finite garbage into the K / V rows past a sample's count, so a read past the count shows."""
import math

import pytest
import torch

import attn_families as fam
import numerics as nm
import osp_ref

pytestmark = pytest.mark.gpu

HD = 96
KSCALE = float(torch.tensor(96**-0.5, dtype=torch.float32) * torch.tensor(math.log2(math.e), dtype=torch.float32))   # the kernel's fp32 constant


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def oops():
    from videosys_amd import open_sora_plan_ops as o

    return o


def tables(n, seed):
    """fp32 (cos, sin) [n, 96] of true rotations: one random angle per (token, chunk, pair), shared by columns i and i + 16."""
    g = torch.Generator().manual_seed(seed)
    ang = (torch.rand(n, 3, 16, generator=g) * 6.0).repeat(1, 1, 2).reshape(n, HD)
    return ang.cos().contiguous(), ang.sin().contiguous()


def rope(x, cos, sin):
    return x * cos + osp_ref.rotate_half_chunks(x) * sin


def rope_err(x, cos, sin):
    return nm.acc(2, (x * cos).abs() + (osp_ref.rotate_half_chunks(x) * sin).abs())


def q_chain96(q, cos, sin):
    """(q^, eq) in float64; q [..., L, 96], cos / sin [L, 96] float64 or None."""
    if cos is None:
        return q, None
    h = rope(q, cos, sin)
    return h, rope_err(q, cos, sin) + nm.rnd(h)


def k_chain96(k, cos, sin):
    h, e = (k, torch.zeros_like(k)) if cos is None else (rope(k, cos, sin), rope_err(k, cos, sin))
    kh = h * KSCALE
    return kh, KSCALE * e + nm.acc(1, kh.abs()) + nm.rnd(kh)


def prep_restated(k, cos, sin):
    """attn_prep_kv96's K image in torch fp32, operation by operation, rounded once: bf16 [..., L, 96]."""
    x = k.float()
    if cos is not None:
        x = x * cos.float() + osp_ref.rotate_half_chunks(x) * sin.float()
    return (x * torch.tensor(KSCALE, dtype=torch.float32)).to(torch.bfloat16)


def to_rows(x, B, H):
    """[B * H, L, 96] -> [B * L, H * 96]."""
    L = x.shape[1]
    return x.view(B, H, L, HD).permute(0, 2, 1, 3).reshape(B * L, H * HD).contiguous()


def from_rows(x, B, H):
    L = x.shape[0] // B
    return x.view(B, L, H, HD).permute(0, 2, 1, 3).reshape(B * H, L, HD)


def make_case(family, n, Lq, Lk, cos_q, sin_q, cos_k, sin_k, seed, lens=None, B=1):
    """q [n, Lq, 96], k, v [n, Lk, 96] bf16 on the CPU, targets [n, Lq, 1] / expect or None.  Retrieval: key norms sqrt(96), q_i = 3.5 x
    (k_t as the kernel sees it, turned back by the query's own rotation): the target's logit is 3.5 * 96 KSCALE = 49 against |others|
    <~ 20, and the worst case of the q and k rounding chains together (2 x 2^-8 x 49 = 0.39 binades) leaves every row a finite
    element bound — at gain 6 (logits of 85) it does not.  Slice s belongs to sample s // (n / B) and its targets stay below that
    sample's count."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(n, Lk, HD, generator=g) + 0.5).to(torch.bfloat16)
    if family == "diffuse":
        return torch.randn(n, Lq, HD, generator=g).to(torch.bfloat16), torch.randn(n, Lk, HD, generator=g).to(torch.bfloat16), v, None, None
    k = torch.randn(n, Lk, HD, generator=g)
    k = (k * (HD**0.5 / k.norm(dim=-1, keepdim=True))).to(torch.bfloat16)
    kd = k.double()
    kr = kd if cos_k is None else rope(kd, cos_k.double(), sin_k.double())
    q, targets = torch.empty(n, Lq, HD, dtype=torch.bfloat16), torch.empty(n, Lq, 1, dtype=torch.int64)
    for s in range(n):
        cnt = Lk if lens is None else lens[s // (n // B)]
        t = fam.target_order(cnt)[(torch.arange(Lq) * 7 + 3) % cnt]
        u = kr[s, t]
        if cos_q is not None:
            u = rope(u, cos_q.double(), -sin_q.double())       # the inverse rotation
        q[s], targets[s, :, 0] = (3.5 * u).to(torch.bfloat16), t
    expect = torch.gather(v.double(), 1, targets.expand(n, Lq, HD))
    return q, k, v, targets, expect


def check(out, ref, what, expect=None, v=None):
    """One Bound over the slices; retrieval: the output is also the target's v (tests/test_gpu_numerics_attention.py::check_stack)."""
    assert ref.vacuous == 0, f"{what}: {ref.vacuous} rows have no finite element bound"
    L, D = ref.out.shape[-2:]
    if expect is not None:
        off = ((1 - ref.weight).clamp_min(0) * torch.exp2(2 * ref.ds_max)).clamp_max(1.0)[..., None]
        allow = 2.0**-7 * expect.abs() + off * (v.abs().amax(dim=-2, keepdim=True) + expect.abs()) + nm.FLOOR
        bad = ~((out.double().reshape(expect.shape) - expect).abs() <= allow)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements are not the target keys' v"
    rep = nm.Bound(what).add(out.reshape(-1, D), ref.out.reshape(-1, D), ref.bound.reshape(-1, D))
    if rep.bad:
        row = rep.worst[1]
        raise AssertionError(f"{rep.message()} — slice {row // L}, row {row % L} of it")
    assert rep.total == ref.out.numel()


def run_prep(oops, k, v, cos, sin, B, H, Lk):
    """prep on the device + the bit-exact check of both images; returns (kp, vt) on the device."""
    d = dev()
    kp, vt = oops.alloc_kv_buffers96(B, H, Lk, d)
    kp.fill_(float("nan")), vt.fill_(float("nan"))            # every element of both images is the kernel's to write
    oops.attn_prep_kv96(to_rows(k, B, H).to(d), to_rows(v, B, H).to(d), None if cos is None else cos.to(d), None if sin is None else sin.to(d),
                        kp, vt, B, H, Lk)
    torch.cuda.synchronize()
    kp_c, vt_c = kp.cpu().view(B * H, -1, HD), vt.cpu().view(B * H, HD, -1)
    want = prep_restated(k, cos, sin)
    assert torch.equal(kp_c[:, :Lk].view(torch.int16), want.view(torch.int16)), "Kp is not the fp32-computed, once-rounded rotation"
    assert torch.equal(vt_c[:, :, :Lk].transpose(1, 2).contiguous().view(torch.int16), v.view(torch.int16)), "Vt is not the transpose of v"
    assert not kp_c[:, Lk:].view(torch.int16).any() and not vt_c[:, :, Lk:].view(torch.int16).any(), "padded keys are not zero"
    return kp, vt


SELF_CASES = [((3, 4, 6), 2), ((2, 5, 13), 3), ((1, 8, 8), 2)]        # 72 = a full tile + 8, 130 = two tiles + 2 and two q-blocks, 64 exactly


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("rope_on", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("thw,H", SELF_CASES, ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else f"H{p}")
def test_flash_d96_self_elementwise(oops, thw, H, rope_on, family):
    B, N = 2, thw[0] * thw[1] * thw[2]
    n = B * H
    cos, sin = tables(N, N + H) if rope_on else (None, None)
    q, k, v, targets, expect = make_case(family, n, N, N, cos, sin, cos, sin, seed=N + 10 * H + rope_on)
    kp, vt = run_prep(oops, k, v, cos, sin, B, H, N)
    c64, s64 = (None, None) if cos is None else (cos.double(), sin.double())
    qh, eq = q_chain96(q.double(), c64, s64)
    kh, ek = k_chain96(k.double(), c64, s64)
    ref = nm.attention_ref(qh, kh, v.double(), eq=eq, ek=ek, targets=targets, denominator="fp32")
    what = f"flash d96 self {family} B{B} H{H} {thw} rope={rope_on}"
    if family == "retrieval":
        fam.check_targets(ref, dict(expect=expect), what)
    d = dev()
    out = torch.full((B * N, H * HD), float("nan"), dtype=torch.bfloat16, device=d)
    oops.flash_attn96(to_rows(q, B, H).to(d), None if cos is None else cos.to(d), None if sin is None else sin.to(d), kp, vt, None, out,
                      B, H, N, N)
    torch.cuda.synchronize()
    check(from_rows(out.cpu(), B, H), ref, what, expect, v.double())


CROSS_CASES = [(8, (8, 5)), (64, (64, 1)), (77, (77, 64)), (130, (130, 65)), (8, None), (77, None), (130, None)]


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("Lk,lens", CROSS_CASES, ids=lambda p: str(p).replace(" ", ""))
def test_flash_d96_cross_elementwise(oops, Lk, lens, family):
    """q_len 72 against Lk text keys, no rotation; kv_lens read on the device (None: every key).  The K / V rows past a sample's count
    hold +-300 / 1000: finite, as the contract asks of masked keys, and ruinous if one of them is read as a key."""
    B, H, Lq = 2, 2, 72
    n = B * H
    q, k, v, targets, expect = make_case(family, n, Lq, Lk, None, None, None, None, seed=Lk + (0 if lens is None else 7), lens=lens, B=B)
    if lens is not None:
        for s in range(n):
            cnt = lens[s // H]
            k[s, cnt:] = 300.0 * (1 - 2 * (torch.arange(Lk - cnt) % 2))[:, None].to(torch.bfloat16)
            v[s, cnt:] = 1000.0
    kp, vt = run_prep(oops, k, v, None, None, B, H, Lk)
    d = dev()
    kv_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=d)
    out = torch.full((B * Lq, H * HD), float("nan"), dtype=torch.bfloat16, device=d)
    oops.flash_attn96(to_rows(q, B, H).to(d), None, None, kp, vt, kv_lens, out, B, H, Lq, Lk)
    torch.cuda.synchronize()
    o = from_rows(out.cpu(), B, H)
    for b in range(B):
        cnt = Lk if lens is None else lens[b]
        sl = slice(b * H, (b + 1) * H)
        kh, ek = k_chain96(k[sl, :cnt].double(), None, None)
        tg = None if targets is None else targets[sl]
        ref = nm.attention_ref(q[sl].double(), kh, v[sl, :cnt].double(), ek=ek, targets=tg, denominator="fp32")
        what = f"flash d96 cross {family} Lk={Lk} lens={lens} sample {b}"
        if family == "retrieval":
            fam.check_targets(ref, dict(expect=expect[sl]), what)
        check(o[sl], ref, what, None if expect is None else expect[sl], v[sl, :cnt].double())
