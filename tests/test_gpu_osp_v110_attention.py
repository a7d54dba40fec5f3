"""-m gpu: the head-dim-72 RoPE attention of Open-Sora-Plan v1.1 (csrc/attention.hip: open_sora_plan_v110_ops.attn_prep_kv_rope +
flash_attn_rope) bit for bit against its contract, element-wise against a float64 softmax (tests/numerics.py attention_ref, one bound
per output element), and ops.attn_temporal in its rope-only mode against the float64 rotate-half reference.

Contract (include/videosys_amd.h).  fp32 tables [tokens, 36], entry p of a row rotates the columns (2p, 2p + 1) of every head:
    q^[2p] = bf16(fp32(q[2p] c) - fp32(q[2p+1] s)),            q^[2p+1] = bf16(fp32(q[2p+1] c) + fp32(q[2p] s))
    k^[2p] = bf16((fp32(k[2p] c) - fp32(k[2p+1] s)) KSCALE),   k^[2p+1] likewise with +
two fp32 products, one fp32 sum, nothing fused, ONE rounding; everything else is ops.attn_prep_kv / ops.flash_attn.  So
  * identity tables (cos 1, sin 0) give the bits of the plain entry points on inputs without zeros (x 1 - y 0 = x exactly);
  * rotating q on the CPU in fp32 with separate mul / add and one .to(bf16), then calling the plain flash kernel, gives the same bits
    as the roped kernel on the un-rotated q.  For k the plain prep cannot stand in the same way: it would round the rotated row to
    bf16 and round again after KSCALE, where the contract has ONE rounding — so Kp of the roped prep is compared with the fp32
    restatement (rotation, KSCALE, one rounding), the way tests/test_gpu_osp_attention.py pins the d96 prep kernel, and Vt, the ones
    rows and the zero padding with what the plain prep writes;
  * the element-wise bound takes the K / V images the kernel reads as given (they are pinned bit for bit) and gives q^ the error
    eq = acc(2, |q c| + |q' s|) + rnd(q^)."""
import math

import pytest
import torch

import attn_families as fam
import numerics as nm
import osp_v110_ref as ref110

pytestmark = pytest.mark.gpu

HD, PAIRS = 72, 36
KSCALE = torch.tensor(0.11785113019775793, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)   # the kernels' fp32 constant
# (q_len, kv_len).  The last two are whole-tile key counts >= 512, where the roped launcher runs its THREE-workgroup instantiation
# (flash_attn_d72_kernel<ABL_ROPE, 3>: no masked tile, the next tile's LDS-DMA pieces between the QK MFMAs) — the kernel of the real
# model's 1 024 keys per frame; everything shorter or ragged runs the two-workgroup one.  8 and 9 key tiles, two query blocks each.
SHAPES = [(1, 1), (33, 63), (64, 64), (129, 65), (200, 130), (130, 512), (200, 576)]


def plain_variant(kv_len):
    """The flash variant id that puts the PLAIN entry point on the kernel form the roped launcher takes at this key count: 3 = the
    three-workgroup streaming kernel (whole tiles, >= 512 keys), 10 = the streaming kernel, never the resident one."""
    return 3 if kv_len >= 512 and kv_len % 64 == 0 else 10
B, H = 2, 3


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vops():
    from videosys_amd import open_sora_plan_v110_ops as o

    return o


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


def tables(n, seed):
    """fp32 (cos, sin) [n, 36] of true rotations: one random angle per (token, pair) in [0, 6)."""
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(n, PAIRS, generator=g) * 6.0
    return ang.cos().contiguous(), ang.sin().contiguous()


def rot(x, cos, sin):
    """Interleaved-pair rotation, operation by operation in the dtype of x (fp32: the kernels' arithmetic; float64: the reference).
    x [..., L, 72], cos / sin [L, 36]."""
    a, b = x[..., 0::2], x[..., 1::2]
    ac, bs, bc, as_ = a * cos, b * sin, b * cos, a * sin
    return torch.stack([ac - bs, bc + as_], dim=-1).flatten(-2)


def rot_err(x, cos, sin):
    a, b = x[..., 0::2].abs(), x[..., 1::2].abs()
    c, s = cos.abs(), sin.abs()
    return nm.acc(2, torch.stack([a * c + b * s, b * c + a * s], dim=-1).flatten(-2))


def to_rows(x, batch, heads):
    L = x.shape[1]
    return x.view(batch, heads, L, HD).permute(0, 2, 1, 3).reshape(batch * L, heads * HD).contiguous()


def from_rows(x, batch, heads):
    L = x.shape[0] // batch
    return x.view(batch, L, heads, HD).permute(0, 2, 1, 3).reshape(batch * heads, L, HD)


def nonzero_bf16(shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) + offset).to(torch.bfloat16)
    x[x == 0] = 1.0
    return x


def prep(fn, k, v, Lk, *tabs):
    d = dev()
    from videosys_amd import ops as o

    kp, vt = o.alloc_kv_buffers(B, H, Lk, d)
    fn(to_rows(k, B, H).to(d), to_rows(v, B, H).to(d), *[t.to(d) for t in tabs], kp, vt, B, H, Lk)
    torch.cuda.synchronize()
    return kp, vt


@pytest.mark.parametrize("Lq,Lk", SHAPES, ids=lambda p: str(p))
def test_identity_tables_give_the_plain_kernels_bits(vops, ops, Lq, Lk):
    n = B * H
    q, k, v = nonzero_bf16((n, Lq, HD), Lq), nonzero_bf16((n, Lk, HD), Lk + 1), nonzero_bf16((n, Lk, HD), Lk + 2, 0.5)
    one, zero = torch.ones(max(Lq, Lk), PAIRS), torch.zeros(max(Lq, Lk), PAIRS)
    kp0, vt0 = prep(lambda k_, v_, kp, vt, *a: ops.attn_prep_kv(k_, v_, None, kp, vt, *a), k, v, Lk)
    kp1, vt1 = prep(vops.attn_prep_kv_rope, k, v, Lk, one[:Lk].contiguous(), zero[:Lk].contiguous())
    assert torch.equal(kp0.view(torch.int16), kp1.view(torch.int16)) and torch.equal(vt0.view(torch.int16), vt1.view(torch.int16))
    d = dev()
    q2 = to_rows(q, B, H).to(d)
    o0 = torch.full((B * Lq, H * HD), float("nan"), dtype=torch.bfloat16, device=d)
    o1 = o0.clone()
    lib = __import__("videosys_amd._lib", fromlist=["load"]).load()
    assert lib.vsys_tune_flash_variant(plain_variant(Lk)) == 0        # the plain entry point on the kernel form the roped one runs here
    try:
        ops.flash_attn(q2, None, kp0, vt0, o0, B, H, Lq, Lk)
        torch.cuda.synchronize()
    finally:
        lib.vsys_tune_flash_variant(0)
    vops.flash_attn_rope(q2, one[:Lq].contiguous().to(d), zero[:Lq].contiguous().to(d), kp1, vt1, o1, B, H, Lq, Lk)
    torch.cuda.synchronize()
    assert not torch.isnan(o1.float()).any()
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))


@pytest.mark.parametrize("Lq,Lk", SHAPES, ids=lambda p: str(p))
def test_pre_rotated_operands_give_the_same_bits(vops, ops, Lq, Lk):
    """q rotated on the CPU (fp32, separate mul / add, one .to(bf16)) through the plain flash kernel == the roped kernel on q; Kp of
    the roped prep == bf16(rot_fp32(k) * KSCALE), Vt and the padding as the plain prep writes them."""
    n = B * H
    q, k, v = nonzero_bf16((n, Lq, HD), 3 * Lq), nonzero_bf16((n, Lk, HD), 3 * Lk + 1), nonzero_bf16((n, Lk, HD), 3 * Lk + 2, 0.5)
    cq, sq = tables(Lq, Lq + 7)
    ck, sk = tables(Lk, Lk + 8)
    kp, vt = prep(vops.attn_prep_kv_rope, k, v, Lk, ck, sk)
    want = (rot(k.float(), ck, sk) * KSCALE).to(torch.bfloat16)
    kp_c = kp.cpu().view(n, -1, HD)
    assert torch.equal(kp_c[:, :Lk].view(torch.int16), want.view(torch.int16)), "Kp is not the fp32-computed, once-rounded rotation"
    assert not kp_c[:, Lk:].view(torch.int16).any(), "Kp rows behind kv_len are not zero"
    kp0, vt0 = prep(lambda k_, v_, kp_, vt_, *a: ops.attn_prep_kv(k_, v_, None, kp_, vt_, *a), k, v, Lk)
    assert torch.equal(vt.view(torch.int16), vt0.view(torch.int16)), "Vt (transpose, ones rows, zero padding) differs from attn_prep_kv's"
    d = dev()
    q_rot = rot(q.float(), cq, sq).to(torch.bfloat16)
    o0 = torch.full((B * Lq, H * HD), float("nan"), dtype=torch.bfloat16, device=d)
    o1 = o0.clone()
    lib = __import__("videosys_amd._lib", fromlist=["load"]).load()
    assert lib.vsys_tune_flash_variant(plain_variant(Lk)) == 0
    try:
        ops.flash_attn(to_rows(q_rot, B, H).to(d), None, kp, vt, o0, B, H, Lq, Lk)
        torch.cuda.synchronize()
    finally:
        lib.vsys_tune_flash_variant(0)
    vops.flash_attn_rope(to_rows(q, B, H).to(d), cq.to(d), sq.to(d), kp, vt, o1, B, H, Lq, Lk)
    torch.cuda.synchronize()
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))


def make_case(family, n, Lq, Lk, cq, sq, ck, sk, seed):
    """q [n, Lq, 72], k, v [n, Lk, 72] bf16.  Retrieval: key norms sqrt(72), q_i = 4 x (k_t as the kernel sees it, turned back by the
    query's own rotation): the target's logit is 4 * 72 KSCALE = 49 against |others| <~ 27 (the figures of the normed retrieval cases
    of tests/test_gpu_numerics_attention.py, whose q chain has two roundings as well)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(n, Lk, HD, generator=g) + 0.5).to(torch.bfloat16)
    if family == "diffuse":
        return torch.randn(n, Lq, HD, generator=g).to(torch.bfloat16), torch.randn(n, Lk, HD, generator=g).to(torch.bfloat16), v, None, None
    k = torch.randn(n, Lk, HD, generator=g)
    k = (k * (HD**0.5 / k.norm(dim=-1, keepdim=True))).to(torch.bfloat16)
    kr = rot(k.double(), ck.double(), sk.double())
    t = fam.target_order(Lk)[(torch.arange(Lq) * 7 + 3) % Lk]
    u = rot(kr[:, t], cq.double(), -sq.double())        # the inverse of the query's rotation
    q = (4.0 * u).to(torch.bfloat16)
    targets = t[None, :, None].expand(n, Lq, 1).contiguous()
    return q, k, v, targets, torch.gather(v.double(), 1, targets.expand(n, Lq, HD))


def check(out, ref, what, expect=None, v=None):
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


def run_elementwise(vops, family, Lq, Lk, cq, sq, ck, sk, seed, what):
    n = B * H
    q, k, v, targets, expect = make_case(family, n, Lq, Lk, cq, sq, ck, sk, seed)
    kp, vt = prep(vops.attn_prep_kv_rope, k, v, Lk, ck, sk)
    kpd = kp[:, :, :Lk].double().reshape(n, Lk, HD).cpu()                      # the images the kernel reads (pinned bit for bit above)
    vd = vt[:, :, :HD, :Lk].transpose(-1, -2).double().reshape(n, Lk, HD).cpu()
    qh = rot(q.double(), cq.double(), sq.double())
    eq = rot_err(q.double(), cq.double(), sq.double()) + nm.rnd(qh)
    ref = nm.attention_ref(qh, kpd, vd, eq=eq, targets=targets)
    if family == "retrieval":
        fam.check_targets(ref, dict(expect=expect), what)
    d = dev()
    out = torch.full((B * Lq, H * HD), float("nan"), dtype=torch.bfloat16, device=d)
    vops.flash_attn_rope(to_rows(q, B, H).to(d), cq.to(d), sq.to(d), kp, vt, out, B, H, Lq, Lk)
    torch.cuda.synchronize()
    check(from_rows(out.cpu(), B, H), ref, what, expect, vd)


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("Lq,Lk", SHAPES, ids=lambda p: str(p))
def test_flash_rope_elementwise(vops, Lq, Lk, family):
    cq, sq = tables(Lq, 11 * Lq)
    ck, sk = tables(Lk, 13 * Lk)
    run_elementwise(vops, family, Lq, Lk, cq, sq, ck, sk, 100 * Lq + Lk, f"flash d72 rope {family} q{Lq} kv{Lk}")


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
def test_flash_rope_elementwise_model_tables(vops, family):
    """The model's own bf16-made 2-D tables of a 5 x 7 token grid (self attention: one table for q and k)."""
    from videosys_amd import open_sora_plan_v110 as m

    cos, sin = m.rope_tables_2d(5, 7, 1.0)
    assert cos.shape == (35, PAIRS) and cos.dtype == torch.float32
    run_elementwise(vops, family, 35, 35, cos, sin, cos, sin, 57, f"flash d72 rope {family} 5x7 grid")


# ------------------------------------------------------------------------------------------------ temporal, rope-only mode
@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("T", [1, 5, 17, 32, 33, 57])
def test_attn_temporal_rope_only_on_permuted_columns(ops, T, family):
    """ops.attn_temporal with tables and no norm weights on q / k whose columns were permuted inside each head (new (2p, 2p + 1) = old
    (p, p + 36)) against the float64 rotate-half attention of the un-permuted q / k (RoPE1D, open_sora_plan_v110_transformer_3d.py
    :199-253).  Rounding chain of the kernel (ops.attn_temporal): the rotation and q * 72^-1/2 each rounded to bf16 at most."""
    from videosys_amd import open_sora_plan_v110 as m

    S, Bt = 3, 1
    C = H * HD
    N = Bt * S * H
    g = torch.Generator().manual_seed(1000 + T)
    cos, sin = m.rope_tables_1d(T, 1.0)                     # [T, 72] fp32, pair p at columns 2p, 2p + 1
    c64, s64 = cos[:, 0::2].double(), sin[:, 0::2].double()  # [T, 36]
    perm = m.head_permutation_1d()
    v = (torch.randn(N, T, HD, generator=g) + 0.5).to(torch.bfloat16)
    if family == "diffuse":
        q, k = torch.randn(N, T, HD, generator=g).to(torch.bfloat16), torch.randn(N, T, HD, generator=g).to(torch.bfloat16)
        targets = expect = None
    else:
        k = torch.randn(N, T, HD, generator=g)
        k = (k * (HD**0.5 / k.norm(dim=-1, keepdim=True))).to(torch.bfloat16)
        kr = ref110.rope_1d(k.double(), c64, s64)
        t = fam.target_order(T)[(torch.arange(T) * 7 + 3) % T]
        q = (4.0 * ref110.rope_1d(kr[:, t], c64, -s64)).to(torch.bfloat16)
        targets = t[None, :, None].expand(N, T, 1).contiguous()
        expect = torch.gather(v.double(), 1, targets.expand(N, T, HD))
    scale = HD**-0.5
    qh = ref110.rope_1d(q.double(), c64, s64)
    kh = ref110.rope_1d(k.double(), c64, s64)
    rerr = lambda x: nm.acc(2, x.abs() * torch.cat([c64, c64], -1).abs() + ref110.rotate_half(x).abs() * torch.cat([s64, s64], -1).abs())
    eq = scale * (rerr(q.double()) + nm.rnd(qh)) + nm.rnd(qh * scale)
    ek = rerr(k.double()) + nm.rnd(kh)
    ref = nm.attention_ref(qh * scale, kh, v.double(), eq=eq, ek=ek, log2_scale=math.log2(math.e), denominator="fp32", targets=targets)
    what = f"attn_temporal rope-only {family} T={T}"
    if family == "retrieval":
        fam.check_targets(ref, dict(expect=expect), what)
    # device layout: rows (b, t, s), columns q | k | v with head h at h * 72; slice n = (b, s, h)
    lay = lambda x: x.view(Bt, S, H, T, HD).permute(0, 3, 1, 2, 4).reshape(Bt * T * S, C)
    qkv = torch.cat([lay(q[..., perm]), lay(k[..., perm]), lay(v)], dim=1).contiguous().to(dev())
    out = torch.full((Bt * T * S, C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.attn_temporal(qkv, C, None, None, cos.to(dev()), sin.to(dev()), out, Bt, T, S, H)
    torch.cuda.synchronize()
    o = out.cpu().view(Bt, T, S, H, HD).permute(0, 2, 3, 1, 4).reshape(N, T, HD)
    check(o, ref, what, expect, v.double())
