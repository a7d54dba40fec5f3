"""-m gpu: the attention kernels, every output element of every (batch, head), against float64 softmax attention with the per-element
bound of tests/numerics.py (attention_ref), on the input families of tests/attn_families.py.  The output buffer is NaN before every
launch; the reference runs on the GPU in float64 and is computed once per case, then shared by every kernel variant of that case.

d72 flash (ops.flash_attn, ops.flash_attn_varlen).  The reference reads back the Kp and Vt images attn_prep_kv wrote (pinned by
test_gpu_numerics_attn_io.py::test_attn_prep_kv_contract), so what is tested is the flash kernel alone: q^ = bf16(bf16(q rstd) w)
(numerics.rms_q_chain; q bit for bit without norm), logits in the exp2 domain, P to bf16, row sum from the same rounded P (the ones
rows of Vt): the "rounded" form of the bound.  Kernels are picked with vsys_tune_flash_variant: 10 streaming, 8 resident (with and
without the keys_exact promise), 3 three workgroups per CU, 14 w64 one item, 16 w64 persistent, 17 / 18 the same two without a
running maximum (ops.rms_key_bound), 0 the default dispatch — each wherever the launcher really takes it for the shape.

Temporal (ops.attn_temporal).  q^ and k^ follow the reference's rounding points (attention_t3.hip t3_piece, RP: x rstd -> bf16, w ->
bf16, rotation -> bf16, q scale -> bf16), which is variant 21; the single-rounding default (0 / 22) and the VALU kernels (4, 9) pass
as "fewer roundings".  The weights are normalised in fp32 and then rounded to bf16 (as the reference's attn.to(dtype)): the "fp32"
form of the bound.  Retrieval through RoPE: <R_t q, R_s k> = <q, R_(s-t) k>, so q_t is the counter-rotated k_pi(t); the norm weights
are equal within each rotary pair, so the weight commutes with the rotation.

CogVideoX d64 (ops.attn_prep_kv64 + ops.flash_attn64).  Joint [text | video] sequence, rope_start = the text length (not a
multiple of 64).  K^ is the Kp image read back with its 16-byte chunk swizzle undone, V the Vt image; q^ = bf16(rope(bf16(LN(q) w +
b))).  The 32-row kernel (default below 2048 keys, variant 12) adds the row sum up from the fp32 P before the cast while the
rounded P feeds the PV product: the "fp32" form; the w64 stream (14, 17, default from 2048 keys) takes the sum from the rounded P on
the matrix pipe: the "rounded" form.  Retrieval is built in the post-LayerNorm, post-RoPE domain: q is the target's K^ counter-rotated
by the query's own position and pushed back through the affine map of the norm.

T5 (ops.t5_attention_mfma, ops.t5_attention).  No 1/sqrt(d); the relative-position bias is the additive logit term of the reference
(the d64 flash kernel with the bias hook: "fp32" form).  Diffuse, and a bias-dominant family: one relative position per head carries
the row (retrieval through the bias table).

A row whose P error bound reaches 1 (AttnRef.vacuous) gets no finite element bound.  Every case asserts that it has none, except the
temporal retrieval cases with norm: their logits of 49 are fixed by the norm weights and pass seven bf16 roundings, so the worst case
of the chain exceeds a binade on every row.  Those rows are held by the expected-value check alone (its allowance is built from the
same logit error); temporal retrieval WITHOUT norm (gain 3.5: logits of 43) and every d72 / d64 retrieval case keep a finite bound.
"""
import math

import pytest
import torch

import attn_families as fam
import numerics as nm

pytestmark = pytest.mark.gpu

HD = 72
LOG2E = math.log2(math.e)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


@pytest.fixture(scope="module")
def lib():
    from videosys_amd import _lib

    return _lib.load()


def norm_weight(seed, centre, spread, pairs=False):
    g = torch.Generator().manual_seed(seed)
    w = centre * (1 + spread * torch.randn(HD // 2 if pairs else HD, generator=g))
    return (w.repeat_interleave(2) if pairs else w).to(torch.bfloat16)


def vacuous_rows(ref, what, allowed=False):
    """Rows without a finite element bound (AttnRef.vacuous: P error bound >= 1).  None anywhere, except where ``allowed``: the temporal
    retrieval cases WITH norm (seven bf16 roundings around logits of 49, which the norm weights fix: the worst case of the chain is
    more than a binade).  There the count is printed, and the rows rest on the expected-value check."""
    rows = ref.out.numel() // ref.out.shape[-1]
    if ref.vacuous:
        print(f"[vacuous] {what}: {ref.vacuous} of {rows} rows have no finite element bound (held by the expected-value check)")
    assert ref.vacuous == 0 or allowed, f"{what}: {ref.vacuous} of {rows} rows have no finite element bound"


def check_stack(out, ref, what, expect=None, v=None, targets=None):
    """out / ref.out / ref.bound [..., L, D]: one Bound over all slices; the failure names the slice of the worst element.
    ``expect`` (retrieval, two-key; ``v`` [..., Lk, D] the values): the output is also the targets' v, to one bf16 rounding (2^-7 |v|
    covers the tie cases) plus what the keys off target can add.  The reference gives them 1 - weight of the row; the kernel's logits
    differ from the reference's by at most ds_max, so its off-target weight is at most (1 - weight) 2^(2 ds_max), spread over
    |v_j - expect| <= max_j |v_jd| + |expect_d|: an allowance per row from the case itself, no constant.  Two targets: their two
    weights are rounded to bf16 separately (different tiles, different adopted maxima): 2 x 2^-8 of |v_target - expect| on top."""
    L, D = ref.out.shape[-2:]
    if expect is not None:
        exp = expect.to(out.device)
        off = ((1 - ref.weight).clamp_min(0) * torch.exp2(2 * ref.ds_max)).clamp_max(1.0)[..., None]
        allow = 2.0**-7 * exp.abs() + off * (v.abs().amax(dim=-2, keepdim=True) + exp.abs()) + nm.FLOOR
        if targets is not None and targets.shape[-1] > 1:
            tv = torch.stack([torch.gather(v, -2, targets[..., i:i + 1].expand(*targets.shape[:-1], D)) for i in range(targets.shape[-1])])
            allow = allow + 2 * (nm.U_BF16 + nm.U_EXP) * (tv - exp).abs().amax(dim=0)
        bad = ~((out.double().reshape(exp.shape) - exp).abs() <= allow)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements are not the target keys' v"
    rep = nm.Bound(what).add(out.reshape(-1, D), ref.out.reshape(-1, D), ref.bound.reshape(-1, D))
    if rep.bad:
        row = rep.worst[1]
        raise AssertionError(f"{rep.message()} — slice {row // L}, row {row % L} of it")
    assert rep.total == ref.out.numel()


# ------------------------------------------------------------------------------------------------ d72 flash
def to_rows(x, batch, heads):
    """[batch * heads, L, 72] -> the 2-D layout of the ops: [batch * L, heads * 72]."""
    L = x.shape[1]
    return x.view(batch, heads, L, HD).permute(0, 2, 1, 3).reshape(batch * L, heads * HD).contiguous()


def from_rows(x, batch, heads):
    L = x.shape[0] // batch
    return x.view(batch, L, heads, HD).permute(0, 2, 1, 3).reshape(batch * heads, L, HD)


def default_branch(batch, heads, q_len, kv_len, bounded, ncu):
    """The kernel launch_flash_attn_d72 takes at variant 0 (attention.hip), from its rule."""
    if (kv_len + 63) // 64 <= 5:
        nqb = (q_len + 255) // 256
        chunks = min(max(ncu // (batch * heads), 1), nqb)
        if nqb >= 2 * chunks:
            return "resident"
    if kv_len >= 2048 and q_len >= 256:
        return "w64-static" if bounded else "w64"
    return "wps3" if kv_len >= 512 and kv_len % 64 == 0 else "wps2"


def flash_variants(q_len, kv_len, norm, kb):
    """(label, variant, k_norm_bound, keys_exact) for every kernel the launcher really runs at this shape."""
    w64 = kv_len >= 256 and q_len >= 256
    whole = kv_len % 64 == 0
    v = [("streaming", 10, None, False)]
    if kv_len <= 320:
        v += [("resident", 8, None, False), ("resident-exact", 8, None, True)]
    if whole:
        v.append(("wps3", 3, None, False))
    if w64:
        v.append(("w64", 14, None, False))
        if norm and kb:
            v.append(("w64-static", 17, kb, False))
        if whole:
            v.append(("w64p", 16, None, False))
            if norm and kb:
                v.append(("w64p-static", 18, kb, False))
    return v


# (q_len, kv_len, batch, heads, norm, default branch on a 256-CU part).  Every q_len of {1, 127, 128, 129, 255, 256, 257, 300, 513} and every kv_len
# of {1, 63, 64, 65, 129, 192, 300, 320, 321, 448, 512, 1024, 2064} appears, each with the diffuse and the retrieval family (two_key and
# ramps join where the shape allows: a ragged second tile / five tiles).
FLASH_SHAPES = [
    (1, 1, 2, 2, False, "wps2"), (127, 63, 2, 2, True, "wps2"), (128, 64, 2, 2, False, "wps2"), (129, 65, 2, 2, True, "wps2"),
    (255, 129, 2, 2, False, "wps2"), (256, 192, 2, 2, True, "wps2"), (257, 300, 2, 2, False, "wps2"), (300, 320, 2, 2, True, "wps2"),
    (513, 321, 2, 2, False, "wps2"), (513, 300, 2, 2, True, "wps2"), (127, 448, 2, 2, True, "wps2"), (257, 512, 2, 2, False, "wps3"),
    (256, 512, 2, 2, True, "wps3"), (513, 1024, 2, 2, True, "wps3"), (129, 1024, 2, 2, False, "wps3"), (300, 2064, 2, 2, True, "w64-static"),
    (257, 2064, 2, 2, False, "w64"), (300, 300, 3, 5, True, "wps2"), (300, 448, 3, 5, False, "wps2"),
    (513, 300, 16, 16, False, "resident"),      # 256 (batch, head) pairs: one chunk each, three query blocks -> the default takes the resident kernel
]


def flash_id(s):
    return f"q{s[0]}-kv{s[1]}-b{s[2]}h{s[3]}-{'norm' if s[4] else 'raw'}-default:{s[5]}"


def test_flash_d72_cases_reach_every_default_branch():
    """The case ids name the branch of a 256-CU part; with the CU count of THIS device every branch must still have a case."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    reached = {default_branch(s[2], s[3], s[0], s[1], s[4], ncu) for s in FLASH_SHAPES}
    assert reached == {"resident", "w64", "w64-static", "wps3", "wps2"}, reached


@pytest.mark.parametrize("shape", FLASH_SHAPES, ids=flash_id)
def test_flash_d72_elementwise(ops, lib, shape):
    q_len, kv_len, batch, heads, norm, branch = shape
    big = batch * heads > 64
    n = batch * heads
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for family in ("diffuse", "retrieval") if big else fam.FAMILIES:
        if (family == "two_key" and (kv_len <= 64 or kv_len % 64 == 0)) or (family == "ramps" and (kv_len < 320 or norm)):
            continue
        peaked = family in ("retrieval", "two_key")
        qw = kw = kb = None
        if norm:   # weights of about 2 for the peaked families (product 4: the target leads by tens of binades, rms_key_bound still holds)
            qw, kw = (norm_weight(s, 2.0 if peaked else 1.0, 0.02 if peaked else 0.1).to(dev()) for s in (q_len, kv_len + 1))
            kb = ops.rms_key_bound(qw, kw)
            assert kb is not None
        kwargs = {"gain": 1.0} if (norm and peaked) else {}
        cases = [fam.FAMILIES[family](q_len, kv_len, 1000 * q_len + kv_len + 17 * i, **kwargs) for i in range(n)]
        q3, k3, v3 = (torch.stack([c[key] for c in cases]).to(dev()) for key in ("q", "k", "v"))
        q2, k2, v2 = to_rows(q3, batch, heads), to_rows(k3, batch, heads), to_rows(v3, batch, heads)
        kp, vt = ops.alloc_kv_buffers(batch, heads, kv_len, dev())
        ops.attn_prep_kv(k2, v2, kw, kp, vt, batch, heads, kv_len)
        torch.cuda.synchronize()
        # ---- reference from the images the kernel reads
        kpd = kp[:, :, :kv_len].double().reshape(n, kv_len, HD)
        vd = vt[:, :, :HD, :kv_len].transpose(-1, -2).double().reshape(n, kv_len, HD)
        qh, eq = nm.rms_q_chain(q3.double(), None if qw is None else qw.double())
        targets = torch.stack([c["targets"] for c in cases]).to(dev()) if peaked else None
        m_extra = qh.norm(dim=-1) * kb if kb else None
        ref = nm.attention_ref(qh, kpd, vd, eq=eq, targets=targets, m_extra=m_extra)
        what = f"{family} {flash_id(shape)}"
        vacuous_rows(ref, what)
        if peaked:
            fam.check_targets(ref, dict(expect=torch.stack([c["expect"] for c in cases])), what)
        if family == "ramps":
            fam.check_ladders(ref.logits, cases[0]["levels"], what)
        # ---- every kernel of this shape against it
        runs = [(f"default({default_branch(batch, heads, q_len, kv_len, bool(kb), ncu)})", 0, kb, False)] + ([] if big else flash_variants(q_len, kv_len, norm, kb))
        if kb and not big:
            runs.append(("default, no promise", 0, None, False))
        for label, variant, bound, exact in runs:
            out = torch.full((batch * q_len, heads * HD), float("nan"), dtype=torch.bfloat16, device=dev())
            assert lib.vsys_tune_flash_variant(variant) == 0
            try:
                ops.flash_attn(q2, qw, kp, vt, out, batch, heads, q_len, kv_len, k_norm_bound=bound, keys_exact=exact)
                torch.cuda.synchronize()
            finally:
                lib.vsys_tune_flash_variant(0)
            check_stack(from_rows(out, batch, heads), ref, f"flash d72 [{label}] {what}",
                        torch.stack([c["expect"] for c in cases]) if peaked else None, vd, targets)


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
def test_flash_d72_varlen_elementwise(ops, lib, family, norm):
    """One launch, four samples with 1, 64, 65 and 300 keys: each sample against its own reference (variant 0: the resident exact
    kernel reading the counts on the device; variant 10: the per-sample launches the entry point falls back to)."""
    lens, heads, q_len = (1, 64, 65, 300), 2, 257
    batch = len(lens)
    qw = kw = None
    if norm:
        qw, kw = (norm_weight(s, 2.0 if family == "retrieval" else 1.0, 0.02).to(dev()) for s in (5, 6))
    kwargs = {"gain": 1.0} if (norm and family == "retrieval") else {}
    cases = [[fam.FAMILIES[family](q_len, L, 77 * L + h, **kwargs) for h in range(heads)] for L in lens]
    q2 = to_rows(torch.stack([c["q"] for row in cases for c in row]).to(dev()), batch, heads)
    k2 = torch.cat([torch.cat([c["k"] for c in row], dim=1) for row in cases]).to(dev())          # packed rows
    v2 = torch.cat([torch.cat([c["v"] for c in row], dim=1) for row in cases]).to(dev())
    keys = ops.VarlenKeys(lens, dev())
    kp, vt = ops.alloc_kv_buffers(batch, heads, max(lens), dev())
    ops.attn_prep_kv_varlen(k2, v2, kw, keys, kp, vt, heads)
    torch.cuda.synchronize()
    refs = []
    for b, L in enumerate(lens):
        q3 = torch.stack([c["q"] for c in cases[b]]).to(dev()).double()
        qh, eq = nm.rms_q_chain(q3, None if qw is None else qw.double())
        targets = torch.stack([c["targets"] for c in cases[b]]).to(dev()) if family == "retrieval" else None
        ref = nm.attention_ref(qh, kp[b, :, :L].double(), vt[b, :, :HD, :L].transpose(-1, -2).double(), eq=eq, targets=targets)
        vacuous_rows(ref, f"varlen {family} sample {b} ({L} keys)")
        if targets is not None:
            fam.check_targets(ref, dict(expect=torch.stack([c["expect"] for c in cases[b]])), f"varlen sample {b} ({L} keys)")
        refs.append(ref)
    for variant in (0, 10):
        out = torch.full((batch * q_len, heads * HD), float("nan"), dtype=torch.bfloat16, device=dev())
        assert lib.vsys_tune_flash_variant(variant) == 0
        try:
            ops.flash_attn_varlen(q2, qw, kp, vt, keys, out, heads, q_len)
            torch.cuda.synchronize()
        finally:
            lib.vsys_tune_flash_variant(0)
        o3 = from_rows(out, batch, heads).view(batch, heads, q_len, HD)
        for b, L in enumerate(lens):
            check_stack(o3[b], refs[b], f"flash d72 varlen [variant {variant}] {family} sample {b} ({L} keys)",
                        torch.stack([c["expect"] for c in cases[b]]) if family == "retrieval" else None,
                        vt[b, :, :HD, :L].transpose(-1, -2).double())


# ------------------------------------------------------------------------------------------------ temporal
FREQS = 1.0 / (10000 ** (torch.arange(0, HD, 2).float() / HD))


def rotate(x, delta):
    """R_delta x on interleaved pairs; delta [..., T] frames (any sign), x [..., T, 72]."""
    ang = (delta[..., None].to(x.dtype) * FREQS.to(x)).repeat_interleave(2, dim=-1)
    x1, x2 = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    rot = torch.stack((-x2, x1), dim=-1).reshape(x.shape)
    return x * ang.cos() + rot * ang.sin()


def temporal_chain(x, w, cos, sin, scale, eps=1e-6):
    """(operand, error bound) of a temporal q / k row in float64 along the reference's rounding points (t3_piece, RP = true)."""
    h, e = x, torch.zeros_like(x)
    if w is not None:
        nrm = x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps)
        h = nrm * w
        e = (nm.rnd(nrm) + nm.acc(HD, nrm.abs())) * w.abs() + nm.rnd(h)
    if cos is not None:
        swap = lambda t: t.reshape(*t.shape[:-1], -1, 2).flip(-1).reshape(t.shape)
        h1, h2 = h.reshape(*h.shape[:-1], -1, 2).unbind(-1)
        rot = torch.stack((-h2, h1), dim=-1).reshape(h.shape)
        hr = h * cos + rot * sin
        e = e * cos.abs() + swap(e) * sin.abs() + nm.acc(2, (h * cos).abs() + (rot * sin).abs()) + nm.rnd(hr)
        h = hr
    if scale is not None:
        h = h * scale
        e = e * scale + nm.rnd(h)
    return h, e


def temporal_inputs(family, B, T, S, H, norm, rope, seed):
    """q, k, v [B, S, H, T, 72] bf16 (CPU), the norm weights, and pi [B, S, H, T] (retrieval) or None."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, S, H, T, HD)
    peaked = family == "retrieval"
    qw = kw = None
    if norm:
        qw, kw = (norm_weight(seed + i, 2.0 if peaked else 1.0, 0.02 if peaked else 0.1, pairs=True) for i in (1, 2))
    v = (torch.randn(shape, generator=g) + 0.5).to(torch.bfloat16)
    if not peaked:
        return torch.randn(shape, generator=g).to(torch.bfloat16), torch.randn(shape, generator=g).to(torch.bfloat16), v, qw, kw, None
    k = torch.randn(shape, generator=g)
    k = (k * (HD**0.5 / k.norm(dim=-1, keepdim=True))).to(torch.bfloat16)
    # pi: a rotation of the frames by a shift that differs from problem to problem (every frame is some query's target; shifts of
    # 0, 1 and T - 1 occur, so the first and the last frame and both sides of frame 32 are hit from near and far)
    shift = (torch.arange(B * S * H).view(B, S, H, 1) * 7) % T
    t = torch.arange(T).view(1, 1, 1, T)
    pi = (t + shift) % T
    kt = torch.gather(k.float(), 3, pi[..., None].expand(shape))
    q = (1.0 if norm else (3.5 if rope else 6.0)) * (rotate(kt, (pi - t).expand(B, S, H, T)) if rope else kt)
    return q.to(torch.bfloat16), k, v, qw, kw, pi


TEMPORAL_CASES = [  # (B, T, S, H, norm, rope)
    (1, 1, 9, 16, True, True), (1, 2, 70, 3, True, False), (1, 31, 9, 16, False, True), (1, 32, 70, 3, True, True),
    (1, 33, 9, 16, False, False), (1, 33, 70, 16, True, True), (1, 40, 70, 3, True, True), (1, 41, 9, 16, True, False),
    (1, 63, 70, 3, False, True), (2, 64, 9, 16, True, True), (2, 64, 9, 3, False, False), (1, 65, 70, 3, True, True),
    (1, 65, 9, 16, False, False),
]


@pytest.mark.parametrize("family", ["diffuse", "retrieval"])
@pytest.mark.parametrize("B,T,S,H,norm,rope", TEMPORAL_CASES)
def test_attn_temporal_elementwise(ops, lib, B, T, S, H, norm, rope, family):
    C = H * HD
    q, k, v, qw, kw, pi = temporal_inputs(family, B, T, S, H, norm, rope, 100 * T + S + H)
    # rows ordered (b, t, s), columns (q | k | v) x head x 72
    qkv = torch.stack([q, k, v], dim=3).permute(0, 4, 1, 3, 2, 5).reshape(B * T * S, 3 * C).contiguous().to(dev())
    cos = sin = cosd = sind = None
    if rope:
        ang = (torch.arange(T, dtype=torch.float32)[:, None] * FREQS).repeat_interleave(2, dim=-1)
        cos, sin = ang.cos().contiguous().to(dev()), ang.sin().contiguous().to(dev())
        cosd, sind = cos.double(), sin.double()        # the fp32 tables the kernel reads, exactly
    qwd, kwd = (None if w is None else w.to(dev()).double() for w in (qw, kw))
    qh, eq = temporal_chain(q.to(dev()).double(), qwd, cosd, sind, HD**-0.5)
    kh, ek = temporal_chain(k.to(dev()).double(), kwd, cosd, sind, None)
    N = B * S * H
    targets = None if pi is None else pi.reshape(N, T, 1).to(dev())
    ref = nm.attention_ref(qh.reshape(N, T, HD), kh.reshape(N, T, HD), v.to(dev()).double().reshape(N, T, HD), eq=eq.reshape(N, T, HD),
                           ek=ek.reshape(N, T, HD), log2_scale=LOG2E, denominator="fp32", targets=targets)
    what = f"{family} B{B} T{T} S{S} H{H} norm={norm} rope={rope}"
    vacuous_rows(ref, what, family == "retrieval" and norm)      # (see the module docstring)
    vt = None
    if targets is not None:
        vt = torch.gather(v.double(), 3, pi[..., None].expand(B, S, H, T, HD)).reshape(N, T, HD)
        fam.check_targets(ref, dict(expect=vt), what)
    qwg, kwg = (None if w is None else w.to(dev()) for w in (qw, kw))
    for variant in (0, 22, 21, 4, 9) if T <= 40 else (0, 22, 21, 9) if T <= 64 else (0, 9):
        out = torch.full((B * T * S, C), float("nan"), dtype=torch.bfloat16, device=dev())
        assert lib.vsys_tune_flash_variant(variant) == 0
        try:
            ops.attn_temporal(qkv, C, qwg, kwg, cos, sin, out, B, T, S, H)
            torch.cuda.synchronize()
        finally:
            lib.vsys_tune_flash_variant(0)
        o = out.view(B, T, S, H, HD).permute(0, 2, 3, 1, 4).reshape(N, T, HD)
        check_stack(o, ref, f"attn_temporal [variant {variant}] {what}", vt, v.to(dev()).double().reshape(N, T, HD))


# ------------------------------------------------------------------------------------------------ CogVideoX d64
D64 = 64
KSCALE64 = D64**-0.5 * LOG2E


def rope64(x, cos, sin, inverse=False):
    """Interleaved-pair rotation as attention64.hip applies it (cos / sin [rows, 64], each value twice); inverse: the transpose."""
    a, b = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    rot = torch.stack((-b, a), dim=-1).reshape(x.shape)
    return x * cos + rot * (-sin if inverse else sin)


def unswizzle_kp64(kp):
    """Kp [..., kv_pad, 64] as attn_prep_kv64 stores it (16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)) -> logical rows."""
    rows = kp.shape[-2]
    sw = (torch.arange(rows, device=kp.device) >> 1) & 7
    idx = (torch.arange(8, device=kp.device)[None, :] ^ sw[:, None])                      # logical chunk c <- physical chunk c ^ sw
    chunks = kp.reshape(*kp.shape[:-1], 8, 8)
    return torch.gather(chunks, -2, idx[:, :, None].expand(*kp.shape[:-2], rows, 8, 8)).reshape(kp.shape)


def q_chain64(q, w, b, cos, sin, eps=1e-6):
    """(q^, eq) of the d64 kernels (attention64.hip): q^ = bf16(rope(bf16(LN(q) w + b))); cos / sin [L, 64] with the text rows set to
    (1, 0), or None.  LayerNorm in fp32 over 64 values: acc(66) on the normalised value (mean, variance, the affine fma)."""
    h, e = q, None
    if w is not None:
        mu = q.mean(dim=-1, keepdim=True)
        n = (q - mu) * torch.rsqrt(((q - mu)**2).mean(dim=-1, keepdim=True) + eps)
        h = n * w + b
        e = nm.acc(D64 + 2, (n * w).abs() + b.abs()) + nm.rnd(h)
    if cos is not None:
        a, bb = h.reshape(*h.shape[:-1], -1, 2).unbind(-1)
        rot = torch.stack((-bb, a), dim=-1).reshape(h.shape)
        hr = h * cos + rot * sin
        swap = lambda t: t.reshape(*t.shape[:-1], -1, 2).flip(-1).reshape(t.shape)
        e0 = torch.zeros_like(h) if e is None else e
        e = e0 * cos.abs() + swap(e0) * sin.abs() + nm.acc(2, (h * cos).abs() + (rot * sin).abs()) + nm.rnd(hr)
        h = hr
    return h, e


# (B, H, Lt, Lv, norm): kv_len = Lt + Lv in {65, 300, 2064}, rope_start = Lt = 20
D64_CASES = [(2, 3, 20, 45, True), (2, 2, 20, 280, True), (2, 2, 20, 280, False), (1, 2, 20, 2044, True), (1, 2, 20, 2044, False)]


# (norm weights small enough for ln_key_bound leave 2064 keys no 12-binade lead: retrieval runs un-normed at that length)
D64_PARAMS = [c + (f,) for c in D64_CASES for f in ("diffuse", "retrieval") if not (f == "retrieval" and c[4] and c[2] + c[3] > 2048)]


@pytest.mark.parametrize("B,H,Lt,Lv,norm,family", D64_PARAMS)
def test_flash_d64_elementwise(ops, lib, B, H, Lt, Lv, norm, family):
    L, C, n = Lt + Lv, H * D64, B * H
    peaked = family == "retrieval"
    g = torch.Generator().manual_seed(L + H + norm)
    centre = 1.95 if peaked else 1.0        # (retrieval: as large as ln_key_bound's |q| |k| <= 60 allows)
    qw, kw = ((centre * (1 + 0.01 * torch.randn(D64, generator=g))).to(torch.bfloat16).to(dev()) for _ in range(2))
    qb, kb_ = ((0.05 * torch.randn(D64, generator=g)).to(torch.bfloat16).to(dev()) for _ in range(2))
    if not norm:
        qw = kw = qb = kb_ = None
    ang = torch.rand(Lv, D64 // 2, generator=g) * 6.0
    cos, sin = (t.repeat_interleave(2, -1).contiguous().to(dev()) for t in (ang.cos(), ang.sin()))
    cosL = torch.cat([torch.ones(Lt, D64, device=dev()), cos]).double()      # per sequence position; text rows: identity
    sinL = torch.cat([torch.zeros(Lt, D64, device=dev()), sin]).double()
    k3 = torch.randn(n, L, D64, generator=g)
    if peaked:
        k3 = k3 * (8.0 / k3.norm(dim=-1, keepdim=True))
    k3 = k3.to(torch.bfloat16).to(dev())
    v3 = (torch.randn(n, L, D64, generator=g) + 0.5).to(torch.bfloat16).to(dev())
    to2 = lambda x: x.view(B, H, L, D64).permute(0, 2, 1, 3).reshape(B * L, C).contiguous()
    kp, vt = ops.alloc_kv_buffers64(B, H, L, dev())
    ops.attn_prep_kv64(to2(k3), to2(v3), kw, kb_, cos, sin, Lt, kp, vt, B, H, L)
    torch.cuda.synchronize()
    khat = unswizzle_kp64(kp)[:, :, :L].double().reshape(n, L, D64)               # exp2 domain, post-LN, post-RoPE
    vd = vt[:, :, :, :L].transpose(-1, -2).double().reshape(n, L, D64)
    assert torch.equal(vd, v3.double()), "Vt is not the transpose of v"
    targets = expect = None
    if peaked:
        t = fam.target_order(L)[(torch.arange(L) * 7 + 3) % L].to(dev())            # onto (7 is coprime with 65, 300 and 2064)
        u = khat[:, t] / KSCALE64                                                    # what q^ should be, up to its length
        x = rope64(u, cosL, sinL, inverse=True)                                       # before the query's own rotation
        q3 = ((x - qb.double()) / qw.double() if norm else 6.0 * x).to(torch.bfloat16)
        targets = t[None, :, None].expand(n, L, 1)
        expect = vd[:, t]
    else:
        q3 = torch.randn(n, L, D64, generator=g).to(torch.bfloat16).to(dev())
    qh, eq = q_chain64(q3.double(), None if qw is None else qw.double(), None if qb is None else qb.double(), cosL, sinL)
    kbound = ops.ln_key_bound(qw, qb, kw, kb_) if norm else None
    if norm:
        assert kbound is not None
    m_extra = qh.norm(dim=-1) * kbound if kbound else None
    refs = {form: nm.attention_ref(qh, khat, vd, eq=eq, targets=targets, m_extra=m_extra, denominator=form) for form in ("fp32", "rounded")}
    what = f"{family} B{B} H{H} L{Lt}+{Lv} norm={norm}"
    for form, ref in refs.items():
        vacuous_rows(ref, f"{what} ({form} form)")
        if peaked:
            fam.check_targets(ref, dict(expect=expect), what)
    w64_ok = L >= 256
    runs = [("default", 0, kbound), ("default, no promise", 0, None), ("two-stage ring", 12, None), ("w64", 14, None)]
    if kbound:
        runs.append(("w64-static", 17, kbound))
    q2 = to2(q3)
    for label, variant, bound in runs:
        if variant == 17 and not w64_ok:
            continue        # (the launcher refuses 17 where the w64 stream does not apply)
        w64 = w64_ok and (variant in (14, 17) or (variant == 0 and L >= 2048))
        out = torch.full((B * L, C), float("nan"), dtype=torch.bfloat16, device=dev())
        assert lib.vsys_tune_flash_variant(variant) == 0
        try:
            ops.flash_attn64(q2, qw, qb, cos, sin, Lt, kp, vt, out, B, H, L, L, k_norm_bound=bound)
            torch.cuda.synchronize()
        finally:
            lib.vsys_tune_flash_variant(0)
        o = out.view(B, L, H, D64).permute(0, 2, 1, 3).reshape(n, L, D64)
        form = "rounded" if w64 else "fp32"
        check_stack(o, refs[form], f"flash d64 [{label}: {form} row sum] {what}", expect, vd, targets)


# ------------------------------------------------------------------------------------------------ T5
T5_CASES = [(2, 150, 4, (150, 97)), (2, 77, 2, (1, 77)), (1, 77, 2, (1,)), (1, 300, 8, (120,))]


@pytest.mark.parametrize("family", ["diffuse", "bias_dominant"])
@pytest.mark.parametrize("B,L,H,lens", T5_CASES)
def test_t5_attention_elementwise(ops, B, L, H, lens, family):
    """Every query row of every sample (rows past the sample's length attend to its valid keys like any other).  bias_dominant: the
    table of head h holds +30 at relative position delta_h and noise elsewhere, q and k are small: row i is carried by key
    i + delta_h wherever that key exists (condition on the reference), the output there is v of that key."""
    inner = H * D64
    g = torch.Generator().manual_seed(L + H + len(lens))
    peaked = family == "bias_dominant"
    qkv = (torch.randn(B * L, 3 * inner, generator=g) * (0.3 if peaked else 1.0))
    qkv[:, 2 * inner:] = torch.randn(B * L, inner, generator=g) + 0.5
    qkv = qkv.to(torch.bfloat16).to(dev())
    rel = torch.randn(H, 2 * L - 1, generator=g)
    delta = torch.tensor([(-3, 0, 5, -40, 1, 64, -1, 17)[h % 8] for h in range(H)])
    if peaked:
        rel[torch.arange(H), delta + L - 1] = 30.0
    center = (L + 127) // 128 * 128 - 1
    tab = torch.zeros(H, center + (L + 63) // 64 * 64)
    tab[:, center - (L - 1):center + L] = rel * LOG2E                      # fp32, exp2 domain: what the matrix-pipe kernel adds
    tab, rel = tab.to(dev()), rel.to(dev())
    idx = (torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1).to(dev())
    bias = tab[:, center - (L - 1):center + L].double()[:, idx]           # [H, L(query), L(key)]
    q, k, v = (qkv[:, i * inner:(i + 1) * inner].double().view(B, L, H, D64).transpose(1, 2) for i in range(3))
    outs = {"mfma": torch.full((B * L, inner), float("nan"), dtype=torch.bfloat16, device=dev()),
            "valu": torch.full((B * L, inner), float("nan"), dtype=torch.bfloat16, device=dev())}
    ops.t5_attention_mfma(qkv, tab, center, lens, B, L, H, out=outs["mfma"])
    ops.t5_attention(qkv, rel, torch.tensor(lens, dtype=torch.int32, device=dev()), B, L, H, out=outs["valu"])
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        ref = nm.attention_ref(q[b], k[b, :, :n], v[b, :, :n], bias=bias[:, :, :n], log2_scale=LOG2E, denominator="fp32")
        what = f"{family} B{B} L{L} H{H} sample {b} ({n} keys)"
        vacuous_rows(ref, what)
        expect = None
        if peaked:
            tgt = torch.arange(L, device=dev())[None, :] + delta.to(dev())[:, None]          # [H, L]
            valid = (tgt >= 0) & (tgt < n)
            assert valid.any()
            p = torch.exp2(ref.logits - ref.logits.amax(dim=-1, keepdim=True))
            w = torch.gather(p, -1, tgt.clamp(0, n - 1)[..., None])[..., 0] / p.sum(dim=-1)
            assert w[valid].min().item() >= fam.MIN_WEIGHT, f"{what}: the bias does not carry the row in the reference"
            expect = torch.gather(v[b, :, :n], 1, tgt.clamp(0, n - 1)[..., None].expand(H, L, D64))
        for name, out in outs.items():
            o = out.view(B, L, H, D64)[b].transpose(0, 1)
            check_stack(o, ref, f"t5_attention [{name}] {what}")
            if peaked:      # v of the key the bias points at, to one bf16 rounding + the off-target weight (<= 2^-12 2^(2 ds_max)) over the spread
                off = (2.0**-12 * torch.exp2(2 * ref.ds_max))[..., None]
                allow = 2.0**-7 * expect.abs() + off * (v[b, :, :n].abs().amax(dim=-2, keepdim=True) + expect.abs()) + nm.FLOOR
                bad = ~((o.double() - expect).abs() <= allow) & valid[..., None]
                assert not bad.any(), f"t5_attention [{name}] {what}: {int(bad.sum())} elements are not v of the key the bias points at"
