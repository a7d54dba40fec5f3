"""-m gpu: the data layouts around the STDiT3 attention kernels, checked element by element against float64 (tests/numerics.py):
attn_prep_kv (the Kp / Vt images the flash kernels read) and the patch embedding / final layer at production geometry.

K/V prep contract (attention.hip attn_prep_kv_kernel; ops.alloc_kv_buffers):
  * Kp [b, h, kv_pad, 72] = bf16(bf16(k rstd) w 72^-1/2 log2 e), rstd = rsqrt(mean(k^2) + eps) of the head's 72 values (w = 1 without
    k_norm): rounding chain rnd(k rstd) |w s| + rnd(Kp) + acc(72) on rstd; rows >= kv_len exactly 0;
  * Vt [b, h, 96, kv_pad]: rows 0-71 the bit-exact transpose of v, rows 72 and 76 = 1.0 over the keys < kv_len (the MFMA then
    accumulates the softmax denominator) and 0 beyond, every column >= kv_len of rows 0-76 exactly 0;
  * Vt rows 73-75 and 77-95 are never written: the caller's buffer holds zeros there (alloc_kv_buffers zero-fills).  The test fills
    every other element with NaN, so anything else the kernel leaves unwritten fails.
"""
import math

import pytest
import torch

import numerics as nm
from oracle import stdit3_oracle as O

pytestmark = pytest.mark.gpu

HD, VT_ROWS = 72, 96
KSCALE = 72**-0.5 * math.log2(math.e)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


def randn(shape, seed, scale=1.0, offset=0.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev()) * scale + offset).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ attn_prep_kv
def nan_kv_buffers(ops, batch, heads, kv_len):
    """Kp / Vt full of NaN except the Vt rows the contract leaves to the caller (73-75, 77-95: zero)."""
    kp, vt = ops.alloc_kv_buffers(batch, heads, kv_len, dev())
    kp.fill_(float("nan"))
    vt.fill_(float("nan"))
    vt[:, :, 73:76] = 0
    vt[:, :, 77:] = 0
    return kp, vt


@pytest.mark.parametrize("batch,heads,kv_len,norm", [(2, 16, 1, True), (2, 16, 63, True), (2, 16, 64, True), (2, 16, 65, True),
                                                     (2, 16, 300, False), (2, 16, 1024, True), (1, 16, 3600, True),
                                                     (38, 16, 1024, True), (3, 5, 300, True)])
def test_attn_prep_kv_contract(ops, batch, heads, kv_len, norm):
    """k and v are column slices of a [rows, 3 C] qkv buffer (stdit3.py spatial attention); k_norm_w = None is the cross-attention
    form (no RMS norm: Kp = bf16(k 72^-1/2 log2 e))."""
    C = heads * HD
    qkv = randn((batch * kv_len, 3 * C), kv_len + heads, 1.0, 0.3)
    k, v = qkv[:, C:2 * C], qkv[:, 2 * C:]
    w = randn((HD,), 7, 0.5, 1.0) if norm else None
    kp, vt = nan_kv_buffers(ops, batch, heads, kv_len)
    kv_pad = kp.shape[2]
    ops.attn_prep_kv(k, v, w, kp, vt, batch, heads, kv_len)
    torch.cuda.synchronize()

    kk = k.double().reshape(batch, kv_len, heads, HD).permute(0, 2, 1, 3)        # [b, h, s, 72]
    if norm:
        rstd = torch.rsqrt((kk**2).mean(-1, keepdim=True) + 1e-6)
        nrm = kk * rstd
        wd = w.double() * KSCALE
        ref = nrm * wd
        bound = (nm.rnd(nrm) + nm.acc(HD, nrm.abs())) * wd.abs() + nm.rnd(ref)
    else:
        ref = kk * KSCALE
        bound = nm.rnd(ref)
    got = kp[:, :, :kv_len]
    nm.check_elementwise(got.reshape(-1, HD), ref.reshape(-1, HD), bound.reshape(-1, HD), f"Kp kv_len={kv_len} norm={norm}")
    assert torch.equal(kp[:, :, kv_len:], torch.zeros_like(kp[:, :, kv_len:])), "Kp rows past kv_len must be exactly 0"

    vv = v.reshape(batch, kv_len, heads, HD).permute(0, 2, 3, 1)                # [b, h, 72, s], bf16
    assert torch.equal(vt[:, :, :HD, :kv_len], vv), "Vt rows 0-71 must be the bit-exact transpose of v"
    ones = torch.zeros(kv_pad, dtype=torch.bfloat16, device=dev())
    ones[:kv_len] = 1.0
    for r in (72, 76):
        assert torch.equal(vt[:, :, r], ones.expand_as(vt[:, :, r])), f"Vt row {r}: 1.0 over the valid keys, 0 beyond"
    assert torch.equal(vt[:, :, :77, kv_len:], torch.zeros_like(vt[:, :, :77, kv_len:])), "Vt columns past kv_len must be 0"
    for r in list(range(73, 76)) + list(range(77, VT_ROWS)):
        assert not vt[:, :, r].any(), f"Vt row {r} must stay 0"


# ------------------------------------------------------------------------------------------------ patch embedding / final layer
C, CIN, COUT, PATCH = 1152, 4, 8, (1, 2, 2)
LATENTS = [(19, 64, 64), (3, 90, 160), (2, 45, 77)]    # config 2 | 720p, a few frames | odd: zero pad + crop, S = 897 ragged over 8


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return dict(
        w=(torch.randn(C, CIN, 1, 2, 2, generator=g) * 0.2).to(torch.bfloat16),
        b=(torch.randn(C, generator=g) * 0.05).to(torch.bfloat16),
        table=(torch.randn(2, C, generator=g) / math.sqrt(C)).to(torch.bfloat16),
        t=(torch.randn(2, C, generator=g) * 0.3).to(torch.bfloat16),
        wf=(torch.randn(PATCH[1] * PATCH[2] * COUT, C, generator=g) / math.sqrt(C)).to(torch.bfloat16),
        bf=(torch.randn(PATCH[1] * PATCH[2] * COUT, generator=g) * 0.05).to(torch.bfloat16))


@pytest.mark.parametrize("T,H,W", LATENTS)
def test_patch_embed_at_production_geometry(ops, T, H, W):
    """out = bf16(bf16(conv(z) + b) + pos) (the conv output is a bf16 tensor before + pos_emb): acc(16) + rnd(conv) + rnd(out);
    B = 2 from one latent (CFG); then every P = 8 shard (patch_embed_shard) equals its rows of the whole-frame output bit for bit."""
    p = _params(T * H + W)
    Hp, Wp = -(-H // 2), -(-W // 2)
    S = Hp * Wp
    z = torch.randn(1, CIN, T, H, W, generator=torch.Generator().manual_seed(H)).to(torch.bfloat16).float()
    pos = O.pos_embed_2d(C, Hp, Wp, 1.0, 32)[0].to(torch.bfloat16)
    zd = torch.cat([z, z]).double()
    conv = O.patch_embed(zd, {"x_embedder.proj.weight": p["w"].double(), "x_embedder.proj.bias": p["b"].double()})
    cabs = O.patch_embed(zd.abs(), {"x_embedder.proj.weight": p["w"].double().abs(), "x_embedder.proj.bias": p["b"].double().abs()})
    conv, cabs = conv.reshape(2, T, S, C), cabs.reshape(2, T, S, C)
    ref = conv + pos.double()
    bound = nm.acc(16, cabs) + nm.rnd(conv) + nm.rnd(ref)
    wd, bd, posd = p["w"].reshape(C, -1).to(dev()), p["b"].to(dev()), pos.to(dev())
    zg = z.to(dev()).contiguous()
    out = ops.patch_embed(zg, wd, bd, posd, 2, PATCH, C)
    nm.check_elementwise(out.reshape(-1, C), ref.to(dev()).reshape(-1, C), bound.to(dev()).reshape(-1, C), f"patch_embed T={T} {H}x{W}")
    P = 8
    Sl = -(-S // P)
    for r in range(P):
        part = ops.patch_embed_shard(zg, wd, bd, posd, 2, PATCH, C, r * Sl, Sl)
        valid = max(0, min(Sl, S - r * Sl))
        assert torch.equal(part[:, :, :valid], out[:, :, r * Sl:r * Sl + valid]), f"P=8 rank {r}"
        assert not part[:, :, valid:].any(), "rows past the last token must be zero"


def _final_ref(x, p, T, Hp, Wp, H, W):
    """T2IFinalLayer + unpatchify in float64 (oracle), and its bound.  Chain of the model in bf16: shift / scale = bf16(table + t),
    m = bf16(bf16(bf16(LN(x)) bf16(1 + scale)) + shift) (LN in fp32), y = bf16(m W^T + b):
    |W| (rnd(shift) + |LN| (rnd(scale) + 2^-8 |1+scale| + 2^-20 |1+scale|) + rnd(LN (1+scale)) + rnd(m)) + acc(C) + rnd(y)."""
    B = x.shape[0]
    xd = x.double()
    td, tab = p["t"].double(), p["table"].double()
    sd = {"final_layer.scale_shift_table": tab, "final_layer.linear.weight": p["wf"].double(), "final_layer.linear.bias": p["bf"].double()}
    y = O.final_layer(xd, td, sd)                                              # [B, N, 32]
    shift, scale = (tab[None] + td[:, None]).chunk(2, dim=1)
    ln = O.layer_norm(xd)
    lnm = ln * (1 + scale)
    m = lnm + shift
    em = nm.rnd(shift) + ln.abs() * (nm.rnd(scale) + (nm.U_BF16 + 2.0**-20) * (1 + scale).abs()) + nm.rnd(lnm) + nm.rnd(m)
    wa = p["wf"].double().abs()
    bound = em @ wa.t() + nm.acc(C, m.abs() @ wa.t() + p["bf"].double().abs()) + nm.rnd(y)
    return y, bound


@pytest.mark.parametrize("T,H,W", LATENTS)
def test_final_layer_at_production_geometry(ops, T, H, W):
    """final_layer (whole frames, pixels) and final_layer_tokens + unpatchify_tokens at P = 8 (ragged last shard on the odd latent)
    against the float64 oracle on every pixel; the sharded form equals the whole-frame form bit for bit."""
    p = _params(T * W + H)
    Hp, Wp = -(-H // 2), -(-W // 2)
    S = Hp * Wp
    p = {k: v.to(dev()) for k, v in p.items()}
    x = randn((2, T * S, C), T + H + W, 1.0, 0.2)
    y, yb = _final_ref(x, p, T, Hp, Wp, H, W)
    ref = O.unpatchify(y, T, Hp, Wp, T, H, W, PATCH, COUT)
    bound = O.unpatchify(yb, T, Hp, Wp, T, H, W, PATCH, COUT)
    args = tuple(p[k] for k in ("table", "t", "wf", "bf"))
    xg = x
    whole = ops.final_layer(xg.view(-1, C), *args, 2, T, Hp, Wp, H, W, PATCH, COUT)
    nm.check_elementwise(whole.reshape(-1, W), ref.reshape(-1, W), bound.reshape(-1, W), f"final_layer T={T} {H}x{W}")
    P = 8
    Sl = -(-S // P)
    xs = xg.view(2, T, S, C)
    toks = []
    for r in range(P):
        part = torch.zeros(2, T, Sl, C, dtype=torch.bfloat16, device=dev())
        valid = max(0, min(Sl, S - r * Sl))
        part[:, :, :valid] = xs[:, :, r * Sl:r * Sl + valid]
        toks.append(ops.final_layer_tokens(part.view(-1, C), *args, 2, T, Sl))
    out = ops.unpatchify_tokens(torch.stack(toks).contiguous(), P, 2, T, Sl, Hp, Wp, H, W, PATCH, COUT)
    assert torch.equal(out, whole), f"P=8 {H}x{W}: sharded final layer differs from the whole-frame one"
