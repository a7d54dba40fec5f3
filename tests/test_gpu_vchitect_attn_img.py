"""-m gpu: vchitect_ops.attn_temporal64_img (vsys_attn_temporal_d64_img, attention_t64.hip) — the temporal attention of Vchitect-2.0 on
the receive image of the sequence-parallel frame -> token switch, rows ordered (slab, b, t % Tl, s).

It is the same kernel body as vchitect_ops.attn_temporal64 with another row address, so the contract is EQUAL BITS: the image is built
from the (b, t, n) tensors with torch indexing, both kernels run, the output image is un-imaged and compared with torch.equal.  The
unread tail of the last slab holds NaN in every input image and in the output image: it must neither reach a result nor be written.
B = 2, heads = 5 (two head groups, three idle waves in the second), n_vid = 3, n_txt = 2; q / k / v of the video are column blocks of
one fused [rows, 3 C] image, as the layer passes them.  (T, Tl):
  (5, 2)   a short last slab          (33, 9)  one key past the 32-key chunk          (70, 18)  a second query pass
  (1, 1)   a single frame             (5, 5)   one slab: the old kernel's call  (3, 5)    one slab longer than T: samples Tl frames apart
One case is also held element-wise against the float64 softmax with the bound of the d64 temporal family
(tests/test_gpu_vchitect_attention.py: attention_ref "fp32", tile 4, rotary error acc(2) + one rounding).

Guard bands (tests/isolation.py): the image operands inside arenas, strided with live gaps on both sides, the tail of the last slab
an INTERIOR guard of every operand (poisoned in the inputs, and required to keep its poison in the outputs)."""
import math

import pytest
import torch

import isolation as iso
import numerics as nm
import vchitect_ref as vr
from isolation import Operand
from test_gpu_numerics_attention import check_stack, vacuous_rows

pytestmark = pytest.mark.gpu

HD = 64
LOG2E = math.log2(math.e)
B, H, S, L = 2, 5, 3, 2
C = H * HD
CASES = [(5, 2), (33, 9), (70, 18), (1, 1), (5, 5), (3, 5)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def to_image(x, T, Tl, n, fill=float("nan")):
    """[B * T * n, W] rows (b, t, i) -> [nslab * B * Tl * n, W] rows (t // Tl, b, t % Tl, i); rows of frames past T hold ``fill``."""
    ns = -(-T // Tl)
    img = torch.full((ns, B, Tl, n, x.shape[1]), fill, dtype=x.dtype, device=x.device)
    xv = x.reshape(B, T, n, x.shape[1])
    for t in range(T):
        img[t // Tl, :, t % Tl] = xv[:, t]
    return img.reshape(ns * B * Tl * n, x.shape[1])


def from_image(img, T, Tl, n):
    ns = -(-T // Tl)
    iv = img.reshape(ns, B, Tl, n, img.shape[1])
    return torch.stack([iv[t // Tl, :, t % Tl] for t in range(T)], dim=1).reshape(B * T * n, img.shape[1])


def tail_mask(T, Tl, n, width):
    """bool [rows, width] of an image: True on the rows of frames past T."""
    return torch.isnan(to_image(torch.zeros(B * T * n, width, device=dev()), T, Tl, n))


def operands(T, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda rows, w, off=0.0: (torch.randn(rows, w, generator=g) + off).to(torch.bfloat16).to(dev())
    qkv = r(B * T * S, 3 * C)
    qkv[:, 2 * C:] += 0.5
    txt = [r(B * T * L, C, 0.5 if i == 2 else 0.0) for i in range(3)]
    cos, sin = (t.to(dev()) for t in vr.rope_tables(T))
    return qkv, txt, cos, sin


@pytest.mark.parametrize("T,Tl", CASES)
def test_image_kernel_equals_the_row_kernel_bit_for_bit(T, Tl):
    from videosys_amd import vchitect_ops as vops

    qkv, txt, cos, sin = operands(T, 4000 + T)
    nan = lambda rows, w=C: torch.full((rows, w), float("nan"), dtype=torch.bfloat16, device=dev())
    ov, ot = nan(B * T * S), nan(B * T * L)
    vops.attn_temporal64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], *txt, cos, sin, ov, ot, B, T, S, L, H)
    qi = to_image(qkv, T, Tl, S)
    ti = [to_image(t, T, Tl, L) for t in txt]
    ovi, oti = nan(qi.shape[0]), nan(ti[0].shape[0])
    vops.attn_temporal64_img(qi[:, :C], qi[:, C:2 * C], qi[:, 2 * C:], *ti, cos, sin, ovi, oti, B, T, Tl, S, L, H)
    torch.cuda.synchronize()
    assert not torch.isnan(ov).any() and not torch.isnan(ot).any()
    assert torch.equal(from_image(ovi, T, Tl, S), ov) and torch.equal(from_image(oti, T, Tl, L), ot)
    # the tail of the last slab was not written (and, the real rows being NaN-free, not read into a result)
    assert torch.isnan(ovi[tail_mask(T, Tl, S, C)]).all() and torch.isnan(oti[tail_mask(T, Tl, L, C)]).all()
    assert int(torch.isnan(ovi).sum()) == int(tail_mask(T, Tl, S, C).sum())


def test_image_kernel_elementwise_against_float64():
    from videosys_amd import vchitect_ops as vops

    T, Tl = 33, 9
    qkv, txt, cos, sin = operands(T, 4100)
    vid = [qkv[:, i * C:(i + 1) * C] for i in range(3)]
    heads_major = lambda x: x.transpose(1, 2).reshape(-1, x.shape[1], HD)
    d3 = lambda x, n: x.double().reshape(B * T, n, C)
    q, k, v = (vr.temporal_tokens(d3(a, S), d3(b, L), B, T, H) for a, b in zip(vid, txt))
    cd, sd = cos.double(), sin.double()
    ref = nm.attention_ref(heads_major(vr.apply_rotary(q, cd, sd)), heads_major(vr.apply_rotary(k, cd, sd)), heads_major(v),
                           eq=heads_major(vr.rotary_error(q, cd, sd)), ek=heads_major(vr.rotary_error(k, cd, sd)),
                           log2_scale=LOG2E / 8, denominator="fp32", tile=4)
    what = f"attn_temporal64_img B{B} T{T} Tl{Tl} S{S}+L{L} H{H}"
    vacuous_rows(ref, what)
    qi = to_image(qkv, T, Tl, S)
    ti = [to_image(t, T, Tl, L) for t in txt]
    ovi = torch.full((qi.shape[0], C), float("nan"), dtype=torch.bfloat16, device=dev())
    oti = torch.full((ti[0].shape[0], C), float("nan"), dtype=torch.bfloat16, device=dev())
    vops.attn_temporal64_img(qi[:, :C], qi[:, C:2 * C], qi[:, 2 * C:], *ti, cos, sin, ovi, oti, B, T, Tl, S, L, H)
    torch.cuda.synchronize()
    ov, ot = from_image(ovi, T, Tl, S), from_image(oti, T, Tl, L)
    check_stack(heads_major(vr.temporal_tokens(ov.reshape(B * T, S, C), ot.reshape(B * T, L, C), B, T, H)), ref, what)


# ------------------------------------------------------------------------------------------------ guard bands
def strided(data, pad_l, pad_r, interior=None):
    return Operand(data, parent=(data.shape[0], pad_l + data.shape[1] + pad_r), at=(0, pad_l), interior=interior)


ISOLATION_CASES = [(5, 2, True), (33, 9, True), (70, 18, False), (5, 5, True), (3, 5, True)]


@pytest.mark.parametrize("T,Tl,rope", ISOLATION_CASES)
def test_isolation_attn_temporal64_img(T, Tl, rope):
    from videosys_amd import vchitect_ops as vops

    qkv, txt, cos, sin = operands(T, 4200 + T)
    mv, mt = tail_mask(T, Tl, S, C), tail_mask(T, Tl, L, C)
    img = lambda x, n: to_image(x.contiguous(), T, Tl, n, fill=0.0)
    o = {}
    for i, name in enumerate(("q", "k", "v")):
        o[name + "_vid"] = strided(img(qkv[:, i * C:(i + 1) * C], S), 8, 16, mv)
        o[name + "_txt"] = strided(img(txt[i], L), 16, 8, mt)
    o["out_vid"] = strided(torch.zeros_like(o["q_vid"].data), 8, 8, mv)
    o["out_txt"] = strided(torch.zeros_like(o["q_txt"].data), 24, 8, mt)
    if rope:
        o["cos"], o["sin"] = Operand(cos), Operand(sin)

    def fn(t):
        vops.attn_temporal64_img(t["q_vid"], t["k_vid"], t["v_vid"], t["q_txt"], t["k_txt"], t["v_txt"], t.get("cos"), t.get("sin"),
                                 t["out_vid"], t["out_txt"], B, T, Tl, S, L, H)

    iso.check_isolated(fn, o, ["out_vid", "out_txt"], what=f"attn_temporal64_img T={T} Tl={Tl} rope={rope}")
