"""-m gpu: the head-dim-96 attention on a sequence-parallel exchange image (open_sora_plan_ops.attn_prep_kv96_img / flash_attn96_img,
csrc/attention96_img.hip) against the base kernels on the gathered rows.  Exact assertions only: the image kernels are the base
kernels' bodies with another row addressing, so they give the same BITS, and equality with the base kernels carries their fp64
element-wise proof (tests/test_gpu_osp_attention.py) over; there is no tolerance here.

B = 2, heads = 3.  Token s of sample b is row (s // seg_len) * slab_rows + b * seg_len + s % seg_len, slab_rows = B * seg_len + extra.
The (len, seg_len, extra) cases are the smallest at which a 16-query MFMA group, a 32-row wave, a 64-key tile and a 128-row query
block all straddle slab boundaries; (130, 50, 2) has a partial last slab of 30, (72, 72, 0) is one slab = the base call, (72, 100, 0) one
slab whose samples lie 100 rows apart.  Every row of an image that belongs to no token holds NaN, in the inputs and in the output:
afterwards the results are NaN-free and the output's NaNs are exactly those rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HD, H, B = 96, 3, 2
C = H * HD
CASES = [(72, 9, 0), (72, 36, 3), (130, 65, 0), (130, 26, 5), (130, 50, 2), (72, 72, 0), (72, 100, 0)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def rnd(shape, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) + offset).to(torch.bfloat16).to(dev())


def tables(n, seed):
    g = torch.Generator().manual_seed(seed)
    ang = (torch.rand(n, 3, 16, generator=g) * 6.0).repeat(1, 1, 2).reshape(n, HD)
    return ang.cos().contiguous().to(dev()), ang.sin().contiguous().to(dev())


def image_rows(n, seg, extra):
    """(row of token (b, s) as a long [B, n], rows of the image, slab stride) by the contract's formula."""
    slab = B * seg + extra
    nslab = -(-n // seg)
    s = torch.arange(n)
    row = (s // seg)[None] * slab + torch.arange(B)[:, None] * seg + (s % seg)[None]
    return row.to(dev()), nslab * slab, slab


def to_image(x, n, seg, extra, fill=float("nan")):
    """[B * n, W] rows (b, s) -> the image; every row that belongs to no token holds ``fill``."""
    row, rows, _ = image_rows(n, seg, extra)
    img = torch.full((rows, x.shape[1]), fill, dtype=x.dtype, device=x.device)
    img[row.reshape(-1)] = x
    return img


def from_image(img, n, seg, extra):
    return img[image_rows(n, seg, extra)[0].reshape(-1)]


def dead_rows(n, seg, extra):
    """bool [rows]: True on the rows of the image that belong to no token."""
    row, rows, _ = image_rows(n, seg, extra)
    dead = torch.ones(rows, dtype=torch.bool, device=dev())
    dead[row.reshape(-1)] = False
    return dead


_BASE = {}


def base(n):
    """The base kernels on the gathered rows, once per length: inputs and results (left unchanged by the tests)."""
    if n not in _BASE:
        from videosys_amd import open_sora_plan_ops as oops

        qkv = rnd((B * n, 3 * C), 9600 + n)
        qkv[:, 2 * C:] += 0.5
        cos, sin = tables(n, n)
        res = dict(qkv=qkv, cos=cos, sin=sin)
        for rope in (True, False):
            kp, vt = oops.alloc_kv_buffers96(B, H, n, dev())
            cs = (cos, sin) if rope else (None, None)
            oops.attn_prep_kv96(qkv[:, C:2 * C], qkv[:, 2 * C:], *cs, kp, vt, B, H, n)
            res["kp", rope], res["vt", rope] = kp, vt
        out = torch.full((B * n, C), float("nan"), dtype=torch.bfloat16, device=dev())
        oops.flash_attn96(qkv[:, :C], cos, sin, res["kp", True], res["vt", True], None, out, B, H, n, n)
        res["out"] = out
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
        _BASE[n] = res
    return _BASE[n]


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("n,seg,extra", CASES)
def test_prep_image_equals_the_base_kernel_bit_for_bit(n, seg, extra, rope):
    from videosys_amd import open_sora_plan_ops as oops

    bs = base(n)
    img = to_image(bs["qkv"], n, seg, extra)
    assert int(torch.isnan(img).all(dim=1).sum()) == int(dead_rows(n, seg, extra).sum())
    kp, vt = oops.alloc_kv_buffers96(B, H, n, dev())
    kp.fill_(float("nan")), vt.fill_(float("nan"))        # every element of both is written (pad keys: zeros)
    cs = (bs["cos"], bs["sin"]) if rope else (None, None)
    oops.attn_prep_kv96_img(img[:, C:2 * C], img[:, 2 * C:], *cs, kp, vt, B, H, n, seg, image_rows(n, seg, extra)[2])
    torch.cuda.synchronize()
    assert not torch.isnan(kp).any() and not torch.isnan(vt).any(), "a row that belongs to no token reached Kp / Vt"
    assert torch.equal(kp, bs["kp", rope]) and torch.equal(vt, bs["vt", rope])


@pytest.mark.parametrize("n,seg,extra", CASES)
def test_flash_image_self_form_equals_the_base_kernel_bit_for_bit(n, seg, extra):
    """q and out are images of DIFFERENT strides: q the q | k | v image (row stride 3C, ``extra`` rows behind a slab), out an image of
    row stride C + 8 with extra + 1 rows behind a slab."""
    from videosys_amd import open_sora_plan_ops as oops

    bs = base(n)
    img = to_image(bs["qkv"], n, seg, extra)
    q_slab = image_rows(n, seg, extra)[2]
    _, out_rows, out_slab = image_rows(n, seg, extra + 1)
    wide = torch.full((out_rows, C + 8), float("nan"), dtype=torch.bfloat16, device=dev())
    out = wide[:, :C]
    oops.flash_attn96_img(img[:, :C], bs["cos"], bs["sin"], bs["kp", True], bs["vt", True], None, out, B, H, n, n, seg, q_slab, out_slab)
    torch.cuda.synchronize()
    assert torch.equal(from_image(out, n, seg, extra + 1), bs["out"])
    dead = dead_rows(n, seg, extra + 1)
    assert torch.isnan(out[dead]).all() and int(torch.isnan(out).any(dim=1).sum()) == int(dead.sum()), \
        "the output's NaNs are not exactly the rows that belong to no token"
    assert torch.isnan(wide[:, C:]).all(), "columns behind heads * 96 were written"


def test_flash_image_cross_form_equals_the_base_kernel_bit_for_bit():
    """130 text keys, kv_lens = [5, 130] read on the device, no RoPE; the 72 queries in slabs of 9."""
    from videosys_amd import open_sora_plan_ops as oops

    n, seg, extra, Lk = 72, 9, 0, 130
    kb = base(Lk)
    q = rnd((B * n, C), 777)
    lens = torch.tensor([5, 130], dtype=torch.int32, device=dev())
    want = torch.full((B * n, C), float("nan"), dtype=torch.bfloat16, device=dev())
    oops.flash_attn96(q, None, None, kb["kp", False], kb["vt", False], lens, want, B, H, n, Lk)
    qi = to_image(q, n, seg, extra)
    _, out_rows, out_slab = image_rows(n, seg, 4)
    out = torch.full((out_rows, C), float("nan"), dtype=torch.bfloat16, device=dev())
    oops.flash_attn96_img(qi, None, None, kb["kp", False], kb["vt", False], lens, out, B, H, n, Lk, seg, image_rows(n, seg, extra)[2], out_slab)
    torch.cuda.synchronize()
    assert not torch.isnan(want).any() and torch.equal(from_image(out, n, seg, 4), want)
    dead = dead_rows(n, seg, 4)
    assert torch.isnan(out[dead]).all() and int(torch.isnan(out).any(dim=1).sum()) == int(dead.sum())
