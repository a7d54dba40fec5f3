"""-m gpu: guard-band tests (tests/isolation.py) of the image forms of the head-dim-96 entry points,
open_sora_plan_ops.attn_prep_kv96_img and open_sora_plan_ops.flash_attn96_img (attention96_img.hip), as
tests/test_gpu_vchitect_attn_img.py tests Vchitect's image kernel.  Exact assertions only, under both guard fills: same bits as the
call on tight operands, every guard byte untouched, every input unchanged.

Operand forms: q / k / v / out are images (tests/test_gpu_osp_attention_img.py's layout) that are column slices of wider parents of
their own; the rows of an image that belong to no token — the gap between batch * seg_len and the slab stride, and the tail of a
partial last slab — are ``interior=`` guard: never read into a result, never written.  Tables tight, Kp / Vt tight with one 64-key
tile of every (batch, head) image as extra guard, kv_lens with other VALID counts as guard."""
import pytest
import torch

import isolation as iso
from isolation import Operand
from test_gpu_osp_attention_img import B, C, H, HD, dead_rows, dev, image_rows, rnd, tables, to_image

pytestmark = pytest.mark.gpu

CASES = [(72, 36, 3), (130, 26, 5), (130, 50, 2), (72, 100, 0)]


def image(data, n, seg, extra, pad_l, pad_r):
    """An image operand: a column slice of a wider parent, the rows of no token as interior guard."""
    img = to_image(data.contiguous(), n, seg, extra, fill=0.0)
    mask = dead_rows(n, seg, extra)[:, None].expand(img.shape).contiguous()
    return Operand(img, parent=(img.shape[0], pad_l + img.shape[1] + pad_r), at=(0, pad_l), interior=mask)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("n,seg,extra", CASES)
def test_isolation_attn_prep_kv96_img(n, seg, extra, rope):
    from videosys_amd import open_sora_plan_ops as oops

    kv_pad = oops.kv_pad_len(n)
    slab = image_rows(n, seg, extra)[2]
    o = {"k": image(rnd((B * n, C), n), n, seg, extra, 8, 16), "v": image(rnd((B * n, C), n + 1, 0.5), n, seg, extra, 16, 8),
         "kp": Operand(torch.zeros(B, H, kv_pad, HD, dtype=torch.bfloat16, device=dev()), guard_elems=B * H * 64 * HD),
         "vt": Operand(torch.zeros(B, H, HD, kv_pad, dtype=torch.bfloat16, device=dev()), guard_elems=B * H * 64 * HD)}
    if rope:
        cos, sin = tables(n, n)
        o["cos"], o["sin"] = Operand(cos), Operand(sin)

    def fn(t):
        oops.attn_prep_kv96_img(t["k"], t["v"], t.get("cos"), t.get("sin"), t["kp"], t["vt"], B, H, n, seg, slab)

    iso.check_isolated(fn, o, ["kp", "vt"], what=f"attn_prep_kv96_img n={n} seg={seg} extra={extra} rope={rope}")


@pytest.mark.parametrize("form", ["self", "cross"])
@pytest.mark.parametrize("n,seg,extra", CASES)
def test_isolation_flash_attn96_img(n, seg, extra, form):
    from videosys_amd import open_sora_plan_ops as oops

    Lk = n if form == "self" else 130
    cos, sin = tables(n, n) if form == "self" else (None, None)
    kv = rnd((B * Lk, 2 * C), Lk + 5)
    kv[:, C:] += 0.5
    kp, vt = oops.alloc_kv_buffers96(B, H, Lk, dev())
    oops.attn_prep_kv96(kv[:, :C], kv[:, C:], cos, sin, kp, vt, B, H, Lk)
    torch.cuda.synchronize()
    q_slab, out_slab = image_rows(n, seg, extra)[2], image_rows(n, seg, extra + 1)[2]
    o = {"q": image(rnd((B * n, C), n + 2), n, seg, extra, 16, 8), "kp": Operand(kp, guard_elems=B * H * 64 * HD),
         "vt": Operand(vt, guard_elems=B * H * 64 * HD),
         "out": image(torch.zeros(B * n, C, dtype=torch.bfloat16, device=dev()), n, seg, extra + 1, 8, 24)}
    if form == "self":
        o["cos"], o["sin"] = Operand(cos), Operand(sin)
    else:
        o["lens"] = Operand(torch.tensor([5, 130], dtype=torch.int32, device=dev()), int_guard=[7, 64, 1, 129])

    def fn(t):
        oops.flash_attn96_img(t["q"], t.get("cos"), t.get("sin"), t["kp"], t["vt"], t.get("lens"), t["out"], B, H, n, Lk, seg, q_slab,
                              out_slab)

    iso.check_isolated(fn, o, ["out"], what=f"flash_attn96_img {form} n={n} seg={seg} extra={extra}")
