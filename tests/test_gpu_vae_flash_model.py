"""-m gpu: the flash path of vae_blocks.attention_core inside the models.  (a) VaeBlocks._attention and the CausalVAE _attention on one
96 x 96 frame at C = 128 (9216 keys: a ValueError / a failed softmax launch before) against a float64 restatement on 256 sampled rows,
within 1.5 x the bf16 floor (the restatement with bf16 roundings at the kernels' store points); (b) the hidden-size-32 fixture decode
of tests/test_gpu_osp_vae.py with the flash path forced, same criterion; (c) unforced at Lp <= 8192: the bits of the parent's launches."""
import math
from types import SimpleNamespace

import pytest
import torch

import osp_vae_ref as R
from test_gpu_osp_vae import case, dev, fixture, rms, weights

pytestmark = pytest.mark.gpu
C, H, W = 128, 96, 96


def attn_weights(seed):
    from videosys_amd.vae_blocks import AttnWeights

    g = torch.Generator().manual_seed(seed)
    lin = lambda: (torch.randn(C, C, generator=g) / math.sqrt(C)).to(torch.bfloat16).to(dev())
    vec = lambda s, o=0.0: (torch.randn(C, generator=g) * s + o).to(torch.bfloat16).to(dev())
    norm = SimpleNamespace(g=vec(0.1, 1.0), b=vec(0.1), eps=1e-6)
    return AttnWeights(norm, lin(), vec(0.02), lin(), vec(0.02), lin(), vec(0.02), lin(), vec(0.02).float())


def block_restated(x, aw, rows, rnd):
    """The block of one frame on ``rows`` in float64; ``rnd`` rounds where the kernels store (V^T without its bias: it is folded into bo)."""
    d = lambda t: t.double()
    xg = x.view(-1, 32, C // 32)
    mu, var = xg.mean(dim=(0, 2), keepdim=True), xg.var(dim=(0, 2), unbiased=False, keepdim=True)
    hn = rnd(((xg - mu) * torch.rsqrt(var + aw.norm.eps)).reshape(-1, C) * d(aw.norm.g) + d(aw.norm.b))
    q, k, v = rnd(hn[rows] @ d(aw.wq).t() + d(aw.bq)), rnd(hn @ d(aw.wk).t() + d(aw.bk)), rnd(hn @ d(aw.wv).t())
    s = (q @ k.t()) * C**-0.5
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = rnd((rnd(p) @ v) / p.sum(dim=-1, keepdim=True))
    return rnd(o @ d(aw.wo).t() + d(aw.bo) + x[rows])


def within_floor(what, out, low, ref):
    err, floor = rms(out - ref), rms(low - ref)
    print(f"[{what}] HIP rms error {err:.4e}, bf16 floor {floor:.4e} (ratio {err / floor:.3f}), output rms {rms(ref):.3f}")
    assert floor < 0.05 * rms(ref), "the floor is vacuous"
    assert err <= 1.5 * floor, f"{what}: HIP rms error {err:.4e} > 1.5 x the bf16 floor {floor:.4e}"


@pytest.mark.parametrize("which", ["decoder2d", "causal"])
def test_attention_block_past_8192_keys(which):
    from videosys_amd.ops import VaeGrid
    from videosys_amd.vae_blocks import VaeBlocks
    from videosys_amd.vae_open_sora_plan import _CausalBlocks

    aw = attn_weights(11)
    x = torch.randn(H * W, C, generator=torch.Generator().manual_seed(12)).to(torch.bfloat16).to(dev())
    blocks = (VaeBlocks if which == "decoder2d" else _CausalBlocks)(dev())
    y, gy = blocks._attention(x, VaeGrid(1, 1, H, W, 0, 0), aw)
    torch.cuda.synchronize()
    rows = torch.arange(0, H * W, 36, device=dev())
    ref, low = (block_restated(x.double(), aw, rows, r) for r in (lambda t: t, lambda t: t.to(torch.bfloat16).double()))
    within_floor(f"{which} 96 x 96", y[rows].double(), low, ref)    # one frame: rows 0 .. L - 1 are its pixels in both output layouts


def test_fixture_decode_on_the_flash_path(monkeypatch):
    from videosys_amd import vae_blocks
    from videosys_amd.vae_open_sora_plan import CausalVAEModelWrapper

    monkeypatch.setattr(vae_blocks, "FORCE_FLASH", True)
    z, tiling = case("a")
    out = CausalVAEModelWrapper(weights(), device=dev()).decode(z.to(dev())).float().cpu()
    within_floor("fixture case a, flash forced", out.double(), R.wrapper_decode(z, weights(), tiling, dtype=torch.bfloat16).double(), fixture()["a"])


@pytest.mark.parametrize("n,L", [(2, 6), (1, 200)])
def test_default_path_keeps_its_bits(n, L):
    from videosys_amd import ops, vae_blocks

    assert not vae_blocks.FORCE_FLASH
    w, Lp, L4 = attn_weights(21), (L + 127) // 128 * 128, (L + 3) // 4 * 4
    hn, xd = (torch.zeros(n, Lp, C, dtype=torch.bfloat16, device=dev()) for _ in range(2))
    g = torch.Generator().manual_seed(22)
    hn[:, :L], xd[:, :L] = (torch.randn(n, L, C, generator=g).to(torch.bfloat16).to(dev()) for _ in range(2))
    hn, xd = hn.view(n * Lp, C), xd.view(n * Lp, C)
    got = vae_blocks.attention_core(hn, xd, n, L, Lp, C, w).view(n, Lp, C)[:, :L]      # ... against the parent's launch sequence:
    q, k = ops.gemm128(hn, w.wq, w.bq), ops.gemm128(hn, w.wk, w.bk)
    vt = torch.empty(n, C, Lp, dtype=torch.bfloat16, device=dev())
    ops.gemm128(w.wv, hn.view(n, Lp, C), out=vt, batch=n, batch_a=0, batch_w=Lp * C, batch_o=C * Lp, M=C)
    s = torch.empty(n, Lp, Lp, dtype=torch.float32, device=dev())
    ops.gemm128(q.view(n, Lp, C), k.view(n, Lp, C), out_f32=s, out_scale=1.0 / math.sqrt(C), batch=n, batch_a=Lp * C, batch_w=Lp * C,
                batch_o=Lp * Lp, M=Lp)
    s[:, :, L:L4] = -3.0e38
    o = torch.empty(n * Lp, C, dtype=torch.bfloat16, device=dev())
    ops.gemm128(ops.softmax_rows(s, n=L4), vt, out=o.view(n, Lp, C), batch=n, batch_a=Lp * Lp, batch_w=C * Lp, batch_o=Lp * C, M=Lp)
    want = ops.gemm128(o, w.wo, w.bo, res=xd).view(n, Lp, C)[:, :L]
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
