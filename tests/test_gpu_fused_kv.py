"""-m gpu: the spatial qkv GEMM with the K/V prep in its epilogue (vsys_gemm_bf16_ln_qkv_kv, gemm2_bf16.hip EPI_LN_QKV_KV) against the
pair of launches it replaces — gemm_ln (open_sora_transformer_3d.py:196-197 + attentions.py:59) followed by attn_prep_kv (the k half
of the qk-norm, attentions.py:75 + normalization.py:28-33, and the Kp / Vt layouts of the flash kernels).

The reference is always the UNFUSED pair on the same inputs.  Required and asserted: q, Kp and Vt (all 96 rows) BIT-equal.  Kp is
bit-equal because both kernels run the k-norm through the same three steps (csrc/common.h KNorm72) on the same bf16 k values; the
float64 fallback bound of tests/test_gpu_numerics_attn_io.py is therefore not used.  Output buffers start full of NaN (as
test_gpu_numerics_attn_io.py::nan_kv_buffers prepares them), so anything the fused launch leaves unwritten fails; the Vt rows it
leaves to the caller by contract (72-95, constants when every key is valid) are set the way the model sets them at allocation."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 72


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from videosys_amd import ops as o

    return o


def nan_kv_buffers(ops, batch, heads, kv_len):
    """Kp / Vt full of NaN except the Vt rows the attn_prep_kv contract leaves to the caller (73-75, 77-95: zero)."""
    kp, vt = ops.alloc_kv_buffers(batch, heads, kv_len, dev())
    kp.fill_(float("nan"))
    vt.fill_(float("nan"))
    vt[:, :, 73:76] = 0
    vt[:, :, 77:] = 0
    return kp, vt


def _site(ops, heads, K, seed, kv_order):
    """One qkv site through vsys_adaln_prescale: (W', cs, cv), in the checkpoint's column order or the K/V one."""
    g = torch.Generator().manual_seed(seed)
    N = 3 * HD * heads
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(dev())
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).to(dev())
    mod = (torch.randn(2 * K, generator=g) * 0.3).to(torch.bfloat16).to(dev())   # shift | scale
    Wp, cs, cv = torch.full_like(W, float("nan")), torch.full((N,), float("nan"), device=dev()), torch.full((N,), float("nan"), device=dev())
    nword = N | (heads << 32 if kv_order else 0)
    sites = torch.tensor([[W.data_ptr(), bias.data_ptr(), Wp.data_ptr(), cs.data_ptr(), cv.data_ptr(), 0, K, nword, K, 0]], dtype=torch.int64).to(dev())
    ops.adaln_prescale(sites, -(-N // 4), mod)
    torch.cuda.synchronize()
    return Wp, cs, cv


def _rows(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x = x * (0.5 + torch.rand(M, 1, generator=g) * 2.0) + 3.0 * torch.randn(M, 1, generator=g)
    x[:, 7] *= 40.0
    return x.to(torch.bfloat16).to(dev())


@pytest.mark.parametrize("heads,K", [(16, 1152), (8, 576)])
def test_prescale_writes_the_kv_column_order(ops, heads, K):
    """Same values, other places: row n of W', cs[n], cv[n] of the K/V-order site sit at column order[n]."""
    Wp, cs, cv = _site(ops, heads, K, 3, False)
    Wq, csq, cvq = _site(ops, heads, K, 3, True)
    col = ops.qkv_kv_column_order(heads).to(dev())
    assert torch.equal(Wq[col], Wp) and torch.equal(csq[col], cs) and torch.equal(cvq[col], cv)
    assert not torch.isnan(Wq.float()).any() and not torch.isnan(csq).any() and not torch.isnan(cvq).any()


# production shape (config 2: 38 frames of 1024 tokens) | two samples, few tiles (the unfused GEMM takes the 128-row geometry there)
# | a ragged last row tile: 97 frames of 64 tokens = 24 tiles of 256 rows + 64 | six frames of 1024 (>= 400 tiles: the kernel the
# model's dispatch rule replaces) | 8 heads
@pytest.mark.parametrize("M,S,heads,K", [(38912, 1024, 16, 1152), (2048, 1024, 16, 1152), (6208, 64, 16, 1152), (6144, 1024, 16, 1152),
                                         (1280, 256, 8, 576)])
def test_fused_equals_gemm_ln_then_attn_prep_kv(ops, M, S, heads, K):
    C = HD * heads
    assert M % S == 0 and (M % 256 != 0) == (M == 6208)
    x = _rows(M, K, M + S)
    kw = (torch.randn(HD, generator=torch.Generator().manual_seed(7)) * 0.5 + 1.0).to(torch.bfloat16).to(dev())
    st = ops.ln_stats_buffer(M, K, dev())
    ops.ln_row_stats(x, st)

    # the unfused pair
    Wp, cs, cv = _site(ops, heads, K, 11, False)
    qkv = torch.full((M, 3 * C), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.gemm_ln(x, Wp, cs, cv, st, out=qkv)
    kp0, vt0 = nan_kv_buffers(ops, M // S, heads, S)
    ops.attn_prep_kv(qkv[:, C:2 * C], qkv[:, 2 * C:], kw, kp0, vt0, M // S, heads, S)

    # the fused launch
    Wq, csq, cvq = _site(ops, heads, K, 11, True)
    q = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device=dev())
    kp1, vt1 = nan_kv_buffers(ops, M // S, heads, S)
    ops.kv_set_constant_rows(vt1)     # what the model does once when it allocates the spatial K/V buffers for this path
    ops.gemm_ln_qkv_kv(x, Wq, csq, cvq, st, kw, q, kp1, vt1, S, heads)
    torch.cuda.synchronize()

    assert not torch.isnan(qkv.float()).any()
    assert torch.equal(q, qkv[:, :C]), "q differs from the unfused GEMM's q columns"
    assert torch.equal(vt1.view(torch.int16), vt0.view(torch.int16)), "Vt (all 96 rows) differs from attn_prep_kv's"
    assert torch.equal(kp1.view(torch.int16), kp0.view(torch.int16)), "Kp differs from attn_prep_kv's"

    # q with a row stride of the caller's choice: the front third of a [M, 3C] buffer
    wide = torch.full((M, 3 * C), float("nan"), dtype=torch.bfloat16, device=dev())
    kp2, vt2 = nan_kv_buffers(ops, M // S, heads, S)
    ops.kv_set_constant_rows(vt2)
    ops.gemm_ln_qkv_kv(x, Wq, csq, cvq, st, kw, wide[:, :C], kp2, vt2, S, heads)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :C], qkv[:, :C]) and torch.isnan(wide[:, C:].float()).all(), "a strided q must leave the rest of the row alone"
    assert torch.equal(kp2.view(torch.int16), kp0.view(torch.int16)) and torch.equal(vt2.view(torch.int16), vt0.view(torch.int16))


def test_unsupported_shapes_are_shape_errors(ops):
    from videosys_amd._lib import VsysError

    heads, K = 16, 1152
    C = HD * heads
    Wq, csq, cvq = _site(ops, heads, K, 11, True)
    kw = torch.ones(HD, dtype=torch.bfloat16, device=dev())
    for M, S in ((3600, 3600), (200, 100)):      # 720p frames (S % 64 != 0) | small ragged frames
        x = _rows(M, K, 1)
        st = ops.ln_stats_buffer(M, K, dev())
        ops.ln_row_stats(x, st)
        kp = torch.zeros(M // S, heads, S, HD, dtype=torch.bfloat16, device=dev())
        vt = torch.zeros(M // S, heads, 96, S, dtype=torch.bfloat16, device=dev())
        q = torch.zeros(M, C, dtype=torch.bfloat16, device=dev())
        with pytest.raises(VsysError):
            ops.gemm_ln_qkv_kv(x, Wq, csq, cvq, st, kw, q, kp, vt, S, heads)
    assert not ops.gemm_ln_qkv_kv_dispatched(2048, 3 * C, K) and ops.gemm_ln_qkv_kv_dispatched(38912, 3 * C, K)


def _model_and_inputs(T):
    from oracle import stdit3_oracle as O
    from videosys_amd.stdit3 import STDiT3, STDiT3Config

    cfg = dict(depth=2, hidden_size=1152, num_heads=16, caption_channels=64, model_max_length=16)
    sd = O.synth_state_dict(**cfg, seed=31)
    sd = {k: (v if k == "rope.freqs" else v.to(torch.bfloat16).float()) for k, v in sd.items()}
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 4, T, 64, 64, generator=g).to(torch.bfloat16).float()      # 32 x 32 patches: S = 1024 tokens per frame
    y = torch.randn(2, 1, 16, 64, generator=g).to(torch.bfloat16).float()
    mask = torch.zeros(1, 16, dtype=torch.long)
    mask[:, :11] = 1
    kw = dict(mask=mask, fps=torch.tensor([24.0, 24.0]), height=torch.tensor([512.0, 512.0]), width=torch.tensor([512.0, 512.0]))
    m = STDiT3(STDiT3Config(**cfg), device="cuda:0")
    m.load_state_dict(sd)
    return m, x, y, kw


def test_stdit3_switch_on_off_same_bits_eager_and_recorded(ops):
    """A depth-2 STDiT3 step (2 x 3 frames of 1024 tokens = 6144 rows: the shape rule picks the fused launch) with the switch on and off:
    bit-equal outputs; eager and recorded-program launches agree; the two forms have programs of their own; the fused step issues no
    attn_prep_kv for its spatial blocks."""
    m, x, y, kw = _model_and_inputs(3)
    t = torch.tensor([500.0, 500.0])
    assert m._fused_kv_ok(2 * 3 * 1024, 1024)
    calls = {"prep": 0, "fused": 0}
    real_prep, real_fused = ops.attn_prep_kv, ops.gemm_ln_qkv_kv

    def prep(*a, **k):
        calls["prep"] += 1
        return real_prep(*a, **k)

    def fused(*a, **k):
        calls["fused"] += 1
        return real_fused(*a, **k)

    ops.attn_prep_kv, ops.gemm_ln_qkv_kv = prep, fused
    try:
        m.fused_kv = True
        out_on = m(x, t, y, **kw).float().cpu()          # recorded
        text_preps = calls["prep"]                       # the once-per-prompt text K/V
        assert calls["fused"] == 2, calls
        out_on2 = m(x, t, y, **kw).float().cpu()         # replayed
        assert m.program_stats["recorded"] == 1 and m.program_stats["replayed"] == 1
        m.fused_kv = False
        out_off = m(x, t, y, **kw).float().cpu()         # its own program
        assert m.program_stats["recorded"] == 2 and calls["prep"] == text_preps + 2 and calls["fused"] == 2
        out_off2 = m(x, t, y, **kw).float().cpu()
        m.use_programs = False
        m.fused_kv = True
        out_on_eager = m(x, t, y, **kw).float().cpu()
        m.fused_kv = False
        out_off_eager = m(x, t, y, **kw).float().cpu()
    finally:
        ops.attn_prep_kv, ops.gemm_ln_qkv_kv = real_prep, real_fused
    assert torch.isfinite(out_on).all()
    assert torch.equal(out_on, out_off), "switch on / off differ"
    assert torch.equal(out_on, out_on2) and torch.equal(out_off, out_off2), "replay differs from the recording step"
    assert torch.equal(out_on, out_on_eager) and torch.equal(out_off, out_off_eager), "eager differs from the launch program"


def test_stdit3_small_step_keeps_the_two_kernel_path(ops):
    """2 x 2 frames = 4096 rows: fewer tiles than the shape dispatch sends to the fused kernel's tile — today's path, whatever the switch."""
    m, x, y, kw = _model_and_inputs(2)
    t = torch.tensor([500.0, 500.0])
    assert not m._fused_kv_ok(2 * 2 * 1024, 1024)
    n = [0]
    real = ops.gemm_ln_qkv_kv

    def fused(*a, **k):
        n[0] += 1
        return real(*a, **k)

    ops.gemm_ln_qkv_kv = fused
    try:
        out = m(x, t, y, **kw)
    finally:
        ops.gemm_ln_qkv_kv = real
    assert n[0] == 0 and torch.isfinite(out.float()).all()
