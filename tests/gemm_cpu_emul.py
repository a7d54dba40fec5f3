"""TEST INFRASTRUCTURE: the GEMM family's three chains restated in torch fp32 on the CPU (fp32 arithmetic, bf16 storage: the kernels'
contract), with the defects tests/test_numerics_cpu.py plants.  Nothing here is compared with a kernel bit for bit: a restatement has to
pass the bounds of tests/gemm_numerics_cases.py / numerics.linear_small_ref, a defect has to fail them.

  gelu_store     EPI_BIAS_GELU: bf16(gelu_tanh(acc + bias)), gelu_tanh in the kernels' form x / (1 + exp2(-2 u log2 e)) (common.h)
  gate_res       EPI_GATE_RES with the two-segment gate, decided PER WAVE of 64 rows as the 16x16x32 epilogue decides it (gemm_bf16.hip):
                 one gate row when the wave's first and last existing row lie in one sample and one segment, else a gather per token
  linear_small   one wave per output: lane l adds elements 8 l .. 8 l + 7 of every pass of 512, the 64 lane sums meet by butterfly
"""
import torch

BF = torch.bfloat16
K0, K1 = 0.7978845608028654, 0.044715


def gelu_tanh32(x):
    u = K0 * x * (1.0 + K1 * x * x)
    e = torch.exp2(u * -2.8853900817779268)          # +inf for very negative x: the quotient is -0
    return x * (1.0 / (1.0 + e))


def silu32(x):
    return x / (1.0 + torch.exp(-x))


def gelu_store(a, w, b, defect=None):
    """defect: "bias_after" = gelu(acc) + bias;  "abs" = gelu(|acc + bias|)."""
    acc = a.float() @ w.float().t()
    bias = b.float() if b is not None else 0.0
    if defect == "bias_after":
        return (gelu_tanh32(acc) + bias).to(BF)
    p = acc + bias
    return gelu_tanh32(p.abs() if defect == "abs" else p).to(BF)


def gate_res(a, w, b, gate, gate_stride, rps, seg_split, gate_alt, res, defect=None):
    """(out, aux) = (bf16(res + u), u = bf16(g_r (acc + bias))).  ``gate``: a view that starts at sample 0's vector.  defect:
      "le"              the segment test with <= for <
      "wave_first_row"  the gate row of the wave's first row for all 64 rows, boundary or not
      "alt_on_video"    gate_alt added on the rows at or behind seg_split instead of those in front of it
      "tile_sample"     the sample index of every row taken from its 128-row tile's first row"""
    M, N = a.shape[0], w.shape[0]
    v = a.float() @ w.float().t()
    if b is not None:
        v = v + b.float()

    def vec(sample, alt):
        return torch.as_strided(gate, (N,), (1,), gate.storage_offset() + sample * gate_stride + (gate_alt if alt else 0)).float()

    def is_alt(pos):
        if seg_split <= 0:
            return False
        inside = pos <= seg_split if defect == "le" else pos < seg_split
        return (not inside) if defect == "alt_on_video" else inside

    def sample_of(r):
        return ((r // 128) * 128 if defect == "tile_sample" else r) // rps

    g = torch.empty(M, N)
    for rowb in range(0, M, 64):
        r_lo, r_hi = rowb, min(rowb + 63, M - 1)
        s_lo, s_hi = sample_of(r_lo), sample_of(r_hi)
        alt_lo, alt_hi = is_alt(r_lo - s_lo * rps), is_alt(r_hi - s_hi * rps)
        if defect == "wave_first_row" or (s_lo == s_hi and alt_lo == alt_hi):
            g[r_lo:r_hi + 1] = vec(s_lo, alt_lo)
        else:
            for r in range(r_lo, r_hi + 1):
                s = sample_of(r)
                g[r] = vec(s, is_alt(r - s * rps))
    u = (v * g).to(BF)
    return (u.float() + res.float()).to(BF), u


def linear_small(x, w, bias=None, act_in="none", act_out="none", out=None, defect=None):
    """defect: "silu_unrounded" = silu(x) kept in fp32 (one rounding fewer: must PASS);  "silu_after" = the SiLU applied to the sum
    instead of to x;  "lane_stride_64" = a lane's second pass starts 64 elements on instead of 512 (elements counted several times)."""
    M, K = x.shape
    xe = x.float()
    if act_in == "silu" and defect != "silu_after":
        xe = silu32(xe)
        if defect != "silu_unrounded":
            xe = xe.to(BF).float()
    prod = xe[:, None, :] * w.float()[None, :, :]                      # [M, N, K]
    if defect == "lane_stride_64":
        lanes = torch.zeros(M, w.shape[0], 64)
        for lane in range(64):
            for k in range(lane * 8, K, 64):
                lanes[:, :, lane] += prod[:, :, k:k + 8].sum(dim=2)
    else:
        passes = -(-K // 512)
        prod = torch.nn.functional.pad(prod, (0, passes * 512 - K))
        lanes = prod.view(M, w.shape[0], passes, 64, 8).sum(dim=4).sum(dim=2)
    width = 32
    while width >= 1:                                                  # wave_sum: butterfly
        lanes = lanes[:, :, :width] + lanes[:, :, width:2 * width]
        width //= 2
    s = lanes[:, :, 0]
    if bias is not None:
        s = s + bias.float()
    if act_in == "silu" and defect == "silu_after":
        s = silu32(s)
    if act_out == "silu":
        s = silu32(s)
    elif act_out == "gelu":
        s = gelu_tanh32(s)
    res = s.to(BF)
    if out is not None:
        out.copy_(res)
        return out
    return res
