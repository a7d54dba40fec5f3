"""Element-wise error bounds for kernels checked against a float64 reference.  TEST INFRASTRUCTURE: imported by the numerics tests
(tests/test_gpu_numerics_*.py, tests/test_numerics_cpu.py) the way tests/fulldepth_util.py is.

Method.  The reference is computed in float64 from the bf16-exact inputs the kernel received.  Every output element gets its own
bound, assembled by the test from the rounding chain of the operation's contract (the reference model run in bf16):
  * ``rnd(v)``      = 2^-8 |v| for every intermediate v the contract rounds to bf16 (unit roundoff of an 8-bit significand),
                      carried through the operations that follow it (a rounding before a multiply by g counts |g| times);
  * ``acc(K, s)``   = K 2^-24 s for an fp32 accumulation of K products whose absolute values sum to s (s = sum_k |a_k b_k|);
  * ``FLOOR``       = a tiny absolute floor (exact zeros, values far below the data's scale).
Each term is a worst case, so an implementation that rounds once fewer than the contract passes as well; what fails is an error
larger than every rounding of the chain together: a wrong element, a wrong operand, a tile left unwritten, partial sums held in
bf16, or an extra rounding where the contract keeps full precision.

A failure names the number of elements outside the bound, the worst one, its tile (256- and 128-row, 192-column: the GEMM
geometries) and the ratio of its error to its bound.
"""
from __future__ import annotations

import torch

U_BF16 = 2.0**-8
U_F32 = 2.0**-24
FLOOR = 2.0**-24


def rnd(v: torch.Tensor) -> torch.Tensor:
    """Worst-case error of rounding ``v`` to bf16."""
    return U_BF16 * v.abs()


def acc(K: int, abs_sum: torch.Tensor) -> torch.Tensor:
    """Worst-case error of an fp32 sum of K products whose absolute values add up to ``abs_sum``."""
    return (K * U_F32) * abs_sum


def bf16_exact(t: torch.Tensor) -> torch.Tensor:
    """``t`` rounded to bf16 and widened to float64 (the value a bf16 tensor holds)."""
    return t.to(torch.bfloat16).double()


def row_chunks(M: int, chunk: int):
    for r0 in range(0, M, chunk):
        yield r0, min(M, r0 + chunk)


def matmul_ref(a: torch.Tensor, w: torch.Tensor):
    """(a @ w^T, |a| @ |w|^T) in float64: the exact product of the bf16 operands and the sum of |a_k w_k| of each element."""
    a64, w64 = a.double(), w.double()
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def tile_of(row: int, col: int) -> str:
    return f"256-row tile {row // 256}, 128-row tile {row // 128}, 192-col tile {col // 192}"


class Bound:
    """Accumulates the element-wise check over row chunks of one output (``add``), then ``check()`` raises with the worst element.

    Non-finite outputs violate every bound."""

    def __init__(self, what: str):
        self.what = what
        self.total = 0
        self.bad = 0
        self.worst = None   # (ratio, row, col, out, ref, bound)

    def add(self, out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, row0: int = 0) -> "Bound":
        out = out.double().reshape(ref.shape[0], -1)
        ref = ref.reshape(out.shape)
        bound = (bound.reshape(out.shape) + FLOOR)
        ratio = (out - ref).abs() / bound
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
        self.total += ratio.numel()
        self.bad += int((ratio > 1.0).sum())
        i = int(ratio.argmax())
        r, c = divmod(i, ratio.shape[1])
        q = float(ratio[r, c])
        if self.worst is None or q > self.worst[0]:
            self.worst = (q, row0 + r, c, float(out[r, c]), float(ref[r, c]), float(bound[r, c]))
        return self

    def message(self) -> str:
        q, r, c, o, f, b = self.worst
        return (f"{self.what}: {self.bad} of {self.total} elements outside the bound; worst at (row {r}, col {c}) [{tile_of(r, c)}]: "
                f"out {o:.6g}, ref {f:.6g}, bound {b:.3g}, |err| / bound = {q:.3g}")

    def check(self) -> None:
        assert self.total > 0, f"{self.what}: nothing was checked"
        assert self.bad == 0, self.message()


def check_elementwise(out, ref, bound, what: str) -> None:
    """One-shot form of Bound for outputs small enough to compare at once (any shape; rows = the first dimension)."""
    Bound(what).add(out, ref, bound).check()


# ------------------------------------------------------------------------------------------------ softmax attention
U_EXP = 2.0**-21   # relative accuracy assumed for v_exp_f32: the kernel guides give no figure, so 2^-21 (about 1 ulp of fp32 with room for
U_RCP = 2.0**-21   # the range reduction) is used for it and for the reciprocal / division of the row sum; both vanish next to 2^-8


class AttnRef:
    """Result of ``attention_ref``: ``out`` and ``bound`` [Lq, Dv] float64, ``weight`` [Lq] = the reference's softmax weight on the keys
    named by ``targets`` (None without targets), ``logits`` [Lq, Lk] (exp2 domain, float64), ``ds_max`` [Lq] = the largest logit error
    bound of the row, ``vacuous`` = the number of rows whose P error bound reaches 1 (their elements get an INFINITE bound: the
    quotient form has broken down there, and a test must hold such rows by other means and say so)."""

    def __init__(self, out, bound, weight, logits, ds_max, vacuous):
        self.out, self.bound, self.weight, self.logits, self.ds_max, self.vacuous = out, bound, weight, logits, ds_max, vacuous


def attention_ref(q, kp, v, *, eq=None, ek=None, bias=None, log2_scale=1.0, m_extra=None, denominator="rounded", targets=None,
                  tile=64, budget=1 << 25) -> AttnRef:
    """softmax attention of one (batch, head) slice — or a stack of slices of one shape: any leading dimensions, shared by all
    arguments — in float64 and its per-element bound, chunked over query rows.

    ``q`` [Lq, D], ``kp`` [Lk, D], ``v`` [Lk, Dv]: the operands the two matrix products see, as float64 (exactly the bf16 values where
    the kernel's operand is a stored tensor; where the kernel derives the operand — a normed q — the float64 value of the contract and
    ``eq`` / ``ek`` [same shape] its worst-case error, None = exact).  Logits s = log2_scale q kp^T (+ ``bias`` [Lq, Lk], float64, in
    the same exp2 domain): the d72 / d64 kernels carry scale log2(e) on Kp (log2_scale = 1), the temporal and T5 kernels multiply
    natural-domain logits by log2(e).  Only valid keys are passed (the caller slices at kv_len).

    Bound, term by term (no global factor):
      logits   ds_j = log2_scale (eq |kp_j| + |q| ek_j + eq ek_j) + acc(D + 10, log2_scale sum_d |q_d kp_jd| + |bias| + M): D + 8 products
               (the head dim padded to whole MFMA chunks) + the subtracted maximum entering the accumulator + the bias add; M is the
               magnitude of what is subtracted: max_j |s_j|, raised to ``m_extra`` [Lq] (|q| k_bound of the kernels without a running max);
      P        p_j = 2^(s_j - m) -> bf16: relative error e_j = 2^-8 + U_EXP + (2^ds_j - 1);
      output   denominator == "rounded": the row sum is the sum of the SAME rounded p_j (the d72 flash kernels: the ones rows of Vt ride
               on the PV MFMA), so numerator and denominator err together and
               o~ - o = sum_j p_j e_j (v_j - o) / sum_j p_j (1 + e_j):  sum_j p_j e_j |v_jd - o_d| / (l (1 - max e)) (infinite from max e = 1 on, see AttnRef.vacuous);  a peaked row
               collapses to rnd(o).  denominator == "fp32": p_j / l is formed in fp32 from the unrounded p_j and THEN rounded to bf16
               (the temporal kernels, as the reference's attn.to(dtype) does), or the rounded p_j feed the PV product while the row sum adds
               up the UNROUNDED fp32 p_j (the 32-row d64 kernel, attention64.hip: lsum += pv before the cast, also under T5's bias hook; the
               d64 w64 stream takes the sum from the rounded P like d72): each weight errs on its own,
               sum_j p_j e'_j |v_jd| / (l (1 - max e')), e' = e + U_RCP + acc(Lk, 1) + (2^max ds - 1) (the sum's own error);
      PV       acc(Lk + 2 ntiles, sum_j p_j |v_jd| / l + |o_d|): Lk products and one rescale of numerator and denominator per tile (the
               rescale factor itself cancels in the quotient);  U_RCP |o_d| for the final division;  rnd(o_d) for the bf16 store.
    """
    assert denominator in ("rounded", "fp32")
    Lq, D = q.shape[-2:]
    Lk, Dv = v.shape[-2:]
    assert kp.shape[-2:] == (Lk, D) and Lk > 0
    ntiles = -(-Lk // tile)
    T = lambda x: x.transpose(-1, -2)
    rows = lambda x, r0, r1: x[..., r0:r1, :]
    ka, va = kp.abs(), v.abs()
    outs, bounds, weights, logits, dsmax = [], [], [], [], []
    vacuous = 0
    nb = max(1, q.numel() // (Lq * D))
    # the largest temporary per query row: [Lk, Dv] for the |v - o| weighting, [Lk] otherwise
    chunk = max(1, min(Lq, budget // (nb * Lk * (Dv if denominator == "rounded" else 1))))
    for r0, r1 in row_chunks(Lq, chunk):
        qc = rows(q, r0, r1)
        s = log2_scale * (qc @ T(kp))
        sabs = log2_scale * (qc.abs() @ T(ka))
        ds = torch.zeros_like(s)
        if eq is not None:
            ds = ds + log2_scale * (rows(eq, r0, r1) @ T(ka))
        if ek is not None:
            ds = ds + log2_scale * ((qc.abs() + (rows(eq, r0, r1) if eq is not None else 0)) @ T(ek))
        if bias is not None:
            s = s + rows(bias, r0, r1)
            sabs = sabs + rows(bias, r0, r1).abs()
        M = s.abs().amax(dim=-1, keepdim=True)
        if m_extra is not None:
            M = torch.maximum(M, m_extra[..., r0:r1, None].abs())
        ds = ds + acc(D + 10, sabs + M)
        e = U_BF16 + U_EXP + (torch.exp2(ds) - 1)
        p = torch.exp2(s - s.amax(dim=-1, keepdim=True))
        l = p.sum(dim=-1, keepdim=True)
        o = (p @ v) / l
        pv_abs = (p @ va) / l
        if denominator == "rounded":
            first = torch.einsum("...qk,...qkd->...qd", p * e, (v[..., None, :, :] - o[..., :, None, :]).abs())
        else:
            e = e + U_RCP + acc(Lk, 1.0) + (torch.exp2(ds.amax(dim=-1, keepdim=True)) - 1)
            first = (p * e) @ va
        emax = e.amax(dim=-1, keepdim=True)
        broken = emax >= 1.0        # (the quotient form holds for every max e < 1 and grows without limit towards it on its own)
        vacuous += int(broken.sum())
        first = torch.where(broken, torch.full_like(first, float("inf")), first / (l * (1 - emax).clamp_min(FLOOR)))
        dsmax.append(ds.amax(dim=-1))
        bounds.append(first + acc(Lk + 2 * ntiles, pv_abs + o.abs()) + U_RCP * o.abs() + rnd(o))
        outs.append(o)
        logits.append(s)
        if targets is not None:
            weights.append(torch.gather(p, -1, rows(targets, r0, r1)).sum(dim=-1) / l[..., 0])
    return AttnRef(torch.cat(outs, dim=-2), torch.cat(bounds, dim=-2), torch.cat(weights, dim=-1) if targets is not None else None,
                   torch.cat(logits, dim=-2), torch.cat(dsmax, dim=-1), vacuous)


def rms_q_chain(q, w, eps=1e-6):
    """(q^, eq) of the d72 flash kernels' query chain (attention.hip finish_q): q^ = bf16(bf16(q rstd) w), rstd = rsqrt(mean(q^2) + eps)
    over the head's 72 values in fp32.  eq = (rnd(q rstd) + acc(72, |q rstd|)) |w| + rnd(q^).  ``w`` None: q is the operand bit for bit."""
    if w is None:
        return q, None
    n = q * torch.rsqrt((q * q).mean(dim=-1, keepdim=True) + eps)
    qh = n * w
    return qh, (rnd(n) + acc(q.shape[-1], n.abs())) * w.abs() + rnd(qh)


# ------------------------------------------------------------------------------------------------ VAE family
# conv_kernel (csrc/conv_bf16.hip: tap-shifted conv and the plain 128-column GEMM), the GroupNorm / SpatialNorm / softmax / first-layer
# kernels of csrc/vae_ops.hip.  Grids are ops.VaeGrid objects (plain Python: no device needed); tensors are float64 on the CPU.
SILU_SLOPE = 1.1   # the largest slope of x / (1 + exp(-x)) is 1.0998 (at x = 2.3994)


def grid_view(rows: torch.Tensor, g, C=None) -> torch.Tensor:
    """The rows of grid ``g`` [g.rows, >= C] as [n, T + tf, Hp, Wp, C] (front frames and borders included; slack rows left out)."""
    C = rows.shape[1] if C is None else C
    return rows.reshape(g.n, g.sample_rows, -1)[:, :(g.T + g.tf) * g.plane].reshape(g.n, g.T + g.tf, g.Hp, g.Wp, -1)[..., :C]


def grid_interior(rows: torch.Tensor, g, C=None) -> torch.Tensor:
    """[n, T, H, W, C]: the voxels of grid ``g`` (what every VAE kernel is compared on)."""
    return grid_view(rows, g, C)[:, g.tf:, g.pad:g.pad + g.H, g.pad:g.pad + g.W]


def conv_gather(a_rows: torch.Tensor, g, cin: int, kt: int, ks: int) -> torch.Tensor:
    """The im2col matrix of a causal (kt, ks, ks) convolution over the padded grid ``g``, [n T H W, kt ks ks cin] float64, column =
    ((a ks + b) ks + c) cin + channel: for every tap the [n, T, H, W, cin] window of the 5-D grid view that starts at frame a (the tf =
    kt - 1 front frames are the causal padding) and at pixel (b, c) of the bordered plane (ks = 3 on a pad = 1 grid; ks = 1 reads the
    voxel itself on any grid).  Stated on voxel coordinates: no flat row arithmetic, unlike the kernel's row shifts."""
    assert g.tf == kt - 1 and (ks == 1 or (ks == 3 and g.pad == 1))
    x = grid_view(a_rows.double(), g, cin)
    taps = []
    for a in range(kt):
        for b in range(ks):
            for c in range(ks):
                h0, w0 = (b, c) if ks == 3 else (g.pad, g.pad)
                taps.append(x[:, a:a + g.T, h0:h0 + g.H, w0:w0 + g.W])
    return torch.cat(taps, dim=-1).reshape(g.n * g.T * g.H * g.W, kt * ks * ks * cin)


def linear_ref(a, w, bias=None, res=None, out_scale=None):
    """conv_kernel's contract on an explicit A [M, K] (the rows themselves for gemm128, ``conv_gather`` for a conv), w [N, K]:
      bf16 out   p = sum_k a_k w_k + b in fp32, s = sum_k |a_k w_k| + |b|:  out = bf16(p), bound acc(K + 1, s) + rnd(p);  with a residual
                 the kernel computes bf16(res + bf16(p)): reference res + p, one more term rnd(res + p);
      fp32 out   (``out_scale`` given; no bias, no residual) out = out_scale p: bound out_scale acc(K + 2, s) — no bf16 term, which is
                 the point of the form (attention scores, split-K partials).
    Returns (ref, bound), float64 [M, N]."""
    K = a.shape[1]
    p, s = matmul_ref(a, w)
    if out_scale is not None:
        assert bias is None and res is None
        return out_scale * p, abs(out_scale) * acc(K + 2, s)
    if bias is not None:
        p, s = p + bias.double(), s + bias.double().abs()
    bound = acc(K + 1, s) + rnd(p)
    if res is not None:
        p = p + res.double()
        bound = bound + rnd(p)
    return p, bound


class NormRef:
    """``ref`` / ``bound`` [n, T, H, W, C]; ``cancel`` = the part of ``bound`` that comes from the error of rstd (the cancellation of
    var = E[x^2] - mu^2, carried to the output); ``n_t`` / ``lanes`` = the launch geometry the statistics term was derived from."""

    def __init__(self, ref, bound, cancel, n_t, lanes):
        self.ref, self.bound, self.cancel, self.n_t, self.lanes = ref, bound, cancel, n_t, lanes

    def cancel_share(self) -> float:
        """The largest share of an element's bound that the rstd (cancellation) term takes."""
        return float((self.cancel / (self.bound + FLOOR)).max())


def _silu64(x):
    return x / (1.0 + torch.exp(-x))


def group_norm_ref(x, groups, gamma, beta, eps, nblk, silu=False, yb=None) -> NormRef:
    """GroupNorm (+ SiLU, or + SpatialNorm + SiLU) of x [n, T, H, W, C] float64 with its per-element bound.

    Contract (vae_ops.hip):  y = [silu](bf16((x - mu) rstd gamma + beta)), statistics per (sample, group) over (T, H, W) and the group's
    channels.  ``yb`` = (Y, B) [n, T, H, W, C] (the SpatialNorm maps ALREADY gathered at every voxel): y = silu(bf16(bf16(nf Y) + B)),
    nf = bf16(GroupNorm(x)).

    Statistics, from the launch geometry (gn_partial_kernel: ``nblk`` blocks per sample, lanes = 256 // (C / 8) position lanes per
    block): a thread adds n_t = ceil(P / (nblk lanes)) positions of 4 channels in fp32, ``lanes`` such sums are added in fp32, the rest is
    double (gn_finalize_kernel); x^2 of a bf16 x is exact in fp32.  With Ka = 4 n_t + lanes additions:
      e_mu   = acc(Ka, E|x|) + 2^-24 |mu|          (the sum; the fp32 store of the mean)
      r_q    = Ka 2^-24                            (relative, on E[x^2]: every term is >= 0)
      d_var  = r_q E[x^2] + 2 |mu| e_mu + e_mu^2   (var = E[x^2] - mu^2 as the kernel forms it)
      r_rstd = d / (2 (1 - d)) + 2^-24, d = d_var / (var + eps): holds the cancellation factor E[x^2] / (var + eps)
    Output: t = (x - mu) rstd gamma, pre = t + beta:
      e_pre  = |rstd gamma| e_mu + |t| r_rstd + 3 2^-24 (|t| + |beta|)     (the fp32 subtract / multiplies / add)
      plain  bound = e_pre + rnd(pre)
      SiLU   bound = SILU_SLOPE (e_pre + rnd(pre)) + rnd(y) + (U_EXP + U_RCP) |y|    (fast exp, fast reciprocal)
      SpatialNorm   E1 = e_pre + rnd(pre);  E2 = |Y| E1 + rnd(pre Y);  E3 = E2 + rnd(pre Y + B);  then SiLU of q = pre Y + B as above."""
    n, T, H, W, C = x.shape
    cg = C // groups
    P = T * H * W
    lanes = 256 // (C // 8)
    n_t = -(-P // (nblk * lanes))
    Ka = 4 * n_t + lanes
    xg = x.reshape(n, P, groups, cg)
    mu = xg.mean(dim=(1, 3), keepdim=True)
    ex2 = (xg * xg).mean(dim=(1, 3), keepdim=True)
    eabs = xg.abs().mean(dim=(1, 3), keepdim=True)
    var = (ex2 - mu * mu).clamp_min(0.0)
    rstd = torch.rsqrt(var + eps)
    e_mu = acc(Ka, eabs) + U_F32 * mu.abs()
    d = (Ka * U_F32 * ex2 + 2 * mu.abs() * e_mu + e_mu * e_mu) / (var + eps)
    assert float(d.max()) < 1.0, "the statistics bound has broken down (d_var >= var + eps)"
    r_rstd = d / (2 * (1 - d)) + U_F32
    ga, be = gamma.double().reshape(groups, cg), beta.double().reshape(groups, cg)
    t = (xg - mu) * rstd * ga
    pre = t + be
    cancel = t.abs() * r_rstd
    e_pre = (rstd * ga).abs() * e_mu + cancel + 3 * U_F32 * (t.abs() + be.abs())
    shape = (n, T, H, W, C)
    pre, e_pre, cancel = pre.reshape(shape), e_pre.reshape(shape), cancel.reshape(shape)
    err, carried = e_pre + rnd(pre), cancel
    if yb is not None:
        Y, B = yb[0].double(), yb[1].double()
        err = Y.abs() * err + rnd(pre * Y)
        carried = Y.abs() * carried
        pre = pre * Y + B
        err = err + rnd(pre)
        silu = True
    if not silu:
        return NormRef(pre, err, carried, n_t, lanes)
    y = _silu64(pre)
    return NormRef(y, SILU_SLOPE * err + rnd(y) + (U_EXP + U_RCP) * y.abs(), SILU_SLOPE * carried, n_t, lanes)


def spatial_norm_maps(yb_rows, n, C, zdims, size):
    """[Y | B] rows over the latent grid ([n zT zH zW, 2C]) -> (Y, B) [n, T, H, W, C] at the voxels of ``size`` = (T, H, W), indexed the
    way the reference model does it (CogVideoXSpatialNorm3D): F.interpolate nearest, the first frame on its own when T is odd and > 1."""
    import torch.nn.functional as F

    zT, zH, zW = zdims
    T, H, W = size
    z = yb_rows.double().reshape(n, zT, zH, zW, 2 * C).permute(0, 4, 1, 2, 3)
    if T > 1 and T % 2 == 1:
        zi = torch.cat([F.interpolate(z[:, :, :1], size=(1, H, W)), F.interpolate(z[:, :, 1:], size=(T - 1, H, W))], dim=2)
    else:
        zi = F.interpolate(z, size=(T, H, W))
    zi = zi.permute(0, 2, 3, 4, 1)
    return zi[..., :C], zi[..., C:]


def softmax_rows_ref(s: torch.Tensor, n: int):
    """softmax_rows_kernel: p_j = bf16(exp(s_j - m) / l) over the first n of ld columns of fp32 scores s [rows, ld].  Relative bound
    2^-8 + 2 U_EXP + U_RCP + acc(n, 1) + |s_j - m| 2^-23: the bf16 store, the fast exp of the element and of the sum's terms, the
    reciprocal of the sum, the fp32 sum of n terms, and the fp32 subtraction + the scaling of the exponent's argument (2^-24 of
    |s_j - m| each).  Returns (ref, bound) [rows, n] float64; columns n .. ld - 1 must be exactly zero and are the caller's to check."""
    x = s.double()[:, :n]
    dlt = x - x.amax(dim=1, keepdim=True)
    e = torch.exp(dlt)
    p = e / e.sum(dim=1, keepdim=True)
    rel = U_BF16 + 2 * U_EXP + U_RCP + acc(n, 1.0) + dlt.abs() * 2.0**-23
    return p, rel * p


def first_im2col_ref(z, kt, kcols, params):
    """first_im2col_kernel: z [4, F, H, W] (bf16 values) -> rows [F H W, kcols]; v = bf16(z scale + shift) per channel,
    u = bf16(pq_w v + pq_b) in fp32, column (tap, channel) of a causal (kt, 3, 3) im2col, exact zeros outside the volume and in columns
    >= 36 kt.  Bound: rnd(v) carried through |pq_w|, + acc(4, sum |pq_w v| + |pq_b|), + rnd(u).  ``params`` are the 28 numbers the
    kernel receives as fp32.  Returns (ref, bound, nonzero mask) [F H W, kcols]; where the mask is False the output must be exactly 0."""
    import torch.nn.functional as F

    prm = torch.tensor([float(v) for v in params], dtype=torch.float32).double()
    scale, shift, pw, pb = prm[0:4], prm[4:8], prm[8:24].reshape(4, 4), prm[24:28]
    _, Fr, H, W = z.shape
    v = z.double() * scale[:, None, None, None] + shift[:, None, None, None]
    u = torch.einsum("oc,cfhw->ofhw", pw, v) + pb[:, None, None, None]
    uabs = torch.einsum("oc,cfhw->ofhw", pw.abs(), v.abs()) + pb.abs()[:, None, None, None]
    bound = torch.einsum("oc,cfhw->ofhw", pw.abs(), rnd(v)) + acc(4, uabs) + rnd(u)
    inside = torch.ones_like(u)

    def cols(x):
        xp = F.pad(x, (1, 1, 1, 1, kt - 1, 0))
        c = [xp[:, a:a + Fr, b:b + H, d:d + W] for a in range(kt) for b in range(3) for d in range(3)]
        m = torch.stack(c, 0).permute(2, 3, 4, 0, 1).reshape(Fr * H * W, kt * 36)
        return torch.cat([m, torch.zeros(Fr * H * W, kcols - kt * 36, dtype=m.dtype)], dim=1)

    return cols(u), cols(bound), cols(inside) > 0


# ------------------------------------------------------------------------------------------------ row-wise family
# The kernels of csrc/rowwise.hip and csrc/t5_ops.hip that surround every GEMM: LayerNorm / RMS norm + modulate, patch embed, final layer,
# timestep embedding, the scheduler steps, the split-K finish.  Every reference is float64 from the bf16-exact (fp32-exact) operands,
# written from the definition on tensor axes; the gathers of per-sample vectors are the CALLER's (tests/rowwise_numerics_cases.py).
U_LIBM = 2.0**-21   # accuracy assumed for rsqrtf, expf, sinf, cosf (relative; absolute for sin / cos, whose values are <= 1): an assumption
                    # like U_EXP and U_RCP above — the device library documents a few ulp of fp32; it vanishes next to 2^-8


class RowStats:
    """mean / rstd of rows in float64 with the error of an fp32 kernel that holds the row in registers and takes TWO passes:
      e_mu   = acc(C, E|x|) + 2^-24 |mu|                       any order of an fp32 sum of C terms; the division by C
      d_var  = acc(C + 4, var) + e_mu^2                        sum (x - mu~)^2: the error c of the mean enters as c^2 ONLY (sum (x - mu) = 0),
                                                               each term carries the subtract's and the square's rounding, all terms >= 0
      r_rstd = d / (2 (1 - d)) + 2 2^-24 + U_LIBM, d = d_var / (var + eps)       the division by C, the + eps, rsqrtf
    There is no E[x^2] / (var + eps) factor anywhere: a one-pass E[x^2] - mu^2 does not fit.  ``rms``: no mean (T5LayerNorm), the same
    with mu = e_mu = 0 and var = E[x^2].  ``exact_mean`` [rows] bool: rows whose every partial sum is exact in fp32 in ANY order (the case
    says which: a constant 1.5, alternating +-2^-10), e_mu = 0 there."""

    def __init__(self, x, eps, rms=False, exact_mean=None):
        C = x.shape[-1]
        self.C = C
        self.mu = torch.zeros_like(x[..., :1]) if rms else x.mean(dim=-1, keepdim=True)
        d = x - self.mu
        self.var = (d * d).mean(dim=-1, keepdim=True)
        self.rstd = torch.rsqrt(self.var + eps)
        self.e_mu = torch.zeros_like(self.mu) if rms else acc(C, x.abs().mean(dim=-1, keepdim=True)) + U_F32 * self.mu.abs()
        if exact_mean is not None:
            self.e_mu = torch.where(exact_mean.reshape(self.mu.shape), torch.zeros_like(self.e_mu), self.e_mu)
        dd = (acc(C + 4, self.var) + self.e_mu**2) / (self.var + eps)
        assert float(dd.max()) < 0.5, "the statistics bound has broken down"
        self.r_rstd = dd / (2 * (1 - dd)) + 2 * U_F32 + U_LIBM
        self.n = d * self.rstd                       # the normalised row
        self.e_n = self.rstd * self.e_mu + self.n.abs() * (self.r_rstd + 2 * U_F32)     # + the subtract and the multiply


def ln_modulate_ref(x, eps, w=None, b=None, shift=None, scale=None, exact_mean=None):
    """LayerNorm + modulate, the contract of adaln_modulate / ln_modulate (rowwise.hip): fp32 up to ONE bf16 store,
    pre = ((x - mu) rstd w + b) (1 + scale) + shift  with w, b [C] and shift, scale [rows, C] ALREADY gathered per row (None = absent).
    With g = w (1 + scale) (the factors present), n = (x - mu) rstd:
      e_pre = |g| e_n + 8 2^-24 (|n g| + |b (1 + scale)| + |shift|)     e_n of RowStats carried through |g|; the <= 6 fp32 operations behind it
      bound = e_pre + rnd(pre).
    Returns (ref, bound, e_pre) [rows, C] float64."""
    st = RowStats(x, eps, exact_mean=exact_mean)
    one = torch.ones_like(x)
    g = one if w is None else one * w.double()
    off = torch.zeros_like(x) if b is None else one * b.double()
    if scale is not None:
        g, off = g * (1 + scale.double()), off * (1 + scale.double())
    sh = torch.zeros_like(x) if shift is None else shift.double()
    pre = st.n * g + off + sh
    e_pre = g.abs() * st.e_n + 8 * U_F32 * ((st.n * g).abs() + off.abs() + sh.abs())
    return pre, e_pre + rnd(pre), e_pre


def bf16_neighbours(v):
    """(vb, ulp, gap): ``v`` float64 rounded to bf16 (as float64), the distance from |vb| to the next bf16 value above it, and the distance
    from v to the nearer of the two rounding boundaries of vb's cell (the midpoints to its neighbours; the cell below a power of two is
    half as wide, which the neighbour below accounts for)."""
    vb16 = v.to(torch.bfloat16).abs()
    big, zero = torch.full_like(vb16, float("inf")), torch.zeros_like(vb16)
    up = torch.nextafter(vb16, big).double()
    dn = torch.where(vb16 > 0, torch.nextafter(vb16, zero), -torch.nextafter(vb16, big)).double()
    m = vb16.double()
    gap = torch.minimum((m + up) / 2 - v.abs(), v.abs() - (m + dn) / 2)
    return v.to(torch.bfloat16).double(), up - m, gap


class Tie:
    """An intermediate that the contract rounds to bf16, held by the NEAR-TIE rule instead of a worst-case rnd(): ``vb`` = bf16 of the
    float64 value, ``flag`` = the elements whose float64 value lies within the fp32 error ``e`` of a bf16 rounding boundary, ``err`` = one
    bf16 ulp of a flagged element and ZERO of an unflagged one (a kernel that follows the contract produces exactly ``vb`` there)."""

    def __init__(self, v, e):
        self.v, self.e = v, e
        self.vb, self.ulp, gap = bf16_neighbours(v)
        self.flag = gap <= e
        self.err = torch.where(self.flag, self.ulp, torch.zeros_like(self.ulp))

    def share(self) -> float:
        return float(self.flag.double().mean())


def final_layer_ref(x, table, tvec, w, bias, eps, exact_mean=None):
    """T2IFinalLayer on token rows x [B, R, C] (R = the rows of a sample), table [2, C], tvec [B, C], w [NOUT, C], bias [NOUT]:
      shift, scale = bf16(table[0] + t_b), bf16(table[1] + t_b)        one fp32 addition of two bf16 values (IEEE), rounded: determined
      a   = bf16(LN(x) (1 + scale) + shift)                            near-tie (Tie) with e_pre of ln_modulate_ref
      out = bf16(sum_c a_c w_nc + bias_n), widened to fp32             bound = sum_c tie_c |w_nc| + acc(C + 1, sum |a w| + |bias|) + rnd(out)
    Returns (ref, bound [B, R, NOUT], the Tie of a)."""
    B, R, C = x.shape
    tb = bf16_exact(table.float()[None] + tvec.float()[:, None])       # [B, 2, C]: ONE fp32 addition (IEEE: determined), then the rounding
    shift, scale = tb[:, 0:1].expand(B, R, C), tb[:, 1:2].expand(B, R, C)
    pre, _, e_pre = ln_modulate_ref(x.double().reshape(B * R, C), eps, shift=shift.reshape(B * R, C), scale=scale.reshape(B * R, C),
                                    exact_mean=exact_mean)
    tie = Tie(pre, e_pre)
    w64 = w.double()
    p = tie.vb @ w64.t() + bias.double()
    s = tie.vb.abs() @ w64.abs().t() + bias.double().abs()
    bound = tie.err @ w64.abs().t() + acc(C + 1, s) + rnd(p)
    return p.reshape(B, R, -1), bound.reshape(B, R, -1), tie


def unpatchify_ref(tok, T, Hp, Wp, patch, Cout, H, W):
    """tok [B, T Hp Wp, ph pw Cout] (channel order (dy, dx, co)) -> [B, Cout, T, H, W], cropped: STDiT3.unpatchify on tensor axes."""
    B = tok.shape[0]
    ph, pw = patch
    v = tok.reshape(B, T, Hp, Wp, ph, pw, Cout).permute(0, 6, 1, 2, 4, 3, 5).reshape(B, Cout, T, Hp * ph, Wp * pw)
    return v[:, :, :, :H, :W]


def patch_embed_ref(z, Bz_to_B, w, bias, pos, patch, C):
    """OpenSoraPatchEmbed3D + pos: z fp32 [Bz, Cin, T, H, W], sample b reads z[b % Bz] (``Bz_to_B`` = B), w [C, Cin, 1, ph, pw], bias [C],
    pos [S, C] -> [B, T, S, C].  x = bf16(z) at the load (one rounding of an fp32 value: determined); F.pad with zeros to whole patches;
      v   = bias + sum_k x_k w_k in fp32, then bf16          near-tie (Tie), e = acc(K + 1, sum |x w| + |bias|)
      out = bf16(bf16(v) + pos)                              bound = tie + 2^-24 |v + pos| + rnd(out)
    Returns (ref, bound [B, T, S, C], the Tie of v)."""
    import torch.nn.functional as F

    Bz, Cin, T, H, W = z.shape
    ph, pw = patch
    x = bf16_exact(z)
    x = F.pad(x, (0, (-W) % pw, 0, (-H) % ph))
    Hp, Wp = x.shape[3] // ph, x.shape[4] // pw
    x = x.repeat(Bz_to_B // Bz, 1, 1, 1, 1)                                         # torch.cat([z, z]): sample b = z[b % Bz]
    cols = x.reshape(Bz_to_B, Cin, T, Hp, ph, Wp, pw).permute(0, 2, 3, 5, 1, 4, 6).reshape(Bz_to_B, T, Hp * Wp, Cin * ph * pw)
    wk = w.double().reshape(C, -1)
    K = wk.shape[1]
    v = cols @ wk.t() + bias.double()
    s = cols.abs() @ wk.abs().t() + bias.double().abs()
    tie = Tie(v, acc(K + 1, s))
    tie.abs_sum = s                                                                 # sum_k |x_k w_k| + |bias|
    out = tie.vb + pos.double()
    return out, tie.err + U_F32 * out.abs() + rnd(out), tie


def rms_norm_ref(x, w, eps):
    """T5LayerNorm: out = bf16(w bf16(x rstd)), rstd = rsqrt(mean(x^2) + eps) in fp32.  n = x rstd is held by the near-tie rule with e_n of
    RowStats(rms); the product of two bf16 values is exact in fp32: bound = tie |w| + rnd(out).  Returns (ref, bound, Tie)."""
    st = RowStats(x.double(), eps, rms=True)
    tie = Tie(st.n, st.e_n)
    out = tie.vb * w.double()
    return out, tie.err * w.double().abs() + rnd(out), tie


def gelu_new64(a):
    import math

    return 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a**3)))


def geglu_ref(h):
    """T5DenseGatedActDense middle on h = [a | b] [rows, 2F]: out = bf16(bf16(gelu_new(a)) b).  The kernel forms gelu_new(a) = a / (1 + E),
    E = exp(-2 u), u = k0 a (1 + k1 a^2), with a fast exp2 and a fast reciprocal:
      e_g = |g| (U_RCP + 2 2^-24 + min(1, E) (U_EXP + 8 2^-24 (1 + |2 u|)))        the quotient, the sum; E's own error weighs E / (1 + E) <= min(1, E)
    (6 fp32 operations form the argument of the exp2, whose error |2 u| multiplies).  g is held by the near-tie rule; bound = tie |b| + rnd(out)."""
    import math

    F_ = h.shape[1] // 2
    a, b = h.double()[:, :F_], h.double()[:, F_:]
    g = gelu_new64(a)
    u2 = (2 * math.sqrt(2.0 / math.pi) * a * (1 + 0.044715 * a * a)).abs()
    E = torch.exp(-2 * math.sqrt(2.0 / math.pi) * a * (1 + 0.044715 * a * a))
    e_g = g.abs() * (U_RCP + 2 * U_F32 + E.clamp_max(1.0) * (U_EXP + 8 * U_F32 * (1 + u2)))
    tie = Tie(g, e_g)
    out = tie.vb * b
    return out, tie.err * b.abs() + rnd(out), tie


def timestep_embedding_ref(t, dim):
    """out[b] = [cos(a_k) | sin(a_k)], a_k = t_b exp(-ln(1e4) k / half), t fp32 [B].  The kernel's angle: the argument of expf is a product
    and a quotient of fp32 values (3 roundings with the constant's), expf, one product:
      e_a = |a| (3 2^-24 ln(1e4) k / half + U_LIBM + 2^-24);   bound = e_a + U_LIBM + rnd(out)       (|d cos| , |d sin| <= e_a)."""
    import math

    half = dim // 2
    k = torch.arange(half, dtype=torch.float64)
    arg = math.log(10000.0) * k / half
    a = t.double()[:, None] * torch.exp(-arg)[None]
    e_a = a.abs() * (3 * U_F32 * arg[None] + U_LIBM + U_F32)
    ref = torch.cat([torch.cos(a), torch.sin(a)], dim=1)
    return ref, torch.cat([e_a, e_a], dim=1) + U_LIBM + rnd(ref)


def f32(v: float) -> float:
    """A Python float as the kernel receives it (an fp32 argument)."""
    return float(torch.tensor(v, dtype=torch.float32))


def cfg_step_ref(z, model_out, guidance, c_z, c_eps, cond_first=True):
    """z' = c_z z + c_eps (u + g (c - u)) on the first Cin of model_out's Cout channels; model_out [2 Bz, Cout, ...], the conditional half
    first when ``cond_first``.  cfg_euler_step is c_z = 1, c_eps = dt.  fp32 in, fp32 out: three to four fp32 operations on the terms,
    bound = acc(4, |c_z z| + |c_eps| (|u| + |g| (|c| + |u|))) — an FMA contraction passes, there is no bf16 term."""
    Bz, Cin = z.shape[:2]
    g, c_z, c_eps = f32(guidance), f32(c_z), f32(c_eps)
    halves = model_out.double().reshape(2, Bz, *model_out.shape[1:])[:, :, :Cin]
    c, u = (halves[0], halves[1]) if cond_first else (halves[1], halves[0])
    ref = c_z * z.double() + c_eps * (u + g * (c - u))
    return ref, acc(4, abs(c_z) * z.double().abs() + abs(c_eps) * (u.abs() + abs(g) * (c.abs() + u.abs())))


def splitk_linear_ref(x, w, nsplit, res=None):
    """ops.linear_skinny: S = nsplit fp32 partials over slices of K (linear_ref's fp32 form: acc(Ks + 2, .) each, Ks = the longest slice),
    summed in fp32 by splitk_reduce[_t] (acc(S + 1, .)), one bf16 rounding; with a residual bf16(bf16(p) + res): one more rnd.
    Returns (ref, bound) [M, N]."""
    K = x.shape[1]
    Ks = -(-(K // 32) // nsplit) * 32
    p, s = matmul_ref(x, w)
    bound = acc(Ks + 2, s) + acc(nsplit + 1, s) + rnd(p)
    if res is not None:
        p = p + res.double()
        bound = bound + rnd(p)
    return p, bound


# ------------------------------------------------------------------------------------------------ GEMM family: activations, linear_small
# The activation epilogues of gemm_bf16.hip / gemm2_bf16.hip (EPI_BIAS_GELU) and linear_small_kernel.  An activation's output error is the
# size of the IMAGE of the argument's error interval, not a global slope times its width: in the tails of gelu_tanh and SiLU the slope is
# next to zero, and that is where the exp of the kernels' fast forms overflows (tests/gemm_numerics_cases.py).


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def _interior_minimum(fn, lo=-3.0, hi=0.0):
    """The one interior minimum of gelu_tanh / SiLU (both fall from 0 to it and rise from it on) by ternary search in float64; the value
    there is flat, so the few 1e-9 the argument is uncertain by move f(x*) by nothing a bound can see."""
    for _ in range(200):
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        fa, fb = float(fn(torch.tensor(a, dtype=torch.float64))), float(fn(torch.tensor(b, dtype=torch.float64)))
        lo, hi = (lo, b) if fa < fb else (a, hi)
    return 0.5 * (lo + hi)


GELU_XMIN = _interior_minimum(gelu_new64)    # -0.7525 (the erf form: -0.7518)
SILU_XMIN = _interior_minimum(silu64)        # -1.2785
ACTIVATIONS = {"none": (None, None), "silu": (silu64, SILU_XMIN), "gelu": (gelu_new64, GELU_XMIN)}


def act_image(act: str, p: torch.Tensor, d: torch.Tensor):
    """(f(p), max |f(y) - f(p)| over y in [p - d, p + d]) for f = ACTIVATIONS[act], float64.  f is monotone on either side of its one
    minimum x*, so the image's ends are f(p - d), f(p + d) and, where the interval holds x*, f(x*).  "none": (p, d)."""
    fn, xmin = ACTIVATIONS[act]
    if fn is None:
        return p, d
    y = fn(p)
    e = torch.maximum((fn(p - d) - y).abs(), (fn(p + d) - y).abs())
    inside = (p - d <= xmin) & (xmin <= p + d)
    fmin = fn(torch.tensor(xmin, dtype=torch.float64, device=p.device))
    return y, torch.where(inside, torch.maximum(e, (fmin - y).abs()), e)


def linear_small_ref(x, w, bias=None, act_in="none", act_out="none"):
    """linear_small_kernel (gemm_bf16.hip): x [M, K], w [N, K], bias [N] (bf16 values), one wave per output element:
      xe  = bf16(silu(x)) when act_in is SiLU (nn.SiLU on a bf16 tensor rounds before the Linear), else x: held by the near-tie rule (Tie)
            with e = |silu(x)| (U_LIBM + U_RCP + 3 2^-24) (expf, the division, the negation / sum / quotient in fp32);
      s   = sum_k xe_k w_k + bias in fp32 in any order:   e_p = tie.err @ |w|^T + acc(K + 1, sum |xe w| + |bias|);
      out = bf16(act_out(s)), the activation in fp32:     bound = image of [p - e_p, p + e_p] under act_out (act_image) + rnd(out)
            + (U_EXP + U_RCP + 8 2^-24) |out| where an activation runs (its fast exp, its reciprocal, the <= 8 fp32 operations around them).
    Returns (ref, bound [M, N] float64, the Tie of xe or None)."""
    K = x.shape[1]
    xd, wd = x.double(), w.double()
    tie = None
    terr = torch.zeros_like(xd)
    if act_in == "silu":
        v = silu64(xd)
        tie = Tie(v, v.abs() * (U_LIBM + U_RCP + 3 * U_F32))
        xd, terr = tie.vb, tie.err
    else:
        assert act_in == "none"
    bd = bias.double() if bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    p = xd @ wd.t() + bd
    e_p = terr @ wd.abs().t() + acc(K + 1, xd.abs() @ wd.abs().t() + bd.abs())
    out, e = act_image(act_out, p, e_p)
    bound = e + rnd(out)
    if act_out != "none":
        bound = bound + (U_EXP + U_RCP + 8 * U_F32) * out.abs()
    return out, bound, tie
