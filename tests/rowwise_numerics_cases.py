"""TEST INFRASTRUCTURE: the cases of the row-wise element-wise checks — seeded CPU operands, the call of the operation, and the float64
reference + bound of tests/numerics.py (row-wise family).  tests/test_gpu_numerics_rowwise.py runs the HIP kernels on them through
videosys_amd.ops / vchitect_ops, tests/test_numerics_rowwise_cpu.py the restatements of tests/rowwise_cpu_emul.py (and their planted
defects).  A case is a dict: ``call(impl, to)`` runs the operation on ``impl`` (an object with the wrappers' signatures) after moving
the operands with ``to`` and returns the output(s); ``ref`` / ``bound`` (float64) or ``exact`` (the bit pattern the output must have).

Which case reaches which template instantiation (launchers of csrc/rowwise.hip, csrc/t5_ops.hip):
  adaln_modulate_kernel<2>        ADALN  c8_*, c1024_*                       (c8: 1 of 64 lanes holds the row)
  adaln_modulate_kernel<3>        ADALN  c1032_r5, c1152_r5, c1152_odd15, c1536_r5, c1032_r1 .. (every odd rows_per_sample at 1024 < C <= 1536)
  adaln_modulate_rows_kernel<2>   ADALN  c1032_r4, c1152_r4, c1152_even17, c1536_r4        (even rows_per_sample; even17: the last wave holds ONE row)
  adaln_modulate_kernel<4>        ADALN  c1544_*, c2048_*
  ln_modulate_kernel<2>           LN     c8_*, c1024_*
  ln_modulate_kernel<3>           LN     c1032_* (every seg_split x every mode), c1536_*
  ln_modulate_kernel<4>           LN     c1544_*, c1920_*, c2048_*
  ln_modulate_kernel<6>           LN     c2056_*, c2304_*, c3072_*
  final_layer_kernel<2>           FINAL  c64_*, c1024_*      <3>  c1032_*, c1152_*, c1536_*      <4>  c1544_*, c2048_*   (and FINAL_TOKENS at c1152)
  rms_norm_rows_kernel<4>         RMS    c8_*, c72_*, c2048_*     <8>  c2056_*, c4096_*     <16>  c4104_*, c8192_*
  patch_embed_kernel, K == 16     PATCH  stdit_c8, stdit_c576, stdit_c1152 and the two shards
  patch_embed_kernel, generic     PATCH  cin8_2x2 (K = 32), cin16_1x1 (K = 16, NOT 2x2: the fall-through), cin4_2x4 (K = 32)

Rows of every LayerNorm / RMS case cycle through four kinds (row r has kind r % 4; a one-row case holds the probe):
  0  mean about 8, standard deviation about 0.25 (on the bf16 grid of [4, 16)): the cancellation probe (sharpened by cancel_probe where the
     row is modulated; mean 0.5 in the final_layer cases, see final_operands);
  1  generic, randn * 2 + 0.3;
  2  alternating +-2^-10: variance 2^-20, next to eps = 1e-6 (tells 1e-6 from 1e-5); every partial sum is exact;
  3  constant 1.5: every partial sum is exact in fp32 in any order, x - mean is exactly 0, so the output is exactly what the contract
     makes of a zero normalised row (the bf16 shift for adaln_modulate) — asserted bit for bit by the tests, on top of the bound.

Near-tie shares (numerics.Tie: the part of the bf16 intermediate that lies within its fp32 error bound of a rounding boundary).  A
condition on the INPUTS, asserted <= 5% for every case by tests/test_numerics_rowwise_cpu.py; as computed on the CPU:
  final_layer    c64_full_co4 0.07%  c1024_crop_co4 0.97%  c1032_full_co8 1.11%  c1152_crop_co8 1.15%  c1536_full_co4 1.57%  c1544_crop_co4 1.50%
                 c2048_full_co8 2.02%  c1152_full_co4 1.13%  c1152_full_co8 1.24%  c1152_crop_co4 1.10%  model_c64 0.07%  model_c1152 1.20%  model_c2048 1.87%
  patch_embed    stdit_c8 0.31%  stdit_c576 0.56%  stdit_c1152 0.57%  cin8_2x2 1.31%  cin16_1x1 0.99%  cin4_2x4 1.27%  stdit_shard_mid 0.48%
                 stdit_shard_past 0.51%  cin8_shard_past 1.88%
  rms_norm_rows  0.00% at one row and at C <= 72;  c2048_r4 0.56%  c2048_r5 0.50%  c2056_r4 0.63%  c2056_r5 0.37%  c4096_r4 3.21%  c4096_r5 2.36%
                 c4104_r4 1.13%  c4104_r5 0.95%  c8192_r4 2.94%  c8192_r5 1.99%
  geglu          small 0.28%  wrap 0.18%
(the share grows with C because the statistics' error bound is the order-agnostic acc(C, .); final_layer's operands are chosen for it, see
final_operands).  gate_add_rows and scale_add_rows need no near-tie rule: fp32 arithmetic on bf16 values followed by a rounding is
determined, so they are compared bit for bit (EXACT_CASES).
"""
import math
import os
import re

import torch

import numerics as nm

BF = torch.bfloat16
TIE_CAP = 0.05
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "videosys_amd", "csrc")


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def norm_rows(rows, C, gen, probe_mean=8.0):
    """[rows, C] bf16 of the four row kinds (module docstring) and the mask of the rows whose partial sums are exact."""
    x = torch.empty(rows, C)
    for r in range(rows):
        kind = r % 4
        if kind == 0:
            x[r] = probe_mean + 0.25 * torch.randn(C, generator=gen)
        elif kind == 1:
            x[r] = torch.randn(C, generator=gen) * 2 + 0.3
        elif kind == 2:
            x[r] = 2.0**-10 * (1 - 2 * (torch.arange(C) % 2))
        else:
            x[r] = 1.5
    exact = torch.tensor([r % 4 >= 2 for r in range(rows)])
    return x.to(BF), exact


def const_rows(rows):
    return [r for r in range(rows) if r % 4 == 3]


def mod_buffer(ns, C, stride, gen, nvec):
    """[ns, stride] bf16: ``nvec`` vectors of C per sample, even ones shift-like (O(1), sample b offset by 1.5 b), odd ones scale-like
    (0.1 randn - 0.3 + 0.25 b): a swap of shift and scale, or of two samples, moves the output by O(1).  The rest of the row is junk."""
    m = torch.full((ns, stride), 77.0)
    for b in range(ns):
        for v in range(nvec):
            m[b, v * C:(v + 1) * C] = (0.5 * torch.randn(C, generator=gen) + 1.0 + 1.5 * b) if v % 2 == 0 else \
                (0.1 * torch.randn(C, generator=gen) - 0.3 + 0.25 * b)
    return m.to(BF)


def cancel_probe(shift0, x0, eps, scale0=None, w=None, b=None):
    """Make the cancellation probe sharp: on every fourth channel the shift of the probe row's sample (``shift0`` [C], written in place)
    becomes minus the bf16 value of the row's modulated normalised value, so the output there is the small residual of two O(1) terms and
    an error of rstd shows at full size instead of hiding under the bf16 rounding of an O(1) output."""
    st = nm.RowStats(x0.double()[None], eps)
    t = st.n[0] * (1.0 if w is None else w.double())
    t = t + (0.0 if b is None else b.double())
    t = t * (1.0 if scale0 is None else 1 + scale0.double())
    shift0[::4] = (-t[::4]).to(BF)


def per_row(vec, rps, rows):
    """[ns, C] -> [rows, C]: row r reads sample r // rps."""
    return vec[:, None, :].expand(vec.shape[0], rps, vec.shape[1]).reshape(-1, vec.shape[1])[:rows]


# ------------------------------------------------------------------------------------------------ adaln_modulate
# name: (C, rows_per_sample, samples, rows cut off the end)
ADALN_ROWS = {"r1": (1, 1, 0), "r4": (2, 2, 0), "r5": (3, 2, 1)}      # r4: a 4-row block holds two samples; r5: odd rows_per_sample, the boundary inside block 0
ADALN_CASES = {f"c{C}_{k}": (C,) + v for C in (8, 1024, 1032, 1152, 1536, 1544, 2048) for k, v in ADALN_ROWS.items()}
ADALN_CASES["c1152_even17"] = (1152, 6, 3, 1)     # two rows per wave, the last wave holds one row; blocks of 8 rows straddle samples
ADALN_CASES["c1152_odd15"] = (1152, 5, 3, 0)      # the <3> fallback
ADALN_EPS = 1e-6


def adaln_case(name):
    C, rps, ns, cut = ADALN_CASES[name]
    gen = _gen("adaln" + name)
    rows = rps * ns - cut
    x, exact = norm_rows(rows, C, gen)
    stride = 6 * C + 8
    mod = mod_buffer(ns, C, stride, gen, 2)
    cancel_probe(mod[0, :C], x[0], ADALN_EPS, mod[0, C:2 * C])
    shift, scale = per_row(mod[:, :C], rps, rows), per_row(mod[:, C:2 * C], rps, rows)
    ref, bound, _ = nm.ln_modulate_ref(x.double(), ADALN_EPS, shift=shift, scale=scale, exact_mean=exact)

    def call(impl, to):
        m = to(mod)
        return impl.adaln_modulate(to(x), m[:, :C], m[:, C:2 * C], rps, stride, eps=ADALN_EPS)

    return dict(name=name, call=call, ref=ref, bound=bound, x=x, const_rows=const_rows(rows), const_value=shift, C=C, rps=rps)


# ------------------------------------------------------------------------------------------------ ln_modulate
LN_MODES = ("both", "affine", "mod", "neither")
LN_RPS, LN_NS = 3, 3          # 9 rows (8 with the cut): blocks of 4 straddle both sample boundaries
# name: (C, seg_split, mode, cut)
LN_CASES = {}
for _i, _C in enumerate((8, 1024, 1032, 1536, 1544, 1920, 2048, 2056, 2304, 3072)):
    LN_CASES[f"c{_C}_seg{_i % 4}_{LN_MODES[_i % 4]}"] = (_C, _i % 4, LN_MODES[_i % 4], _i % 2)
    LN_CASES[f"c{_C}_seg{(_i + 2) % 4}_{LN_MODES[(_i + 1) % 4]}"] = (_C, (_i + 2) % 4, LN_MODES[(_i + 1) % 4], 1 - _i % 2)
for _s in range(4):           # seg_split 0, 1, rows_per_sample - 1, rows_per_sample x every mode at one width
    for _m in LN_MODES:
        LN_CASES.setdefault(f"c1032_seg{_s}_{_m}", (1032, _s, _m, 0))
LN_EPS = 1e-5                 # (the wrapper's default: CogVideoX)


def ln_case(name):
    C, seg, mode, cut = LN_CASES[name]
    gen = _gen("ln" + name)
    rows = LN_RPS * LN_NS - cut
    x, exact = norm_rows(rows, C, gen)
    affine, modulated = mode in ("both", "affine"), mode in ("both", "mod")
    w = (1 + 0.3 * torch.randn(C, generator=gen)).to(BF) if affine else None
    b = (0.4 * torch.randn(C, generator=gen)).to(BF) if affine else None
    stride, alt = 6 * C + 8, 2 * C + 8
    mod = torch.full((LN_NS, stride), 77.0, dtype=BF)       # two blocks of (shift, scale): the main one at 0, the text one at ``alt``; junk around
    mod[:, :2 * C] = mod_buffer(LN_NS, C, 2 * C, gen, 2)
    mod[:, alt:alt + 2 * C] = -mod_buffer(LN_NS, C, 2 * C, gen, 2)
    shift = scale = None
    if modulated:
        o0 = alt if seg > 0 else 0          # the block row 0 reads
        cancel_probe(mod[0, o0:o0 + C], x[0], LN_EPS, mod[0, o0 + C:o0 + 2 * C], w, b)
        # rows whose position inside the sample is < seg_split read the vectors ``alt`` elements further on
        text = (torch.arange(LN_RPS) < seg)[None, :, None].expand(LN_NS, LN_RPS, C).reshape(-1, C)[:rows]
        shift = torch.where(text, per_row(mod[:, alt:alt + C], LN_RPS, rows), per_row(mod[:, :C], LN_RPS, rows))
        scale = torch.where(text, per_row(mod[:, alt + C:alt + 2 * C], LN_RPS, rows), per_row(mod[:, C:2 * C], LN_RPS, rows))
    ref, bound, _ = nm.ln_modulate_ref(x.double(), LN_EPS, w=w, b=b, shift=shift, scale=scale, exact_mean=exact)
    const_value = None        # (with an affine the zero row gives b (1 + scale) + shift: held by the bound, whose e_mu is 0 there)
    if not affine:
        const_value = shift if modulated else torch.zeros(rows, C, dtype=BF)

    def call(impl, to):
        m = to(mod)
        return impl.ln_modulate(to(x), None if w is None else to(w), None if b is None else to(b), m[:, :C] if modulated else None,
                                m[:, C:2 * C] if modulated else None, LN_RPS, mod_stride=stride, seg_split=seg, mod_alt=alt, eps=LN_EPS)

    return dict(name=name, call=call, ref=ref, bound=bound, x=x, const_rows=const_rows(rows), const_value=const_value, C=C, seg=seg)


# ------------------------------------------------------------------------------------------------ final_layer
FL_B, FL_T, FL_HP, FL_WP, FL_PATCH = 2, 2, 3, 2, (1, 2, 2)
FL_EPS = 1e-6
# name: (C, (H, W) crop, Cout, flavour of the Linear: see final_operands)
FINAL_CASES = {}
for _i, _C in enumerate((64, 1024, 1032, 1152, 1536, 1544, 2048)):
    FINAL_CASES[f"c{_C}_{'crop' if _i % 2 else 'full'}_co{4 + 4 * (_i // 2 % 2)}"] = (_C, (5, 3) if _i % 2 else (6, 4), 4 + 4 * (_i // 2 % 2), "sharp")
for _hw in ((6, 4), (5, 3)):
    for _co in (4, 8):
        FINAL_CASES.setdefault(f"c1152_{'crop' if _hw == (5, 3) else 'full'}_co{_co}", (1152, _hw, _co, "sharp"))
for _C in (64, 1152, 2048):
    FINAL_CASES[f"model_c{_C}"] = (_C, (5, 3), 8, "model")
FINAL_TOKENS_P = (2, 4)        # ranks: Sl = 3 (no padding), Sl = 2 (8 > 6 tokens: two padding tokens per frame)


def final_operands(name):
    """Operands of one FINAL_CASES entry.  The shift row of the table is O(3) and the t vectors are small (+-0.3, the two samples 0.6
    apart), so the activation a = LN(x) (1 + scale) + shift sits around 3 where a bf16 cell is wide: the worst-case error of an
    order-agnostic fp32 mean (acc(C, .), 2048 terms) then reaches a rounding boundary for under 5% of the activations.  For the same
    reason the probe row has mean 0.5, not 8.  ``sharp`` cases: w ~ 1 / sqrt(C), small bias — a wrong weight or activation shows.
    ``model`` cases: tiny weights (0.03 / sqrt(C)) and a bias of magnitude 3.2 .. 3.8, so every output lies in the upper part of
    [2, 4): there the bound's rnd(out) = 2^-8 |out| leaves room above the half ulp (2^-7) that the output's own rounding may take, and the
    rounding noise of the bf16 activations (about 1e-4 here) fits into it — the one regime in which an activation kept in fp32 passes."""
    C, (H, W), Cout, flavour = FINAL_CASES[name]
    gen = _gen("final" + name)
    S, nout = FL_HP * FL_WP, FL_PATCH[1] * FL_PATCH[2] * Cout
    x, exact = norm_rows(FL_B * FL_T * S, C, gen, probe_mean=0.5)
    table = torch.stack([0.3 * torch.randn(C, generator=gen) + 3.0, 0.1 * torch.randn(C, generator=gen)]).to(BF)     # [shift; scale] rows
    tvec = torch.stack([0.3 * torch.randn(C, generator=gen) + 0.3 * (1 - 2 * b) for b in range(FL_B)]).to(BF)
    sign = 1 - 2.0 * (torch.arange(nout) % 2)
    if flavour == "model":
        w = (0.03 * torch.randn(nout, C, generator=gen) / math.sqrt(C)).to(BF)
        bias = ((3.2 + 0.6 * torch.rand(nout, generator=gen)) * sign).to(BF)
    else:
        w = (torch.randn(nout, C, generator=gen) / math.sqrt(C)).to(BF)
        bias = (0.5 * torch.randn(nout, generator=gen)).to(BF)
    return dict(C=C, H=H, W=W, Cout=Cout, S=S, nout=nout, x=x, exact=exact, table=table, tvec=tvec, w=w, bias=bias, flavour=flavour)


def final_case(name):
    o = final_operands(name)
    C, S, H, W, Cout = o["C"], o["S"], o["H"], o["W"], o["Cout"]
    tok, tb, tie = nm.final_layer_ref(o["x"].reshape(FL_B, FL_T * S, C), o["table"], o["tvec"], o["w"], o["bias"], FL_EPS, exact_mean=o["exact"])
    pix = lambda t: nm.unpatchify_ref(t, FL_T, FL_HP, FL_WP, FL_PATCH[1:], Cout, H, W)

    def call(impl, to):
        return impl.final_layer(to(o["x"]), to(o["table"]), to(o["tvec"]), to(o["w"]), to(o["bias"]), FL_B, FL_T, FL_HP, FL_WP, H, W, FL_PATCH, Cout,
                                eps=FL_EPS)

    def call_tokens(impl, to, P):
        """The sequence-parallel route: every rank runs final_layer_tokens on its Sl tokens of every frame (padding tokens hold junk rows),
        the gathered [P, B, T, Sl, NOUT] goes through unpatchify_tokens."""
        Sl = -(-S // P)
        xs = torch.full((FL_B, FL_T, P * Sl, C), 3.0, dtype=BF)
        xs[:, :, :S] = o["x"].reshape(FL_B, FL_T, S, C)
        parts = [impl.final_layer_tokens(to(xs[:, :, r * Sl:(r + 1) * Sl].contiguous().reshape(-1, C)), to(o["table"]), to(o["tvec"]), to(o["w"]),
                                         to(o["bias"]), FL_B, FL_T, Sl, eps=FL_EPS) for r in range(P)]
        return impl.unpatchify_tokens(torch.stack(parts).contiguous(), P, FL_B, FL_T, Sl, FL_HP, FL_WP, H, W, FL_PATCH, Cout)

    return dict(o, name=name, call=call, call_tokens=call_tokens, ref=pix(tok), bound=pix(tb), tie=tie)


# ------------------------------------------------------------------------------------------------ patch_embed
# name: (Cin, (ph, pw), C, Bz, B, shard (s0, Sl) or None);  T = 2, H x W = 9 x 7 (odd: one padded row and column at 2x2)
PE_T, PE_H, PE_W = 2, 9, 7
PATCH_CASES = {
    "stdit_c8": (4, (2, 2), 8, 1, 2, None), "stdit_c576": (4, (2, 2), 576, 1, 2, None), "stdit_c1152": (4, (2, 2), 1152, 1, 2, None),
    "cin8_2x2": (8, (2, 2), 576, 2, 4, None),          # generic loop, K = 32; Bz = 2 -> B = 4: b % Bz differs from a clamped b
    "cin16_1x1": (16, (1, 1), 8, 2, 4, None),          # K = 16 but not 2x2: the fall-through of the K == 16 branch
    "cin4_2x4": (4, (2, 4), 1152, 1, 2, None),         # K = 32, W padded 7 -> 8
    "stdit_shard_mid": (4, (2, 2), 576, 1, 2, (8, 8)),     # s0 > 0
    "stdit_shard_past": (4, (2, 2), 576, 1, 2, (16, 8)),   # tokens 20 .. 23 do not exist: exactly zero rows
    "cin8_shard_past": (8, (2, 2), 8, 2, 4, (15, 7)),
}


def patch_operands(name):
    Cin, (ph, pw), C, Bz, B, shard = PATCH_CASES[name]
    gen = _gen("patch" + name)
    Hp, Wp = -(-PE_H // ph), -(-PE_W // pw)
    K = Cin * ph * pw
    z = torch.randn(Bz, Cin, PE_T, PE_H, PE_W, generator=gen) * 1.5          # fp32, NOT on the bf16 grid: the load rounds it
    w = (torch.randn(C, Cin, 1, ph, pw, generator=gen) / math.sqrt(K)).to(BF)
    bias = (0.5 * torch.randn(C, generator=gen)).to(BF)
    pos = torch.randn(Hp * Wp, C, generator=gen).to(BF)
    return dict(Cin=Cin, patch=(1, ph, pw), C=C, Bz=Bz, B=B, shard=shard, S=Hp * Wp, Hp=Hp, Wp=Wp, z=z, w=w, bias=bias, pos=pos)


def patch_case(name):
    o = patch_operands(name)
    ref, bound, tie = nm.patch_embed_ref(o["z"], o["B"], o["w"], o["bias"], o["pos"], o["patch"][1:], o["C"])
    zero_from = None
    if o["shard"] is not None:      # the tokens s0 .. s0 + Sl - 1; tokens past S are zero rows (bound 0: exactly zero)
        s0, Sl = o["shard"]
        pad = max(0, s0 + Sl - o["S"])
        cut = lambda t: torch.cat([t[:, :, s0:s0 + Sl], torch.zeros(o["B"], PE_T, pad, o["C"], dtype=t.dtype)], dim=2)
        ref, bound, zero_from = cut(ref), cut(bound), Sl - pad

    def call(impl, to):
        a = (to(o["z"]), to(o["w"]), to(o["bias"]), to(o["pos"]), o["B"], o["patch"], o["C"])
        return impl.patch_embed(*a) if o["shard"] is None else impl.patch_embed_shard(*a, *o["shard"])

    return dict(o, name=name, call=call, ref=ref, bound=bound, tie=tie, zero_from=zero_from)


# ------------------------------------------------------------------------------------------------ rms_norm_rows, geglu
RMS_CASES = {f"c{C}_r{r}": (C, r) for C in (8, 72, 2048, 2056, 4096, 4104, 8192) for r in (1, 4, 5)}
RMS_EPS = 1e-6


def rms_case(name):
    C, rows = RMS_CASES[name]
    gen = _gen("rms" + name)
    x, _ = norm_rows(rows, C, gen)
    w = (1 + 0.3 * torch.randn(C, generator=gen)).to(BF)
    ref, bound, tie = nm.rms_norm_ref(x, w, RMS_EPS)
    return dict(name=name, call=lambda impl, to: impl.rms_norm_rows(to(x), to(w), eps=RMS_EPS), ref=ref, bound=bound, tie=tie, x=x, w=w, C=C)


def launcher_cap(fname, launcher):
    """The grid cap (blocks) of ``launcher`` read from its source: ``if (grid > N) grid = N`` inside the launcher, or the cap of
    stream_grid() when the launcher uses that."""
    src = open(os.path.join(CSRC, fname)).read()
    body = src[src.index(f"int {launcher}("):]
    body = body[:body.index("\n}\n")]
    m = re.search(r"if \(grid > ([0-9* ]+)\) grid = ([0-9* ]+);", body)
    if m is None:
        assert "stream_grid(" in body, launcher
        m = re.search(r"b > (\d+) \? (\d+) : b", src)
    a, b = (math.prod(int(v) for v in g.split("*")) for g in m.groups())
    assert a == b
    return a


BLOCK = 256
# the caps the wrap cases below were sized for (blocks of 256 threads); tests/test_numerics_rowwise_cpu.py holds them against the launchers
CAPS = {"gate_add_rows": ("rowwise.hip", "launch_gate_add_rows", 8192), "add_rows": ("rowwise.hip", "launch_add_rows", 8192),
        "add_bcast_rows": ("rowwise.hip", "launch_add_bcast_rows", 8192), "scale_add_rows": ("rowwise.hip", "launch_scale_add_rows", 8192),
        "copy_4d": ("rowwise.hip", "launch_copy_4d", 8192), "geglu": ("t5_ops.hip", "launch_geglu", 8192),
        "gather_rows": ("t5_ops.hip", "launch_gather_rows", 8192), "im2col_patch": ("rowwise.hip", "launch_im2col_patch", 16384),
        "unpatchify_cvx": ("rowwise.hip", "launch_unpatchify_cvx", 16384)}
WRAP_ROWS_1152 = 14564         # x 144 chunks = 2 097 216 = 8192 x 256 + 64: the second trip of the grid-stride loop holds 64 chunks


def wraps(op, items):
    """True when ``items`` work items are a few more than one trip of the capped grid."""
    cap = CAPS[op][2] * BLOCK
    return cap < items <= cap + 16384 * 8


# geglu: name -> (rows, F, period).  The wrap case repeats a block of ``period`` rows: the bound is checked on the first and the last
# block (the last lies in the second trip), and every block must equal the first bit for bit (the kernel is element-wise).
GEGLU_CASES = {"small": (5, 72, None), "wrap": (8256, 2048, 64)}      # 8256 x 256 chunks = 8192 x 256 + 16384: rows 8192 .. are the second trip


def geglu_items(name):
    rows, F_, _ = GEGLU_CASES[name]
    return rows * (F_ // 8)


def geglu_case(name):
    rows, F_, period = GEGLU_CASES[name]
    gen = _gen("geglu" + name)
    n = rows if period is None else period
    blk = torch.cat([2.0 * torch.randn(n, F_, generator=gen), torch.randn(n, F_, generator=gen)], dim=1).to(BF)
    h = blk if period is None else blk.repeat(rows // period, 1)
    ref, bound, tie = nm.geglu_ref(blk)
    return dict(name=name, call=lambda impl, to: impl.geglu(to(h)), ref=ref, bound=bound, tie=tie, h=h, period=period, rows=rows)


# ------------------------------------------------------------------------------------------------ timestep embedding, scheduler steps
TIMESTEPS = [0.0, 1.0, 37.5, 999.0, 1000.0, 0.03125, 512.25]
TS_DIMS = (256, 6, 130)


def timestep_case(dim):
    t = torch.tensor(TIMESTEPS, dtype=torch.float32)
    ref, bound = nm.timestep_embedding_ref(t, dim)
    return dict(call=lambda impl, to: impl.timestep_embedding(to(t), dim), ref=ref, bound=bound, t=t, dim=dim)


# name: (kind, Bz, Cin, Cout, thw shape, cond_first)
CFG_CASES = {"euler": ("euler", 2, 4, 8, (3, 5, 7), True), "euler_cin_eq_cout": ("euler", 1, 4, 4, (2, 9, 31), True),
             "linear_cond_first": ("linear", 2, 4, 8, (3, 5, 7), True), "linear_uncond_first": ("linear", 2, 4, 8, (3, 5, 7), False),
             "linear_16ch": ("linear", 2, 16, 32, (1, 3, 3), False)}
CFG_G, CFG_DT, CFG_CZ, CFG_CEPS = 7.5, -0.0333, 1.0173, -0.2519


def cfg_case(name):
    kind, Bz, Cin, Cout, thw, cond_first = CFG_CASES[name]
    gen = _gen("cfg" + name)
    z = torch.randn(Bz, Cin, *thw, generator=gen)
    mo = torch.randn(2 * Bz, Cout, *thw, generator=gen)
    mo[Bz:] += 1.0                          # the halves differ: an inverted cond_first moves the result by O(g)
    if kind == "euler":
        ref, bound = nm.cfg_step_ref(z, mo, CFG_G, 1.0, CFG_DT, True)
        call = lambda impl, to: impl.cfg_euler_step(to(z).clone(), to(mo), CFG_G, CFG_DT)
    else:
        ref, bound = nm.cfg_step_ref(z, mo, CFG_G, CFG_CZ, CFG_CEPS, cond_first)
        call = lambda impl, to: impl.cfg_linear_step(to(z).clone(), to(mo), CFG_G, CFG_CZ, CFG_CEPS, cond_first=cond_first)
    return dict(name=name, call=call, ref=ref, bound=bound, z=z, mo=mo)


# ------------------------------------------------------------------------------------------------ split-K finish (ops.linear_skinny)
# (pad, nsplit, res, M): pad 128 = the 128-column kernel + splitk_reduce_t, pad 384 = the 256 x 384 tile + splitk_reduce
SKINNY_N, SKINNY_K = 256, 768        # slices of 256 columns at nsplit = 3
SKINNY_CASES = [(pad, ns, res, M) for pad in (128, 384) for ns in (1, 3) for res in (False, True) for M in (1, 37, 65)]


def skinny_case(pad, nsplit, res, M):
    gen = torch.Generator().manual_seed(pad + 10 * nsplit + M)
    Mp = -(-M // pad) * pad
    x = torch.full((Mp, SKINNY_K), float("nan"))      # rows past M are multiplied and never stored
    x[:M] = torch.randn(M, SKINNY_K, generator=gen)
    x = x.to(BF)
    w = (torch.randn(SKINNY_N, SKINNY_K, generator=gen) / math.sqrt(SKINNY_K)).to(BF)
    r = torch.randn(Mp, SKINNY_N, generator=gen).to(BF) if res else None
    ref, bound = nm.splitk_linear_ref(x[:M], w, nsplit, None if r is None else r[:M])
    call = lambda impl, to: impl.linear_skinny(to(x), M, to(w), res=None if r is None else to(r), nsplit=nsplit)[:M]
    return dict(call=call, ref=ref, bound=bound, x=x, w=w, r=r, M=M, nsplit=nsplit)


# ------------------------------------------------------------------------------------------------ exactly-defined kernels (bit for bit)
# Each entry: name -> builder returning dict(call=..., exact=<the tensor the output must equal bit for bit>, items=<work items of the
# launch>, op=<key of CAPS or None>).  ``exact`` is a torch restatement on tensor axes; bf16 arithmetic is fp32 arithmetic on bf16 values
# followed by one rounding (IEEE: determined), which is what the contract of every one of these kernels says.
def _bf(shape, gen, scale=1.0):
    return (scale * torch.randn(*shape, generator=gen)).to(BF)


def x_mod_table(name):
    gen = _gen("mod_table")
    nblk, B, C6 = 3, 2, 6 * 72
    table, t = _bf((nblk, C6), gen), _bf((B, C6), gen)
    exact = (table.float()[:, None] + t.float()[None]).to(BF)
    return dict(call=lambda impl, to: impl.mod_table(to(table), to(t)), exact=exact, items=0, op=None)


def x_add_rows(name):
    gen = _gen("add_rows" + name)
    n8 = 37 if name == "small" else CAPS["add_rows"][2] * BLOCK + 40
    x, y = _bf((n8, 8), gen), _bf((n8, 8), gen)
    return dict(call=lambda impl, to: impl.add_rows(to(x).clone(), to(y)), exact=(x.float() + y.float()).to(BF), items=n8, op="add_rows")


def x_add_bcast_rows(name):
    gen = _gen("add_bcast" + name)
    rows, C, group, period = (23, 72, 3, 4) if name == "small" else (WRAP_ROWS_1152, 1152, 7, 5)
    x, e = _bf((rows, C), gen), _bf((period + 1, C), gen)
    # row r reads e[(r // group) % period]: rows ordered (outer, period, group)
    n_outer = -(-rows // (group * period))
    ee = e[:period][None, :, None].expand(n_outer, period, group, C).reshape(-1, C)[:rows]
    return dict(call=lambda impl, to: impl.add_bcast_rows(to(x).clone(), to(e), group, period), exact=(x.float() + ee.float()).to(BF),
                items=rows * C // 8, op="add_bcast_rows")


def x_gate_add_rows(name):
    """x += bf16(gate * y): the product of two bf16 values is exact in fp32, so both roundings are determined.  Two segments per sample."""
    gen = _gen("gate_add" + name)
    rows, C, rps, seg = (23, 72, 6, 2) if name == "small" else (WRAP_ROWS_1152, 1152, 3641, 600)
    ns = -(-rows // rps)
    x, y = _bf((rows, C), gen), _bf((rows, C), gen)
    stride, alt = 6 * C + 8, 3 * C + 8
    gate = _bf((ns, stride), gen)
    text = (torch.arange(rps) < seg)[None, :, None].expand(ns, rps, C).reshape(-1, C)[:rows]
    g = torch.where(text, per_row(gate[:, alt:alt + C], rps, rows), per_row(gate[:, :C], rps, rows))
    exact = (x.float() + (g.float() * y.float()).to(BF).float()).to(BF)
    return dict(call=lambda impl, to: impl.gate_add_rows(to(x).clone(), to(y), to(gate)[:, :C], rps, stride, seg_split=seg, gate_alt=alt), exact=exact,
                items=rows * C // 8, op="gate_add_rows")


def x_scale_add_rows(name):
    """out = bf16(bf16(a * 1.1f) + b), every operand with a row stride larger than C."""
    gen = _gen("scale_add" + name)
    rows, C = (23, 72) if name == "small" else (WRAP_ROWS_1152, 1152)
    A, B_, O = _bf((rows, C + 8), gen), _bf((rows, C + 16), gen), torch.full((rows, C + 24), 5.0, dtype=BF)
    scale = nm.f32(1.1)
    exact = O.clone()
    exact[:, 8:8 + C] = ((A[:, :C].float() * torch.tensor(scale, dtype=torch.float32)).to(BF).float() + B_[:, 16:].float()).to(BF)

    def call(impl, to):
        o = to(O).clone()
        impl.scale_add_rows(to(A)[:, :C], to(B_)[:, 16:], 1.1, out=o[:, 8:8 + C])
        return o

    return dict(call=call, exact=exact, items=rows * C // 8, op="scale_add_rows")


def x_copy_4d(name):
    """dst[i0][i1][i2][:] = src[i0][i1][i2][:], zero where i1 >= n1_valid or i2 >= n2_valid; both sides strided (a permuted source)."""
    gen = _gen("copy4d" + name)
    n0, n1, n2, C, v1, v2 = (2, 3, 5, 72, 2, 4) if name == "small" else (2, 33, 250, 1024, 32, 249)
    src = _bf((n1, n0, n2, C + 8), gen)                       # stored (i1, i0, i2): the copy permutes the two outer axes
    dst = torch.full((n0, n1, n2, C), 5.0, dtype=BF)
    exact = torch.zeros(n0, n1, n2, C, dtype=BF)
    exact[:, :v1, :v2] = src.permute(1, 0, 2, 3)[:, :v1, :v2, :C]
    sstr, dstr = (src.stride(1), src.stride(0), src.stride(2)), (dst.stride(0), dst.stride(1), dst.stride(2))
    return dict(call=lambda impl, to: impl.copy_4d(to(src), to(dst).clone(), n0, n1, n2, C, sstr, dstr, n1_valid=v1, n2_valid=v2), exact=exact,
                items=n0 * n1 * n2 * C // 8, op="copy_4d")


def x_copy_4d_batch(name):
    gen = _gen("copy4dbatch")
    n0, n1, n2, C = 2, 3, 4, 16
    src = _bf((2, n0, n1, n2, C), gen)
    dst = torch.full((2, n0, n1 + 1, n2 + 1, C), 5.0, dtype=BF)
    exact = dst.clone()
    exact[:] = 0
    exact[:, :, :n1, :n2] = src
    sn, dn = src[0].numel(), dst[0].numel()
    ds = dst.stride()
    descs = [(p * sn, p * dn, n0, n1 + 1, n2 + 1, C, src.stride(1), src.stride(2), src.stride(3), ds[1], ds[2], ds[3], n1, n2) for p in range(2)]

    def call(impl, to):
        d = to(dst).clone()
        impl.copy_4d_batch(to(src), d, descs)
        return d

    return dict(call=call, exact=exact, items=0, op=None)


def x_gather_rows(name):
    gen = _gen("gather" + name)
    n, C, vocab = (9, 72, 11) if name == "small" else (CAPS["gather_rows"][2] * BLOCK // 64 + 3, 512, 100)
    table = _bf((vocab, C), gen)
    ids = torch.randint(0, vocab, (n,), generator=gen)
    ids[0], ids[1], ids[2], ids[-1], ids[-2] = -5, vocab + 7, vocab - 1, vocab, 0      # clamped at 0 and at vocab - 1
    return dict(call=lambda impl, to: impl.gather_rows(to(table), to(ids)), exact=table[ids.clamp(0, vocab - 1)], items=n * C // 8, op="gather_rows")


def x_im2col_patch(name):
    """out[(b, f, hp, wp)][(c, dy, dx)] = bf16(z[b % Bz][f][c][hp p + dy][wp p + dx])."""
    gen = _gen("im2col" + name)
    Bz, B, F_, Cin, H, W, p = (2, 4, 3, 16, 6, 10, 2) if name == "small" else (1, 2, 9, 16, 122, 122, 2)
    z = torch.randn(Bz, F_, Cin, H, W, generator=gen)
    zz = z.repeat(B // Bz, 1, 1, 1, 1)
    exact = zz.reshape(B, F_, Cin, H // p, p, W // p, p).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, Cin * p * p).to(BF)
    return dict(call=lambda impl, to: impl.im2col_patch(to(z), B, p), exact=exact, items=exact.numel(), op="im2col_patch")


def x_unpatchify_cvx(name):
    """x [(b, f, hp, wp)][ldx >= Cout p p], channel order (c, dy, dx) -> fp32 [B, F, Cout, Hp p, Wp p]."""
    gen = _gen("unpatch_cvx" + name)
    B, F_, Hp, Wp, Cout, p, ldx = (2, 3, 3, 5, 16, 2, 72) if name == "small" else (2, 9, 61, 61, 16, 2, 72)
    x = _bf((B * F_ * Hp * Wp, ldx), gen)
    exact = x[:, :Cout * p * p].float().reshape(B, F_, Hp, Wp, Cout, p, p).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, F_, Cout, Hp * p, Wp * p)
    return dict(call=lambda impl, to: impl.unpatchify_cvx(to(x), B, F_, Hp, Wp, Cout, p), exact=exact.contiguous(), items=exact.numel(), op="unpatchify_cvx")


def x_unpatchify_tokens(name):
    """tok [P, B, T, Sl, (dy, dx, co)] (rank r holds tokens r Sl ..; tokens >= Hp Wp are padding) -> [B, Cout, T, H, W], cropped."""
    gen = _gen("unpatch_tok" + name)
    P, B, T, Hp, Wp, H, W, Cout = 4, 2, 2, 3, 2, 5, 3, 8
    Sl = -(-Hp * Wp // P)
    tok = torch.randn(P, B, T, Sl, 4 * Cout, generator=gen)
    seq = tok.permute(1, 2, 0, 3, 4).reshape(B, T, P * Sl, 4 * Cout)[:, :, :Hp * Wp].reshape(B, T * Hp * Wp, 4 * Cout)
    exact = nm.unpatchify_ref(seq, T, Hp, Wp, (2, 2), Cout, H, W).contiguous()
    return dict(call=lambda impl, to: impl.unpatchify_tokens(to(tok), P, B, T, Sl, Hp, Wp, H, W, (1, 2, 2), Cout), exact=exact, items=0, op=None)


EXACT_CASES = {"mod_table": (x_mod_table, ("small",)), "add_rows": (x_add_rows, ("small", "wrap")),
               "add_bcast_rows": (x_add_bcast_rows, ("small", "wrap")), "gate_add_rows": (x_gate_add_rows, ("small", "wrap")),
               "scale_add_rows": (x_scale_add_rows, ("small", "wrap")), "copy_4d": (x_copy_4d, ("small", "wrap")),
               "copy_4d_batch": (x_copy_4d_batch, ("small",)), "gather_rows": (x_gather_rows, ("small", "wrap")),
               "im2col_patch": (x_im2col_patch, ("small", "wrap")), "unpatchify_cvx": (x_unpatchify_cvx, ("small", "wrap")),
               "unpatchify_tokens": (x_unpatchify_tokens, ("small",))}
EXACT_IDS = [(op, size) for op, (_, sizes) in EXACT_CASES.items() for size in sizes]


def exact_case(op, size):
    return EXACT_CASES[op][0](size)
