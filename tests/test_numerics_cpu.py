"""The element-wise bound of tests/numerics.py on synthetic data (no GPU): a correctly rounded result and a result with one
rounding fewer than the contract pass; each of four planted GEMM defects fails, and the failure names the tile.  Second half: the
softmax-attention bound (numerics.attention_ref) against a CPU emulation of the d72 flash contract and its planted defects.  Third part:
the VAE family's bounds (conv / gemm128, GroupNorm, SpatialNorm, softmax_rows, first layer) against the restatements of
tests/vae_cpu_emul.py and their planted defects, and the refusal of ops.conv for temporal taps over more than one sample.  Fourth part:
the GEMM family beyond STDiT3's launches (GELU store, the per-row two-segment gate, linear_small: tests/gemm_numerics_cases.py) against
the restatements of tests/gemm_cpu_emul.py and their planted defects."""
import pytest
import torch
import torch.nn.functional as F

import attn_families as fam
import gemm_cpu_emul as gemu
import gemm_numerics_cases as gc
import numerics as nm
import vae_cpu_emul as emu
import vae_numerics_cases as vc

M, N, K = 1024, 384, 1024


def _operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K**0.5).to(torch.bfloat16)
    # a bias of the accumulator's own scale: the epilogue's sum then cancels on many elements, where an extra rounding shows
    b = torch.randn(N, generator=g).to(torch.bfloat16)
    return a, w, b


def _bias_case(seed=0):
    """Contract: out = bf16(a @ w^T + b), fp32 accumulation.  Chain: acc(K) + one rounding of the output."""
    a, w, b = _operands(seed)
    ref, s = nm.matmul_ref(a, w)
    ref = ref + b.double()
    bound = nm.acc(K, s + b.double().abs()) + nm.rnd(ref)
    return a, w, b, ref, bound


def _check(out, ref, bound, what="synthetic"):
    nm.Bound(what).add(out, ref, bound).check()


def test_correctly_rounded_result_passes():
    a, w, b, ref, bound = _bias_case()
    _check(ref.to(torch.bfloat16), ref, bound)
    # the fp32-accumulated form the kernels compute passes too
    _check((a.float() @ w.float().t() + b.float()).to(torch.bfloat16), ref, bound)


def test_element_two_ulps_off_fails():
    a, w, b, ref, bound = _bias_case()
    out = ref.to(torch.bfloat16)
    bits = out.view(torch.int16)
    r, c = 700, 200
    bits[r, c] += 2                      # two ulps away from the correctly rounded value (same sign, same binade or the next)
    with pytest.raises(AssertionError, match=r"1 of .* worst at \(row 700, col 200\) \[256-row tile 2, 128-row tile 5, 192-col tile 1\]"):
        _check(out, ref, bound)


def test_partial_sums_rounded_to_bf16_every_64_terms_fail():
    a, w, b, ref, bound = _bias_case()
    part = torch.zeros(M, N, dtype=torch.bfloat16)
    for k0 in range(0, K, 64):
        part = (part.float() + a[:, k0:k0 + 64].float() @ w[:, k0:k0 + 64].float().t()).to(torch.bfloat16)
    out = (part.float() + b.float()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="outside the bound"):
        _check(out, ref, bound)


def test_extra_rounding_in_the_epilogue_fails():
    """bf16(bf16(acc) + b): the accumulator rounded before the bias is added (the contract adds in fp32, then rounds once)."""
    a, w, b, ref, bound = _bias_case()
    accum = (a.float() @ w.float().t()).to(torch.bfloat16)
    out = (accum.float() + b.float()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="outside the bound"):
        _check(out, ref, bound)


def test_unwritten_256_row_tile_fails_and_is_named():
    a, w, b, ref, bound = _bias_case()
    out = ref.to(torch.bfloat16)
    out[512:768] = 0
    with pytest.raises(AssertionError, match=r"98\d\d\d of .* \[256-row tile 2,"):
        _check(out, ref, bound)


def test_chunked_check_reports_global_rows():
    a, w, b, ref, bound = _bias_case()
    out = ref.to(torch.bfloat16)
    out[900, 17] = float("nan")
    rep = nm.Bound("chunks")
    for r0, r1 in nm.row_chunks(M, 256):
        rep.add(out[r0:r1], ref[r0:r1], bound[r0:r1], row0=r0)
    with pytest.raises(AssertionError, match=r"1 of 393216 .* \(row 900, col 17\)"):
        rep.check()


def test_gate_residual_chain_accepts_one_rounding_fewer():
    """Contract x + g * proj(a) = bf16(x + bf16(g * bf16(a W^T + b))): three roundings.  The bound built from that chain accepts
    the contract itself, the two-rounding form the GEMM epilogue computes (bf16(x + bf16(g (acc + b)))) and a single rounding."""
    a, w, b = _operands(1)
    g = torch.Generator().manual_seed(2)
    b = (b.float() * 0.1).to(torch.bfloat16)
    gate = torch.randn(N, generator=g).to(torch.bfloat16)
    x = torch.randn(M, N, generator=g).to(torch.bfloat16)
    p, s = nm.matmul_ref(a, w)
    p = p + b.double()
    gd, xd = gate.double(), x.double()
    ref = xd + gd * p
    bound = gd.abs() * (nm.acc(K, s + b.double().abs()) + nm.rnd(p)) + nm.rnd(gd * p) + nm.rnd(ref)
    acc32 = a.float() @ w.float().t() + b.float()
    three = (x.float() + (gate.float() * acc32.to(torch.bfloat16).float()).to(torch.bfloat16).float()).to(torch.bfloat16)
    two = (x.float() + (gate.float() * acc32).to(torch.bfloat16).float()).to(torch.bfloat16)
    one = ref.to(torch.bfloat16)
    for out in (three, two, one):
        _check(out, ref, bound, "gate + residual")
    # ... and the gate of the neighbouring sample on one 128-row tile does not pass
    bad = two.clone()
    gate2 = torch.randn(N, generator=g).to(torch.bfloat16)
    bad[256:384] = (x[256:384].float() + (gate2.float() * acc32[256:384]).to(torch.bfloat16).float()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match=r"128-row tile 2,"):
        _check(bad, ref, bound, "gate + residual")


# ------------------------------------------------------------------------------------------------ softmax attention


def emulate_d72(qh, kp, v, kv_len, *, static_m=None, defect=None):
    """The d72 flash contract in fp32 / bf16 on the CPU (attention.hip): 64-key tiles, online softmax in the exp2 domain, P rounded to
    bf16, the row sum taken from the rounded P, O and the row sum rescaled only when some row of a 32-row group sees a tile maximum
    more than 8 above the adopted one (the first tile adopts its maximum, signed), one final division, bf16 output.  ``static_m``
    [Lq]: the form without a running maximum (subtract |q^| k_bound, never rescale).  kp / v [kv_pad, 72] hold what lies behind kv_len
    (zeros after attn_prep_kv).  ``defect`` plants one of the errors the bound must catch."""
    Lq, kv_pad = qh.shape[0], kp.shape[0]
    q32, k32, v32 = qh.float(), kp.float(), v.float()
    limit = kv_pad if defect == "mask_at_kv_pad" else kv_len - 1 if defect == "drop_last_key" else kv_len
    m = torch.zeros(Lq, 1) if static_m is None else static_m.float()[:, None]
    o, l = torch.zeros(Lq, v.shape[1]), torch.zeros(Lq, 1)
    for t in range(kv_pad // 64):
        ks, vs = k32[64 * t:64 * t + 64], v32[64 * t:64 * t + 64]
        s = q32 @ ks.t() - m
        s[:, max(0, limit - 64 * t):] = -1e30
        if static_m is None:
            mx = s.amax(dim=1, keepdim=True)
            for r0 in range(0, Lq, 32):
                g = slice(r0, r0 + 32)
                if t == 0 or bool((mx[g] > 8.0).any()):
                    delta = mx[g] if t == 0 else mx[g].clamp_min(0.0)
                    m[g] += delta
                    s[g] -= delta
                    stale = defect == "stale_scale" or (defect == "stale_scale_8_to_16" and bool(((delta > 8.0) & (delta <= 16.0)).any()))
                    if t != 0 and not stale:
                        o[g] *= torch.exp2(-delta)
                        l[g] *= torch.exp2(-delta)
        p = torch.exp2(s).to(torch.bfloat16)
        if defect == "p_4_bits":
            p = (p.view(torch.int16) & -16).view(torch.bfloat16)     # 7 stored significand bits -> 3 (+ the hidden one)
        if defect == "swap_v_columns" and t == 1:
            vs = vs.clone()
            vs[[3, 17]] = vs[[17, 3]]
        o += p.float() @ vs
        if not (defect == "rowsum_tile0" and t > 0):
            l += p.float().sum(dim=1, keepdim=True)
    if defect == "rowsum_tile0":
        l = l * (kv_pad // 64)     # (scaled so that the defect is not a trivial factor: still the wrong sum)
    out = (o / l).to(torch.bfloat16)
    if defect == "row_xor_32":
        idx = torch.arange(Lq) ^ 32
        out = out[torch.where(idx < Lq, idx, torch.arange(Lq))]
    return out


ATTN_LQ = 128
DEFECTS = ("drop_last_key", "swap_v_columns", "stale_scale", "stale_scale_8_to_16", "rowsum_tile0", "p_4_bits", "row_xor_32", "mask_at_kv_pad")


@pytest.fixture(scope="module")
def attn_cases():
    """(family, kv_len) -> operands, float64 reference and bound; computed once, never modified."""
    cases = {}
    for kv_len in (1024, 65, 321):
        for name, build in fam.FAMILIES.items():
            if (name == "ramps" and kv_len < 320) or (name == "two_key" and kv_len % 64 == 0):
                continue
            c = build(ATTN_LQ, kv_len, 100 + kv_len)
            kv_pad = -(-kv_len // 64) * 64
            kp = torch.zeros(kv_pad, fam.HD, dtype=torch.bfloat16)
            vp = torch.zeros(kv_pad, fam.HD, dtype=torch.bfloat16)
            kp[:kv_len], vp[:kv_len] = fam.prep_k(c["k"]), c["v"]
            # what a buffer prepared for a longer text holds behind kv_len: finite, non-zero (only the kv_pad mask defect reads it)
            g = torch.Generator().manual_seed(kv_len)
            kp_dirty, vp_dirty = kp.clone(), vp.clone()
            kp_dirty[kv_len:] = (0.2 * torch.randn(kv_pad - kv_len, fam.HD, generator=g)).to(torch.bfloat16)
            vp_dirty[kv_len:] = torch.randn(kv_pad - kv_len, fam.HD, generator=g).to(torch.bfloat16)
            ref = nm.attention_ref(c["q"].double(), kp[:kv_len].double(), vp[:kv_len].double(), targets=c["targets"])
            assert ref.vacuous == 0
            if c["targets"] is not None:
                fam.check_targets(ref, c, f"{name} kv_len={kv_len}")
            if name == "ramps":
                fam.check_ladders(ref.logits, c["levels"], f"ramps kv_len={kv_len}")
            cases[name, kv_len] = dict(c, kp=kp_dirty, vp=vp_dirty, ref=ref, kv_len=kv_len)
    return cases


def _passes(out, case):
    rep = nm.Bound("attention").add(out, case["ref"].out, case["ref"].bound)
    return rep.bad == 0


def test_attention_emulation_passes_on_every_family(attn_cases):
    for (name, kv_len), c in attn_cases.items():
        out = emulate_d72(c["q"], c["kp"], c["vp"], kv_len)
        nm.Bound(f"d72 emulation, {name}, kv_len={kv_len}").add(out, c["ref"].out, c["ref"].bound).check()
        if c["expect"] is not None:     # retrieval / two-key: v of the targets to about one bf16 ulp
            assert ((out.double() - c["expect"]).abs() <= 2.0**-7 * c["expect"].abs() + 2.0**-9).all()


def test_attention_emulation_without_running_max_passes(attn_cases):
    """Subtract |q^| k_bound (k_bound = the largest Kp row norm) instead of a running maximum: same softmax, same bound with M raised."""
    for (name, kv_len), c in attn_cases.items():
        kb = c["kp"][:kv_len].float().norm(dim=1).max()
        m = c["q"].float().norm(dim=1) * kb
        if float(m.max()) > 120.0:      # (far outside the kernels' promise |q| k_bound <= 60: P would leave fp32's range)
            continue
        out = emulate_d72(c["q"], c["kp"], c["vp"], kv_len, static_m=m)
        ref = nm.attention_ref(c["q"].double(), c["kp"][:kv_len].double(), c["vp"][:kv_len].double(), m_extra=m.double())
        nm.Bound(f"d72 emulation without running max, {name}, kv_len={kv_len}").add(out, ref.out, ref.bound).check()


# which families must catch which planted defect (at least these; the test also requires that NOTHING passes everywhere)
CAUGHT_BY = {
    ("drop_last_key", 1024): ("retrieval",), ("drop_last_key", 65): ("retrieval", "two_key"),
    ("swap_v_columns", 1024): ("retrieval",), ("stale_scale", 1024): ("ramps",), ("stale_scale_8_to_16", 1024): ("ramps",), ("rowsum_tile0", 1024): ("diffuse", "retrieval"),
    ("p_4_bits", 1024): ("diffuse",), ("row_xor_32", 1024): ("diffuse", "retrieval"), ("mask_at_kv_pad", 65): ("diffuse",),
    ("mask_at_kv_pad", 321): ("diffuse", "ramps"),
}


@pytest.mark.parametrize("defect,kv_len", sorted(CAUGHT_BY))
def test_attention_planted_defect_fails(attn_cases, defect, kv_len):
    caught = {name for (name, n), c in attn_cases.items() if n == kv_len and not _passes(emulate_d72(c["q"], c["kp"], c["vp"], kv_len, defect=defect), c)}
    print(f"{defect} at kv_len={kv_len}: caught by {sorted(caught)}")
    assert set(CAUGHT_BY[defect, kv_len]) <= caught, f"{defect} at kv_len={kv_len} is caught only by {sorted(caught)}"


def test_attention_bound_fp32_denominator_form():
    """The temporal contract (weights normalised in fp32, THEN rounded to bf16) passes the "fp32" form; on a two-key row (weights 1/2)
    it also passes the "rounded" form, but on diffuse rows it must not be held to it: the rounded weights no longer sum to 1."""
    c = fam.diffuse(64, 40, 5)
    q, k, v = c["q"].double() * fam.HD**-0.5, c["k"].double(), c["v"].double()
    s = (q @ k.t()).float()
    w = torch.softmax(s, dim=1).to(torch.bfloat16)
    out = (w.float() @ v.float()).to(torch.bfloat16)
    ref = nm.attention_ref(q, k, v, log2_scale=1.4426950408889634, denominator="fp32")
    nm.check_elementwise(out, ref.out, ref.bound, "fp32-denominator emulation")
    out_bad = (w.float() @ v.float().roll(1, 0)).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="outside the bound"):
        nm.check_elementwise(out_bad, ref.out, ref.bound, "fp32-denominator emulation, v shifted by one key")


# ------------------------------------------------------------------------------------------------ VAE family
# The bounds of numerics.linear_ref / group_norm_ref / softmax_rows_ref / first_im2col_ref on the cases of tests/vae_numerics_cases.py:
# the restatements of tests/vae_cpu_emul.py (fp32 arithmetic, bf16 storage: the kernels' contract) pass, every planted defect fails.
NBLK = 128     # ops._GN_NBLK (asserted below)


def _fails(out, ref, bound):
    return nm.Bound("defect").add(out, ref, bound).bad > 0


def test_gn_nblk_is_the_wrappers():
    from videosys_amd import ops

    assert ops._GN_NBLK == NBLK


@pytest.mark.parametrize("kt,ks,pad", [(1, 3, 1), (3, 3, 1), (3, 1, 0), (3, 1, 1)])
def test_conv_gather_reference_is_conv3d_in_float64(kt, ks, pad):
    """numerics.conv_gather + one float64 matmul = F.conv3d in float64 over the zero-padded volume (two samples: the gather works on
    voxel coordinates, so it has no trouble with n > 1)."""
    from videosys_amd.ops import VaeGrid

    n, T, H, W, cin, cout = 2, 3, 4, 5, 32, 8
    gen = torch.Generator().manual_seed(kt * 10 + ks + pad)
    x5 = torch.randn(n, T, H, W, cin, generator=gen).to(torch.bfloat16)
    w = torch.randn(cout, kt, ks, ks, cin, generator=gen).to(torch.bfloat16)
    g = VaeGrid(n, T, H, W, pad, kt - 1)
    rows = vc.grid_rows(vc.storage(x5, g, border=0.0), g)
    got = nm.conv_gather(rows, g, cin, kt, ks) @ w.double().reshape(cout, -1).t()
    sp = ks // 2
    want = F.conv3d(F.pad(x5.double().permute(0, 4, 1, 2, 3), (sp, sp, sp, sp, kt - 1, 0)), w.double().permute(0, 4, 1, 2, 3))
    # (two float64 sums of the same exact products in different orders)
    assert (got.reshape(n, T, H, W, cout) - want.permute(0, 2, 3, 4, 1)).abs().max().item() <= 1e-12


@pytest.fixture(scope="module")
def conv_cases():
    return {name: vc.conv_case(name) for name in vc.CONV_CASES}


def _interior_rows(out_rows, c):
    return nm.grid_interior(out_rows, c["og"], c["cout"]).reshape(-1, c["cout"])


def test_conv_restatements_pass_on_every_case(conv_cases):
    for name, c in conv_cases.items():
        a, res = vc.grid_rows(c["a_buf"], c["g"]), vc.conv_res_rows(c)
        out = emu.conv(a, c["g"], c["w"], c["b"], c["cin"], c["kt"], c["ks"], res=res)
        nm.Bound(f"conv (conv3d restatement) {name}").add(_interior_rows(out, c), c["ref"], c["bound"]).check()
        if c["g"].n == 1:
            out = emu.conv_taps(a, c["g"], c["w"], c["b"], c["cin"], c["kt"], c["ks"], res=res)
            nm.Bound(f"conv (row-shift restatement) {name}").add(_interior_rows(out, c), c["ref"], c["bound"]).check()


@pytest.mark.parametrize("defect,names", [("bf16_partials", ("27taps_M312", "cshift2_108tiles", "time_only_pad0", "M35_9tiles")),
                                          ("ktile_left", ("27taps_M312", "cshift2_108tiles", "time_only_pad1", "xcd_27tiles")),
                                          ("res_next_row", ("27taps_M312", "time_only_pad0"))])
def test_conv_planted_defect_fails(conv_cases, defect, names):
    for name in names:
        c = conv_cases[name]
        out = emu.conv_taps(vc.grid_rows(c["a_buf"], c["g"]), c["g"], c["w"], c["b"], c["cin"], c["kt"], c["ks"], res=vc.conv_res_rows(c), defect=defect)
        assert _fails(_interior_rows(out, c), c["ref"], c["bound"]), f"{defect} passes on {name}"


def test_gemm128_restatement_passes_and_fp32_form_has_no_bf16_term():
    for K in vc.GEMM_K:
        for M in (1, 257):
            a, w, b, r = vc.gemm_operands(M, 128, K, K + M)
            for bias, res in ((None, None), (b, None), (None, r), (b, r)):
                ref, bound = nm.linear_ref(a, w, bias, res)
                nm.check_elementwise(emu.gemm128(a, w, bias, res), ref, bound, f"gemm128 K={K} M={M}")
    a, w, _, _ = vc.gemm_operands(200, 256, 64, 3)
    ref, bound = nm.linear_ref(a, w, out_scale=0.125)
    s32 = (a.float() @ w.float().t()) * 0.125
    nm.check_elementwise(s32, ref, bound, "fp32 score form")
    with pytest.raises(AssertionError, match="outside the bound"):       # scores rounded to bf16 on the way: what the form exists to avoid
        nm.check_elementwise(s32.to(torch.bfloat16), ref, bound, "fp32 score form through bf16")


@pytest.fixture(scope="module")
def gn_cases():
    return {name: vc.gn_case(name, NBLK, small=True) for name in vc.GN_CASES}


def _gn_emulated(c, defect=None):
    mean, rstd = emu.gn_stats_geometry(c["x5"], c["groups"], vc.GN_EPS, NBLK, defect=defect)
    return emu.gn_apply_chunks(c["x5"], mean, rstd, c["groups"], c["gamma"], c["beta"], c["silu"], defect=defect)


def test_group_norm_restatements_pass_on_every_case(gn_cases):
    for name, c in gn_cases.items():
        r = c["r"]
        nm.Bound(f"group norm (kernel-order restatement) {name}").add(_gn_emulated(c), r.ref.reshape(-1, c["C"]), r.bound.reshape(-1, c["C"])).check()
        # ... and through the wrapper-shaped restatement (torch's own fp32 group_norm), destination grid included
        y = c["y_buf"].clone()
        emu.group_norm(vc.grid_rows(c["x_buf"], c["gs"]), c["gs"], vc.grid_rows(y, c["gd"]), c["gd"], c["C"], c["gamma"], c["beta"], vc.GN_EPS,
                       c["silu"], groups=c["groups"])
        nm.Bound(f"group norm (torch restatement) {name}").add(nm.grid_interior(vc.grid_rows(y, c["gd"]), c["gd"]).reshape(-1, c["C"]),
                                                                r.ref.reshape(-1, c["C"]), r.bound.reshape(-1, c["C"])).check()
        assert vc.outside_interior_unchanged(y, c["y_buf"], c["gd"], c["C"])
    off = gn_cases["offset_mean8"]["r"]
    print(f"offset case: the rstd (cancellation) term takes up to {off.cancel_share():.3f} of an element's bound at n_t = {off.n_t}")
    assert off.n_t == 8 and 0.0 < off.cancel_share() < 1.0


@pytest.mark.parametrize("defect,names", [("upper_half_stats", ("two_samples_cg4", "cg12_idle", "cg12_silu_pad")), ("sample0_stats", ("two_samples_cg4",)),
                                          ("q_bf16", ("8_per_thread", "offset_mean8", "65552_rows"))])
def test_group_norm_planted_defect_fails(gn_cases, defect, names):
    for name in names:
        c = gn_cases[name]
        assert _fails(_gn_emulated(c, defect), c["r"].ref.reshape(-1, c["C"]), c["r"].bound.reshape(-1, c["C"])), f"{defect} passes on {name}"


def test_spatial_norm_restatement_passes_and_the_next_latent_voxel_fails():
    for T, zT, C in vc.SN_CASES:
        c = vc.sn_case(T, zT, C, NBLK)
        mean, rstd = emu.gn_stats_geometry(c["x5"], c["groups"], vc.GN_EPS, NBLK)
        ref, bound = c["r"].ref.reshape(-1, C), c["r"].bound.reshape(-1, C)
        maps = emu.spatial_norm_gather(c["yb"], c["n"], C, c["zdims"], c["x5"].shape[1:4])
        out = emu.gn_apply_chunks(c["x5"], mean, rstd, c["groups"], c["gamma"], c["beta"], True, yb=maps)
        nm.Bound(f"spatial norm restatement T={T} zT={zT} C={C}").add(out, ref, bound).check()
        bad = emu.spatial_norm_gather(c["yb"], c["n"], C, c["zdims"], c["x5"].shape[1:4], defect="zw_plus_1")
        out = emu.gn_apply_chunks(c["x5"], mean, rstd, c["groups"], c["gamma"], c["beta"], True, yb=bad)
        assert _fails(out, ref, bound), f"latent voxel zw + 1 passes at T={T} zT={zT} C={C}"
        out = emu.gn_apply_chunks(c["x5"], mean, rstd, c["groups"], c["gamma"], c["beta"], True, yb=maps, defect="sample0_stats")
        assert _fails(out, ref, bound)


@pytest.mark.parametrize("case", vc.SOFTMAX_CASES, ids=lambda c: f"{c[0]}x{c[1]}of{c[2]}")
def test_softmax_rows_restatement_passes_and_defects_fail(case):
    rows, n, ld, kinds = vc.SOFTMAX_CPU_SCALE.get(case, case)
    s = vc.softmax_scores(rows, n, ld, kinds)
    vc.check_softmax(emu.softmax_rows(s, n), s, n, f"softmax restatement {rows} x {n} of {ld}")
    if n > 1024:
        with pytest.raises(AssertionError, match="outside the bound"):
            vc.check_softmax(emu.softmax_rows(s, n, defect="sum_first_1024"), s, n, "columns >= 1024 left out of the sum")
    if ld > n:
        s2 = s.clone()
        s2[:, n:] = s2[:, :1]         # (finite scores behind n, so that the un-zeroed columns hold ordinary probabilities)
        with pytest.raises(AssertionError, match="not exactly zero"):
            vc.check_softmax(emu.softmax_rows(s2, n, defect="pad_not_zeroed"), s2, n, "padded columns not zeroed")


@pytest.mark.parametrize("kt,kcols", [(3, 128), (1, 64)])
def test_first_layer_restatement_passes_and_a_shifted_tap_fails(kt, kcols):
    z, params, ref, bound, mask = vc.first_case(kt, kcols)
    out = emu.vae_first_im2col(z, kt, kcols, params)
    vc.check_first(out, ref, bound, mask, f"first layer kt={kt}")
    bad = out.clone()
    bad[:, 0:4] = out[:, 4:8]         # tap 0 holding tap 1's pixels
    with pytest.raises(AssertionError):
        vc.check_first(bad, ref, bound, mask, "first layer, tap shifted")


def test_conv_refuses_temporal_taps_on_more_than_one_sample():
    """ops.conv shifts FLAT rows: with n > 1 the output grid (T plane rows per sample) and the input grid ((T + tf) plane rows per sample)
    drift apart from the second sample on.  The wrapper refuses before it looks at a tensor (so: no device needed, nothing launched)."""
    from videosys_amd import ops

    g = ops.VaeGrid(2, 3, 4, 4, 1, 2)
    a = torch.zeros(g.rows, 32, dtype=torch.bfloat16)
    w = torch.zeros(128, 32 * 27, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="wrong sample"):
        ops.conv(a, g, w, None, 32, 3, 3)
    with pytest.raises(ValueError, match="wrong sample"):                    # temporal-only taps all the same
        ops.conv(torch.zeros(ops.VaeGrid(3, 2, 4, 4, 0, 2).rows, 32, dtype=torch.bfloat16), ops.VaeGrid(3, 2, 4, 4, 0, 2), w[:, :96], None, 32, 3, 1)
    g1 = ops.VaeGrid(2, 1, 4, 4, 1, 0, sample_rows=40)                        # slack rows per sample: the same drift without temporal taps
    with pytest.raises(ValueError, match="wrong sample"):
        ops.conv(torch.zeros(g1.rows, 32, dtype=torch.bfloat16), g1, w[:, :288], None, 32, 1, 3)
    with pytest.raises(ops._lib.VsysError, match="no CPU fallback"):          # what is allowed reaches the device check (still no launch)
        ops.conv(torch.zeros(ops.VaeGrid(2, 1, 4, 4, 1, 0).rows, 32, dtype=torch.bfloat16), ops.VaeGrid(2, 1, 4, 4, 1, 0), w[:, :288], None, 32, 1, 3)


# ------------------------------------------------------------------------------------------------ GEMM family: the other models' sites
# The tables of tests/gemm_numerics_cases.py at scaled-down rows (CPU operands, the same generators): the restatements of
# tests/gemm_cpu_emul.py pass every bound, every planted defect fails.
def _bad(reps):
    return sum(r.bad for r in reps)


def test_gemm_tables_match_the_dispatch_rule():
    gc.assert_tables_match_rule()
    import test_gpu_numerics_gemm as tg      # the rule of the existing file and its restatement here agree on ids 0 and 8

    for cu in (80, 256, 304):
        for M, N, K, epi, _ in gc.table_rows():
            if epi != "gelu":
                assert tg.dispatch_rule(M, N, K, epi, 0, cu) == gc.dispatch_rule(M, N, K, epi, cu)
    assert gc.kernel_of(1, 192, 64, "gate", 8, 256) == "sched8 mf32" and tg.dispatch_rule(1, 192, 64, "gate", 8, 256) == "sched8"


def test_row_gates_without_a_segment_is_gate_rows_and_with_one_follows_the_definition():
    import test_gpu_numerics_gemm as tg

    N = 24
    for M, rps in ((130, 7), (257, 257), (300, 100), (64, 1)):
        ns = -(-M // rps)
        mod = gc.randn((ns, 3 * N + 8), M + rps, "cpu")
        for r0, r1 in ((0, M), (M // 3, M - 1)):
            assert torch.equal(gc.row_gates(mod[0, N:], mod.stride(0), rps, 0, 0, r0, r1, N),
                               tg.gate_rows(mod[0, N:], mod.stride(0), rps, r0, r1, N))
        for split in (1, rps // 2, rps):
            if split == 0:
                continue
            got = gc.row_gates(mod[0, :N], mod.stride(0), rps, split, 2 * N, 0, M, N)
            for r in range(M):                 # the definition, row by row
                b = r // rps
                want = mod[b, 2 * N:3 * N] if r - b * rps < split else mod[b, :N]
                assert torch.equal(got[r], want.double()), (M, rps, split, r)


GELU_CPU = [(260, 384, 1152), (260, 384, 1536), (260, 384, 1600), (132, 384, 3072), (131, 192, 64)]


@pytest.mark.parametrize("M,N,K", GELU_CPU)
def test_gelu_restatement_passes_and_planted_defects_fail(M, N, K):
    a, w, b = gc.gelu_operands(M, N, K, 7 * K + M, "cpu")
    gc.check_gemm(gemu.gelu_store(a, w, b), a, w, b, f"GELU restatement {M} x {N} x {K}", gelu=True, tails=True)
    gc.check_gemm(gemu.gelu_store(a, w, None), a, w, None, f"GELU restatement {M} x {N} x {K}, no bias", gelu=True, tails=True)
    for defect in ("bias_after", "abs"):
        assert _bad(gc.gemm_bounds(gemu.gelu_store(a, w, b, defect), a, w, b, defect, gelu=True)) > 0, f"{defect} passes"
    # a non-finite or a non-zero tail fails: the overflow branch's result replaced by what a global-slope bound would let through
    out = gemu.gelu_store(a, w, b)
    p = a.double() @ w.double().t() + b.double()
    r, c = divmod(int(p.argmin()), N)
    assert float(p[r, c]) <= -gc.TAIL and float(out[r, c]) == 0.0
    for wrong in (float("nan"), -2.0**-8):
        bad = out.clone()
        bad[r, c] = wrong
        assert _bad(gc.gemm_bounds(bad, a, w, b, "tail", gelu=True)) == 1


def test_erf_gelu_share_outside_the_tanh_bound():
    """A limit, reported and not asserted to be large: over most of the range a worst-case bound on a bf16 output cannot tell erf GELU from
    tanh GELU (they differ by at most 4.7e-4).  The share of a GELU case's elements on which the swap is outside the bound is printed for
    the ledger; it only has to be a share (some elements do tell them apart, most do not)."""
    M, N, K = 260, 384, 1152
    a, w, b = gc.gelu_operands(M, N, K, 7 * K + M, "cpu")
    p = a.float() @ w.float().t() + b.float()
    out = torch.nn.functional.gelu(p).to(torch.bfloat16)
    rep = gc.gemm_bounds(out, a, w, b, "erf GELU under the tanh bound", gelu=True)[0]
    share = rep.bad / rep.total
    print(f"erf GELU for tanh GELU at {M} x {N} x {K}: {rep.bad} of {rep.total} elements ({100 * share:.2f} %) outside the bound")
    assert 0.0 < share < 0.5


def _gate2_cpu(M, rps, split, bias=True):
    N, K = gc.GATE2_N, gc.GATE2_K
    a, w, b = gc.operands(M, N, K, 11 * M + rps + split, "cpu")
    mod = gc.randn((-(-M // rps), 3 * N), 13 * M + rps, "cpu")       # gate | junk | alternative gate
    res = gc.randn((M, N), 17 * M + split, "cpu", 1.0, 0.5)
    return a, w, (b if bias else None), mod, res


@pytest.mark.parametrize("M,rps,split,what", gc.GATE2_SMALL, ids=[f"M{c[0]}_rps{c[1]}_split{c[2]}" for c in gc.GATE2_SMALL])
def test_two_segment_gate_restatement_passes(M, rps, split, what):
    N = gc.GATE2_N
    for bias in (True, False):
        a, w, b, mod, res = _gate2_cpu(M, rps, split, bias)
        out, aux = gemu.gate_res(a, w, b, mod[0, :N], 3 * N, rps, split, 2 * N, res)
        gc.check_gemm(out, a, w, b, f"gate2 restatement M={M} rps={rps} split={split} bias={bias} ({what})", gate=mod[0, :N], gate_stride=3 * N,
                      rps=rps, seg_split=split, gate_alt=2 * N, res=res, aux=aux)


# which rows of GATE2_SMALL must catch which defect (module docstring of gemm_cpu_emul.py); the others hold no row the defect moves
GATE2_CAUGHT = {
    "le": (0, 1, 2, 3),
    "wave_first_row": (0, 2, 3),          # (row 1 has every boundary on a wave edge: the one-row form is right there)
    "alt_on_video": (0, 1, 2, 3, 5),
    "tile_sample": (0, 2, 3),             # (row 1: the sample boundaries lie on tile edges)
}


@pytest.mark.parametrize("defect", sorted(GATE2_CAUGHT))
def test_two_segment_gate_planted_defect_fails(defect):
    N = gc.GATE2_N
    for i, (M, rps, split, what) in enumerate(gc.GATE2_SMALL):
        a, w, b, mod, res = _gate2_cpu(M, rps, split)
        out, aux = gemu.gate_res(a, w, b, mod[0, :N], 3 * N, rps, split, 2 * N, res, defect=defect)
        reps = gc.gemm_bounds(out, a, w, b, defect, gate=mod[0, :N], gate_stride=3 * N, rps=rps, seg_split=split, gate_alt=2 * N, res=res, aux=aux)
        if i in GATE2_CAUGHT[defect]:
            assert reps[0].bad > 0 and reps[1].bad > 0, f"{defect} passes on M={M} rps={rps} split={split}"
        else:
            assert _bad(reps) == 0, f"{defect} should not move a row of M={M} rps={rps} split={split}"


LS_ACTS = {"none": "none", "silu": "silu", "gelu": "gelu"}


@pytest.mark.parametrize("name", list(gc.LS_CASES))
def test_linear_small_restatement_passes_and_tie_share_is_capped(name):
    full = gc.ls_case(name)
    if full["tie"] is not None:
        share = full["tie"].share()
        print(f"linear_small {name}: near-tie share {100 * share:.2f} %")
        assert share <= gc.TIE_CAP
        if full["M"] * full["K"] <= 64:
            assert share == 0.0
    c = gc.ls_case(name, max_rows=5, max_cols=72)
    out, buf = c["run"](gemu.linear_small, LS_ACTS)
    rep = nm.Bound(f"linear_small restatement {name}").add(out, c["ref"], c["bound"])
    print(rep.message())
    rep.check()
    assert gc.slack_untouched(buf, c["N"]) and c["operands_intact"]()


def test_linear_small_planted_defects():
    def bad(name, defect):
        c = gc.ls_case(name, max_rows=5, max_cols=72)
        out = gemu.linear_small(c["x"], c["w"], c["b"], c["act_in"], c["act_out"], defect=defect)
        return nm.Bound(defect).add(out, c["ref"], c["bound"]).bad

    # One rounding fewer (the SiLU left in fp32) on the flagged-free cases.  It passes on the one-row case.  It does NOT pass in general,
    # and is not meant to: the near-tie rule holds an unflagged xe to EXACTLY bf16(silu(x)) (Tie.err = 0), so at K = 8 the unrounded
    # form's sum_k (silu(x_k) - xe_k) w_k (up to 2^-9 |silu(x_k) w_k| a term) can exceed acc(9, .) + rnd(out) where the sum cancels:
    # 4 of the 15 elements of m3_n5_k8_silu_in.  The count is printed, the rule is not widened for it.
    assert gc.ls_case("m1_n3_k8_silu_in")["tie"].share() == 0.0 and bad("m1_n3_k8_silu_in", "silu_unrounded") == 0
    assert gc.ls_case("m3_n5_k8_silu_in")["tie"].share() == 0.0
    print(f"SiLU left unrounded on m3_n5_k8_silu_in: {bad('m3_n5_k8_silu_in', 'silu_unrounded')} of 15 elements outside the bound")
    for name in ("m3_n5_k8_silu_in", "m2_n5_k512_silu_in", "m3_n72_k4096_silu_in", "modulation_table"):
        assert bad(name, "silu_after") > 0, f"SiLU after the product passes on {name}"
    for name in ("m2_n5_k520", "m3_n5_k520_silu_in", "m2_n1152_k520_gelu"):
        assert bad(name, "lane_stride_64") > 0, f"lane stride 64 passes on {name}"


def test_activation_image_is_tight_in_the_tails_and_holds_the_minimum():
    for act, xmin in (("gelu", -0.7525), ("silu", -1.2785)):     # (tanh GELU; the erf form has its minimum at -0.7518)
        assert abs(nm.ACTIVATIONS[act][1] - xmin) < 1e-4
        fn = nm.ACTIVATIONS[act][0]
        p = torch.tensor([-40.0, -16.0, -12.0, xmin + 0.01, 0.0, 3.0, 16.0], dtype=torch.float64)
        d = torch.tensor([0.2, 0.0625, 0.05, 0.02, 0.01, 0.01, 0.0625], dtype=torch.float64)
        y, e = nm.act_image(act, p, d)
        grid = p[:, None] + d[:, None] * torch.linspace(-1, 1, 2001, dtype=torch.float64)[None]
        brute = (fn(grid) - y[:, None]).abs().amax(dim=1)
        assert bool((e >= brute - 1e-15).all()) and bool((e <= brute + 1e-9).all())
        assert float(e[0]) < 1e-12 and (act == "silu" or float(e[2]) < 2.0**-24)     # a global slope would give ~ d there
