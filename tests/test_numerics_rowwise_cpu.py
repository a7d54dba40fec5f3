"""No GPU: the bounds of the row-wise family (tests/numerics.py) on the cases of tests/rowwise_numerics_cases.py.  The restatements of
tests/rowwise_cpu_emul.py (fp32 arithmetic, bf16 where the contract rounds) pass every case; every planted defect fails on the cases
CAUGHT_BY names; the layout references agree with oracle/stdit3_oracle.py and F.layer_norm in float64; the near-tie share of every case
stays under 5% and every wrap case is a few chunks more than one trip of its launcher's capped grid.

Rounding once fewer than the contract passes where the chain's bound carries a worst-case rnd() for that rounding (the split-K residual)
and where the case's operands keep the dropped rounding's noise under one ulp of the output (final_layer's activation: see
rowwise_numerics_cases.final_operands).  Where an intermediate is held by the near-tie rule, the kernel must round it: a patch-embed
latent left unrounded is accepted only within that rounding's own worst case plus ONE ulp of the conv output it may push across a boundary."""
import pytest
import torch
import torch.nn.functional as F

import numerics as nm
import rowwise_cpu_emul as emu
import rowwise_numerics_cases as rc

ident = lambda t: t
GOOD = emu.Emul()


def run(c, impl=GOOD, key="call", *a):
    return c[key](impl, ident, *a)


def passes(out, c):
    return nm.Bound("x").add(out, c["ref"], c["bound"]).bad == 0


@pytest.fixture(scope="module")
def adaln():
    return {n: rc.adaln_case(n) for n in rc.ADALN_CASES}


@pytest.fixture(scope="module")
def ln():
    return {n: rc.ln_case(n) for n in rc.LN_CASES}


@pytest.fixture(scope="module")
def final():
    return {n: rc.final_case(n) for n in rc.FINAL_CASES}


@pytest.fixture(scope="module")
def patch():
    return {n: rc.patch_case(n) for n in rc.PATCH_CASES}


@pytest.fixture(scope="module")
def rms():
    return {n: rc.rms_case(n) for n in rc.RMS_CASES}


@pytest.fixture(scope="module")
def families(adaln, ln, final, patch, rms):
    return dict(adaln=adaln, ln=ln, final=final, patch=patch, rms=rms)


def check_const_rows(out, c, what):
    if c["const_value"] is not None:
        for r in c["const_rows"]:
            assert torch.equal(out[r], c["const_value"][r]), f"{what}: the constant row {r} is not exactly the zero row's value"


# ------------------------------------------------------------------------------------------------ the restatements pass
def test_restatements_pass_on_every_norm_case(families):
    for fam in ("adaln", "ln", "rms"):
        for name, c in families[fam].items():
            out = run(c)
            nm.check_elementwise(out, c["ref"], c["bound"], f"{fam} {name}")
            if fam != "rms":
                check_const_rows(out, c, f"{fam} {name}")


def test_final_layer_restatement_and_token_route_pass(final):
    for name, c in final.items():
        nm.check_elementwise(run(c), c["ref"], c["bound"], f"final_layer {name}")
    for name in ("c1152_full_co4", "c1152_crop_co8"):
        for P in rc.FINAL_TOKENS_P:
            nm.check_elementwise(run(final[name], GOOD, "call_tokens", P), final[name]["ref"], final[name]["bound"], f"final_layer_tokens {name} P={P}")


def test_patch_embed_restatement_passes_and_padding_rows_are_zero(patch):
    for name, c in patch.items():
        out = run(c)
        nm.check_elementwise(out, c["ref"], c["bound"], f"patch_embed {name}")
        if c["zero_from"] is not None:
            assert c["zero_from"] < out.shape[2] or name == "stdit_shard_mid"
            assert int((out[:, :, c["zero_from"]:].float() != 0).sum()) == 0


@pytest.mark.parametrize("name", list(rc.GEGLU_CASES))
def test_geglu_restatement_passes(name):
    c = rc.geglu_case(name)
    n = c["ref"].shape[0]
    out = run(dict(c, call=lambda impl, to: impl.geglu(c["h"][:n])))       # (the wrap case: one period; the GPU test runs all of it)
    nm.check_elementwise(out, c["ref"], c["bound"], f"geglu {name}")
    assert c["tie"].share() <= rc.TIE_CAP
    assert not passes(emu.Emul("geglu_erf").geglu(c["h"][:n]), c), "erf-GELU passes"
    if name == "wrap":
        assert rc.wraps("geglu", rc.geglu_items(name)) and (c["rows"] - c["period"]) * (c["h"].shape[1] // 16) >= rc.CAPS["geglu"][2] * rc.BLOCK


@pytest.mark.parametrize("dim", rc.TS_DIMS)
def test_timestep_embedding_restatement_passes_and_defects_fail(dim):
    c = rc.timestep_case(dim)
    nm.check_elementwise(run(c), c["ref"], c["bound"], f"timestep_embedding dim={dim}")
    import oracle.stdit3_oracle as oracle

    nm.check_elementwise(oracle.timestep_embedding(c["t"], dim).to(torch.bfloat16), c["ref"], c["bound"], "the oracle's timestep_embedding")
    for defect in ("ts_halves_swapped", "ts_half_minus_1"):
        assert not passes(run(c, emu.Emul(defect)), c), f"{defect} passes at dim={dim}"


@pytest.mark.parametrize("name", list(rc.CFG_CASES))
def test_cfg_step_restatement_passes_and_inverted_cond_first_fails(name):
    c = rc.cfg_case(name)
    nm.check_elementwise(run(c), c["ref"], c["bound"], f"cfg {name}")
    assert not passes(run(c, emu.Emul("cfg_cond_first_inverted")), c)
    # an FMA contraction (one rounding fewer) passes: the step in float64, rounded once
    assert passes(c["ref"].float(), c)


@pytest.mark.parametrize("pad,nsplit,res,M", rc.SKINNY_CASES)
def test_splitk_linear_restatement_passes(pad, nsplit, res, M):
    c = rc.skinny_case(pad, nsplit, res, M)
    nm.check_elementwise(run(c), c["ref"], c["bound"], f"linear_skinny {pad} {nsplit} {res} {M}")
    if res:
        nm.check_elementwise(run(c, emu.Emul("skinny_res_one_rounding")), c["ref"], c["bound"], "one rounding fewer")
        bad = (c["x"][:M].float() @ c["w"].float().t()).to(torch.bfloat16).float() + c["r"][:M].roll(1, 1).float()      # the residual one column off
        assert not passes(bad.to(torch.bfloat16), c)


# ------------------------------------------------------------------------------------------------ rounding once fewer
def test_final_layer_with_fp32_activation_passes_and_bf16_partial_sums_fail(final):
    for name, c in final.items():
        if c["flavour"] == "model":
            nm.check_elementwise(run(c, emu.Emul("final_fp32_activation")), c["ref"], c["bound"], f"final_layer {name}, activation kept in fp32")
        if c["C"] >= 1024:
            assert not passes(run(c, emu.Emul("final_bf16_partials")), c), f"final_layer {name}: bf16 partial sums pass"


def test_patch_embed_with_unrounded_latent_is_within_its_own_rounding_and_one_ulp(patch):
    """The latent is off the bf16 grid on purpose (the load's rounding is part of the contract).  Leaving it unrounded moves the conv sum
    by at most sum_k rnd(z_k) |w_k| and with it, now and then, the bf16 value of the conv output by one ulp: accepted within those two."""
    for name, c in patch.items():
        out = run(c, emu.Emul("patch_latent_unrounded"))
        extra = c["tie"].ulp + nm.U_BF16 * c["tie"].abs_sum
        if c["shard"] is not None:
            s0, Sl = c["shard"]
            extra = torch.cat([extra[:, :, s0:s0 + Sl], torch.zeros_like(c["ref"])[:, :, :max(0, s0 + Sl - c["S"])]], dim=2)
        nm.check_elementwise(out, c["ref"], c["bound"] + extra, f"patch_embed {name}, latent not rounded")


# ------------------------------------------------------------------------------------------------ planted defects
# (family, defect) -> the cases that must catch it (at least these)
CAUGHT_BY = {
    ("adaln", "var_c_minus_1"): ("c8_r1", "c8_r5"),          # 8 / 7: visible at the narrow width; at C >= 1024 it is 2^-11 of the row, under one bf16 ulp
    ("ln", "var_c_minus_1"): ("c8_seg0_both", "c8_seg2_affine"),
    ("rms", "var_c_minus_1"): ("c8_r4", "c72_r4"),
    ("adaln", "eps_swapped"): ("c8_r5", "c1152_r5", "c1152_even17", "c2048_r5"),        # the +-2^-10 row (row 2)
    ("adaln", "no_eps"): ("c8_r5", "c1152_r5", "c2048_r5"),
    ("ln", "eps_swapped"): ("c1032_seg0_both", "c3072_seg1_affine"),
    ("rms", "eps_swapped"): ("c8_r4", "c4104_r5"),
    ("adaln", "padded_width"): ("c8_r1", "c1032_r4", "c1152_r5", "c1544_r1"),
    ("ln", "padded_width"): ("c1032_seg0_both", "c1920_seg1_affine", "c2056_seg3_neither", "c2304_seg0_both"),
    ("rms", "padded_width"): ("c72_r1", "c2056_r4", "c4104_r5"),
    ("adaln", "one_pass"): ("c1152_r1", "c1152_even17", "c2048_r5"),                    # the mean-8 row (rows 0, 4, ..)
    ("ln", "one_pass"): ("c3072_seg1_affine",),
    ("adaln", "sample_rps_plus_1"): ("c1152_r4", "c1152_r5", "c1152_even17", "c1152_odd15"),
    ("adaln", "sample_0"): ("c8_r4", "c1152_r5", "c1152_even17", "c2048_r4"),
    ("ln", "sample_rps_plus_1"): ("c1032_seg0_both", "c1032_seg1_mod"),
    ("ln", "sample_0"): ("c1032_seg0_both", "c2056_seg1_both"),
    ("adaln", "shift_scale_swapped"): ("c8_r1", "c1152_r4", "c2048_r5"),
    ("ln", "shift_scale_swapped"): ("c1032_seg2_mod", "c1032_seg3_both"),
    ("ln", "seg_split_off_by_one"): ("c1032_seg1_mod", "c1032_seg2_both", "c1032_seg1_both"),
    ("adaln", "tail_stats"): ("c1152_r4", "c1152_even17", "c1032_r4", "c1536_r4"),
    ("final", "final_scale_row_for_shift"): tuple(rc.FINAL_CASES),
    ("patch", "patch_pad_is_edge"): ("stdit_c8", "stdit_c1152", "cin8_2x2", "cin4_2x4", "stdit_shard_mid"),
    ("patch", "patch_b_clamped"): ("cin8_2x2", "cin16_1x1", "cin8_shard_past"),
    ("rms", "rms_minus_mean"): ("c8_r1", "c2048_r4", "c8192_r5"),
}


@pytest.mark.parametrize("fam,defect", sorted(CAUGHT_BY))
def test_planted_defect_fails(families, fam, defect):
    caught = {name for name, c in families[fam].items() if not passes(run(c, emu.Emul(defect)), c)}
    print(f"{fam} {defect}: caught by {sorted(caught)}")
    assert set(CAUGHT_BY[fam, defect]) <= caught, f"{defect} is not caught by {sorted(set(CAUGHT_BY[fam, defect]) - caught)}"


def test_final_layer_wrong_sample_fails(final):
    """The t vector of sample 0 for every row."""
    for name, c in final.items():
        bad = dict(c, tvec=c["tvec"][:1].expand(2, -1).contiguous())
        out = emu.Emul().final_layer(bad["x"], bad["table"], bad["tvec"], bad["w"], bad["bias"], rc.FL_B, rc.FL_T, rc.FL_HP, rc.FL_WP, c["H"], c["W"],
                                     rc.FL_PATCH, c["Cout"], eps=rc.FL_EPS)
        assert not passes(out, c), name


# ------------------------------------------------------------------------------------------------ the references themselves
def test_near_tie_share_is_under_the_cap(final, patch, rms):
    worst = {}
    for fam, cases in (("final_layer", final), ("patch_embed", patch), ("rms_norm_rows", rms)):
        for name, c in cases.items():
            share = c["tie"].share()
            worst[fam] = max(worst.get(fam, 0.0), share)
            assert share <= rc.TIE_CAP, f"{fam} {name}: {share:.3%} of the intermediate lies within its error of a bf16 boundary"
    print({k: f"{v:.2%}" for k, v in worst.items()})


def test_tie_flags_exactly_the_values_near_a_boundary():
    v = torch.tensor([1.0 + 2.0**-8 + 1e-7, 1.0 + 2.0**-8 + 1e-3, 1.0 - 2.0**-9 - 1e-7, 3.0, 0.0], dtype=torch.float64)
    t = nm.Tie(v, torch.full_like(v, 1e-6))
    assert t.flag.tolist() == [True, False, True, False, True]      # (a zero within its error of the smallest bf16 value: one tiny ulp)
    assert t.err.tolist()[:3] == [2.0**-7, 0.0, 2.0**-8] and float(t.vb[2]) == 1.0 - 2.0**-8 and float(t.vb[3]) == 3.0


def test_ln_reference_is_layer_norm_in_float64(adaln, ln):
    for cases, eps in ((adaln, rc.ADALN_EPS), (ln, rc.LN_EPS)):
        for name, c in cases.items():
            x = c["x"].double()
            plain, _, _ = nm.ln_modulate_ref(x, eps)
            assert torch.allclose(plain, F.layer_norm(x, (x.shape[1],), eps=eps), rtol=1e-12, atol=1e-12), name


def test_patch_and_unpatchify_references_agree_with_the_oracle(patch, final):
    import oracle.stdit3_oracle as oracle

    for name, c in patch.items():
        if c["shard"] is not None:
            continue
        zb = nm.bf16_exact(c["z"]).repeat(c["B"] // c["Bz"], 1, 1, 1, 1)
        sd = {"x_embedder.proj.weight": c["w"].double(), "x_embedder.proj.bias": c["bias"].double()}
        want = oracle.patch_embed(zb, sd, c["patch"])                                   # [B, T S, C]
        got = c["tie"].v.reshape(c["B"], -1, c["C"])
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), name
    # the oracle's position table has one row per token in the order of its patch_embed (s = hp Wp + wp): the layout of ``pos``
    c = patch["stdit_c8"]
    pos = oracle.pos_embed_2d(c["C"], c["Hp"], c["Wp"], 1.0, c["Hp"])[0].to(torch.bfloat16)
    assert pos.shape == (c["S"], c["C"])
    ref, _, tie = nm.patch_embed_ref(c["z"], c["B"], c["w"], c["bias"], pos, c["patch"][1:], c["C"])
    sd = {"x_embedder.proj.weight": c["w"].double(), "x_embedder.proj.bias": c["bias"].double()}
    want = oracle.patch_embed(nm.bf16_exact(c["z"]).repeat(c["B"], 1, 1, 1, 1), sd, c["patch"]).reshape(ref.shape) + pos.double()
    assert bool(((ref - want).abs() <= tie.ulp).all())          # (the reference rounds the conv output to bf16, the oracle does not)
    for name, c in final.items():
        tok = torch.randn(rc.FL_B, rc.FL_T * c["S"], c["nout"], dtype=torch.float64)
        want = oracle.unpatchify(tok, rc.FL_T, rc.FL_HP, rc.FL_WP, rc.FL_T, c["H"], c["W"], rc.FL_PATCH, c["Cout"])
        assert torch.equal(nm.unpatchify_ref(tok, rc.FL_T, rc.FL_HP, rc.FL_WP, rc.FL_PATCH[1:], c["Cout"], c["H"], c["W"]), want)


def test_final_layer_reference_agrees_with_the_oracle(final):
    import oracle.stdit3_oracle as oracle

    c = final["c1152_full_co4"]
    sd = {"final_layer.scale_shift_table": c["table"].double(), "final_layer.linear.weight": c["w"].double(), "final_layer.linear.bias": c["bias"].double()}
    x = c["x"].double().reshape(rc.FL_B, -1, c["C"])
    want = oracle.final_layer(x, c["tvec"].double(), sd)
    tok, bound, _ = nm.final_layer_ref(x, c["table"], c["tvec"], c["w"], c["bias"], rc.FL_EPS)
    # the oracle keeps float64 throughout; the contract's bf16 shift / scale / activation are within the roundings the bound's terms name
    assert float((tok - want).abs().max()) < 2.0**-6 * float(want.abs().max())


@pytest.mark.parametrize("op", sorted(rc.CAPS))
def test_launcher_caps_are_the_ones_the_wrap_cases_were_sized_for(op):
    fname, launcher, cap = rc.CAPS[op]
    assert rc.launcher_cap(fname, launcher) == cap


@pytest.mark.parametrize("op,size", rc.EXACT_IDS)
def test_exact_cases_are_well_formed_and_wrap(op, size):
    c = rc.exact_case(op, size)
    assert c["exact"].numel() > 0 and bool(torch.isfinite(c["exact"].float()).all())
    if size == "wrap":
        assert rc.wraps(c["op"], c["items"]), f"{op}: {c['items']} items against a cap of {rc.CAPS[c['op']][2] * rc.BLOCK}"


def test_exact_restatements_of_the_two_rounding_adds():
    """gate_add_rows: the restatement of rowwise_cpu_emul agrees bit for bit with the case's own statement of the contract (two
    statements of x + bf16(gate y)); a single rounding of x + gate y is NOT the same bits, nor is the main gate on the text rows."""
    c = rc.exact_case("gate_add_rows", "small")
    assert torch.equal(run(c), c["exact"])

    class OneRounding(emu.Emul):
        def gate_add_rows(self, x, y, gate, rows_per_sample, gate_stride, seg_split=0, gate_alt=0):
            g = (emu.Emul.gate_add_rows(self, torch.zeros_like(x), torch.ones_like(y), gate, rows_per_sample, gate_stride, seg_split, gate_alt)).float()
            return (x.float() + g * y.float()).to(torch.bfloat16)

    class OneSegment(emu.Emul):
        def gate_add_rows(self, x, y, gate, rows_per_sample, gate_stride, seg_split=0, gate_alt=0):
            return emu.Emul.gate_add_rows(self, x, y, gate, rows_per_sample, gate_stride, 0, 0)

    assert not torch.equal(run(c, OneRounding()), c["exact"])
    assert not torch.equal(run(c, OneSegment()), c["exact"])
