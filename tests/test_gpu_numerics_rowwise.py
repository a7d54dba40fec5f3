"""GPU: the row-wise kernels of csrc/rowwise.hip and csrc/t5_ops.hip element by element against a float64 reference, each element under
the bound of its own rounding chain, or bit for bit where the arithmetic is exactly defined (tests/numerics.py, row-wise family; cases,
operands and the table of which case reaches which template instantiation: tests/rowwise_numerics_cases.py; the bounds' own meta-tests
and the planted defects: tests/test_numerics_rowwise_cpu.py).  The kernels are called through videosys_amd.ops / vchitect_ops only.
Every bounded test prints the worst |err| / bound."""
import pytest
import torch

import numerics as nm
import rowwise_numerics_cases as rc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def to(t):
    return t.to(dev())


class _Ops:
    """videosys_amd.ops with vchitect_ops.scale_add_rows beside it: the one namespace the cases call."""

    def __getattr__(self, name):
        from videosys_amd import ops, vchitect_ops

        return getattr(vchitect_ops, name) if name == "scale_add_rows" else getattr(ops, name)


OPS = _Ops()


def run(c, key="call", *a):
    out = c[key](OPS, to, *a)
    torch.cuda.synchronize()
    return out.cpu()


def check(out, c, what):
    rep = nm.Bound(what).add(out, c["ref"], c["bound"])
    print(rep.message())
    rep.check()


def check_const_rows(out, c, what):
    if c["const_value"] is not None:
        for r in c["const_rows"]:
            assert torch.equal(out[r], c["const_value"][r]), f"{what}: the constant row {r} is not exactly the zero row's value"


@pytest.mark.parametrize("name", list(rc.ADALN_CASES))
def test_adaln_modulate_elementwise(name):
    c = rc.adaln_case(name)
    out = run(c)
    check(out, c, f"adaln_modulate {name} {rc.ADALN_CASES[name]}")
    check_const_rows(out, c, f"adaln_modulate {name}")


@pytest.mark.parametrize("name", list(rc.LN_CASES))
def test_ln_modulate_elementwise(name):
    c = rc.ln_case(name)
    out = run(c)
    check(out, c, f"ln_modulate {name} {rc.LN_CASES[name]}")
    check_const_rows(out, c, f"ln_modulate {name}")


@pytest.mark.parametrize("name", list(rc.FINAL_CASES))
def test_final_layer_elementwise(name):
    c = rc.final_case(name)
    assert c["tie"].share() <= rc.TIE_CAP
    check(run(c), c, f"final_layer {name} {rc.FINAL_CASES[name]}")


@pytest.mark.parametrize("P", rc.FINAL_TOKENS_P)
@pytest.mark.parametrize("name", ["c1152_full_co4", "c1152_crop_co8"])
def test_final_layer_tokens_and_unpatchify_tokens_elementwise(name, P):
    c = rc.final_case(name)
    check(run(c, "call_tokens", P), c, f"final_layer_tokens + unpatchify_tokens {name} P={P}")


@pytest.mark.parametrize("name", list(rc.PATCH_CASES))
def test_patch_embed_elementwise(name):
    c = rc.patch_case(name)
    assert c["tie"].share() <= rc.TIE_CAP
    out = run(c)
    check(out, c, f"patch_embed {name} {rc.PATCH_CASES[name]}")
    if c["zero_from"] is not None:
        assert int((out[:, :, c["zero_from"]:].float() != 0).sum()) == 0, "padding tokens are not exactly zero rows"


@pytest.mark.parametrize("name", list(rc.RMS_CASES))
def test_rms_norm_rows_elementwise(name):
    c = rc.rms_case(name)
    assert c["tie"].share() <= rc.TIE_CAP
    check(run(c), c, f"rms_norm_rows {name}")


@pytest.mark.parametrize("name", list(rc.GEGLU_CASES))
def test_geglu_elementwise(name):
    c = rc.geglu_case(name)
    out = c["call"](OPS, to)
    torch.cuda.synchronize()
    n = c["ref"].shape[0]
    check(out[:n].cpu(), c, f"geglu {name}, first block")
    if c["period"] is not None:      # the last block lies in the second trip of the grid-stride loop; every block repeats the first
        check(out[-n:].cpu(), c, f"geglu {name}, last block")
        assert bool((out.view(-1, n, out.shape[1]) == out[:n]).all()), "a block of the repeated input differs from the first"


@pytest.mark.parametrize("dim", rc.TS_DIMS)
def test_timestep_embedding_elementwise(dim):
    c = rc.timestep_case(dim)
    check(run(c), c, f"timestep_embedding dim={dim}")


@pytest.mark.parametrize("name", list(rc.CFG_CASES))
def test_cfg_step_elementwise(name):
    c = rc.cfg_case(name)
    check(run(c), c, f"cfg step {name} {rc.CFG_CASES[name]}")


@pytest.mark.parametrize("pad,nsplit,res,M", rc.SKINNY_CASES)
def test_linear_skinny_splitk_reduce_elementwise(pad, nsplit, res, M):
    c = rc.skinny_case(pad, nsplit, res, M)
    check(run(c), c, f"linear_skinny pad={pad} nsplit={nsplit} res={res} M={M}")


@pytest.mark.parametrize("op,size", rc.EXACT_IDS)
def test_exactly_defined_kernels_bit_for_bit(op, size):
    c = rc.exact_case(op, size)
    out = run(c)
    assert out.dtype == c["exact"].dtype and out.shape == c["exact"].shape
    same = out == c["exact"]
    assert bool(same.all()), f"{op} {size}: {int((~same).sum())} of {same.numel()} elements differ; the first at flat index {int((~same).flatten().nonzero()[0])}"


@pytest.mark.parametrize("what", ["adaln_modulate", "ln_modulate", "final_layer", "rms_norm_rows"])
def test_width_past_the_widest_instantiation_is_refused(what):
    """A row wider than the registers of the widest template must be an error from the launcher, never a launch."""
    from videosys_amd import _lib

    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev())
    with pytest.raises(_lib.VsysError):
        if what == "adaln_modulate":
            OPS.adaln_modulate(bf(4, 2056), bf(1, 2056), bf(1, 2056), 4, 0)
        elif what == "ln_modulate":
            OPS.ln_modulate(bf(4, 3080), None, None, None, None, 4)
        elif what == "final_layer":
            OPS.final_layer(bf(6, 2056), bf(2, 2056), bf(1, 2056), bf(16, 2056), bf(16), 1, 1, 3, 2, 6, 4, (1, 2, 2), 4)
        else:
            OPS.rms_norm_rows(bf(4, 8200), bf(8200))
