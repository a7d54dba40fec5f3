"""The guard-band harness (tests/isolation.py) tested on itself, without a GPU: plain torch functions stand in for kernels on CPU
tensors.  A correct function passes on contiguous and on row-strided operands; each deliberately wrong one fails with a message that
names the operand and the side.  Then the coverage ratchet: every public function of videosys_amd/ops.py that launches a kernel is
named in the case table (tests/isolation_cases.py) or, with a reason, in its NOT_COVERED."""
import ast
import os

import pytest
import torch

import isolation as iso
import isolation_cases as cases
from isolation import Operand

M, N, K = 17, 24, 16


def operands(strided):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g).to(torch.bfloat16)
    out = torch.zeros(M, N, dtype=torch.bfloat16)
    if strided:
        return {"x": Operand(x, parent=(M, K + 16), at=(0, 8)), "w": Operand(w), "out": Operand(out, parent=(M, N + 16), at=(0, 8))}
    return {"x": Operand(x), "w": Operand(w), "out": Operand(out)}


def raw(t, extra_rows=0, extra_cols=0):
    """The memory around a view as the 'kernel' sees it: rows of the view's stride, reaching past its shape."""
    return torch.as_strided(t, (t.shape[0] + extra_rows, t.shape[1] + extra_cols), t.stride(), t.storage_offset())


def roomy(t):
    """True on an arena view.  (torch refuses an out-of-bounds view of a tight CPU tensor, so the wrong stand-ins overreach where
    there is memory to overreach into — the tight run then equals the correct function, as it does for a real tail bug whose stray
    store lands in a neighbouring allocation.)"""
    return t.untyped_storage().nbytes() > t.numel() * t.element_size()


def good(t):
    t["out"].copy_((t["x"].float() @ t["w"].float().t()).to(torch.bfloat16))


def failure(fn, ops_, outputs=("out",), inplace=(), fills=iso.FILLS):
    with pytest.raises(iso.IsolationError) as e:
        iso.check_isolated(fn, ops_, outputs, inplace, fills=fills)
    return e.value


@pytest.mark.parametrize("strided", [False, True])
def test_correct_function_passes(strided):
    iso.check_isolated(good, operands(strided), ["out"])


def test_in_place_and_integer_operands_pass():
    ids = torch.tensor([3, 0, 5], dtype=torch.int64)
    o = {"x": Operand(torch.arange(12.0).reshape(3, 4), parent=(3, 8), at=(0, 2)), "tab": Operand(torch.arange(24.0).reshape(6, 4)),
         "ids": Operand(ids, int_guard=[1])}
    iso.check_isolated(lambda t: t["x"].add_(t["tab"][t["ids"]]), o, ["x"], ["x"])


@pytest.mark.parametrize("strided", [False, True])
def test_write_one_row_past_M(strided):
    def fn(t):
        good(t)
        if roomy(t["out"]):
            raw(t["out"], 1)[M, :] = 1.0
    err = failure(fn, operands(strided))
    d = [d for d in err.damages if d.operand == "out"]
    assert d and all(x.side.startswith("behind") or x.side.startswith("gap") for x in d), str(err)
    assert any(x.side.startswith("behind") and x.first[1] == M and x.first[2] == 0 for x in d), str(err)
    assert "operand 'out'" in str(err) and "bytes differ" in str(err)


def test_write_8_elements_past_the_last_column_of_a_strided_out():
    def fn(t):
        good(t)
        if roomy(t["out"]):                               # a 16-byte store hanging over the row's right edge
            raw(t["out"], 0, 8)[3, N:N + 8] = 2.0
    err = failure(fn, operands(True))
    assert len(err.damages) == 2                        # one per fill
    for d in err.damages:
        assert d.operand == "out" and d.side.startswith("gap") and d.first[1:] == (3, N) and d.last[1:] == (3, N + 7) and d.nbytes > 0


def test_row_M_of_the_input_in_a_reduction():
    def fn(t):
        good(t)
        src = raw(t["x"], 1) if roomy(t["x"]) else torch.cat([t["x"], torch.zeros(1, K, dtype=torch.bfloat16)])
        t["out"][0, 0] = src.float().sum().to(torch.bfloat16)
    err = failure(fn, operands(True))
    assert all(d.operand == "out" and d.side.startswith("output differs") for d in err.damages), str(err)


def pad_key_operands():
    g = torch.Generator().manual_seed(2)
    k = torch.randn(8, 4, generator=g)
    dead = torch.zeros(8, 4, dtype=torch.bool)
    dead[5:] = True                                       # three pad keys
    return {"k": Operand(k, interior=dead), "out": Operand(torch.zeros(4))}


def test_pad_key_read_that_only_the_nan_fill_shows():
    """0 * pad: zero for every finite pad key, NaN for a NaN one."""
    def fn(t):
        wgt = torch.tensor([1.0] * 5 + [0.0] * 3)
        t["out"].copy_((wgt[:, None] * t["k"]).sum(0))
    o = pad_key_operands()
    assert not iso.run_isolated(fn, o, ["out"], fill="max")
    found = iso.run_isolated(fn, o, ["out"], fill="nan")
    assert found and found[0].operand == "out" and "NaN / Inf the tight run does not hold" in found[0].side


def test_pad_key_read_that_only_the_huge_fill_shows():
    """A max that drops NaN operands (as the hardware's max instructions do): the NaN pad key vanishes, the huge one wins."""
    def fn(t):
        m = torch.zeros(4)
        for row in t["k"]:
            m = torch.fmax(m, row)                        # fmax drops a NaN operand; the pad keys take part (the bug)
        t["out"].copy_(m)
    o = pad_key_operands()
    assert not iso.run_isolated(fn, o, ["out"], fill="nan")
    found = iso.run_isolated(fn, o, ["out"], fill="max")
    assert found and found[0].operand == "out"
    assert "guard fill 'max'" in str(failure(fn, o))


def test_input_modified_without_being_declared_in_place():
    def fn(t):
        good(t)
        t["w"][2, 3] += 1.0
    err = failure(fn, operands(True))
    assert [d.operand for d in err.damages] == ["w", "w"] and "input modified" in err.damages[0].side and err.damages[0].first[1:] == (2, 3)


def test_part_of_the_output_left_unwritten():
    def fn(t):
        t["out"][:M - 1].copy_((t["x"].float() @ t["w"].float().t()).to(torch.bfloat16)[:M - 1])
    err = failure(fn, operands(True))
    assert len(err.damages) == 2
    for d in err.damages:
        assert d.operand == "out" and d.first[1:] == (M - 1, 0) and d.last[1:] == (M - 1, N - 1)


def test_write_in_front_and_into_the_interior_guard():
    def fn(t):
        good(t)
        if roomy(t["out"]):
            torch.as_strided(t["out"], (8,), (1,), t["out"].storage_offset() - 8 - 8)[:] = 3.0      # in front of the parent
    err = failure(fn, operands(True))
    assert any(d.operand == "out" and d.side.startswith("in front") for d in err.damages), str(err)

    def fn2(t):
        t["out"].copy_(t["k"].sum(0) * 0 + 1)
        t["k"][6, 1] = 0.5                               # a pad key written
    err = failure(fn2, pad_key_operands())
    assert any(d.operand == "k" and d.side.startswith("interior") and d.first[1:] == (6, 1) for d in err.damages), str(err)


def test_guard_rule():
    o = Operand(torch.zeros(10, 1152, dtype=torch.bfloat16), parent=(10, 3456), at=(0, 1152))
    assert o.band >= 256 * 3456 and o.band * 2 >= iso.MIN_GUARD_BYTES
    assert Operand(torch.zeros(3, dtype=torch.float32)).band * 4 >= iso.MIN_GUARD_BYTES
    assert iso.fill_bits(torch.bfloat16, "nan") == 0x7FA5 and torch.isnan(torch.tensor([0x7FA5], dtype=torch.int16).view(torch.bfloat16)).all()
    assert torch.tensor([iso.fill_bits(torch.float32, "max")], dtype=torch.int32).view(torch.float32).item() == torch.finfo(torch.float32).max


# ------------------------------------------------------------------------------------------------ coverage ratchet
def kernel_launching_ops():
    """Public module-level functions of videosys_amd/ops.py that reach ``_call`` (directly or through another function of the module)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "videosys_amd", "ops.py")
    tree = ast.parse(open(path).read())
    calls = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            calls[node.name] = {n.func.id for n in ast.walk(node) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
    reach = {"_call"}
    while True:
        more = {f for f, c in calls.items() if c & reach} - reach
        if not more:
            break
        reach |= more
    return sorted(f for f in reach if not f.startswith("_")), sorted(f for f in calls if not f.startswith("_"))


def test_every_kernel_launching_op_has_a_case_or_a_reason():
    launching, public = kernel_launching_ops()
    assert len(launching) >= 50, launching
    covered = cases.covered_ops()
    missing = [f for f in launching if f not in covered and f not in cases.NOT_COVERED]
    assert not missing, f"ops without an isolation case (add a row to tests/isolation_cases.py): {missing}"
    assert not [f for f in launching if f in cases.NOT_COVERED], "NOT_COVERED holds host-side helpers and the named exclusions only"
    unknown = [f for f in covered if f not in launching]
    assert not unknown, f"the case table names functions that launch nothing or do not exist: {unknown}"
    for f in public:
        assert f in covered or f in cases.NOT_COVERED, f"public function {f} of ops.py is neither covered nor listed with a reason"
    for name, why in cases.NOT_COVERED.items():
        assert isinstance(why, str) and len(why) > 8, name


def test_case_table_is_data():
    names = [c.name for c in cases.CASES]
    assert len(names) == len(set(names)), "case names are the test ids: they must be unique"
    assert {c.family for c in cases.CASES} == {"gemm", "flash72", "temporal", "d64", "rowwise", "vae_t5"}
    for c in cases.CASES:
        assert callable(c.builder) and c.ops and c.gemm_variants and c.flash_variants
