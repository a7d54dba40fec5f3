"""CPU: the instruction count of the GEMM epilogues stays where the "epilogue diet" put it.

tools/epilogue_mix.py cross-compiles gemm_bf16.hip and counts, per wave, the instructions of each gate + residual kernel's K loop
and of everything behind it.  Against the two committed records (profiles/epilogue_mix_parent.json: the tree before the change,
profiles/epilogue_mix_branch.json: the tree with it):
  * the K loop is the parent's — every class of vector, matrix, LDS, memory and wait instruction has the parent's count (the class
    "rest" = scalar bookkeeping and branches is left out: the compiler moves an s_mov in or out of the loop when code BEHIND it changes,
    gemm_kernel<2, ...> 66 -> 65, with the loop's source untouched);
  * the non-MFMA v_* instructions behind the loop are fewer than the parent's, and no more than the branch record's, so a later
    change cannot quietly put them back.
The numbers come from the two JSON files."""
import functools
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = ["gemm_bf16.hip"]   # (gemm2_bf16.hip is in both records with equal counts: its part of the diet was measured and not kept)


def _record(name):
    with open(os.path.join(ROOT, "profiles", name)) as fh:
        return json.load(fh)


BRANCH = _record("epilogue_mix_branch.json")
PARENT = _record("epilogue_mix_parent.json")
CASES = [(src, k) for src in SOURCES for k in BRANCH.get(src, {})]


@functools.lru_cache(maxsize=None)
def _now(tmp):
    out = os.path.join(tmp, "mix.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "epilogue_mix.py")] +
                       [os.path.join(ROOT, "videosys_amd", "csrc", s) for s in SOURCES] + ["--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def now(tmp_path_factory):
    return _now(str(tmp_path_factory.mktemp("epilogue_mix")))


def test_records_name_the_same_kernels():
    assert CASES, "the branch record is empty"
    for src, k in CASES:
        assert k in PARENT.get(src, {}), f"{k} is not in the parent record"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,kernel", CASES)
def test_epilogue_instruction_count(now, src, kernel):
    got, parent, branch = now[src][kernel], PARENT[src][kernel], BRANCH[src][kernel]
    loop = {c: n for c, n in got["k_loop"]["classes"].items() if c != "rest"}
    assert loop == {c: n for c, n in parent["k_loop"]["classes"].items() if c != "rest"}, f"{kernel}: the K loop changed"
    n = got["after"]["valu_non_mfma"]
    print(f"{kernel}: non-MFMA VALU behind the K loop: parent {parent['after']['valu_non_mfma']}, record {branch['after']['valu_non_mfma']}, now {n}")
    assert n < parent["after"]["valu_non_mfma"], f"{kernel}: {n} non-MFMA VALU behind the loop, the parent had {parent['after']['valu_non_mfma']}"
    assert n <= branch["after"]["valu_non_mfma"], f"{kernel}: {n} non-MFMA VALU behind the loop, the record has {branch['after']['valu_non_mfma']}"
