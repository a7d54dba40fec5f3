"""CPU: csrc/conv_down_bf16.hip cross-compiled for gfx950 with the build's own flags — no scratch, no spills and the 256 registers
that two workgroups of 256 threads per CU (the shape in the file header) leave a wave.  Compile-time resource metadata only."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge
from test_build_resources import CSRC, HIPCC

SRC = "conv_down_bf16.hip"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_conv_down2_kernel_fits_two_workgroups_per_cu():
    assert SRC in ge.SOURCES
    r = subprocess.run([HIPCC] + ge.FLAGS + ge.SOURCE_FLAGS[SRC] + ["-c", os.path.join(CSRC, SRC), "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
        elif cur is not None and (m := re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?:\s+(\d+)", line)):
            cur[m.group(1).strip()] = int(m.group(2))
    hits = {k: v for k, v in usage.items() if "conv_down2_kernel" in k}
    assert len(hits) == 1, list(usage)
    (name, res), = hits.items()
    assert res.get("ScratchSize", 0) == 0 and res.get("VGPRs Spill", 0) == 0 and res.get("SGPRs Spill", 0) == 0, f"{name}: {res}"
    assert 0 < res.get("VGPRs", 0) <= 256 and res.get("Occupancy", 0) >= 2, f"{name}: {res}"
