"""CPU: csrc/attention_vae.hip cross-compiled for gfx950 with the build's flags — no scratch, no spills, at most the 256 registers of two
waves per SIMD for every head dim.  LDS <= 160 KB is a static_assert of the source: the compile succeeding pins it.  Metadata only."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge
from test_build_resources import CSRC, HIPCC

SRC = "attention_vae.hip"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_vae_flash_kernels_fit_their_budget():
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
    hits = {k: v for k, v in usage.items() if "vae_flash_attn_kernel" in k}
    assert len(hits) == 3, list(usage)        # NB = 1, 2, 4
    for name, res in hits.items():
        assert res.get("ScratchSize", 0) == 0 and res.get("VGPRs Spill", 0) == 0 and res.get("SGPRs Spill", 0) == 0, f"{name}: {res}"
        assert 0 < res.get("VGPRs", 0) + res.get("AGPRs", 0) <= 256 and res.get("Occupancy", 0) >= 2, f"{name}: {res}"
