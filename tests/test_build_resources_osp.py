"""CPU: cross-compile csrc/attention96.hip for gfx950 and check the resources its launch assumes, in the manner of
tests/test_build_resources.py: no scratch and no VGPR spills in either kernel, the flash kernel within the 256 registers and half a
CU's LDS that two workgroups per CU leave it (__launch_bounds__(256, 2)), and its MFMA work on v_mfma_f32_16x16x32_bf16 only."""
import os
import re
import subprocess

import pytest

from test_build_resources import CSRC, HIPCC, _usage

SRC = "attention96.hip"


@pytest.mark.parametrize("pattern,max_vgpr", [("flash_attn_d96_kernel", 256), ("attn_prep_kv96_kernel", 128)])
def test_d96_kernels_have_no_scratch_and_no_spills(pattern, max_vgpr):
    hits = {k: v for k, v in _usage(SRC).items() if pattern in k}
    assert len(hits) == 1, f"{pattern}: {list(_usage(SRC))}"
    for name, res in hits.items():
        assert res.get("ScratchSize", 0) == 0, f"{name} uses scratch: {res}"
        assert res.get("VGPRs Spill", 0) == 0 and res.get("SGPRs Spill", 0) == 0, f"{name} spills: {res}"
        assert 0 < res.get("VGPRs", 0) <= max_vgpr, f"{name}: {res.get('VGPRs')} VGPRs"
        assert res.get("LDS Size", 0) <= 80 * 1024, f"{name}: {res.get('LDS Size')} bytes of LDS"


def test_d96_flash_runs_on_the_16x16x32_mfma(tmp_path):
    out = tmp_path / "a96.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, SRC)],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    mfma = re.findall(r"^\s*(v_mfma_\w+)", out.read_text(), flags=re.M)
    # one 64-key tile: 2 query groups x (4 key tiles x 3 depth chunks for Q K^T + 2 key groups x 6 output tiles for P V)
    assert mfma and set(mfma) == {"v_mfma_f32_16x16x32_bf16"} and len(mfma) == 48, (sorted(set(mfma)), len(mfma))
