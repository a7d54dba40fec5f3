"""CPU: cross-compile csrc/attention96_img.hip for gfx950 and check the resources its launches assume, as
tests/test_build_resources_osp.py does for the plain instantiations: no scratch and no spills in either image kernel, the flash kernel
within the 256 registers and half a CU's LDS that two workgroups per CU leave it (__launch_bounds__(256, 2)), and the file's MFMA
work the same 48 v_mfma_f32_16x16x32_bf16 as the plain file's — the image addressing adds integer work to the prologue and the
epilogue and nothing to the key loop."""
import os
import re
import subprocess

import pytest

from test_build_resources import CSRC, HIPCC, _usage

SRC = "attention96_img.hip"


@pytest.mark.parametrize("pattern,max_vgpr", [("flash_attn_d96_kernel", 256), ("attn_prep_kv96_img_kernel", 128)])
def test_d96_image_kernels_have_no_scratch_and_no_spills(pattern, max_vgpr):
    hits = {k: v for k, v in _usage(SRC).items() if pattern in k}
    assert len(hits) == 1, f"{pattern}: {list(_usage(SRC))}"
    for name, res in hits.items():
        assert "Img" in name or "img" in name, f"{name} is not an image instantiation"
        assert res.get("ScratchSize", 0) == 0, f"{name} uses scratch: {res}"
        assert res.get("VGPRs Spill", 0) == 0 and res.get("SGPRs Spill", 0) == 0, f"{name} spills: {res}"
        assert 0 < res.get("VGPRs", 0) <= max_vgpr, f"{name}: {res.get('VGPRs')} VGPRs"
        assert res.get("LDS Size", 0) <= 80 * 1024, f"{name}: {res.get('LDS Size')} bytes of LDS"


def test_d96_image_flash_runs_on_the_16x16x32_mfma(tmp_path):
    out = tmp_path / "a96_img.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, SRC)],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    mfma = re.findall(r"^\s*(v_mfma_\w+)", out.read_text(), flags=re.M)
    assert mfma and set(mfma) == {"v_mfma_f32_16x16x32_bf16"} and len(mfma) == 48, (sorted(set(mfma)), len(mfma))
