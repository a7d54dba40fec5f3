"""CPU: the code object of csrc/conv_time_down_bf16.hip that build() produced — the MFMA kernel's metadata says 222 VGPRs (at most 256:
two workgroups of 256 threads per CU), no scratch, no spills and the 65536 bytes of (static) LDS that two workgroups per CU leave
each, as the file header states; the pool-only kernel uses no LDS and no scratch."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

OBJ = os.path.join(ge.CSRC, "build", "ship", "conv_time_down_bf16.o")
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
FIELDS = r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)"


@pytest.mark.skipif(not (os.path.exists(ge._hipcc()) and os.path.exists(READELF)), reason="ROCm toolchain not installed")
@pytest.mark.parametrize("kernel, vgprs, lds", [("conv_time_down2_kernel", 222, 65536), ("time_pool_down2_kernel", 64, 0)])
def test_conv_time_down2_kernel_resources(tmp_path, kernel, vgprs, lds):
    assert "conv_time_down_bf16.hip" in ge.SOURCES and ge.SOURCE_FLAGS["conv_time_down_bf16.hip"] == ge._NO_PK_F32
    ge.build()
    obj = shutil.copy(OBJ, str(tmp_path / "k.o"))                 # the offload bundles are extracted beside the file
    subprocess.run([OBJDUMP, "--offloading", obj], check=True, capture_output=True, cwd=str(tmp_path))
    (co,) = [str(f) for f in tmp_path.iterdir() if f.name.endswith("gfx950")]
    notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = [b for b in notes.split("- .agpr_count:")[1:] if kernel in b]
    assert len(blocks) == 1, notes[-2000:]
    meta = {k: int(v) for k, v in re.findall(FIELDS, blocks[0])}
    assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, meta
    assert 0 < meta["vgpr_count"] <= vgprs <= 256 and meta["group_segment_fixed_size"] == lds and 2 * lds <= 160 * 1024, meta
