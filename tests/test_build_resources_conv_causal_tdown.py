"""CPU: the code object of csrc/conv_causal_tdown_bf16.hip that build() produced — the kernel's metadata says at most 256 VGPRs (two
workgroups of 256 threads per CU), no scratch, no spills and the 65536 bytes of (static) LDS that two workgroups per CU leave each, as
the file header states."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

SRC = "conv_causal_tdown_bf16.hip"
OBJ = os.path.join(ge.CSRC, "build", "ship", SRC.replace(".hip", ".o"))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
FIELDS = r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)"


@pytest.mark.skipif(not (os.path.exists(ge._hipcc()) and os.path.exists(READELF)), reason="ROCm toolchain not installed")
def test_conv_causal_tdown2_kernel_resources(tmp_path):
    assert SRC in ge.SOURCES and ge.SOURCE_FLAGS[SRC] == ge._NO_PK_F32
    ge.build()
    obj = shutil.copy(OBJ, str(tmp_path / "k.o"))                 # the offload bundles are extracted beside the file
    subprocess.run([OBJDUMP, "--offloading", obj], check=True, capture_output=True, cwd=str(tmp_path))
    (co,) = [str(f) for f in tmp_path.iterdir() if f.name.endswith("gfx950")]
    notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, text=True).stdout
    blocks = [b for b in notes.split("- .agpr_count:")[1:] if "conv_causal_tdown2_kernel" in b]
    assert len(blocks) == 1, notes[-2000:]
    meta = {k: int(v) for k, v in re.findall(FIELDS, blocks[0])}
    assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, meta
    assert 0 < meta["vgpr_count"] <= 256 and meta["group_segment_fixed_size"] == 65536, meta
