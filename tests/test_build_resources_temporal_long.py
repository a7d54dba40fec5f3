"""CPU: csrc/attention_tlong.hip cross-compiled for gfx950 with the build's own flags — no scratch, no VGPR spills and the 256
registers that two workgroups per CU (two waves per SIMD, the target in the file header) leave a wave; the host-side refusals of the
T > 64 path of vsys_attn_temporal_d72, all returned before any launch; and the 16 s preset's latent length."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge
from test_build_resources import CSRC, HIPCC

SRC = "attention_tlong.hip"
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_long_temporal_kernels_fit_two_workgroups_per_cu():
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
    hits = {k: v for k, v in usage.items() if "attn_temporal_d72_long_kernel" in k}
    assert len(hits) == 3, list(usage)        # norm + RoPE, neither, RoPE only
    for name, res in hits.items():
        assert res.get("ScratchSize", 0) == 0 and res.get("VGPRs Spill", 0) == 0, f"{name}: {res}"
        assert 0 < res.get("VGPRs", 0) <= 256, f"{name}: {res.get('VGPRs')} VGPRs"


def test_long_temporal_refusals_come_before_any_launch():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # an aligned address that is never dereferenced: every call below is refused before any launch

    def call(qkv=P, rs=216 * 3, C=216, qw=None, kw=None, cos=None, sin=None, out=P, os_=216, B=1, T=300, S=4, heads=3):
        return lib.vsys_attn_temporal_d72(qkv, rs, C, qw, kw, cos, sin, out, os_, B, T, S, heads, 1e-6, None)

    assert call(rs=650) == VSYS_ERR_SHAPE and call(os_=220) == VSYS_ERR_SHAPE and call(C=220) == VSYS_ERR_SHAPE
    assert call(qw=P, kw=P) == VSYS_ERR_SHAPE                               # norm without RoPE past the VALU kernel's 284 frames
    assert call(S=1 << 20, rs=3456, C=1152, heads=16) == VSYS_ERR_SHAPE      # a 32-frame block's span passes 31 bits
    assert call(B=1 << 15, S=1 << 15, heads=16, C=1152, rs=3456) == VSYS_ERR_SHAPE      # more units than a grid holds
    assert call(qkv=None) == VSYS_ERR_ARG and call(cos=P) == VSYS_ERR_ARG and call(qw=P) == VSYS_ERR_ARG
    # (these three were VSYS_ERR_SHAPE — any T >= 285 was — before the block-loop kernel)
    assert call(qkv=P + 2) == VSYS_ERR_ALIGN and call(out=P + 8) == VSYS_ERR_ALIGN and call(cos=P + 2, sin=P) == VSYS_ERR_ALIGN
    assert call(T=285, qkv=P + 2, qw=P, kw=P, cos=P, sin=P) == VSYS_ERR_ALIGN


def test_the_16s_preset_is_120_latent_frames():
    from videosys_amd.open_sora_geometry import get_num_frames
    from videosys_amd.pipeline_open_sora import get_latent_size

    assert get_num_frames("16s") == 408 and get_latent_size(get_num_frames("16s"), 720, 1280)[0] == 120
