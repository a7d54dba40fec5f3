"""CPU: cross-compile csrc/vae_osp.hip for gfx950 and check the resources of the two kernels of the Open-Sora-Plan v1.1 pipeline, in the
manner of tests/test_build_resources_osp.py: no scratch, no VGPR or SGPR spills, no static LDS.  Both are compiled with
__launch_bounds__(256) — four waves per workgroup, which by itself would allow 512 registers per lane — and are streaming kernels
that hide memory latency with resident waves alone, so the bound asserted is the one FULL occupancy needs: at most 64 VGPRs (eight
waves per SIMD on CDNA, 512 / 8).  vsys_cfg_pndm_step carries four pointers and twelve doubles as kernel arguments next to its
operands: the SGPR-spill assertion is what keeps that argument block from growing past the scalar file."""
import pytest

from test_build_resources import _usage

SRC = "vae_osp.hip"


@pytest.mark.parametrize("pattern", ["upsample_time2x_kernelILb0E", "upsample_time2x_kernelILb1E", "cfg_pndm_kernel"])
def test_v110_pipeline_kernels_have_no_scratch_no_spills_and_full_occupancy(pattern):
    hits = {k: v for k, v in _usage(SRC).items() if pattern in k}
    assert len(hits) == 1, f"{pattern}: {list(_usage(SRC))}"
    for name, res in hits.items():
        assert res.get("ScratchSize", 0) == 0, f"{name} uses scratch: {res}"
        assert res.get("VGPRs Spill", 0) == 0 and res.get("SGPRs Spill", 0) == 0, f"{name} spills: {res}"
        assert 0 < res.get("VGPRs", 0) <= 64, f"{name}: {res.get('VGPRs')} VGPRs (more than eight waves per SIMD leave)"
        assert res.get("AGPRs", 0) == 0, f"{name}: {res.get('AGPRs')} AGPRs"
        assert res.get("LDS Size", 0) == 0, f"{name}: {res.get('LDS Size')} bytes of static LDS"
