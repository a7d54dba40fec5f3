"""CPU: cross-compile csrc/attention.hip for gfx950 and check the resources the launches of Open-Sora-Plan v1.1's two kernels assume,
in the manner of tests/test_build_resources_osp.py: no scratch and no spills; the roped flash instantiations (ABL_ROPE = 7) within
the registers of their launch bounds — 256 at two workgroups per CU, 168 at three, where the instantiation is compiled without the
masked tile and so, unlike the plain one, has no spill code at all — and within the LDS two / three workgroups per CU leave them (the
two K/V stages are dynamic LDS: 2 x 23 040 bytes); the roped prep kernel within 128 registers and its 10 KiB V tile."""
import pytest

from test_build_resources import _usage

SRC = "attention.hip"


@pytest.mark.parametrize("pattern,max_vgpr,max_lds", [("flash_attn_d72_kernelILi7ELi2E", 256, 0), ("flash_attn_d72_kernelILi7ELi3E", 168, 0),
                                                      ("attn_prep_kv_rope_kernel", 128, 10240)])
def test_v110_rope_kernels_have_no_scratch_and_no_spills(pattern, max_vgpr, max_lds):
    hits = {k: v for k, v in _usage(SRC).items() if pattern in k}
    assert len(hits) == 1, f"{pattern}: {list(_usage(SRC))}"
    for name, res in hits.items():
        assert res.get("ScratchSize", 0) == 0, f"{name} uses scratch: {res}"
        assert res.get("VGPRs Spill", 0) == 0 and res.get("SGPRs Spill", 0) == 0, f"{name} spills: {res}"
        assert 0 < res.get("VGPRs", 0) <= max_vgpr, f"{name}: {res.get('VGPRs')} VGPRs"
        assert res.get("LDS Size", 0) <= max_lds, f"{name}: {res.get('LDS Size')} bytes of static LDS"


def test_only_the_two_roped_flash_instantiations_exist():
    """The roped entry point never runs the resident-K/V kernel: no ABL_ROPE instantiation with RES."""
    names = [k for k in _usage(SRC) if "flash_attn_d72_kernelILi7E" in k]
    assert sorted(n.split("flash_attn_d72_kernel")[1][:12] for n in names) == ["ILi7ELi2ELb0", "ILi7ELi3ELb0"], names
