"""Shared by the no-GPU tests of the launch-program op table: the entry points that got their codes after vsys_scale_add_rows (59),
and the check that a coded entry point's command arity is the one of its prototype in include/videosys_amd.h."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# codes 60..74 in declaration order (op codes are ABI: recorded programs hold them)
LATER = ("vsys_attn_prep_kv96", "vsys_flash_attn_d96", "vsys_attn_prep_kv96_img", "vsys_flash_attn_d96_img", "vsys_attn_prep_kv_rope",
         "vsys_flash_attn_d72_rope", "vsys_clip_attention_d64", "vsys_splitk_reduce_bias_act", "vsys_vae_first_im2col_nc",
         "vsys_pixels_to_u8", "vsys_upsample_trilinear2x", "vsys_cfg_ancestral_step", "vsys_pixels_to_u8_trunc", "vsys_upsample_time2x",
         "vsys_cfg_pndm_step")
TOO_WIDE = "vsys_attn_temporal_d64_img"      # the one launch entry point that does not fit a vsys_cmd


def header():
    return open(os.path.join(ROOT, "include", "videosys_amd.h")).read()


def prototype_counts(name, hdr=None):
    """(integer / pointer, float) parameters of ``name``'s prototype in the header, the trailing ``void* stream`` excluded."""
    m = re.search(rf"\nint {name}\(([^;]*?)\);", hdr or header(), flags=re.S)
    assert m, f"{name} has no prototype in include/videosys_amd.h"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params[-1] == "void* stream", name
    nf = sum(p.rsplit(" ", 1)[0] == "float" for p in params[:-1])
    return len(params) - 1 - nf, nf


def assert_coded(names):
    """Every name has an op code, and vsys_program_op_info(code) reports the arity of the header prototype."""
    from videosys_amd import _lib, _opcodes

    lib, hdr = _lib.load(), header()
    for n in names:
        assert n in _opcodes.OPCODES, n
        ni, nf = ctypes.c_int(), ctypes.c_int()
        assert lib.vsys_program_op_info(_opcodes.OPCODES[n], ctypes.byref(ni), ctypes.byref(nf)) == 0, n
        assert (ni.value, nf.value) == prototype_counts(n, hdr), n
        assert re.search(rf"#define VSYS_OP_{n[5:].upper()}\s+{_opcodes.OPCODES[n]}\n", hdr), n
