"""No GPU: the Vchitect-2.0 entry points in the header, the library's exports, the ctypes table and the generated op table — the new
entries are there and every name and op code that existed before them is unchanged (op codes are ABI: recorded programs hold them).
Host-side argument checks of vsys_attn_temporal_d64 / vsys_scale_add_rows (a refused call launches nothing).  The restatement
tests/vchitect_ref.py against an independent torch formulation (complex multiply, F.scaled_dot_product_attention)."""
import ctypes
import os
import re

import torch

import vchitect_ref as vr
from op_table import LATER, TOO_WIDE, assert_coded, prototype_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3

# entry point -> VSYS_OP code before vsys_attn_temporal_d64 was added
OPCODES_BEFORE = {
    "vsys_gemm_bf16": 1, "vsys_linear_small": 2, "vsys_adaln_modulate": 3, "vsys_mod_table": 4, "vsys_timestep_embedding": 5,
    "vsys_patch_embed": 6, "vsys_final_layer": 7, "vsys_cfg_euler_step": 8, "vsys_add_rows": 9, "vsys_copy_4d_batch": 10,
    "vsys_attn_prep_kv": 11, "vsys_flash_attn_d72": 12, "vsys_attn_temporal_d72": 13, "vsys_add_bcast_rows": 14,
    "vsys_gemm_bf16_gate2": 15, "vsys_ln_modulate": 16, "vsys_gate_add_rows": 17, "vsys_attn_prep_kv64": 18, "vsys_flash_attn_d64": 19,
    "vsys_patch_embed_shard": 20, "vsys_final_layer_tokens": 21, "vsys_unpatchify_tokens": 22, "vsys_gemm_bf16_ln": 23,
    "vsys_gemm_bf16_stats": 24, "vsys_adaln_prescale": 25, "vsys_ln_row_stats": 26, "vsys_gemm_bf16_gate_res_add": 27,
    "vsys_flash_attn_d72_kb": 28, "vsys_flash_attn_d64_kb": 29, "vsys_flash_attn_d72_exact": 30, "vsys_p2p_exchange": 31,
    "vsys_cfg_linear_step": 32, "vsys_copy_4d": 33, "vsys_im2col_patch": 34, "vsys_unpatchify_cvx": 35, "vsys_gather_rows": 36,
    "vsys_rms_norm_rows": 37, "vsys_geglu": 38, "vsys_splitk_reduce_t": 39, "vsys_t5_attention": 40, "vsys_gemm_skinny_slices": 41,
    "vsys_splitk_reduce": 42, "vsys_t5_attention_mfma": 43, "vsys_conv_bf16": 44, "vsys_gn_stats": 45, "vsys_gn_apply": 46,
    "vsys_regrid": 47, "vsys_subsample": 48, "vsys_spatial_norm_apply": 49, "vsys_blend_edge": 50, "vsys_d2s_time": 51,
    "vsys_vae_first_im2col": 52, "vsys_extract_planar": 53, "vsys_softmax_rows": 54, "vsys_attn_prep_kv_varlen": 55,
    "vsys_flash_attn_d72_varlen": 56, "vsys_gemm_bf16_ln_qkv_kv": 57,
}
NEW = ("vsys_attn_temporal_d64", "vsys_scale_add_rows")


def test_op_table_keeps_every_code_and_adds_the_new_entries():
    from videosys_amd import _lib, _opcodes

    for name, code in OPCODES_BEFORE.items():
        assert _opcodes.OPCODES.get(name) == code, name
    new = {n: c for n, c in _opcodes.OPCODES.items() if n not in OPCODES_BEFORE and n not in LATER}
    assert set(new) == set(NEW)
    assert sorted(new.values()) == [58, 59]
    # every entry point coded since then, in declaration order, and nothing else
    assert [(n, _opcodes.OPCODES.get(n)) for n in LATER] == list(zip(LATER, range(60, 75)))
    assert len(_opcodes.OPCODES) == len(OPCODES_BEFORE) + len(NEW) + len(LATER) == 74
    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VSYS_OP_(\w+)\s+(\d+)", hdr)}
    assert defines.pop("COUNT") == 75
    assert defines == {n[5:].upper(): c for n, c in _opcodes.OPCODES.items()}
    assert "#define VSYS_ABI_VERSION 1" in re.sub(r"[ \t]+", " ", hdr)
    m = re.search(r"#define VSYS_CMD_MAX_INT (\d+)\n#define VSYS_CMD_MAX_FLOAT (\d+)", hdr)
    assert (int(m.group(1)), int(m.group(2))) == (24, 4)          # the command record did not grow
    for n in NEW:
        assert re.search(rf"\nint {n}\(", hdr) and n in _lib.SIGNATURES
        nargs = len(_lib.SIGNATURES[n]) - 1
        assert sum(t is not _lib._f32 for t in _lib.SIGNATURES[n][:-1]) <= 24 and nargs > 0


def test_library_exports_and_arity():
    from videosys_amd import _lib, _opcodes

    lib = _lib.load()
    assert_coded(LATER)
    for n in list(OPCODES_BEFORE) + list(NEW) + list(LATER):
        assert hasattr(lib, n), n
        ni, nf = ctypes.c_int(), ctypes.c_int()
        assert lib.vsys_program_op_info(_opcodes.OPCODES[n], ctypes.byref(ni), ctypes.byref(nf)) == 0
        sig = _lib.SIGNATURES[n][:-1]
        assert (ni.value, nf.value) == (sum(t is not _lib._f32 for t in sig), sum(t is _lib._f32 for t in sig)), n
    assert lib.vsys_abi_version() == 1


def test_an_entry_point_has_a_code_exactly_when_it_fits_a_command():
    """Over every prototype of the header whose last parameter is the stream: in OPCODES if and only if its integer / pointer count is
    at most VSYS_CMD_MAX_INT (24) and its float count at most VSYS_CMD_MAX_FLOAT (4); exactly one entry point is outside."""
    from videosys_amd import _opcodes

    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    launch = {n: kinds[:-1] for n, (kinds, _) in _opcodes.ENTRY_POINTS.items()
              if re.search(rf"\nint {n}\([^;]*?void\* stream\);", hdr, flags=re.S)}
    outside = set()
    for n, kinds in launch.items():
        ni, nf = len(kinds) - kinds.count("f"), kinds.count("f")
        assert (ni, nf) == prototype_counts(n), n
        fits = ni <= 24 and nf <= 4
        assert (n in _opcodes.OPCODES) == fits, (n, ni, nf)
        if not fits:
            outside.add(n)
    assert outside == {TOO_WIDE}
    assert prototype_counts(TOO_WIDE) == (26, 0)
    assert set(_opcodes.OPCODES) == set(launch) - outside


def test_host_side_argument_checks():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # a 16-byte aligned address that is never dereferenced: every call below is refused before any launch

    def temporal(B=1, T=4, S=3, L=2, heads=2, ld=128, vid=P, txt=P, cos=P, sin=P, out=P, qp=None):
        q = vid if qp is None else qp
        return lib.vsys_attn_temporal_d64(q, ld, vid, ld, vid, ld, txt, ld, txt, ld, txt, ld, cos, sin, out, ld, out if txt else None, ld,
                                          B, T, S, L, heads, None)

    assert temporal(T=0) == VSYS_ERR_SHAPE
    assert temporal(heads=0) == VSYS_ERR_SHAPE
    assert temporal(S=0, L=0) == VSYS_ERR_SHAPE
    assert temporal(B=0) == VSYS_ERR_SHAPE
    assert temporal(ld=64) == VSYS_ERR_SHAPE                     # a row narrower than heads * 64
    assert temporal(ld=132) == VSYS_ERR_ALIGN                    # a stride that is no multiple of 8 elements
    assert temporal(qp=P + 2) == VSYS_ERR_ALIGN                  # a pointer off the 16-byte grid
    assert temporal(sin=None) == VSYS_ERR_ARG                    # one RoPE table without the other
    assert temporal(vid=None) == VSYS_ERR_ARG                    # S > 0 without video rows
    assert temporal(txt=None) == VSYS_ERR_ARG                    # L > 0 without text rows
    assert temporal(T=1 << 31) == VSYS_ERR_SHAPE

    def combine(rows=4, C=64, lda=64, ldb=64, ldo=64, a=P, b=P, out=P):
        return lib.vsys_scale_add_rows(a, lda, b, ldb, out, ldo, rows, C, 1.1, None)

    assert combine(a=None) == VSYS_ERR_ARG
    assert combine(C=60) == VSYS_ERR_SHAPE
    assert combine(lda=56) == VSYS_ERR_SHAPE
    assert combine(ldb=68) == VSYS_ERR_ALIGN
    assert combine(out=P + 8) == VSYS_ERR_ALIGN
    assert combine(rows=-1) == VSYS_ERR_SHAPE
    assert combine(rows=0) == 0                                  # nothing to do, nothing launched


def test_restatement_matches_an_independent_formulation():
    """apply_rotary against view_as_complex * polar (the reference's own expression), the three attentions against
    F.scaled_dot_product_attention on tensors rearranged as the reference rearranges them."""
    import torch.nn.functional as F

    B, T, S, L, H = 2, 3, 5, 4, 2
    C = H * 64
    g = torch.Generator().manual_seed(0)
    t = {n: torch.randn(B * T, S if n.endswith("vid") else L, C, generator=g).to(torch.bfloat16).double()
         for n in ("q_vid", "k_vid", "v_vid", "q_txt", "k_txt", "v_txt")}
    cos, sin = vr.rope_tables(T)
    freqs = 1.0 / (vr.THETA ** (torch.arange(0, 64, 2).float() / 64))
    cis = torch.polar(torch.ones(T, 32), torch.outer(torch.arange(T, dtype=torch.float), freqs))
    assert torch.equal(cis.real, cos) and torch.equal(cis.imag, sin)
    x = torch.randn(7, T, H, 64, generator=g, dtype=torch.float64)
    xc = torch.view_as_complex(x.reshape(7, T, H, 32, 2)) * cis.to(torch.complex128).view(1, T, 1, 32)
    assert torch.allclose(vr.apply_rotary(x, cos.double(), sin.double()), torch.view_as_real(xc).flatten(3), atol=1e-14)
    # temporal: (B T) S H C -> (B S) T H C by hand
    SL = S + L
    def to_t(a, b):
        j = torch.cat([a, b], dim=1).view(B, T, SL, H, 64).permute(0, 2, 1, 3, 4).reshape(B * SL, T, H, 64)
        return j
    q, k, v = to_t(t["q_vid"], t["q_txt"]), to_t(t["k_vid"], t["k_txt"]), to_t(t["v_vid"], t["v_txt"])
    rot = lambda y: torch.view_as_real(torch.view_as_complex(y.reshape(B * SL, T, H, 32, 2)) * cis.to(torch.complex128).view(1, T, 1, 32)).flatten(3)
    o = F.scaled_dot_product_attention(rot(q).transpose(1, 2), rot(k).transpose(1, 2), v.transpose(1, 2)).transpose(1, 2)
    o = o.reshape(B, SL, T, C).permute(0, 2, 1, 3).reshape(B * T, SL, C)
    ov, ot = vr.temporal_attention(*(t[n] for n in ("q_vid", "k_vid", "v_vid", "q_txt", "k_txt", "v_txt")), cos.double(), sin.double(),
                                   B, T, H, round_rope=False)
    assert torch.allclose(torch.cat([ov, ot], dim=1), o, atol=1e-12)
    # spatial
    j = lambda a, b: torch.cat([a, b], dim=1).view(B * T, SL, H, 64).transpose(1, 2)
    o = F.scaled_dot_product_attention(j(t["q_vid"], t["q_txt"]), j(t["k_vid"], t["k_txt"]), j(t["v_vid"], t["v_txt"]))
    want = vr.spatial_attention(*(t[n] for n in ("q_vid", "k_vid", "v_vid", "q_txt", "k_txt", "v_txt")), H)
    assert torch.allclose(want, o.transpose(1, 2).reshape(B * T, SL, C), atol=1e-12)
    # cross: the reference's lines 781-798 on the same tensors
    ky = t["k_txt"][0].unsqueeze(0).view(B, -1, H, 64).transpose(1, 2)
    vy = t["v_txt"][0].unsqueeze(0).view(B, -1, H, 64).transpose(1, 2)
    qy = torch.cat([t["q_vid"], t["q_txt"]], dim=1).view(B, T, SL, H, 64).permute(0, 2, 1, 3, 4).reshape(B, SL * T, H, 64).transpose(1, 2)
    o = F.scaled_dot_product_attention(qy, ky, vy).transpose(1, 2).reshape(B, SL, T, C).permute(0, 2, 1, 3).reshape(B * T, SL, C)
    assert torch.allclose(vr.cross_attention(t["q_vid"], t["q_txt"], t["k_txt"], t["v_txt"], B, T, H), o, atol=1e-12)
    a, b = torch.randn(4, 8, generator=g).to(torch.bfloat16), torch.randn(4, 8, generator=g).to(torch.bfloat16)
    assert torch.equal(vr.combine_bf16(a, b), ((a.float() * torch.tensor(1.1).float()).to(torch.bfloat16).float() + b.float()).to(torch.bfloat16))
