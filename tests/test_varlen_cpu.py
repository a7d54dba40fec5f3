"""No GPU: the host side of varlen cross-attention (a prompt batch whose samples have different token counts).

* the two C entry points (vsys_attn_prep_kv_varlen, vsys_flash_attn_d72_varlen) are declared in include/videosys_amd.h, exported by the
  cross-compiled library, bound in the ctypes table and numbered in the launch-program op table — all four agree on the arguments;
* ``stdit3.text_lengths``: the helper that turns a padding mask or a list of lengths into (y_lens, cu_seqlens), and what it rejects;
* the argument checks of both entry points that need no device (they read the HOST copy of the lengths and return before any launch).
"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsys_attn_prep_kv_varlen", "vsys_flash_attn_d72_varlen")
VSYS_ERR_SHAPE, VSYS_ERR_ARG = -1, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from videosys_amd import _lib

    return _lib.load()


def _prototypes():
    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    out = {}
    for name, args in re.findall(r"\nint (vsys_\w+)\(([^;]*?)\);", hdr, flags=re.S):
        out[name] = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
    return hdr, out


def test_varlen_entry_points_header_symbols_ctypes_and_op_table_agree(lib):
    from videosys_amd import _lib, program

    hdr, protos = _prototypes()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VSYS_OP_([A-Z0-9_]+)\s+(\d+)", hdr)}
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/videosys_amd.h"
        assert hasattr(lib, name), f"{name} is not exported by libvideosys_amd.so"
        params = protos[name]
        assert params[-1] == "void* stream"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(params), f"{name}: ctypes table has {len(sig)} arguments, the header {len(params)}"
        for p, t in zip(params, sig):
            ty = p.rsplit(" ", 1)[0]
            want = ctypes.c_float if ty == "float" else ctypes.c_void_p if ty.endswith("*") else ctypes.c_int64
            assert t is want, f"{name}: parameter {p!r} is bound as {t}"
        op = program.OPCODES[name]
        assert defines[name[len("vsys_"):].upper()] == op
        ni, nf = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.vsys_program_op_info(op, ctypes.byref(ni), ctypes.byref(nf)) == 0
        nfloat = sum(1 for t in sig[:-1] if t is ctypes.c_float)
        assert (ni.value, nf.value) == (len(sig) - 1 - nfloat, nfloat)
    # the lengths travel as a device array AND a host copy (header: what the kernels read / what the entry point decides with)
    assert [p for p in protos[NEW[0]] if "cu_seqlens" in p] == ["const int* cu_seqlens", "const int* cu_seqlens_host"]
    assert [p for p in protos[NEW[1]] if "kv_lens" in p] == ["const int* kv_lens", "const int* kv_lens_host"]
    # the older codes are ABI: the new entry points were numbered behind them
    assert program.OPCODES["vsys_flash_attn_d72_exact"] == 30 and min(program.OPCODES[n] for n in NEW) > 30


def test_varlen_entry_points_reject_bad_lengths_on_the_host(lib):
    """Counts < 1 or > kv_pad, and a missing array, are answered from the host copy: VSYS_ERR_SHAPE / VSYS_ERR_ARG with no launch
    (this machine has no device: a launch attempt could not return these codes).  The pointers are never dereferenced."""
    fake = ctypes.c_void_p(0x1000)      # stands for device memory; the argument checks come first
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    prep = lambda cu, kv_pad=320, dev=fake: lib.vsys_attn_prep_kv_varlen(fake, 2304, fake, 2304, None, dev, cu, fake, fake, len(cu) - 1 if cu else 2,
                                                                         16, kv_pad, 1e-6, None)
    flash = lambda lens, kv_pad=320, dev=fake: lib.vsys_flash_attn_d72_varlen(fake, 1152, None, fake, fake, dev, lens, fake, 1152,
                                                                              len(lens) if lens else 2, 16, 1024, kv_pad, 1e-6, None)
    assert prep(i32(0, 300, 300, 341)) == VSYS_ERR_SHAPE          # an empty sample
    assert prep(i32(0, 300, 299)) == VSYS_ERR_SHAPE               # offsets running backwards
    assert prep(i32(0, 300, 341), kv_pad=256) == VSYS_ERR_SHAPE   # 300 keys into a 256-key buffer
    assert prep(i32(0, 300, 341), kv_pad=300) == VSYS_ERR_SHAPE   # kv_pad not a multiple of 64
    assert prep(i32(-1, 299, 340)) == VSYS_ERR_SHAPE
    assert prep(None) == VSYS_ERR_ARG and prep(i32(0, 300, 341), dev=None) == VSYS_ERR_ARG
    assert flash(i32(300, 0, 41, 7)) == VSYS_ERR_SHAPE
    assert flash(i32(300, -3)) == VSYS_ERR_SHAPE
    assert flash(i32(300, 41), kv_pad=256) == VSYS_ERR_SHAPE
    assert flash(i32(300, 41), kv_pad=310) == VSYS_ERR_SHAPE
    assert flash(None) == VSYS_ERR_ARG and flash(i32(300, 41), dev=None) == VSYS_ERR_ARG
    assert lib.vsys_strerror(VSYS_ERR_SHAPE) == b"unsupported shape"


def test_text_lengths_from_masks_and_lists():
    import torch

    from videosys_amd.stdit3 import text_lengths

    L = 12
    m = torch.zeros(2, L, dtype=torch.long)
    m[0, :9] = 1
    m[1, :4] = 1
    assert text_lengths(mask=m) == ([9, 4], [0, 9, 13])                                   # ragged
    assert text_lengths(mask=m.tolist()) == ([9, 4], [0, 9, 13])                          # nested lists
    assert text_lengths(mask=m, batch=4) == ([9, 4, 9, 4], [0, 9, 13, 22, 26])            # one mask for the cond and null halves (CFG)
    assert text_lengths(mask=m.bool(), batch=2) == ([9, 4], [0, 9, 13])
    e = torch.ones(3, L, dtype=torch.long)
    assert text_lengths(mask=e) == ([L] * 3, [0, L, 2 * L, 3 * L])                         # equal lengths
    assert text_lengths(y_lens=[300, 41, 300, 41], packed_rows=682) == ([300, 41, 300, 41], [0, 300, 341, 641, 682])
    assert text_lengths(y_lens=torch.tensor([5, 5]).tolist(), batch=2) == ([5, 5], [0, 5, 10])


def test_text_lengths_rejections():
    import torch

    from videosys_amd.stdit3 import text_lengths

    hole = torch.tensor([[1, 1, 0, 1, 0, 0], [1, 1, 1, 0, 0, 0]])
    with pytest.raises(ValueError, match="prefix"):
        text_lengths(mask=hole)                                    # a mask that is not a prefix of ones
    with pytest.raises(ValueError, match="prefix"):
        text_lengths(mask=[[0, 1, 1], [1, 1, 1]])
    with pytest.raises(ValueError, match="at least one"):
        text_lengths(mask=torch.tensor([[1, 1, 0], [0, 0, 0]]))    # an empty sample
    with pytest.raises(ValueError, match="at least one"):
        text_lengths(y_lens=[7, 0])
    with pytest.raises(ValueError, match="sum to"):
        text_lengths(y_lens=[7, 3], packed_rows=11)                # the packed text holds another number of rows
    with pytest.raises(ValueError):
        text_lengths(mask=torch.ones(2, 4), batch=3)               # 2 mask rows cannot be repeated over 3 samples
    with pytest.raises(ValueError):
        text_lengths(y_lens=[4, 4], batch=4)
    with pytest.raises(ValueError):
        text_lengths()


def test_ragged_batch_off_the_device_is_refused_not_computed_elsewhere():
    """The ragged path exists as HIP kernels only (their key counts live in device memory): a model that is not on a HIP device
    refuses a ragged batch in either input form with a ValueError that says so, before any kernel wrapper is called; equal lengths
    keep working there (the host-flow tests run the model on the CPU with the kernels faked)."""
    import torch

    from test_stdit3_hostflow_cpu import CFG, _inputs, fake_ops
    from oracle import stdit3_oracle as O
    from videosys_amd.stdit3 import STDiT3, STDiT3Config

    x, y, kw = _inputs()
    t = torch.tensor([500.0, 500.0])
    with fake_ops() as f:
        m = STDiT3(STDiT3Config(**CFG), device="cpu")
        m.load_state_dict(O.synth_state_dict(**CFG, seed=3))
        mask = torch.zeros(2, 16, dtype=torch.long)
        mask[0, :11] = 1
        mask[1, :4] = 1
        before = dict(f.calls)
        with pytest.raises(ValueError, match="HIP device"):
            m(x, t, y, **dict(kw, mask=mask))
        assert f.calls.get("attn_prep_kv", 0) == before.get("attn_prep_kv", 0) and f.calls.get("flash_attn", 0) == before.get("flash_attn", 0)
        mask[1, :11] = 1
        assert m(x, t, y, **dict(kw, mask=mask)).shape == (2, 8, 5, 8, 8)
        p = STDiT3(STDiT3Config(skip_y_embedder=True, **CFG), device="cpu")
        p.load_state_dict(O.synth_state_dict(**CFG, seed=3))
        with pytest.raises(ValueError, match="HIP device"):
            p(x, t, torch.randn(1, 15, CFG["hidden_size"]), **dict(kw, mask=[11, 4]))
