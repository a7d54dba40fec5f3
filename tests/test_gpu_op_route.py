"""-m gpu: the three ways a launch reaches the attention entry points of Open-Sora-Plan — vsys_attn_prep_kv96 + vsys_flash_attn_d96,
their forms on an exchange image, vsys_attn_prep_kv_rope + vsys_flash_attn_d72_rope — give the same BITS on the same buffers:

  (a) the entry point called directly through ctypes;
  (b) the wrapper, eager: ops._call -> torch.ops.vsys.launch with the entry point's op code;
  (c) the wrapper under program.Recorder(), then Program.run(): two vsys_cmd records in ONE command array, no host action.

(c) is replayed AFTER every input (the device key counts included) has been overwritten in place with a second draw and is compared
with (b) on that draw: a replay reads the recorded addresses, not recorded values.  What the kernels compute is held element-wise by
tests/test_gpu_osp_attention.py, test_gpu_osp_attention_img.py and test_gpu_osp_v110_attention.py; nothing here has a tolerance.

Shapes: the smallest at which the routes could differ.  d96: batch 2, heads 2, 72 keys padded to 128, 72 queries and 130 (crosses one
128-row query block), device key counts [72, 17] or none, with RoPE tables and without.  Image forms: the same in slabs of seg_len 36
(two full key slabs) and 65 (the last key slab is partial), slab_rows = batch * seg_len.  d72: batch 1, heads 2; 72 keys / 130 queries
is the two-workgroup launch, 512 keys (a multiple of 64) / 64 queries the three-workgroup one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, KV = 2, 2, 72


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def bits(t):
    """A bf16 tensor as its bit patterns (rows no token owns stay NaN on every route: NaN == NaN here)."""
    return t.contiguous().view(torch.int16)


def draw(shape, seed, dtype=torch.bfloat16):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev())


def angles(n, width, seed):
    a = torch.rand(n, width, generator=torch.Generator().manual_seed(seed)) * 6.0
    return a.cos().contiguous().to(dev()), a.sin().contiguous().to(dev())


def stream():
    return torch.cuda.current_stream().cuda_stream


def check_routes(inputs, outputs, clear, direct, wrapper, codes):
    """``inputs``: {name: (tensor, second draw)}; ``outputs``: the tensors the pair writes; ``clear()`` puts them into their state
    before a call; ``direct()`` / ``wrapper()`` issue prep + flash on these buffers through ctypes / through the wrappers."""
    from videosys_amd import _lib, _opcodes, program

    assert _lib.torch_ops() is not None, "the torch.ops.vsys fragment is not loaded: (b) would not be the launch route"
    assert [_opcodes.OPCODES[n] for n in codes] == list(codes.values())

    def issue(fn):
        clear()
        fn()
        torch.cuda.synchronize()
        return [bits(t).clone() for t in outputs]

    b1 = issue(wrapper)                    # (first: the wrapper's checks hold the shapes before the bare ctypes call)
    assert not any(torch.isnan(t).all() for t in outputs), "a launch wrote nothing"
    a1 = issue(direct)
    clear()
    with program.Recorder() as rec:
        wrapper()
    prog = rec.finish()
    assert prog is not None, rec.invalid
    torch.cuda.synchronize()
    c1 = [bits(t).clone() for t in outputs]
    assert prog.n_launches == 2 and len(prog.segments) == 1 and isinstance(prog.segments[0], tuple), "not one command array of two launches"
    assert [c.op for c in prog.segments[0][0]] == list(codes.values())
    for name, x, y, z in zip(("prep kp", "prep vt", "flash out"), a1, b1, c1):
        assert torch.equal(x, y), f"{name}: ctypes and torch.ops.vsys.launch differ"
        assert torch.equal(y, z), f"{name}: the recording call differs from the eager one"
    for t, second in inputs.values():
        t.copy_(second)
    b2 = issue(wrapper)
    assert not torch.equal(b2[2], b1[2]), "the second draw gives the first draw's output: the case shows nothing"
    clear()
    prog.run()
    torch.cuda.synchronize()
    for name, y, z in zip(("prep kp", "prep vt", "flash out"), b2, [bits(t) for t in outputs]):
        assert torch.equal(y, z), f"{name}: the replay on overwritten inputs differs from the eager call on them"


def d96_case(q_len, lens, rope, seg):
    """seg None: the base entry points; else both on exchange images of slabs of ``seg`` tokens per sample."""
    from videosys_amd import _lib
    from videosys_amd import open_sora_plan_ops as oops

    C = H * 96
    img = seg is not None
    rows = lambda n: B * n if not img else -(-n // seg) * B * seg
    seed = 1000 * q_len + (seg or 0)
    q, kv = draw((rows(q_len), C), seed), draw((rows(KV), 2 * C), seed + 1)        # k | v side by side: row stride 2C
    inputs = {"q": (q, draw(q.shape, seed + 2)), "kv": (kv, draw(kv.shape, seed + 3))}
    qt = kt = (None, None)
    if rope:
        qt, kt = angles(q_len, 96, seed + 4), angles(KV, 96, seed + 5)
        for k, (t, s) in enumerate(zip(qt + kt, angles(q_len, 96, seed + 6) + angles(KV, 96, seed + 7))):
            inputs[f"table{k}"] = (t, s)
    kl = None
    if lens:
        kl = torch.tensor([72, 17], dtype=torch.int32, device=dev())
        inputs["kv_lens"] = (kl, torch.tensor([41, 72], dtype=torch.int32, device=dev()))
    kp, vt = oops.alloc_kv_buffers96(B, H, KV, dev())
    assert kp.shape[-2] == 128
    out = torch.empty(rows(q_len), C, dtype=torch.bfloat16, device=dev())
    k, v = kv[:, :C], kv[:, C:]
    p = lambda t: None if t is None else t.data_ptr()
    lib = _lib.load()

    def direct():
        tail_p, tail_f = ((seg, B * seg), (seg, B * seg, B * seg)) if img else ((), ())
        prep = lib.vsys_attn_prep_kv96_img if img else lib.vsys_attn_prep_kv96
        flash = lib.vsys_flash_attn_d96_img if img else lib.vsys_flash_attn_d96
        _lib.check(prep(p(k), k.stride(0), p(v), v.stride(0), p(kt[0]), p(kt[1]), p(kp), p(vt), B, H, KV, 128, *tail_p, stream()), "prep")
        _lib.check(flash(p(q), q.stride(0), p(qt[0]), p(qt[1]), p(kp), p(vt), p(kl), p(out), out.stride(0), B, H, q_len, KV, 128, *tail_f,
                         stream()), "flash")

    def wrapper():
        if img:
            oops.attn_prep_kv96_img(k, v, *kt, kp, vt, B, H, KV, seg, B * seg)
            oops.flash_attn96_img(q, *qt, kp, vt, kl, out, B, H, q_len, KV, seg, B * seg, B * seg)
        else:
            oops.attn_prep_kv96(k, v, *kt, kp, vt, B, H, KV)
            oops.flash_attn96(q, *qt, kp, vt, kl, out, B, H, q_len, KV)

    names = ("vsys_attn_prep_kv96_img", "vsys_flash_attn_d96_img") if img else ("vsys_attn_prep_kv96", "vsys_flash_attn_d96")
    codes = dict(zip(names, (62, 63) if img else (60, 61)))
    clear = lambda: [t.fill_(float("nan")) for t in (kp, vt, out)]      # (the prep writes every element of kp and vt)
    check_routes(inputs, (kp, vt, out), clear, direct, wrapper, codes)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("lens", [True, False], ids=["kv_lens", "all_keys"])
@pytest.mark.parametrize("q_len", [72, 130])
def test_d96_pair_same_bits_on_every_route(q_len, lens, rope):
    d96_case(q_len, lens, rope, None)


@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("lens", [True, False], ids=["kv_lens", "all_keys"])
@pytest.mark.parametrize("q_len", [72, 130])
@pytest.mark.parametrize("seg", [36, 65])
def test_d96_image_pair_same_bits_on_every_route(seg, q_len, lens, rope):
    d96_case(q_len, lens, rope, seg)


@pytest.mark.parametrize("kv_len,q_len", [(72, 130), (512, 64)], ids=["two_workgroups", "three_workgroups"])
def test_d72_rope_pair_same_bits_on_every_route(kv_len, q_len):
    from videosys_amd import _lib
    from videosys_amd import open_sora_plan_v110_ops as vops

    Bt, C = 1, H * 72
    seed = 7200 + kv_len
    q, kv = draw((Bt * q_len, C), seed), draw((Bt * kv_len, 2 * C), seed + 1)
    qt, kt = angles(q_len, 36, seed + 4), angles(kv_len, 36, seed + 5)
    inputs = {"q": (q, draw(q.shape, seed + 2)), "kv": (kv, draw(kv.shape, seed + 3))}
    for k, (t, s) in enumerate(zip(qt + kt, angles(q_len, 36, seed + 6) + angles(kv_len, 36, seed + 7))):
        inputs[f"table{k}"] = (t, s)
    kp, vt = vops.alloc_kv_buffers(Bt, H, kv_len, dev())
    kv_pad = kp.shape[-2]
    out = torch.empty(Bt * q_len, C, dtype=torch.bfloat16, device=dev())
    k, v = kv[:, :C], kv[:, C:]
    lib = _lib.load()

    def direct():
        _lib.check(lib.vsys_attn_prep_kv_rope(k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), kt[0].data_ptr(), kt[1].data_ptr(),
                                              kp.data_ptr(), vt.data_ptr(), Bt, H, kv_len, kv_pad, stream()), "prep")
        _lib.check(lib.vsys_flash_attn_d72_rope(q.data_ptr(), q.stride(0), qt[0].data_ptr(), qt[1].data_ptr(), kp.data_ptr(), vt.data_ptr(),
                                                out.data_ptr(), out.stride(0), Bt, H, q_len, kv_len, kv_pad, stream()), "flash")

    def wrapper():
        vops.attn_prep_kv_rope(k, v, *kt, kp, vt, Bt, H, kv_len)
        vops.flash_attn_rope(q, *qt, kp, vt, out, Bt, H, q_len, kv_len)

    def clear():     # (the prep leaves some rows of vt alone, which must be zero on entry: ops.alloc_kv_buffers)
        kp.zero_(), vt.zero_(), out.fill_(float("nan"))

    check_routes(inputs, (kp, vt, out), clear, direct, wrapper, {"vsys_attn_prep_kv_rope": 64, "vsys_flash_attn_d72_rope": 65})
