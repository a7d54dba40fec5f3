"""CPU (-m "not gpu") tests of the host side: C-ABI exports, PAB/RFLOW mirrors vs reference-minted goldens,
DSP pack/unpack plans over a real 2-rank gloo group, and the no-fallback rule."""
import json
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT, load_golden
from ref_trace import ref_trace  # noqa: F401  (fixture)
from oracle import stdit3_oracle as O


def test_library_exports_every_declared_symbol():
    """Every prototype of the two public headers, parsed HERE (not by the generator that writes the table), against the ctypes table:
    same names, same argument types element for element, same return type."""
    import ctypes

    import __graft_entry__ as ge

    ge.build()
    from videosys_amd import _lib

    lib = _lib.load()

    def prototypes(header):
        text, out = open(os.path.join(ROOT, "include", header)).read(), {}
        for ret, name, args in re.findall(r"^(int|const char\*) (vsys_\w+)\(([^;]*?)\);", text, flags=re.S | re.M):
            params = [a.strip() for a in re.sub(r"\s+", " ", args).split(",")]
            types = []
            for prm in ([] if params == ["void"] else params):
                ty = prm.rsplit(" ", 1)[0]
                types.append(ctypes.c_void_p if ty.endswith("*") else {"float": ctypes.c_float, "int64_t": ctypes.c_int64, "int": ctypes.c_int}[ty])
            out[name] = (types, ctypes.c_int if ret == "int" else ctypes.c_char_p)
        return text, out

    hdr, declared = prototypes("videosys_amd.h")
    assert len(declared) >= 16
    assert set(declared) == set(re.findall(r"\b(vsys_[a-z0-9_]+)\s*\(", hdr)), "a declaration the prototype pattern does not read"
    assert set(declared) == set(_lib.SIGNATURES), "ctypes table out of sync with the header"
    for name, (types, ret) in declared.items():
        assert hasattr(lib, name), f"{name} declared in include/videosys_amd.h but not exported"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(types) and all(a is b for a, b in zip(sig, types)), f"{name}: bound as {sig}, declared as {types}"
        fn = getattr(lib, name)
        assert list(fn.argtypes) == types and fn.restype is ret, name
    assert [n for n, (_, ret) in declared.items() if ret is not ctypes.c_int] == ["vsys_strerror"]
    _, lab = prototypes("videosys_amd_lab.h")
    assert set(lab) == set(_lib.LAB_SIGNATURES) == {"vsys_lab_flash_debug_buffer", "vsys_gemm_streamk_plan"}
    for name, (types, ret) in lab.items():
        sig = _lib.LAB_SIGNATURES[name]
        assert len(sig) == len(types) and all(a is b for a, b in zip(sig, types)) and _lib.RESTYPES[name] is ret, name
        assert not hasattr(lib, name), f"{name}: a lab entry point in the shipped library"
    assert lib.vsys_abi_version() == 1
    assert lib.vsys_strerror(-1) == b"unsupported shape"


def test_c_abi_wrappers_reject_bad_arguments_before_any_launch():
    """The entry points whose wrappers share a file-local helper in csrc/capi.hip (GEMM head, flash d72 / d64, copy descriptors) and
    vsys_conv_bf16: a null operand, a count past int, batch * heads > 65535, a negative key-norm bound and a bad descriptor are answered
    with the same code as ever and in the same order of checks, with no launch (there is no device here; the pointers are never read)."""
    import ctypes

    import __graft_entry__ as ge

    ge.build()
    from videosys_amd import _lib

    lib = _lib.load()
    SHAPE, ARG = -1, -3
    P, BIG = 0x10000, 1 << 31

    # flash d72: the trio shares its checks (the bound is the _kb variant's extra argument)
    def d72(name, q=P, kp=P, vt=P, out=P, batch=2, heads=16, q_len=1024, kv_len=300, kv_pad=320, extra=()):
        return getattr(lib, name)(q, 1152, None, kp, vt, out, 1152, batch, heads, q_len, kv_len, kv_pad, 1e-6, *extra, None)

    for name, extra in (("vsys_flash_attn_d72", ()), ("vsys_flash_attn_d72_exact", ()), ("vsys_flash_attn_d72_kb", (4.0,))):
        for op in ("q", "kp", "vt", "out"):
            assert d72(name, extra=extra, **{op: None}) == ARG, (name, op)
        for n in ("batch", "heads", "q_len", "kv_len", "kv_pad"):
            assert d72(name, extra=extra, **{n: BIG}) == SHAPE, (name, n)
            assert d72(name, extra=extra, **{n: -1}) == SHAPE, (name, n)
        assert d72(name, extra=extra, batch=4096, heads=16) == SHAPE          # batch * heads = 65536
        assert d72(name, extra=extra, q=None, batch=BIG) == ARG               # the operands are looked at first
    assert d72("vsys_flash_attn_d72_kb", extra=(-0.5,)) == ARG
    assert d72("vsys_flash_attn_d72_kb", extra=(float("nan"),)) == ARG
    assert d72("vsys_flash_attn_d72_kb", extra=(-0.5,), batch=BIG) == ARG

    # flash d64: the pair
    def d64(name, q=P, ln_w=None, ln_b=None, kp=P, vt=P, out=P, rope_start=0, rope_len=0, batch=2, heads=16, q_len=512, kv_len=512,
            kv_pad=512, extra=()):
        return getattr(lib, name)(q, 1024, ln_w, ln_b, None, None, rope_start, rope_len, kp, vt, out, 1024, batch, heads, q_len, kv_len,
                                  kv_pad, 1e-6, *extra, None)

    for name, extra in (("vsys_flash_attn_d64", ()), ("vsys_flash_attn_d64_kb", (4.0,))):
        for op in ("q", "kp", "vt", "out"):
            assert d64(name, extra=extra, **{op: None}) == ARG, (name, op)
        assert d64(name, extra=extra, ln_w=P) == ARG and d64(name, extra=extra, ln_b=P) == ARG      # LayerNorm weight without bias
        for n in ("batch", "heads", "q_len", "kv_len", "kv_pad", "rope_start", "rope_len"):
            assert d64(name, extra=extra, **{n: BIG}) == SHAPE, (name, n)
            assert d64(name, extra=extra, **{n: -1}) == SHAPE, (name, n)
        assert d64(name, extra=extra, ln_w=P, batch=BIG) == ARG
    assert d64("vsys_flash_attn_d64_kb", extra=(-1.0,)) == ARG and d64("vsys_flash_attn_d64_kb", extra=(float("nan"),)) == ARG

    # GEMM entry points: (x, ldx, w, ldw, bias, out, ldo, M, N, K) head, then each one's own operands
    def gemm(x=P, w=P, out=P, M=256, N=1152, K=1152, epi=0, gate=None, res=None, aux=None, rps=0):
        return lib.vsys_gemm_bf16(x, K, w, K, None, out, N, M, N, K, epi, gate, 0, rps, res, N, aux, N, None)

    assert gemm(x=None) == ARG and gemm(w=None) == ARG and gemm(out=None) == ARG
    assert gemm(M=BIG) == SHAPE and gemm(N=BIG) == SHAPE and gemm(K=BIG) == SHAPE and gemm(rps=BIG) == SHAPE and gemm(M=-1) == SHAPE
    assert gemm(epi=0, gate=P) == ARG and gemm(epi=1, res=P) == ARG and gemm(epi=0, aux=P) == ARG    # only EPI_GATE_RES takes them
    assert gemm(x=None, M=BIG) == ARG and gemm(M=BIG, gate=P) == SHAPE

    def gemm_ln(x=P, wp=P, cs=P, cv=P, out=P, stats=P, M=256, N=3456, K=1152, epi=0):
        return lib.vsys_gemm_bf16_ln(x, K, wp, K, cs, cv, out, N, M, N, K, epi, stats, M, 1e-6, None)

    for op in ("x", "wp", "cs", "cv", "out", "stats"):
        assert gemm_ln(**{op: None}) == ARG, op
    assert gemm_ln(M=BIG) == SHAPE and gemm_ln(N=BIG) == SHAPE and gemm_ln(K=BIG) == SHAPE
    assert gemm_ln(epi=2) == ARG
    assert gemm_ln(K=1000) == SHAPE and gemm_ln(K=96 * 13) == SHAPE          # whole 96-column partials, at most 12 of them

    def qkv_kv(x=P, stats=P, knw=P, q=P, kp=P, vt=P, M=1024, K=1152, S=256, heads=16):
        return lib.vsys_gemm_bf16_ln_qkv_kv(x, K, P, K, P, P, stats, M, knw, q, 1152, kp, vt, M, K, S, heads, 1e-6, 1e-6, None)

    for op in ("x", "stats", "knw", "q", "kp", "vt"):
        assert qkv_kv(**{op: None}) == ARG, op
    assert qkv_kv(M=BIG) == SHAPE and qkv_kv(K=BIG) == SHAPE and qkv_kv(S=BIG) == SHAPE
    assert qkv_kv(heads=0) == SHAPE and qkv_kv(heads=4097) == SHAPE and qkv_kv(K=1000) == SHAPE

    def gemm_stats(x=P, out=P, stats=P, M=256, rps=0):
        return lib.vsys_gemm_bf16_stats(x, 1152, P, 1152, None, out, 1152, M, 1152, 1152, None, 0, rps, None, 1152, stats, M, None)

    assert gemm_stats(x=None) == ARG and gemm_stats(out=None) == ARG and gemm_stats(stats=None) == ARG
    assert gemm_stats(M=BIG) == SHAPE and gemm_stats(rps=BIG) == SHAPE

    def gate_res_add(x=P, out=P, res=P, M=256, rps=0):
        return lib.vsys_gemm_bf16_gate_res_add(x, 1152, P, 1152, None, out, 1152, M, 1152, 1152, None, 0, rps, res, 1152, None, None, None, None, 0,
                                               None)

    assert gate_res_add(x=None) == ARG and gate_res_add(out=None) == ARG and gate_res_add(res=None) == ARG
    assert gate_res_add(M=BIG) == SHAPE and gate_res_add(rps=BIG) == SHAPE

    def gate2(x=P, out=P, gate=P, M=256, rps=128, split=16):
        return lib.vsys_gemm_bf16_gate2(x, 1152, P, 1152, None, out, 1152, M, 1152, 1152, gate, 0, rps, split, 1152, None, 1152, None, 1152, None)

    assert gate2(x=None) == ARG and gate2(out=None) == ARG and gate2(gate=None) == ARG
    assert gate2(M=BIG) == SHAPE and gate2(rps=BIG) == SHAPE and gate2(split=BIG) == SHAPE
    assert gate2(split=-1) == SHAPE and gate2(split=129) == SHAPE              # the text rows are a prefix of the sample

    def skinny(w=P, x=P, part=P, rows=4, rows_padded=16, N=4096, K=4096, nsplit=4):
        return lib.vsys_gemm_skinny_slices(w, K, x, K, part, rows, rows_padded, N, K, nsplit, None)

    assert skinny(w=None) == ARG and skinny(x=None) == ARG and skinny(part=None) == ARG
    assert skinny(rows_padded=BIG) == SHAPE and skinny(N=BIG) == SHAPE and skinny(K=BIG) == SHAPE and skinny(nsplit=BIG) == SHAPE
    assert skinny(nsplit=0) == SHAPE and skinny(K=4100) == SHAPE and skinny(rows=0) == SHAPE and skinny(rows=17) == SHAPE
    assert skinny(K=64, nsplit=3) == SHAPE                                     # the last slice would be empty

    # copy descriptors: 14 words per problem (vsys_copy_4d_batch), 17 (vsys_p2p_exchange)
    def desc(words=14, n=1, **over):
        base = dict(src_off=0, dst_off=0, n0=2, n1=3, n2=4, C=64, ss0=768, ss1=256, ss2=64, ds0=768, ds1=256, ds2=64, n1_valid=3, n2_valid=4,
                    dst=P, flag=P, remote=0)
        base.update(over)
        return (ctypes.c_int64 * (words * n))(*(list(base.values())[:words] * n))

    batch = lambda src=P, dst=P, nops=1, d=None: lib.vsys_copy_4d_batch(src, dst, nops, desc() if d is None else d, None)
    assert batch(src=None) == ARG and batch(dst=None) == ARG and lib.vsys_copy_4d_batch(P, P, 1, None, None) == ARG
    assert batch(nops=-1) == SHAPE and batch(nops=17, d=desc(n=17)) == SHAPE
    for k in ("n0", "n1", "n2", "C", "n1_valid", "n2_valid"):
        assert batch(d=desc(**{k: BIG})) == SHAPE and batch(d=desc(**{k: -1})) == SHAPE, k
    assert batch(d=desc(src_off=-8)) == SHAPE and batch(d=desc(dst_off=-8)) == SHAPE

    def p2p(src=P, nops=1, d=None, my_flags=P, n_flags=2, self_index=0, state=P):
        return lib.vsys_p2p_exchange(src, nops, desc(17) if d is None else d, my_flags, n_flags, self_index, state, 1000, None)

    assert p2p(src=None) == ARG and p2p(my_flags=None) == ARG and p2p(state=None) == ARG
    assert lib.vsys_p2p_exchange(P, 1, None, P, 2, 0, P, 1000, None) == ARG
    assert p2p(nops=-1) == SHAPE and p2p(nops=17, d=desc(17, n=17)) == SHAPE and p2p(n_flags=BIG) == SHAPE
    assert p2p(self_index=-1) == SHAPE and p2p(self_index=2) == SHAPE
    for k in ("n0", "n1", "n2", "C", "n1_valid", "n2_valid"):
        assert p2p(d=desc(17, **{k: BIG})) == SHAPE, k
    assert p2p(d=desc(17, src_off=-8)) == SHAPE and p2p(d=desc(17, dst_off=-8)) == SHAPE
    assert p2p(d=desc(17, dst=0)) == SHAPE                                     # a problem without a destination

    # vsys_conv_bf16
    def conv(a=P, w=P, bias=None, res=None, out=P, out32=None, M=4096, N=128, cin=128, kt=3, kh=3, kw=3, row_pitch=66, plane_pitch=4356, batch=1):
        return lib.vsys_conv_bf16(a, cin, w, cin * kt * kh * kw, bias, res, N, out, out32, N, M, N, cin, kt, kh, kw, row_pitch, plane_pitch, batch,
                                  0, 0, 0, 1.0, None)

    assert conv(a=None) == ARG and conv(w=None) == ARG
    assert conv(out=None) == ARG and conv(out32=P) == ARG                      # exactly one of the two outputs
    assert conv(out=None, out32=P, bias=P) == ARG and conv(out=None, out32=P, res=P) == ARG
    for n in ("M", "N", "cin", "row_pitch", "plane_pitch", "batch"):
        assert conv(**{n: BIG}) == SHAPE, n
    assert conv(kt=0) == SHAPE and conv(kt=4) == SHAPE and conv(kh=2) == SHAPE and conv(kh=4, kw=4) == SHAPE and conv(cin=0) == SHAPE
    assert conv(cin=1 << 27) == SHAPE                                          # 27 taps: K past int
    assert conv(plane_pitch=(1 << 31) - 1) == SHAPE                            # the farthest tap's row offset past int


def test_no_cpu_fallback():
    """Ops must refuse CPU tensors instead of silently computing elsewhere."""
    from videosys_amd import ops
    from videosys_amd._lib import VsysError

    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(VsysError):
        ops.gemm(x, torch.zeros(192, 64, dtype=torch.bfloat16))
    with pytest.raises(VsysError):
        ops.add_rows(x, x)
    # and nothing in the product imports the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, "videosys_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle|from\s+\.+\s*oracle|import_module\([\"']oracle", src, re.M), \
                    f"{f} imports the oracle"


def test_pab_manager_matches_reference_schedule():
    from videosys_amd import pab
    from videosys_amd.pipeline_open_sora import OpenSoraPABConfig

    with open(os.path.join(GOLDEN, "pab_schedule_c2.json")) as f:
        g = json.load(f)
    cfg = OpenSoraPABConfig(mlp_broadcast=False)
    assert [cfg.spatial_threshold, cfg.spatial_range] == [g["cfg"]["spatial"][:2], g["cfg"]["spatial"][2]]
    pab.set_pab_manager(cfg)
    pab.update_steps(g["steps"])
    try:
        cnt = {"spatial": 0, "temporal": 0, "cross": 0}
        flags = {k: [] for k in cnt}
        fns = {"spatial": pab.if_broadcast_spatial, "temporal": pab.if_broadcast_temporal, "cross": pab.if_broadcast_cross}
        for _ in range(2):
            for t in g["timesteps_int"]:
                for k in cnt:
                    fl, cnt[k] = fns[k](t, cnt[k])
                    flags[k].append(fl)
        assert flags == g["flags"]
        assert pab.enable_pab()
    finally:
        pab.set_pab_manager(None)
    assert not pab.enable_pab()
    assert pab.if_broadcast_spatial(500, 3) == (False, 3)


def test_rflow_timesteps_match_reference():
    from videosys_amd.rflow import RFLOW

    fx = load_golden("rflow_small.pt")
    s = RFLOW(num_sampling_steps=30, cfg_scale=7.0, use_timestep_transform=True)
    ts = s.prepare_timesteps(1, dict(height=torch.tensor([512.0]), width=torch.tensor([512.0]),
                                     num_frames=torch.tensor([64.0])))
    torch.testing.assert_close(torch.cat(ts), fx["ts30_c2"], rtol=1e-6, atol=1e-4)
    assert [int(t.to(torch.bfloat16)[0]) for t in ts] == fx["ts30_c2_bf16_int"]


def test_config_surface_and_latent_size():
    import videosys_amd as V
    from videosys_amd.pipeline_open_sora import get_latent_size

    cfg = V.OpenSoraConfig(num_sampling_steps=30, cfg_scale=7.0, num_gpus=1)
    assert cfg.pipeline_cls is V.OpenSoraPipeline and cfg.num_gpus == 1 and cfg.enable_pab is False
    assert cfg.transformer == "hpcai-tech/OpenSora-STDiT-v3" and cfg.tiling_size == 4 and cfg.cpu_offload is False
    p = V.OpenSoraPABConfig()
    assert (p.spatial_range, p.temporal_range, p.cross_range, p.mlp_broadcast) == (2, 4, 6, True)
    assert p.cross_threshold == [450, 930] and 676 in p.mlp_spatial_broadcast_config
    assert get_latent_size(64, 512, 512) == (19, 64, 64)
    assert get_latent_size(128, 720, 1280) == (38, 90, 160)
    assert get_latent_size(1, 512, 512) == (1, 64, 64)
    # every frame count against the reference's arithmetic (autoencoder_kl_open_sora.py:424-439, 706-717: 17-frame micro batches,
    # each padded up to a multiple of the temporal factor 4, then divided by it; spatial / 8)
    for nf in range(1, 300):
        want = (nf // 17) * ((17 + 3) // 4) + ((nf % 17 + 3) // 4 if nf % 17 else 0)
        assert get_latent_size(nf, 360, 640) == (want, 45, 80), nf


def test_host_tables_match_oracle():
    from videosys_amd.stdit3 import pos_embed_2d, rope_tables, synth_state_dict, STDiT3Config

    torch.testing.assert_close(pos_embed_2d(576, 8, 6, 0.5, 7)[None], O.pos_embed_2d(576, 8, 6, 0.5, 7))
    freqs = 1.0 / (10000 ** (torch.arange(0, 72, 2).float() / 72))
    c, s = rope_tables(freqs, 19, torch.float32)
    co, so = O.rope_table(freqs, 19)
    torch.testing.assert_close(c, co)
    torch.testing.assert_close(s, so)
    cfg = dict(depth=1, hidden_size=144, num_heads=2, caption_channels=32, model_max_length=8)
    a = synth_state_dict(STDiT3Config(**cfg), seed=9)
    b = O.synth_state_dict(**cfg, seed=9)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ DSP over gloo
def torch_copy_executor(src, dst, ops):
    """Test-only executor with the semantics of vsys_copy_4d (the product executor is the HIP kernel)."""
    s, d = src.reshape(-1), dst.reshape(-1)
    for o in ops:
        for i0 in range(o.n0):
            for i1 in range(o.n1):
                for i2 in range(o.n2):
                    do = o.dst_off + i0 * o.dstr[0] + i1 * o.dstr[1] + i2 * o.dstr[2]
                    if i1 < o.n1_valid and i2 < o.n2_valid:
                        so = o.src_off + i0 * o.sstr[0] + i1 * o.sstr[1] + i2 * o.sstr[2]
                        d[do:do + o.run] = s[so:so + o.run]
                    else:
                        d[do:do + o.run] = 0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dsp_worker(rank, world, port, B, T, S, C, ret):
    try:
        from videosys_amd import dsp

        dsp.initialize(rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}", backend="gloo")
        pm = dsp.ParallelManager(1, 1, world)
        assert pm.sp_size == world and pm.sp_rank == rank and pm.dp_rank == 0
        dsp.set_pad("temporal", T, pm.sp_group)
        dsp.set_pad("spatial", S, pm.sp_group)
        assert dsp.get_pad("temporal") == O.dsp_pad(T, world) and dsp.get_pad("spatial") == O.dsp_pad(S, world)
        sp = dsp.SequenceParallel(pm.sp_group, copy_executor=torch_copy_executor)
        g = torch.Generator().manual_seed(123)
        x = torch.randn(B, T, S, C, generator=g).to(torch.bfloat16)
        shards = O.dsp_split_sequence(x.float(), world, dim=2)
        t_ref = O.dsp_all_to_all(shards, 1, 2, O.dsp_pad(T, world), O.dsp_pad(S, world))
        local = sp.split(x)
        assert torch.equal(local.float(), shards[rank])
        tsh = sp.to_temporal_shard(local, S)
        assert torch.equal(tsh.float(), t_ref[rank]), "to_temporal_shard"
        back = sp.to_spatial_shard(tsh, T, local.shape[2])
        assert torch.equal(back, local), "round trip"
        full = sp.gather(back, S)
        assert torch.equal(full, x), "gather"
        # the function-level operators under the reference's names (comm.py), same group, against the same restatement
        from videosys_amd import comm

        with torch.no_grad():
            pt, ps = O.dsp_pad(T, world), O.dsp_pad(S, world)
            loc = comm.split_sequence(x, pm.sp_group, dim=2, grad_scale="down", pad=comm.get_pad("spatial"))
            assert torch.equal(loc.float(), shards[rank]), "comm.split_sequence"
            tsh2 = comm.all_to_all_with_pad(loc, pm.sp_group, scatter_dim=1, gather_dim=2, scatter_pad=pt, gather_pad=ps)
            assert torch.equal(tsh2.float(), t_ref[rank]), "comm.all_to_all_with_pad"
            back2 = comm.all_to_all_with_pad(tsh2, pm.sp_group, scatter_dim=2, gather_dim=1, scatter_pad=ps, gather_pad=pt)
            assert torch.equal(back2, loc), "comm round trip"
            assert torch.equal(comm.gather_sequence(back2, pm.sp_group, dim=2, grad_scale="up", pad=ps), x), "comm.gather_sequence"
            # no pads: all_to_all_comm with negative dimensions; frames-first layout through the *_from_second_dim pair
            e = torch.arange(2 * world * 3 * world * 2, dtype=torch.float32).view(2, world * 3, world * 2)
            mine = comm.split_sequence(e, pm.sp_group, dim=-1)
            sw = comm.all_to_all_comm(mine, pm.sp_group, scatter_dim=-2, gather_dim=-1)
            assert torch.equal(sw, O.dsp_split_sequence(e, world, 1)[rank]), "comm.all_to_all_comm"
            f = x.float().reshape(B * T, S, C)
            fl = comm.split_from_second_dim(f, B, pm.sp_group)
            assert torch.equal(fl, O.dsp_split_sequence(x.float(), world, 1)[rank].reshape(-1, S, C)), "split_from_second_dim"
            assert torch.equal(comm.gather_from_second_dim(fl, B, pm.sp_group), f), "gather_from_second_dim"
            assert torch.equal(comm.gather_sequence(mine[0], pm.sp_group, dim=0), torch.cat([v[0] for v in O.dsp_split_sequence(e, world, 2)], 0))
        try:
            comm.split_sequence(x.float().requires_grad_(), pm.sp_group, dim=2)
            raise AssertionError("a tensor with a graph must be refused")
        except NotImplementedError:
            pass
        ret.put((rank, "ok"))
    except Exception as e:  # noqa
        import traceback

        ret.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("T,S", [(5, 12), (4, 7)])
def test_dsp_two_ranks_gloo(T, S):
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dsp_worker, args=(r, 2, port, 2, T, S, 16, ret)) for r in range(2)]
    for p in procs:
        p.start()
    res = [ret.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, status in res:
        assert status == "ok", f"rank {rank}: {status}"


def _ref_comm_worker(rank, world, port, ret):
    """Runs the REFERENCE's comm.py functions (replayed per rank from tests/golden/ref_traces/; live through oracle/ref_loader.py
    while minting) and this build's videosys_amd.comm on the same tensors over the same gloo group.  gloo has no list all-to-all, so ``dist.all_to_all`` — the one
    collective the reference's ``_all_to_all_func`` issues — is served by all_to_all_single here; the reference's own
    tensor_split / contiguous / cat / pad / narrow logic runs unchanged."""
    try:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)

        def list_all_to_all(outs, ins, group=None):
            send = torch.stack(ins)
            recv = torch.empty_like(send)
            dist.all_to_all_single(recv, send, group=group)
            for o, r in zip(outs, recv.unbind(0)):
                o.copy_(r)

        dist.all_to_all = list_all_to_all
        from ref_trace import Trace

        tr = Trace(f"test_host_cpu__comm_gloo_rank{rank}")

        class _R:   # the reference's comm.py, live only while minting the trace (tests/ref_trace.py)
            def __getattr__(self, name):
                def call(*a, **k):
                    def live():
                        from oracle import ref_loader

                        return getattr(ref_loader.load_reference_modules()["comm"], name)(*a, **k)
                    return tr.value(live)
                return call

        R = _R()
        from videosys_amd import comm as M

        g = torch.Generator().manual_seed(7)
        grp = dist.group.WORLD
        with torch.no_grad():
            for shape, sdim, gdim in (((2, 5, 12, 8), 1, 2), ((2, 4, 7, 8), 2, 1), ((3, 6, 10), 1, 2), ((2, 19, 6, 4), 1, 2)):
                x = torch.randn(*shape, generator=g)
                n_s, n_g = x.shape[sdim], x.shape[gdim]
                pad_s, pad_g = (world - n_s % world) % world, (world - n_g % world) % world
                # at rest: sharded along gdim (padded); the switch scatters sdim and gathers gdim
                a = R.split_sequence(x, grp, dim=gdim, grad_scale="down", pad=pad_g)
                b = M.split_sequence(x, grp, dim=gdim, grad_scale="down", pad=pad_g)
                assert torch.equal(a, b), ("split_sequence", shape)
                a2 = R.all_to_all_with_pad(a, grp, scatter_dim=sdim, gather_dim=gdim, scatter_pad=pad_s, gather_pad=pad_g)
                b2 = M.all_to_all_with_pad(b, grp, scatter_dim=sdim, gather_dim=gdim, scatter_pad=pad_s, gather_pad=pad_g)
                assert a2.shape == b2.shape and torch.equal(a2, b2), ("all_to_all_with_pad", shape)
                a3 = R.all_to_all_with_pad(a2, grp, scatter_dim=gdim, gather_dim=sdim, scatter_pad=pad_g, gather_pad=pad_s)
                b3 = M.all_to_all_with_pad(b2, grp, scatter_dim=gdim, gather_dim=sdim, scatter_pad=pad_g, gather_pad=pad_s)
                assert torch.equal(a3, b3) and torch.equal(b3, b), ("switch back", shape)
                if not pad_s:
                    assert torch.equal(R.all_to_all_comm(a, grp, sdim, gdim), M.all_to_all_comm(b, grp, sdim, gdim)), ("all_to_all_comm", shape)
                # pad value other than zero, pad registry
                assert torch.equal(R.split_sequence(x, grp, gdim, 1.0, pad_g, -3), M.split_sequence(x, grp, gdim, 1.0, pad_g, -3))
                R.set_pad("temporal", n_s, grp), M.set_pad("temporal", n_s, grp)
                assert R.get_pad("temporal") == M.get_pad("temporal") == pad_s
            f = torch.randn(2 * 5, 3, 4, generator=g)
            R.set_pad("temporal", 5, grp), M.set_pad("temporal", 5, grp)
            assert torch.equal(R.split_from_second_dim(f, 2, grp), M.split_from_second_dim(f, 2, grp))
        tr.close()
        ret.put((rank, "ok"))
    except Exception:  # noqa
        import traceback

        ret.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_comm_operators_equal_the_reference_functions_over_gloo():
    """SURVEY §8a row a13 at the function level: split_sequence / all_to_all_with_pad / all_to_all_comm / split_from_second_dim /
    set_pad of videosys_amd.comm against the reference's comm.py itself, two real processes, bit-equal."""
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ref_comm_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    res = [ret.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, status in res:
        assert status == "ok", f"rank {rank}: {status}"


@pytest.mark.parametrize("T,S", [(19, 16), (38, 24)])
def test_dsp_eight_ranks_gloo(T, S):
    """The BASELINE degree (P = 8) with the frame counts of configs 2 and 4: T = 19 -> 3 padded frames per rank, ranks 6 / 7
    hold 1 / 0 valid frames; T = 38 -> 5 per rank, rank 7 holds 3.  Same checks as the 2-rank test, 8 real processes."""
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dsp_worker, args=(r, 8, port, 2, T, S, 8, ret)) for r in range(8)]
    for p in procs:
        p.start()
    res = [ret.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, status in res:
        assert status == "ok", f"rank {rank}: {status}"


def test_dsp_switch_cost_model():
    """dsp.choose_spatial_switch: what travels through the exchange of a spatial block.  At every BASELINE geometry the padded
    qkv GEMM costs less than tripling the message, so the reference's order stays; a frame count that pads badly on a slow GEMM
    flips it."""
    from videosys_amd import dsp

    for B, T, S, P in ((2, 19, 1024, 8), (2, 19, 1024, 4), (2, 38, 3600, 8)):
        m = dsp.choose_spatial_switch(B, T, S, 1152, P)
        assert m["order"] == "activations" and m["padded_frames_per_rank"] == B * -(-T // P)
        f = dsp.choose_spatial_switch(B, T, S, 1152, P, scatter="flat")
        assert f["order"] == "activations" and f["padded_frames_per_rank"] == -(-B * T // P) <= m["padded_frames_per_rank"]
    # config 2 at the BASELINE degree: 5 frames on the busiest rank instead of 6 (4.75 ideal)
    assert (dsp.frames_per_rank(2, 19, 8, "sample"), dsp.frames_per_rank(2, 19, 8, "flat")) == (6, 5)
    assert (dsp.frames_per_rank(2, 38, 8, "sample"), dsp.frames_per_rank(2, 38, 8, "flat")) == (10, 10)
    m = dsp.choose_spatial_switch(2, 9, 1024, 1152, 8, gemm_tflops=50.0, a2a_gbytes_s=900.0)
    assert m["order"] == "qkv" and m["gemm_extra_us"] > m["comm_extra_us"]


@pytest.mark.parametrize("B,T,S,P", [(2, 19, 16, 8), (2, 38, 24, 8), (2, 5, 12, 4), (2, 1, 8, 4), (1, 7, 9, 2)])
def test_dsp_flat_scatter_and_chunked_switch_in_process(B, T, S, P):
    """The two layouts of the T-shard phase and the chunked (overlap) form of the switch, all P ranks as threads of this process
    (tools/local_group.py implements the group protocol of dsp.py):
      * "sample" (reference layout) equals the oracle's all_to_all_with_pad restatement;
      * "flat" — the [B,T,Sl,C] shard viewed as [1,B*T,Sl,C] — hands rank r the frames r*Fp .. of the flattened (sample, frame)
        axis, Fp = ceil(B*T/P) <= B*ceil(T/P), each frame whole and un-mixed;
      * moving a rank's frame block in two chunks (the overlap path) fills exactly the same T-shard tensor, and the chunked way
        back restores the S-shard bit for bit."""
    from tools.local_group import LocalWorld
    from videosys_amd import dsp

    C = 8
    g = torch.Generator().manual_seed(B * 100 + T)
    x = torch.randn(B, T, S, C, generator=g).to(torch.bfloat16)
    shards = O.dsp_split_sequence(x.float(), P, dim=2)
    Sl = shards[0].shape[2]
    t_ref = O.dsp_all_to_all(shards, 1, 2, O.dsp_pad(T, P), O.dsp_pad(S, P))
    xf = x.reshape(1, B * T, S, C)
    Fp = -(-B * T // P)

    def rank_fn(r, group):
        sp = dsp.SequenceParallel(group, copy_executor=torch_copy_executor)
        assert (sp.P, sp.rank) == (P, r)
        local = sp.split(x)
        assert torch.equal(local.float(), shards[r])
        # reference layout
        tsh = sp.to_temporal_shard(local, S)
        assert torch.equal(tsh.float(), t_ref[r]), "sample scatter vs oracle"
        assert torch.equal(sp.to_spatial_shard(tsh, T, Sl), local)
        # flat layout: whole frames of the flattened axis, zero frames past the end
        lf = local.reshape(1, B * T, Sl, C)
        tf = sp.to_temporal_shard(lf, S)
        assert tf.shape == (1, Fp, S, C)
        for j in range(Fp):
            f = r * Fp + j
            want = xf[0, f] if f < B * T else torch.zeros(S, C, dtype=x.dtype)
            assert torch.equal(tf[0, j], want), f"flat scatter: rank {r} frame {j}"
        assert torch.equal(sp.to_spatial_shard(tf, B * T, Sl).reshape(B, T, Sl, C), local)
        # chunked switch (two chunks of the rank's block, private staging buffers)
        if Fp >= 2:
            h = -(-Fp // 2)
            parts = [sp.to_temporal_shard(lf, S, tag=f"_{i}", chunk=ck) for i, ck in enumerate(((0, h), (h, Fp)))]
            assert torch.equal(torch.cat(parts, 1), tf), "chunked to_temporal_shard"
            back = torch.full((1, B * T, Sl, C), 7.0, dtype=x.dtype)
            for i, ck in enumerate(((0, h), (h, Fp))):
                sp.to_spatial_shard(parts[i], B * T, Sl, out=back, tag=f"_{i}", chunk=ck, Tp=Fp)
            assert torch.equal(back, lf), "chunked to_spatial_shard"
        full = sp.gather(local, S)
        assert torch.equal(full, x)
        return "ok"

    assert LocalWorld(P, timeout=60).run(rank_fn) == ["ok"] * P


# ------------------------------------------------------------------------------------------------ Ulysses over gloo
def _ulysses_worker(rank, world, port, B, Lt, Lv, C, ret):
    try:
        from videosys_amd import dsp

        dsp.initialize(rank=rank, world_size=world, init_method=f"tcp://127.0.0.1:{port}", backend="gloo")
        pm = dsp.ParallelManager(1, 1, world)
        up = dsp.UlyssesParallel(pm.sp_group, copy_executor=torch_copy_executor)
        Lvl = up.shard_len(Lv)
        hw = C // world
        g = torch.Generator().manual_seed(321)
        full = torch.randn(B, Lt + Lv, 3 * C, generator=g).to(torch.bfloat16)      # q | k | v of the whole sequence
        attn = torch.randn(B, Lt + Lv, C, generator=g).to(torch.bfloat16)          # attention output, all heads

        def local_rows(t):  # [text | this rank's video shard, zero padded] as the model holds them at rest
            out = torch.zeros(B, Lt + Lvl, t.shape[-1], dtype=t.dtype)
            out[:, :Lt] = t[:, :Lt]
            nv = max(0, min(Lvl, Lv - rank * Lvl))
            out[:, Lt:Lt + nv] = t[:, Lt + rank * Lvl: Lt + rank * Lvl + nv]
            return out

        # what the reference computes: all_to_all_comm(scatter heads, gather sequence) + _remove_extra_encoder
        # (cogvideox_transformer_3d.py:45-62,112-123) == the rank's head slice of q, k, v over the whole un-padded sequence
        want = torch.cat([full[..., i * C + rank * hw: i * C + (rank + 1) * hw] for i in range(3)], -1)
        got = up.scatter_heads(local_rows(full).view(-1, 3 * C), B, Lt, Lv, C)
        assert torch.equal(got.view(B, Lt + Lv, 3 * hw), want), "scatter_heads"
        # way back: _add_extra_encoder + all_to_all_comm(scatter sequence, gather heads) (:64-86,160-165)
        back = up.gather_heads(attn[..., rank * hw:(rank + 1) * hw].contiguous().view(-1, hw), B, Lt, Lv, C)
        assert torch.equal(back.view(B, Lt + Lvl, C), local_rows(attn)), "gather_heads"
        ret.put((rank, "ok"))
    except Exception:  # noqa
        import traceback

        ret.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("Lt,Lv", [(3, 10), (5, 7)])
def test_ulysses_two_ranks_gloo(Lt, Lv):
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ulysses_worker, args=(r, 2, port, 2, Lt, Lv, 32, ret)) for r in range(2)]
    for p in procs:
        p.start()
    res = [ret.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, status in res:
        assert status == "ok", f"rank {rank}: {status}"


def _ref_rflow_module(name):
    """The reference's scheduling_rflow_open_sora.py, live (only while minting a trace)."""
    import importlib.util

    from oracle import ref_loader

    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_loader.REFERENCE_ROOT, "videosys/schedulers/scheduling_rflow_open_sora.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def test_timestep_transform_bitwise_equals_reference_function(ref_trace):
    """videosys_amd.rflow.timestep_transform against the reference function itself (scheduling_rflow_open_sora.py:47-70; its
    results replayed from tests/golden/ref_traces/) on 5250 (geometry, step) pairs: the fp32 results must be bit-identical."""
    import itertools

    from videosys_amd.rflow import timestep_transform

    cases = [dict(height=torch.tensor([H]), width=torch.tensor([W]), num_frames=torch.tensor([F]))
             for H, W, F in itertools.product([256., 360., 480., 512., 720.], [256., 480., 512., 640., 1280.], [1., 17., 34., 51., 64., 102., 128.])]
    steps = [torch.tensor([(1 - k / 30) * 1000.0]) for k in range(30)]

    def live():
        ref = _ref_rflow_module("ref_rflow")
        return torch.stack([ref.timestep_transform(t, kw, num_timesteps=1000) for kw in cases for t in steps])

    want = ref_trace.value(live)
    got = torch.stack([timestep_transform(t, kw, num_timesteps=1000) for kw in cases for t in steps])
    assert want.shape == got.shape and want.dtype == got.dtype and torch.equal(got, want)


def test_timestep_transform_bf16_geometry_equals_reference_function(ref_trace):
    """The reference hands height / width / num_frames to timestep_transform as tensors of the MODEL dtype
    (data_process.py:798-805: bf16, so 854 arrives as 856 and the ratio is computed in bf16 before the fp32 timestep promotes
    it).  The pipeline builds them the same way (open_sora_geometry.prepare_multi_resolution_info): bitwise equal schedules
    (the reference function's results replayed from tests/golden/ref_traces/)."""
    import itertools

    from videosys_amd import open_sora_geometry as G
    from videosys_amd.rflow import RFLOW, timestep_transform

    steps = [torch.tensor([(1 - k / 30) * 1000.0]) for k in range(30)]
    for (H, W), F in itertools.product([(480, 854), (720, 1280), (512, 512), (240, 426), (1080, 1920)], [1, 51, 64, 102, 408]):
        kw = G.prepare_multi_resolution_info(1, (H, W), F, 24, dtype=torch.bfloat16)
        assert kw["width"].dtype == torch.bfloat16 and float(kw["width"][0]) == float(torch.tensor(float(W)).to(torch.bfloat16))
        want = ref_trace.value(lambda: torch.stack([_ref_rflow_module("ref_rflow_bf16").timestep_transform(t, kw, num_timesteps=1000) for t in steps]))
        for t, w in zip(steps, want.unbind(0)):
            assert torch.equal(timestep_transform(t, kw, num_timesteps=1000), w)
        # and through the sampler's own schedule builder
        ts = RFLOW(num_sampling_steps=30, use_timestep_transform=True).prepare_timesteps(1, kw)
        assert len(ts) == len(want) and all(torch.equal(a, b) for a, b in zip(ts, want.unbind(0)))


def test_open_sora_geometry_vocabulary_matches_reference_tables(ref_trace):
    """Every (resolution, aspect_ratio) pair of generate()'s vocabulary returns exactly the reference's size — or fails the same
    assert — and the duration names map to the same frame counts (golden minted from data_process.py by
    oracle/make_golden_geometry.py; the tables re-derived from the reference file replayed from tests/golden/ref_traces/)."""
    from videosys_amd import open_sora_geometry as G

    with open(os.path.join(GOLDEN, "opensora_image_sizes.json")) as f:
        gold = json.load(f)
    assert len(gold["image_sizes"]) == 13 * 17

    def live_tables():
        from oracle.make_golden_geometry import reference_tables

        lit, res_tab = reference_tables()
        live = {f"{res}|{ar}": (list(lit[tab][key]) if key in lit[tab] else None)
                for res, tab in res_tab.items() for ar, key in lit["ASPECT_RATIO_MAP"].items()}
        return dict(image_sizes=live, ratio_keys=dict(lit["ASPECT_RATIO_MAP"]), num_frames=dict(lit["NUM_FRAMES_MAP"]))

    live = ref_trace.value(live_tables)
    assert live["image_sizes"] == gold["image_sizes"], "golden out of date with the reference file"
    tables = [gold, live]
    for tab in tables:
        for pair, want in tab["image_sizes"].items():
            res, ar = pair.split("|")
            if want is None:
                with pytest.raises(AssertionError):
                    G.get_image_size(res, ar)
            else:
                assert list(G.get_image_size(res, ar)) == want, pair
        for ar, key in tab["ratio_keys"].items():
            assert G.ratio_key(ar) == key
        for name, n in tab["num_frames"].items():
            assert G.get_num_frames(name) == n
    assert G.get_num_frames(64) == 64 and G.get_num_frames("17") == 17
    with pytest.raises(AssertionError):
        G.get_image_size("512", "1:1")   # BASELINE's 512x512 cannot be named through the reference's own tables
    with pytest.raises(KeyError):
        G.get_image_size("480p", "7:5")


def test_open_sora_prompt_preparation():
    """prepare_prompt = extract_json_from_prompts + split_prompt / extract_prompts_loop + append_score_to_prompts +
    text_preprocessing of the reference (pipeline_open_sora.py:548-615,705-792) for the text-to-video case."""
    from videosys_amd.pipeline_open_sora import OpenSoraPipeline as P

    assert P.prepare_prompt("  A Sunset over the SEA ") == "a sunset over the sea aesthetic score: 6.5."   # tag appended, THEN cleaned
    assert P.prepare_prompt("A cat") == "a cat aesthetic score: 6.5."
    assert P.prepare_prompt("A cat", aes=None) == "a cat"
    assert P.prepare_prompt("A cat", aes=7, flow=3.25, camera_motion="pan right") == \
        "a cat aesthetic score: 7.0. motion score: 3.2. camera motion: pan right."
    assert P.prepare_prompt("a dog aesthetic score: 5.0.") == "a dog aesthetic score: 5.0."
    assert P.prepare_prompt("|0| a beautiful day |2| a rainy day", aes=None, loop_i=0) == "a beautiful day"
    assert P.prepare_prompt("|0| a beautiful day |2| a rainy day", aes=None, loop_i=2) == "a rainy day"
    assert P.prepare_prompt('A cat{"reference_path": "", "mask_strategy": ""}', aes=None) == "a cat"
    assert P.prepare_prompt('A cat{"reference_path": "x.png", "mask_strategy": "0"}', aes=None) == "a cat"   # the tail is generate()'s
    with pytest.raises(AssertionError):
        P.prepare_prompt('A cat{"foo": 1}')


def test_caption_cleaner_matches_the_reference():
    """caption.py against outputs minted from the reference's own _clean_caption / text_preprocessing
    (oracle/make_golden_caption.py; pipeline_open_sora.py:298-424): one application, the double application the pipeline uses,
    and the plain lower-case + strip form."""
    import json

    from conftest import GOLDEN
    from videosys_amd import caption as C

    with open(os.path.join(GOLDEN, "clean_caption_cases.json")) as fh:
        cases = json.load(fh)
    assert len(cases) >= 20
    for c in cases:
        assert C.clean_caption(c["in"]) == c["once"], c["in"]
        assert C.text_preprocessing(c["in"]) == c["twice"], c["in"]
        assert C.text_preprocessing(c["in"], False) == c["plain"], c["in"]
        # LattePipeline._text_preprocessing (the diffusers IFPipeline copy: no strip inside the ftfy / unescape step)
        assert C.text_preprocessing(c["in"], True, mid_strip=False) == c["latte_twice"], c["in"]
        assert C.text_preprocessing(c["in"], False, mid_strip=False) == c["latte_plain"], c["in"]
    # html step (bs4 absent here: the standard library's html.parser, which is bs4's backend for features="html.parser")
    assert C.clean_caption("a <b>bold</b> claim &lt;3") == "a bold claim <3"
    assert C.BAD_PUNCT.sub(" ", "a#b\\c/d*e") == "a b c d e"


def test_videosys_alias_package_exports_reference_names():
    """``from videosys import ...`` (the import line of every reference example) resolves to this build; run in a subprocess because
    oracle/ref_loader.py parks the REFERENCE tree under the same module name for the oracle tests."""
    import subprocess
    import sys

    code = ("import videosys, videosys_amd\n"
            "from videosys import (initialize, VideoSysEngine, OpenSoraConfig, OpenSoraPABConfig, OpenSoraPipeline, LatteConfig,\n"
            "                      LattePABConfig, LattePipeline, CogVideoXConfig, CogVideoXPABConfig, CogVideoXPipeline)\n"
            "assert VideoSysEngine is videosys_amd.VideoSysEngine and OpenSoraConfig().pipeline_cls is OpenSoraPipeline\n"
            "try:\n    from videosys import VchitectConfig\n    raise SystemExit(3)\nexcept ImportError as e:\n    assert 'outside' in str(e)\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-800:]


def _reference_videosys_imports():
    """Every ``from videosys... import`` of the reference's examples / eval scripts / tests as [file, module, [names]], live only
    while minting a trace."""
    import ast
    import glob

    from oracle import ref_loader

    ref, out = ref_loader.REFERENCE_ROOT, []
    for pat in ("examples/**/*.py", "eval/**/*.py", "tests/**/*.py"):
        for f in sorted(glob.glob(os.path.join(ref, pat), recursive=True)):
            with open(f) as fh:
                tree = ast.parse(fh.read())
            for n in ast.walk(tree):
                if isinstance(n, ast.ImportFrom) and n.module and n.module.split(".")[0] == "videosys":
                    out.append([os.path.relpath(f, ref), n.module, [a.name for a in n.names]])
    return out


def test_reference_module_paths_resolve_to_this_build(ref_trace):
    """The submodule imports of the reference's inference examples, eval scripts and tests (``from videosys.core.pab.pab_mgr import
    ...``) resolve through the alias table of videosys/__init__.py; every ``from videosys... import`` of its examples / eval / tests
    (the list replayed from tests/golden/ref_traces/) is checked, except the families and the training stack outside the hot path.
    Subprocess: see the test above."""
    import subprocess
    import sys

    imports = ref_trace.value(_reference_videosys_imports)
    code = r"""
import importlib, json, os
import videosys, videosys_amd
from videosys.core.pab.pab_mgr import PABConfig, set_pab_manager, update_steps, enable_pab, if_broadcast_spatial, get_mlp_output
from videosys.utils.utils import save_video, set_seed, batch_func, str_to_dtype, all_exists
from videosys.utils.test import empty_cache
from videosys.utils.logging import init_logger
from videosys.core.distributed.parallel_mgr import ParallelManager, initialize
from videosys.core.distributed.comm import all_to_all_with_pad, gather_sequence, get_pad, set_pad, split_sequence, all_to_all_comm
from videosys.core.pipeline.pipeline import VideoSysPipeline, VideoSysPipelineOutput
from videosys.core.engine.engine import VideoSysEngine
from videosys.schedulers.scheduling_rflow_open_sora import RFLOW, timestep_transform
from videosys.schedulers.scheduling_ddim_cogvideox import CogVideoXDDIMScheduler
from videosys.models.modules.normalization import LlamaRMSNorm
from videosys.models.transformers.open_sora_transformer_3d import STDiT3_XL_2, STDiT3, STDiT3Config
from videosys.models.transformers.latte_transformer_3d import LatteT2V
from videosys.models.transformers.cogvideox_transformer_3d import CogVideoXTransformer3DModel
from videosys.models.autoencoders.autoencoder_kl_open_sora import OpenSoraVAE_V1_2
from videosys.models.autoencoders.autoencoder_kl_cogvideox import AutoencoderKLCogVideoX
from videosys.pipelines.open_sora import OpenSoraConfig, OpenSoraPABConfig, OpenSoraPipeline
from videosys.pipelines.open_sora.data_process import get_image_size, get_num_frames, read_from_path, prepare_multi_resolution_info
from videosys.pipelines.latte import LatteConfig, LattePABConfig, LattePipeline
from videosys.pipelines.cogvideox.pipeline_cogvideox import CogVideoXPipeline
import videosys.core.pab.pab_mgr as alias
assert alias is videosys_amd.pab and VideoSysEngine is videosys_amd.VideoSysEngine and issubclass(OpenSoraPipeline, VideoSysPipeline)
set_pab_manager(PABConfig(cross_broadcast=True, cross_threshold=[100, 900], cross_range=2))
assert videosys_amd.pab.PAB_MANAGER is not None and alias.PAB_MANAGER is videosys_amd.pab.PAB_MANAGER
set_pab_manager(None)
o = VideoSysPipelineOutput(video=7)
assert o["video"] == 7 and o[0] == 7 and o.to_tuple() == (7,)
skip = ("videosys.training", "videosys.core.dcp", "videosys.utils.training", "videosys.models.open_sora")
skip_names = {"OpenSoraPlanConfig", "OpenSoraPlanV110PABConfig", "OpenSoraPlanV120PABConfig", "VchitectConfig", "VchitectPABConfig",
              "DynamicParallelManager", "set_distributed_state", "merge_args"}
bad, seen = [], 0
for f, module, names in json.loads(os.environ["VSYS_REF_IMPORTS"]):
    if not module.startswith(skip):
        m = importlib.import_module(module)
        for name in names:
            seen += 1
            if name not in skip_names and not hasattr(m, name):
                bad.append((f, module, name))
assert seen > 50 and not bad, bad
print("ok")
"""
    env = dict(os.environ, VSYS_REF_IMPORTS=json.dumps(imports))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-1500:]


_EXAMPLE_ENGINE = r"""
import inspect, json, os, sys, types
import videosys

calls = []

class Engine:
    def __init__(self, config):
        assert hasattr(config, "pipeline_cls") and isinstance(config.num_gpus, int)
        self.config = config
    def generate(self, *a, **k):
        sig = inspect.signature(self.config.pipeline_cls.generate)
        bound = sig.bind(None, *a, **k)           # TypeError if the reference's call does not fit
        calls.append((self.config.pipeline_cls.__name__, sorted(bound.arguments)))
        return types.SimpleNamespace(video=["frames"])
    def save_video(self, video, path):
        assert video == "frames" and path.endswith(".mp4")
"""


def _reference_example_calls():
    """Runs the reference's examples/inference/{open_sora,latte,cogvideox}/sample.py and tests/pipelines/<family>/test_<family>.py
    unchanged against this build with a recording engine (live only while minting a trace) and returns what they did as data:
    per engine, the config it was given (class name + arguments) and its generate / save_video calls in order."""
    import subprocess
    import sys

    from oracle import ref_loader

    code = _EXAMPLE_ENGINE + r"""
import runpy

keep, made, engines = [], {}, []

def enc(v):
    if id(v) in made:
        return {"__config__": made[id(v)]}
    json.dumps(v)                             # plain data only
    return v

def recording(name, cls):
    def make(*a, **k):
        obj = cls(*a, **k)
        keep.append(obj)
        made[id(obj)] = [name, [enc(x) for x in a], {kk: enc(x) for kk, x in k.items()}]
        return obj
    return make

for n in dir(videosys):
    if n.endswith("Config"):
        setattr(videosys, n, recording(n, getattr(videosys, n)))

class RecordingEngine(Engine):
    def __init__(self, config):
        super().__init__(config)
        self.rec = {"config": made[id(config)], "calls": []}
        engines.append(self.rec)
    def generate(self, *a, **k):
        self.rec["calls"].append(["generate", [enc(x) for x in a], {kk: enc(x) for kk, x in k.items()}])
        return super().generate(*a, **k)
    def save_video(self, video, path):
        self.rec["calls"].append(["save_video", path])
        return super().save_video(video, path)

videosys.VideoSysEngine = RecordingEngine
import torch
torch.cuda.empty_cache = lambda: None
ran = 0
ref = sys.argv[1]
for fam in ("open_sora", "latte", "cogvideox"):
    for path in (f"{ref}/examples/inference/{fam}/sample.py", f"{ref}/tests/pipelines/{fam}/test_{fam}.py"):
        ns = runpy.run_path(path, run_name="not_main")
        for name, fn in ns.items():
            if callable(fn) and getattr(fn, "__module__", None) is None or name.startswith(("run_", "test_")):
                if not name.startswith(("run_", "test_")):
                    continue
                import itertools
                marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]   # the tests' own parameter grids
                names = [m.args[0] for m in marks]
                for combo in itertools.product(*[m.args[1] for m in marks]):
                    fn(**dict(zip(names, combo)))
                    ran += 1
print(json.dumps({"ran": ran, "engines": engines}))
"""
    r = subprocess.run([sys.executable, "-c", code, ref_loader.REFERENCE_ROOT], cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_reference_example_scripts_run_against_this_build(ref_trace):
    """The reference's own examples/inference/{open_sora,latte,cogvideox}/sample.py and its pipeline tests, as they drive the
    engine (every config they build, every ``engine.generate(...)`` / ``save_video`` call, replayed from tests/golden/ref_traces/;
    _reference_example_calls mints it by running the scripts unchanged against this build): every config is accepted and every
    generate call binds to the pipeline's ``generate`` signature.  The engine is replaced by a recorder (no GPU here); the same call
    shapes run on the device in tests/test_gpu_pipeline.py.  Subprocess: see the alias test above."""
    import subprocess
    import sys

    recorded = ref_trace.value(_reference_example_calls)
    code = _EXAMPLE_ENGINE + r"""
data = json.loads(os.environ["VSYS_REF_EXAMPLES"])

def dec(v):
    return build(v["__config__"]) if isinstance(v, dict) and "__config__" in v else v

def build(rec):
    name, a, k = rec
    return getattr(videosys, name)(*[dec(x) for x in a], **{kk: dec(x) for kk, x in k.items()})

import torch
torch.cuda.empty_cache = lambda: None
for e in data["engines"]:
    engine = Engine(build(e["config"]))
    for c in e["calls"]:
        if c[0] == "generate":
            engine.generate(*[dec(x) for x in c[1]], **{k: dec(x) for k, x in c[2].items()})
        else:
            engine.save_video("frames", c[1])
ran = data["ran"]
assert ran >= 18 and len(calls) >= ran, (ran, len(calls))
assert {c[0] for c in calls} == {"OpenSoraPipeline", "LattePipeline", "CogVideoXPipeline"}
print("ok", ran, len(calls))
"""
    env = dict(os.environ, VSYS_REF_EXAMPLES=json.dumps(recorded))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-400:], r.stderr[-1500:])


def test_torch_custom_ops_are_registered():
    """``torch.ops.vsys.*`` (north_star: "through PyTorch-ROCm custom ops"; csrc/torch_binding.cpp, a C++ TORCH_LIBRARY fragment built
    by build()): the fragment loads, both ops carry their schemas, a CPU tensor / a wrong arity / an unknown op code raise from C++
    (no fallback, no launch), the product's ``ops._call`` routes through it and maps the error to VsysError, and the generated
    dispatch table is fresh against include/videosys_amd.h."""
    from videosys_amd import _lib, ops
    from videosys_amd._lib import VsysError

    tv = _lib.torch_ops()
    assert tv is not None, "libvideosys_torch.so was not built / loaded (python -c 'import __graft_entry__ as g; g.build()')"
    assert str(tv.launch.default._schema) == "vsys::launch(int op, Tensor?[] tensors, int[] ints, float[] floats, int stream) -> ()"
    assert str(tv.program_run.default._schema) == "vsys::program_run(Tensor cmds, int n, int[] streams) -> ()"
    x = torch.zeros(2, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="HIP device tensors"):
        tv.launch(9, [x, x, None], [0, 0, 16], [], 0)               # vsys_add_rows on CPU tensors
    with pytest.raises(RuntimeError, match="takes 3 integer and 0 float"):
        tv.launch(9, [None], [0], [], 0)
    with pytest.raises(RuntimeError, match="unknown op code"):
        tv.launch(9999, [], [], [], 0)
    with pytest.raises(RuntimeError, match="do not fit"):
        tv.program_run(torch.zeros(8, dtype=torch.uint8), 1, [0])
    with pytest.raises(VsysError):
        ops.add_rows(x, x)                                           # the wrapper's own device check, same error type
    import subprocess
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "videosys_amd", "csrc", "gen", "program_gen.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, "csrc/program_ops.inc / the VSYS_OP block / _opcodes.py are stale: run csrc/gen/program_gen.py\n" + r.stdout


def test_launch_program_op_table_matches_header_and_signatures():
    """Launch programs (include/videosys_amd.h, videosys_amd/program.py): every recordable entry point has a VSYS_OP code equal to
    the header's #define, and the C replay loop expects exactly the integer / float argument counts of the ctypes signature
    (the recorder splits a launch's arguments by those types)."""
    import ctypes

    from videosys_amd import _lib, program

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VSYS_OP_([A-Z0-9_]+)\s+(\d+)", hdr)}
    count = defines.pop("COUNT")
    assert len(defines) == count - 1 == len(program.OPCODES)
    for name, op in program.OPCODES.items():
        assert defines[name[len("vsys_"):].upper()] == op, name
        argtypes = _lib.SIGNATURES[name][:-1]      # the trailing stream is not an argument of a command
        ni, nf = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.vsys_program_op_info(op, ctypes.byref(ni), ctypes.byref(nf)) == 0
        want_f = sum(1 for t in argtypes if t is ctypes.c_float)
        assert (ni.value, nf.value) == (len(argtypes) - want_f, want_f), name
        assert ni.value <= program.N_INT and nf.value <= program.N_FLOAT
    assert lib.vsys_program_op_info(0, ctypes.byref(ni), ctypes.byref(nf)) != 0
    assert lib.vsys_program_op_info(count, ctypes.byref(ni), ctypes.byref(nf)) != 0
    assert ctypes.sizeof(program.VsysCmd) == 4 + 4 + 8 * program.N_INT + 4 * program.N_FLOAT
    # an empty program is a no-op; a command with an unknown op or stream slot is rejected before anything is enqueued
    failed = ctypes.c_int64(-1)
    assert lib.vsys_program_run(None, 0, None, 0, ctypes.byref(failed)) == 0
    cmds = (program.VsysCmd * 1)()
    cmds[0].op, cmds[0].stream = 99, 0
    streams = (ctypes.c_void_p * 1)(None)
    assert lib.vsys_program_run(cmds, 1, streams, 1, ctypes.byref(failed)) != 0 and failed.value == 0
    cmds[0].op, cmds[0].stream = 9, 3
    assert lib.vsys_program_run(cmds, 1, streams, 1, ctypes.byref(failed)) != 0


# ---- the LAB flavour of the library (-DVSYS_LAB: ablation / stamp variants, gemm3 / gemm4) must keep compiling (it
# silently broke once), and its host-only stream-K planner (GEMM lab variant 80, include/videosys_amd_lab.h) is checked here
@pytest.fixture(scope="module")
def lab_lib(tmp_path_factory):
    import ctypes
    import shutil

    import __graft_entry__ as G

    if shutil.which(G._hipcc()) is None and not os.path.exists(G._hipcc()):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("lab") / "libvideosys_amd_lab.so")
    G.compile_library(out, lab=True)     # objects are cached under videosys_amd/csrc/build/lab
    lib = ctypes.CDLL(out)
    for name in ("vsys_lab_flash_debug_buffer", "vsys_gemm_streamk_plan", "vsys_gemm_bf16", "vsys_tune_gemm_variant"):
        assert hasattr(lib, name), name
    return lib


def test_lab_build_compiles_and_accepts_lab_ids(lab_lib):
    for v in (60, 70, 80, 31, 40, 61, 78, 84):
        assert lab_lib.vsys_tune_gemm_variant(v) == 0, v
    assert lab_lib.vsys_tune_gemm_variant(0) == 0
    for v in (1, 2):
        assert lab_lib.vsys_tune_flash_variant(v) == 0, v
    assert lab_lib.vsys_tune_flash_variant(5) != 0       # the ping-pong flash kernel is gone from every flavour
    assert lab_lib.vsys_tune_flash_variant(0) == 0


def test_shipped_build_rejects_lab_ids():
    from videosys_amd import _lib

    lib = _lib.load()
    if hasattr(lib, "vsys_lab_flash_debug_buffer"):
        pytest.skip("the in-tree library is a lab build")
    for v in (60, 70, 80, 31, 40, 61):
        assert lib.vsys_tune_gemm_variant(v) != 0, f"lab GEMM id {v} accepted by the shipped library"
    for v in (1, 2, 5, 6):
        assert lib.vsys_tune_flash_variant(v) != 0, f"lab flash id {v} accepted by the shipped library"
    assert not hasattr(lib, "vsys_gemm_streamk_plan")


_LAB = {}


def _streamk_plan(ntiles, nt, grid):
    import ctypes

    import numpy as np

    lib = _LAB["lib"]
    lib.vsys_gemm_streamk_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    cap = grid * 8
    segs = np.zeros((cap, 4), dtype=np.int32)
    nseg = ctypes.c_int(0)
    n = lib.vsys_gemm_streamk_plan(ntiles, nt, grid, segs.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(nseg))
    assert n >= 0, n
    return (segs[:n].reshape(grid, nseg.value, 4) if n else None), nseg.value


@pytest.mark.parametrize("ntiles,nt,grid", [
    (912, 18, 256),    # config 2: proj / cross-attention GEMMs (38 912 rows x 1152 columns, K = 1152): 3.56 rounds
    (912, 72, 256),    # fc2 (K = 4608)
    (2736, 18, 256),   # qkv: 10.69 rounds
    (3648, 18, 256),   # fc1: 14.25 rounds
    (300, 8, 256), (511, 4, 256), (257, 18, 256), (700, 33, 128),
])
def test_streamk_plan_covers_partial_round_exactly_once(lab_lib, ntiles, nt, grid):
    _LAB["lib"] = lab_lib
    segs, nseg_max = _streamk_plan(ntiles, nt, grid)
    rem = ntiles % grid
    first = ntiles - rem
    if segs is None:
        # only legal when a cut would leave a piece shorter than two K-tiles (tiny rounds): every shape of the denoise path splits
        assert (ntiles, nt) not in [(912, 18), (912, 72), (2736, 18), (3648, 18)]
        return
    cover = {t: [0] * nt for t in range(first, ntiles)}
    dump_of = {}
    for b in range(grid):
        rows = segs[b]
        live = [r for r in rows if r[0] >= 0]
        assert len(live) < nseg_max and rows[len(live)][0] == -1                      # terminated list
        assert all(r[0] < 0 for r in rows[len(live):])
        kinds = [int(r[2]) & 0xff for r in live]
        assert kinds == sorted(kinds, key=lambda k: {1: 0, 0: 1, 2: 2}[k])            # DUMP first, FINAL last
        assert kinds.count(1) <= 1 and kinds.count(2) <= 1                            # one workspace slot per workgroup
        for r in live:
            lin, kb, ke, kind, nsrc = int(r[0]), int(r[1]) & 0xffff, int(r[1]) >> 16, int(r[2]) & 0xff, int(r[2]) >> 8
            assert first <= lin < ntiles and lin % 8 == b % 8                         # the tile stays on the workgroup's XCD
            assert 0 <= kb < ke <= nt and ke - kb >= 2                                # the K loop needs two K-tiles
            for k in range(kb, ke):
                cover[lin][k] += 1
            if kind == 0:
                assert kb == 0 and ke == nt and nsrc == 0
            elif kind == 1:
                assert ke < nt and nsrc == 0
                dump_of[b] = (lin, kb, ke)
            else:
                assert kind == 2 and kb > 0 and ke == nt and nsrc >= 1 and b - 8 * nsrc >= 0
    assert all(c == 1 for t in cover.values() for c in t)                            # every K-tile of every tile exactly once
    # a FINAL reads the slots of b - 8, ..., b - 8 nsrc: exactly the other ranges of its tile, contiguous in K, lower-numbered
    for b in range(grid):
        for r in segs[b]:
            if r[0] >= 0 and (int(r[2]) & 0xff) == 2:
                lin, kb, nsrc = int(r[0]), int(r[1]) & 0xffff, int(r[2]) >> 8
                pieces = sorted(dump_of[b - 8 * k] for k in range(1, nsrc + 1))
                assert all(p[0] == lin for p in pieces)
                assert pieces[0][1] == 0 and pieces[-1][2] == kb
                assert all(pieces[i][2] == pieces[i + 1][1] for i in range(len(pieces) - 1))
    # balance: the longest workgroup list is within two K-tiles of the ideal share
    work = [sum((int(r[1]) >> 16) - (int(r[1]) & 0xffff) for r in segs[b] if r[0] >= 0) for b in range(grid)]
    assert max(work) <= -(-rem * nt // grid) + 2


def test_streamk_plan_not_split_when_no_partial_round(lab_lib):
    _LAB["lib"] = lab_lib
    assert _streamk_plan(512, 18, 256)[0] is None      # whole rounds only
    assert _streamk_plan(200, 18, 256)[0] is None      # fewer tiles than workgroups
    assert _streamk_plan(912, 3, 256)[0] is None       # K loop too short to cut


# ---------------------------------------------------------------------------------------------------- Open-Sora conditioning
def test_mask_strategy_helpers_match_the_reference():
    """open_sora_condition.py against values minted from the reference's own functions (oracle/make_golden_xmask.py:
    pipeline_open_sora.py:795-854)."""
    from conftest import load_golden
    from videosys_amd import open_sora_condition as K

    fx = load_golden("stdit3_xmask_small.pt")
    for v, p, m, want in fx["nearest"]:
        assert K.find_nearest_point(v, p, m) == want, (v, p, m)
    for c in fx["mask_strategy"]:
        assert K.parse_mask_strategy(c["ms"]) == [list(g) for g in c["parsed"]], c["ms"]
        z = c["z_in"].clone()
        masks = K.apply_mask_strategy(z, c["refs"], [c["ms"]], c["loop_i"], align=c["align"])
        assert torch.equal(z, c["z_out"]), c["ms"]
        assert torch.equal(masks, c["masks"]), (c["ms"], masks, c["masks"])
    assert K.apply_mask_strategy(torch.zeros(1, 4, 5, 2, 2), [], [], 0) is None
    with pytest.raises(AssertionError):
        K.parse_mask_strategy("0,0,0,0,1,0,9")


def test_conditioning_prompt_and_loop_helpers(tmp_path):
    from videosys_amd import open_sora_condition as K

    texts, refs, ms = K.extract_json_from_prompts(['a cat {"reference_path": "a.png;b.png", "mask_strategy": "0;0,1,0,-1,1"}', "plain"],
                                                  ["", "x.png"], ["", ""])
    assert texts == ["a cat ", "plain"] and refs == ["a.png;b.png", "x.png"] and ms == ["0;0,1,0,-1,1", ""]
    with pytest.raises(AssertionError):
        K.extract_json_from_prompts(['p {"bogus": 1}'], [""], [""])
    with pytest.raises(AssertionError):
        K.extract_json_from_prompts(['p {"a": 1} {"b": 2}'], [""], [""])
    assert K.dframe_to_frame(5) == 17 and K.dframe_to_frame(10) == 34
    with pytest.raises(AssertionError):
        K.dframe_to_frame(4)
    # append_generated (:857-871): the continuation rule, for a sample without and one with earlier references / strategy
    enc = lambda v: torch.full((v.shape[0], 4, 5, 2, 2), 7.0)
    r0 = torch.zeros(4, 1, 2, 2)
    refs, ms = K.append_generated(enc, torch.zeros(2, 3, 17, 16, 16), [None, [r0]], ["", "0"], 1, 5, 0.25)
    assert len(refs[0]) == 1 and len(refs[1]) == 2 and refs[1][0] is r0 and float(refs[1][1].mean()) == 7.0
    assert ms == ["1,0,-5,0,5,0.25", "0;1,1,-5,0,5,0.25"]
    # the strategy it wrote pastes the last 5 latent frames of the new reference over the first 5 of the next z
    z = torch.zeros(2, 4, 15, 2, 2)
    masks = K.apply_mask_strategy(z, [[torch.arange(10.0).view(1, 10, 1, 1).expand(4, 10, 2, 2)], refs[1]], ms, 1, align=5)
    assert z[0, 0, :5, 0, 0].tolist() == [5.0, 6.0, 7.0, 8.0, 9.0] and float(z[0, :, 5:].abs().max()) == 0
    assert masks[0].tolist() == [0.25] * 5 + [1.0] * 10
    # references: latents pass through, pixels go through the encoder, an image file is resized to cover + centre-cropped
    from PIL import Image
    import numpy as np

    arr = np.zeros((40, 100, 3), dtype=np.uint8)
    arr[:, :50, 0] = 255
    path = str(tmp_path / "ref.png")
    Image.fromarray(arr).save(path)
    pix = K.read_from_path(path, (32, 32))
    assert pix.shape == (3, 1, 32, 32) and float(pix.min()) >= -1 and float(pix.max()) <= 1
    assert float(pix[0, 0, :, :12].mean()) > 0.9 and float(pix[0, 0, :, 20:].mean()) < -0.9   # 100x40 -> 80x32 -> crop 24..56
    seen = []

    def enc2(v):
        seen.append(tuple(v.shape))
        return torch.zeros(v.shape[0], 4, 1, 4, 4)

    lat = torch.ones(4, 3, 4, 4)
    out = K.collect_references_batch(["", path, [lat, torch.zeros(3, 17, 32, 32)]], enc2, (32, 32))
    assert out[0] == [] and out[1][0].shape == (4, 1, 4, 4) and out[2][0] is lat and out[2][1].shape == (4, 1, 4, 4)
    assert seen == [(1, 3, 1, 32, 32), (1, 3, 17, 32, 32)]
    with pytest.raises(NotImplementedError):
        K.read_from_path("clip.mp4", (32, 32))
    with pytest.raises(RuntimeError):
        K.collect_references_batch([path], None, (32, 32))


def test_every_entry_point_of_the_header_cites_what_it_replaces():
    """include/videosys_amd.h: the comment in front of every exported function names the reference file (``*.py:line``) it replaces,
    says that the piece is third-party in the reference, or states that there is no reference counterpart."""
    with open(os.path.join(ROOT, "include", "videosys_amd.h")) as fh:
        s = fh.read()
    missing = []
    for m in re.finditer(r"^(?:int|const char\*|void|int64_t)\s+(vsys_\w+)\(", s, flags=re.M):
        pre = s[:m.start()]
        j = pre.rfind("*/")
        i = pre.rfind("/*", 0, j)
        c = pre[i:j].lower()
        if not (".py" in c or "no reference counterpart" in c or "third-party" in c):
            missing.append(m.group(1))
    assert not missing, missing


def _ref_class_ast(rel, cls):
    """The ClassDef node of ``cls`` in the reference file ``rel`` (videosys/...), live only while minting a trace."""
    import ast

    from oracle import ref_loader

    with open(os.path.join(ref_loader.REFERENCE_ROOT, "videosys", rel)) as fh:
        return next(n for n in ast.parse(fh.read()).body if isinstance(n, ast.ClassDef) and n.name == cls)


def test_generate_accepts_every_keyword_of_the_reference(ref_trace):
    """Every keyword of the reference's ``generate`` (Open-Sora, Latte, CogVideoX pipelines) exists on this build's ``generate``
    (values the path cannot honour are refused with an error that says so, not with a TypeError about the keyword)."""
    import ast
    import inspect

    from videosys_amd.pipeline_cogvideox import CogVideoXPipeline
    from videosys_amd.pipeline_latte import LattePipeline
    from videosys_amd.pipeline_open_sora import OpenSoraPipeline

    def keywords(path, cls):   # the reference's generate() parameter names (replayed from tests/golden/ref_traces/)
        fn = next(it for it in _ref_class_ast(path, cls).body if isinstance(it, ast.FunctionDef) and it.name == "generate")
        return [a.arg for a in fn.args.args + fn.args.kwonlyargs if a.arg != "self"]

    for path, cls, ours in (("pipelines/open_sora/pipeline_open_sora.py", "OpenSoraPipeline", OpenSoraPipeline),
                            ("pipelines/latte/pipeline_latte.py", "LattePipeline", LattePipeline),
                            ("pipelines/cogvideox/pipeline_cogvideox.py", "CogVideoXPipeline", CogVideoXPipeline)):
        want = ref_trace.value(lambda: keywords(path, cls))
        assert len(want) > 3, (cls, want)
        have = set(inspect.signature(ours.generate).parameters)
        assert not [a for a in want if a not in have], (cls, [a for a in want if a not in have])


def test_pipelines_and_engine_have_every_method_of_the_reference_classes(ref_trace):
    """Every method / property name of the reference's pipeline classes and of its engine exists on this build's classes (a call
    site written against the reference finds what it calls)."""
    import ast

    from videosys_amd.engine import VideoSysEngine
    from videosys_amd.pipeline_cogvideox import CogVideoXPipeline
    from videosys_amd.pipeline_latte import LattePipeline
    from videosys_amd.pipeline_open_sora import OpenSoraPipeline

    internal = {"_create_pipeline"}   # runs inside the worker process here (engine._worker_main), not a method of the engine
    for path, cls, ours in (("pipelines/open_sora/pipeline_open_sora.py", "OpenSoraPipeline", OpenSoraPipeline),
                            ("pipelines/latte/pipeline_latte.py", "LattePipeline", LattePipeline),
                            ("pipelines/cogvideox/pipeline_cogvideox.py", "CogVideoXPipeline", CogVideoXPipeline),
                            ("core/engine/engine.py", "VideoSysEngine", VideoSysEngine)):
        names = ref_trace.value(lambda: [it.name for it in _ref_class_ast(path, cls).body if isinstance(it, ast.FunctionDef)])
        assert len(names) > 3, (cls, names)
        missing = [n for n in names if not hasattr(ours, n) and n not in internal]
        assert not missing, (cls, missing)


class _FakeText:
    """(embeddings [B, 1, L, 8], mask [B, L]) like t5.T5TextEncoder; deterministic in the prompt text; records what it was asked."""

    def __init__(self, L=12):
        self.max_length, self.calls = L, []

    def __call__(self, prompts):
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        self.calls.append(prompts)
        emb, mask = [], torch.zeros(len(prompts), self.max_length, dtype=torch.long)
        for b, q in enumerate(prompts):
            g = torch.Generator().manual_seed(sum(q.encode()) + 7)
            emb.append(torch.randn(1, self.max_length, 8, generator=g))
            mask[b, :min(len(q.split()) + 1, self.max_length)] = 1
        return torch.stack(emb, 0), mask


def test_latte_prompt_helpers_follow_the_reference():
    """encode_prompt / mask_text_embeddings / _text_preprocessing / check_inputs / prepare_latents of LattePipeline
    (pipeline_latte.py:278-284, 287-445, 465-531, 649-672) — host logic, no device needed."""
    from types import SimpleNamespace

    from videosys_amd.pipeline_latte import LattePipeline

    pipe = object.__new__(LattePipeline)
    pipe.text_encoder = te = _FakeText()
    pipe.scheduler = SimpleNamespace(init_noise_sigma=1.0)
    assert pipe._text_preprocessing("  A Cat  ") == ["a cat"] and pipe._text_preprocessing(["A", "B "], clean_caption=False) == ["a", "b"]
    assert pipe._text_preprocessing("see www.example.com <b>A Cat</b>", clean_caption=True) == ["see a cat"]
    # one prompt: cut to its token count, the negative with it; the negative is encoded once per prompt
    pe, ne = pipe.encode_prompt("a red cat", "", True)
    full, m = _FakeText()("a red cat")
    keep = int(m.sum())
    assert keep == 4 and pe.shape == (1, keep, 8) and ne.shape == (1, keep, 8) and torch.equal(pe, full[:, 0, :keep])
    assert te.calls == [["a red cat"], [""]]
    # a batch: zeroed past each prompt's tokens, full length kept; the negatives untouched
    te.calls.clear()
    pe, ne = pipe.encode_prompt(["a red cat", "dog"], "blurry", True)
    full, m = _FakeText()(["a red cat", "dog"])
    assert te.calls[1] == ["blurry", "blurry"] and pe.shape == (2, 12, 8) and ne.shape == (2, 12, 8)
    assert torch.equal(pe, full[:, 0] * m[:, :, None]) and bool((pe[1, 2:] == 0).all()) and bool((ne[1, 2:] != 0).any())
    # no guidance: no negative; mask_feature off: nothing cut
    pe, ne = pipe.encode_prompt("a red cat", "", False, mask_feature=False)
    assert ne is None and pe.shape == (1, 12, 8)
    e4, kept = pipe.mask_text_embeddings(full[:1], m[:1])
    assert e4.shape == (1, 1, 4, 8) and kept == 4
    with pytest.raises(ValueError):
        pipe.check_inputs("a", 513, 512, None, 1)
    with pytest.raises(ValueError):
        pipe.check_inputs("a", 512, 512, None, 0)
    with pytest.raises(ValueError):
        pipe.check_inputs(None, 512, 512, None, 1)
    with pytest.raises(ValueError):
        pipe.check_inputs("a", 512, 512, None, 1, prompt_embeds=torch.zeros(1, 2, 8))
    with pytest.raises(ValueError):
        pipe.check_inputs(None, 512, 512, None, 1, prompt_embeds=torch.zeros(1, 2, 8), negative_prompt_embeds=torch.zeros(1, 3, 8))
    pipe.check_inputs(None, 512, 512, None, 1, prompt_embeds=torch.zeros(1, 2, 8), negative_prompt_embeds=torch.zeros(1, 2, 8))
    g = torch.Generator().manual_seed(3)
    z = pipe.prepare_latents(2, 4, 16, 256, 256, torch.float32, "cpu", g)
    assert z.shape == (2, 4, 16, 32, 32) and torch.equal(z, torch.randn(2, 4, 16, 32, 32, generator=torch.Generator().manual_seed(3)))
    with pytest.raises(ValueError):
        pipe.prepare_latents(2, 4, 16, 256, 256, torch.float32, "cpu", [g])


def test_cogvideox_prompt_helpers_follow_the_reference():
    """encode_prompt / _get_t5_prompt_embeds / check_inputs / prepare_latents of CogVideoXPipeline
    (pipeline_cogvideox.py:211-332, 334-357, 385-434)."""
    from types import SimpleNamespace

    from videosys_amd.pipeline_cogvideox import CogVideoXPipeline

    pipe = object.__new__(CogVideoXPipeline)
    pipe.text_encoder = te = _FakeText(L=226)
    pipe.scheduler = SimpleNamespace(init_noise_sigma=1.0)
    pe, ne = pipe.encode_prompt(["a red cat", "dog"], None, True)
    assert te.calls == [["a red cat", "dog"], ["", ""]] and pe.shape == ne.shape == (2, 226, 8)
    pe, ne = pipe.encode_prompt("dog", None, False)
    assert ne is None and pe.shape == (1, 226, 8)
    assert pipe._get_t5_prompt_embeds("dog", num_videos_per_prompt=2).shape == (2, 226, 8)
    with pytest.raises(TypeError):
        pipe.encode_prompt(["a"], ("b",), True)
    with pytest.raises(ValueError):
        pipe.encode_prompt(["a", "b"], ["c"], True)
    with pytest.raises(ValueError):   # the attached encoder pads to 226
        pipe.encode_prompt("a", None, True, max_sequence_length=100)
    with pytest.raises(ValueError):
        pipe.check_inputs("a", 480, 721, None, ["latents"])
    with pytest.raises(ValueError):
        pipe.check_inputs("a", 480, 720, None, ["frames"])
    with pytest.raises(ValueError):
        pipe.check_inputs("a", 480, 720, "b", ["latents"], negative_prompt_embeds=torch.zeros(1, 2, 8))
    pipe.check_inputs("a", 480, 720, None, ["latents", "prompt_embeds"])
    z = pipe.prepare_latents(1, 16, 49, 480, 720, torch.float32, "cpu", torch.Generator().manual_seed(1))
    assert z.shape == (1, 13, 16, 60, 90)
    assert pipe.guidance_scale is None and pipe.num_timesteps == 0 and pipe.interrupt is False
    pipe.fuse_qkv_projections()
    assert pipe.fusing_transformer
    pipe.unfuse_qkv_projections()
    assert not pipe.fusing_transformer


def test_local_checkpoint_directories_are_read_like_from_pretrained(tmp_path, monkeypatch):
    """model_path = a local directory in the Hugging Face layout: ``transformer/config.json`` sets the geometry (a 5b checkpoint
    under any directory name), sharded ``*.safetensors`` are merged, ``scheduler/scheduler_config.json`` and ``vae/config.json``
    supply snr_shift_scale / scaling_factor (pipeline_cogvideox.py:146-160, pipeline_latte.py:208-217 from_pretrained calls).
    The device models are replaced by recorders: this is the host-side loading logic only."""
    import json
    from types import SimpleNamespace

    from safetensors.torch import save_file

    from videosys_amd import pipeline_cogvideox as PC, pipeline_latte as PL, utils as U

    root = tmp_path / "my_ckpt"
    for sub in ("transformer", "scheduler", "vae"):
        (root / sub).mkdir(parents=True)
    (root / "transformer" / "config.json").write_text(json.dumps(dict(_class_name="CogVideoXTransformer3DModel", num_attention_heads=48,
                                                                       num_layers=42, use_rotary_positional_embeddings=True)))
    save_file({"a.weight": torch.ones(2)}, str(root / "transformer" / "diffusion_pytorch_model-00001-of-00002.safetensors"))
    save_file({"b.weight": torch.zeros(3)}, str(root / "transformer" / "diffusion_pytorch_model-00002-of-00002.safetensors"))
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(_class_name="CogVideoXDDIMScheduler", snr_shift_scale=1.0,
                                                                              timestep_spacing="trailing")))
    (root / "vae" / "config.json").write_text(json.dumps(dict(scaling_factor=0.7)))
    save_file({"decoder.x": torch.ones(1)}, str(root / "vae" / "diffusion_pytorch_model.safetensors"))

    cfg, sd = U.read_component(str(root), "transformer")
    assert cfg["num_layers"] == 42 and sorted(sd) == ["a.weight", "b.weight"]
    assert U.read_component(str(root), "missing") == ({}, None) and U.read_component("THUDM/CogVideoX-2b", "transformer") == ({}, None)

    seen = {}

    class FakeModel:
        def __init__(self, num_attention_heads=30, attention_head_dim=64, num_layers=30, use_rotary_positional_embeddings=False,
                     patch_size=2, in_channels=16, out_channels=16, text_embed_dim=4096, time_embed_dim=512, device=None, **kw):
            self.config = SimpleNamespace(num_attention_heads=num_attention_heads, num_layers=num_layers, patch_size=patch_size,
                                          use_rotary_positional_embeddings=use_rotary_positional_embeddings,
                                          attention_head_dim=attention_head_dim, text_embed_dim=text_embed_dim)
            self.parallel_manager = SimpleNamespace(dp_rank=0)

        def load_state_dict(self, sd):
            seen["sd"] = sorted(sd)

    class FakeVAE:
        def __init__(self, sd, device=None, scaling_factor=None, use_tiling=True):
            seen["vae"] = (sorted(sd), scaling_factor)

    import videosys_amd.vae_cogvideox as VC

    monkeypatch.setattr(PC, "CogVideoXTransformer3DModel", FakeModel)
    monkeypatch.setattr(VC, "CogVideoXVAE", FakeVAE)
    pipe = PC.CogVideoXPipeline(PC.CogVideoXConfig(model_path=str(root)), device="cpu")
    assert pipe.transformer.config.num_layers == 42 and pipe.transformer.config.use_rotary_positional_embeddings
    assert seen["sd"] == ["a.weight", "b.weight"] and seen["vae"] == (["decoder.x"], 0.7)
    two_b = PC.CogVideoXDDIMScheduler(snr_shift_scale=3.0)
    five_b = PC.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
    assert torch.equal(pipe.scheduler.alphas_cumprod, five_b.alphas_cumprod) and not torch.equal(two_b.alphas_cumprod, five_b.alphas_cumprod)

    # Latte: <model_path>/transformer + vae_temporal_decoder
    lroot = tmp_path / "latte"
    for sub in ("transformer", "vae_temporal_decoder"):
        (lroot / sub).mkdir(parents=True)
    (lroot / "transformer" / "config.json").write_text(json.dumps(dict(num_layers=3, caption_channels=64, norm_num_groups=32)))
    save_file({"w": torch.ones(1)}, str(lroot / "transformer" / "diffusion_pytorch_model.safetensors"))
    save_file({"d": torch.ones(1)}, str(lroot / "vae_temporal_decoder" / "diffusion_pytorch_model.safetensors"))

    class FakeLatte:
        def __init__(self, num_layers=28, caption_channels=4096, video_length=16, device=None, **unused):
            seen["latte"] = (num_layers, caption_channels, sorted(unused))
            self.config = SimpleNamespace(num_layers=num_layers, caption_channels=caption_channels)
            self.parallel_manager = SimpleNamespace(dp_rank=0)

        def load_state_dict(self, sd):
            seen["latte_sd"] = sorted(sd)

    import videosys_amd.vae_svd_temporal as VS

    monkeypatch.setattr(PL, "LatteT2V", FakeLatte)
    monkeypatch.setattr(VS, "AutoencoderKLTemporalDecoder", lambda sd, device=None: ("svd", sorted(sd)))
    lp = PL.LattePipeline(PL.LatteConfig(model_path=str(lroot)), device="cpu")
    assert seen["latte"] == (3, 64, []) and seen["latte_sd"] == ["w"] and lp.vae_decoder == ("svd", ["d"])


def test_pipeline_constructors_take_the_reference_components(tmp_path, monkeypatch, ref_trace):
    """The constructors keep the reference's parameter names and order (pipeline_open_sora.py:194-204, pipeline_latte.py:192-202,
    pipeline_cogvideox.py:124-134); ready-made components are adopted: a torch module holding reference weights is read through
    state_dict() / config, this build's own objects and schedulers are used as they are, a local ``text_encoder/`` + ``tokenizer``
    pair becomes the T5 callable.  Device models are recorders (host logic only)."""
    import ast
    import inspect
    import json
    from types import SimpleNamespace

    from safetensors.torch import save_file

    from videosys_amd import pipeline_cogvideox as PC, pipeline_latte as PL, pipeline_open_sora as PO
    import videosys_amd.t5 as T5

    def init_params(path, cls):   # the reference constructor's parameter names (replayed from tests/golden/ref_traces/)
        init = next(it for it in _ref_class_ast(path, cls).body if isinstance(it, ast.FunctionDef) and it.name == "__init__")
        return [a.arg for a in init.args.args]

    for path, cls, ours in (("pipelines/open_sora/pipeline_open_sora.py", "OpenSoraPipeline", PO.OpenSoraPipeline),
                            ("pipelines/latte/pipeline_latte.py", "LattePipeline", PL.LattePipeline),
                            ("pipelines/cogvideox/pipeline_cogvideox.py", "CogVideoXPipeline", PC.CogVideoXPipeline)):
        want = ref_trace.value(lambda: init_params(path, cls))
        have = [k for k, v in inspect.signature(ours.__init__).parameters.items() if v.kind == v.POSITIONAL_OR_KEYWORD]
        assert have == want, (cls, have, want)

    seen = {}

    class FakeT5:
        def __init__(self, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, vocab_size=32128, device=None, **kw):
            self.config = SimpleNamespace(d_model=d_model, num_layers=num_layers, vocab_size=vocab_size)

        def load_state_dict(self, sd):
            seen["t5_sd"] = sorted(sd)

    monkeypatch.setattr(T5, "T5Encoder", FakeT5)

    class FakeCog:
        def __init__(self, num_attention_heads=30, attention_head_dim=64, num_layers=30, use_rotary_positional_embeddings=False,
                     patch_size=2, in_channels=16, out_channels=16, text_embed_dim=4096, time_embed_dim=512, device=None, **kw):
            self.config = SimpleNamespace(num_layers=num_layers, text_embed_dim=text_embed_dim, num_attention_heads=num_attention_heads)
            self.parallel_manager = SimpleNamespace(dp_rank=0)

        def load_state_dict(self, sd):
            seen["cog_sd"] = sorted(sd)

    monkeypatch.setattr(PC, "CogVideoXTransformer3DModel", FakeCog)

    class RefModule:   # stands for a torch module of the reference: state_dict() + .config
        config = SimpleNamespace(num_layers=42, num_attention_heads=48, use_rotary_positional_embeddings=True, _name_or_path="x")

        def state_dict(self):
            return {"blocks.0.w": torch.ones(1)}

    root = tmp_path / "ckpt"
    (root / "text_encoder").mkdir(parents=True)
    (root / "text_encoder" / "config.json").write_text(json.dumps(dict(d_model=256, d_kv=64, d_ff=512, num_layers=2, num_heads=4,
                                                                        vocab_size=100, model_type="t5")))
    save_file({"shared.weight": torch.zeros(100, 256)}, str(root / "text_encoder" / "model.safetensors"))
    tok = lambda *a, **k: None
    sched = PC.CogVideoXDDIMScheduler(snr_shift_scale=2.0)
    vae = lambda z: z
    pipe = PC.CogVideoXPipeline(PC.CogVideoXConfig(model_path=str(root)), tok, None, vae, RefModule(), sched, device="cpu")
    assert pipe.transformer.config.num_layers == 42 and seen["cog_sd"] == ["blocks.0.w"]          # the module's geometry and weights
    assert pipe.scheduler is sched and pipe.vae is vae and pipe.vae_decoder is vae
    te = pipe.text_encoder                                                                       # <model_path>/text_encoder + tokenizer
    assert type(te).__name__ == "T5TextEncoder" and te.tokenizer is tok and pipe.tokenizer is tok and seen["t5_sd"] == ["shared.weight"]
    assert te.max_length == 226 and te.use_attention_mask is False and te.encoder.config.d_model == 256
    with pytest.raises(NotImplementedError):
        PC.CogVideoXPipeline(PC.CogVideoXConfig(model_path=str(root)), tok, None, vae, RefModule(), sched, device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError):   # a text-encoder MODULE needs its tokenizer
        PC.CogVideoXPipeline(PC.CogVideoXConfig(model_path="THUDM/CogVideoX-2b"), None, RefModule(), vae, RefModule(), sched, device="cpu")
    # a REAL transformers.T5EncoderModel handed over with its tokenizer: geometry from its config, weights from its state dict
    from transformers import T5Config, T5EncoderModel

    hf = T5EncoderModel(T5Config(d_model=128, d_kv=64, d_ff=256, num_layers=1, num_heads=2, vocab_size=64, feed_forward_proj="gated-gelu"))
    pipe3 = PC.CogVideoXPipeline(PC.CogVideoXConfig(model_path="THUDM/CogVideoX-2b"), tok, hf, transformer=FakeCog(), device="cpu")
    assert pipe3.text_encoder.encoder.config.d_model == 128 and pipe3.text_encoder.encoder.config.num_layers == 1
    assert "shared.weight" in seen["t5_sd"] and "encoder.block.0.layer.0.SelfAttention.q.weight" in seen["t5_sd"]
    with pytest.raises(TypeError):    # a foreign scheduler (e.g. the DPM one) has no fused-step coefficients
        PC.CogVideoXPipeline(PC.CogVideoXConfig(model_path="THUDM/CogVideoX-2b"), transformer=FakeCog(), scheduler=SimpleNamespace(step=print),
                             device="cpu")
    # own objects pass through; fp16 request accepted (same width, computed in bf16)
    own = FakeCog(num_layers=30)
    pipe2 = PC.CogVideoXPipeline(PC.CogVideoXConfig(model_path="THUDM/CogVideoX-2b"), transformer=own, text_encoder=lambda p: p,
                                 device="cpu", dtype=torch.float16)
    assert pipe2.transformer is own and pipe2.text_encoder("x") == "x" and pipe2.vae is None


def test_save_video_writes_a_playable_file_without_an_encoder_package(tmp_path):
    """utils.save_video (utils/utils.py:84-92): with imageio absent the frames land in a Motion-JPEG AVI; the container is parsed
    back here (RIFF sizes, stream header, index) and every frame decoded."""
    import io
    import struct

    import numpy as np
    from PIL import Image

    from videosys_amd.utils import save_video

    try:
        import imageio
        if hasattr(imageio, "mimwrite"):   # (oracle/ref_loader.py parks an empty stub of this name in the test process)
            pytest.skip("imageio present: the reference's own writer runs")
    except ImportError:
        pass
    T, H, W = 6, 48, 80
    yy, xx = np.mgrid[0:H, 0:W]
    v = np.stack([np.stack([(xx * 3 + t * 10) % 256, (yy * 5) % 256, np.full_like(xx, t * 40)], -1) for t in range(T)]).astype(np.uint8)
    path = save_video(torch.from_numpy(v), str(tmp_path / "clips" / "sunset.mp4"), fps=8)
    assert path.endswith("sunset.avi") and os.path.isfile(path)
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and d[8:12] == b"AVI " and struct.unpack("<I", d[4:8])[0] == len(d) - 8
    h = d.index(b"avih")
    usec, _, _, flags, total, _, streams, _, w, hgt = struct.unpack("<10I", d[h + 8:h + 48])
    assert (usec, total, streams, w, hgt) == (125000, T, 1, W, H) and flags & 0x10
    sh = d.index(b"strh")
    assert d[sh + 8:sh + 16] == b"vidsMJPG"
    scale, rate = struct.unpack("<II", d[sh + 28:sh + 36])
    assert rate / scale == 8
    movi = d.index(b"movi")
    idx = d.index(b"idx1", movi)
    assert struct.unpack("<I", d[idx + 4:idx + 8])[0] == 16 * T
    for n in range(T):
        tag, fl, off, size = struct.unpack("<4sIII", d[idx + 8 + 16 * n:idx + 24 + 16 * n])
        at = movi + off
        assert tag == b"00dc" and fl == 0x10 and d[at:at + 4] == b"00dc" and struct.unpack("<I", d[at + 4:at + 8])[0] == size
        img = np.asarray(Image.open(io.BytesIO(d[at + 8:at + 8 + size])).convert("RGB"))
        assert img.shape == (H, W, 3) and np.abs(img.astype(int) - v[n].astype(int)).mean() < 4.0
    # and back: the reader used for video references (open_sora_condition.read_from_path on .avi clips)
    from videosys_amd.open_sora_condition import read_from_path
    from videosys_amd.utils import read_mjpeg_avi

    back = read_mjpeg_avi(path)
    assert len(back) == T and back[0].size == (W, H) and np.abs(np.asarray(back[2]).astype(int) - v[2].astype(int)).mean() < 4.0
    clip = read_from_path(path, (24, 40))
    assert tuple(clip.shape) == (3, T, 24, 40) and -1.0 <= float(clip.min()) and float(clip.max()) <= 1.0
    with pytest.raises(NotImplementedError):
        read_from_path(str(tmp_path / "other.mp4"), (24, 40))
    # float frames [T, 3, H, W] in [0, 1] (Latte's single-image branch) and an explicit .avi name
    p2 = save_video(torch.from_numpy(v[:1]).permute(0, 3, 1, 2).float() / 255, str(tmp_path / "img.avi"), fps=8)
    assert p2.endswith("img.avi") and open(p2, "rb").read(4) == b"RIFF"


def test_progress_wrap_is_a_bar_on_request_only():
    """utils.progress_wrap (scheduling_rflow_open_sora.py:219): tqdm when asked (rank 0 of a group, or no group), the plain
    iterable otherwise; same items either way."""
    from videosys_amd.utils import progress_wrap

    items = list(enumerate([5, 6, 7]))
    assert progress_wrap(items, False) is items
    bar = progress_wrap(items, True, disable=True)
    assert type(bar).__name__.startswith("tqdm") and list(bar) == items


def test_caption_cleaner_equals_the_reference_on_generated_text(ref_trace):
    """Property test (hypothesis): caption.clean_caption / text_preprocessing against the reference's own functions compiled from
    its files (oracle/make_golden_caption.reference_cleaners), Open-Sora and Latte variants, on text assembled from the token
    classes the rules target (urls, html, entities, ids, sizes, CJK, dashes, quotes, shipping spam ...).  The two third-party steps
    are the same stand-ins on both sides (NFC for ftfy.fix_text, the standard library's html.parser for BeautifulSoup(...).text),
    so what is compared is the rule sequence.  The reference's results are replayed from tests/golden/ref_traces/."""
    import unicodedata

    from hypothesis import HealthCheck, given, settings, strategies as st

    from oracle.make_golden_caption import reference_cleaners
    from videosys_amd import caption as C

    soup = C._html_text
    try:
        import bs4  # noqa: F401
        pytest.skip("bs4 present: the product uses it, the stand-in comparison does not apply")
    except ImportError:
        pass
    try:
        import ftfy  # noqa: F401
        pytest.skip("ftfy present: the product uses it, the stand-in comparison does not apply")
    except ImportError:
        pass
    cleaners = []

    def reference(s):   # live only while minting the trace
        if not cleaners:
            cleaners.extend(reference_cleaners(fix_text=lambda t: unicodedata.normalize("NFC", t), soup_text=soup))
        ref_os, ref_latte = cleaners
        return (ref_os._clean_caption(s), ref_os.text_preprocessing(s), ref_os.text_preprocessing(s, False), ref_latte._clean_caption(s),
                ref_latte._text_preprocessing(s, clean_caption=True)[0])
    pieces = st.sampled_from([
        "a cat", "Sunset", "over the sea", " ", "  ", ",", ".", "..", "...", ":", " : ", ";", "!", "?", "-", "_", "--", "—", "–", "\\n", "\n",
        "https://example.com/a/b", "www.test.org", "http://x.co", "foo.com/page", "mail@host.ru", "@user_1", "#12", "#123456", "1234567",
        "192.168.0.1", "12:30 ", "IMG_001.jpg", "clip.mp4", "a.png", "jpg image", "png images", "<b>bold</b>", "<person>", "<br/>", "&amp;",
        "&quot;", "&lt;tag&gt;", "&#39;", "&amp", "湖边", "日落", "ｶﾀｶﾅ", "㈱", "“q”", "‘s’", "`tick`", "«g»", "\"", "'", "''", "\"\"", "(x)", "[y]",
        "{z}", "|", "/", "\\", "*", "~", "®", "™", "©", "free shipping", "worldwide free shipping", "download free", "free download",
        "click for more", "click on here", "page 12", "jc6640", "abc123def", "6640vc231", "j2d1a2a", "1920x1080", "3.5x2", "12×8", "10х10",
        "a%20b", "a+b", "é", "é", "ﬁ", "Ａ", "word.Word", "x,y", "a/b", "this-is-my-cute-cat", "this_is_my_cute_cat", ".hidden", "'lead",
        "trail:", "trail-", "+", "A1B2C3", "v2", "4k", "8K UHD", "№5", "½", "·", "•", "º", "¿que?", "¡hola!", "§2",
    ])
    text = st.lists(pieces, min_size=1, max_size=12).map("".join)

    @settings(max_examples=400, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))   # (a loaded box is not a failure)
    @given(text)
    def check(s):
        os_once, os_twice, os_plain, latte_once, latte_twice = ref_trace.lookup(s, lambda: reference(s))
        assert C.clean_caption(s) == os_once, ("open-sora once", s)
        assert C.text_preprocessing(s) == os_twice, ("open-sora twice", s)
        assert C.text_preprocessing(s, False) == os_plain, ("open-sora plain", s)
        assert C.clean_caption(s, mid_strip=False) == latte_once, ("latte once", s)
        assert C.text_preprocessing(s, True, mid_strip=False) == latte_twice, ("latte twice", s)

    check()


def test_mask_strategy_helpers_equal_the_reference_on_generated_cases(ref_trace):
    """Property test (hypothesis): parse_mask_strategy / find_nearest_point / apply_mask_strategy / append_generated /
    dframe_to_frame of open_sora_condition.py against the reference's own functions compiled from pipeline_open_sora.py:795-875,
    over generated strategies (all six fields, negative starts, several groups, several loops, alignment on / off).  The reference's
    results are replayed from tests/golden/ref_traces/."""
    import ast

    from hypothesis import HealthCheck, given, settings, strategies as st

    from videosys_amd import open_sora_condition as K

    ns = {}

    def ref(name):   # the reference function, live only while minting the trace
        if not ns:
            from oracle import ref_loader

            path = os.path.join(ref_loader.REFERENCE_ROOT, "videosys/pipelines/open_sora/pipeline_open_sora.py")
            want = {"MASK_DEFAULT", "parse_mask_strategy", "find_nearest_point", "apply_mask_strategy", "append_generated", "dframe_to_frame"}
            ns["torch"] = torch
            for node in ast.parse(open(path).read()).body:
                name_ = getattr(node, "name", None) or (node.targets[0].id if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) else None)
                if name_ in want:
                    exec(compile(ast.Module([node], []), path, "exec"), ns)
        return ns[name]

    group = st.tuples(st.integers(0, 2), st.integers(0, 1), st.integers(-6, 6), st.integers(-6, 12), st.integers(0, 8),
                      st.sampled_from([0.0, 0.3, 0.5, 1.0]), st.integers(1, 6))
    to_str = lambda gs: ";".join(",".join(str(v) for v in g[:g[6]]) for g in gs)

    @settings(max_examples=300, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(st.lists(group, min_size=0, max_size=3), st.integers(0, 2), st.sampled_from([None, 5]), st.integers(5, 15), st.integers(1, 12),
           st.integers(0, 10 ** 6))
    def check(groups, loop_i, align, Tz, Tref, seed):
        ms = to_str(groups)
        assert K.parse_mask_strategy(ms) == ref_trace.lookup(("parse", ms), lambda: ref("parse_mask_strategy")(ms))
        g = torch.Generator().manual_seed(seed)
        z = torch.randn(1, 4, Tz, 2, 2, generator=g)
        refs = [[torch.randn(4, Tref, 2, 2, generator=g), torch.randn(4, Tref + 2, 2, 2, generator=g)]]
        zb = z.clone()

        def reference():
            za = z.clone()
            masks = ref("apply_mask_strategy")(za, refs, [ms], loop_i, align=align)
            return za, masks

        try:
            za, want_masks = ref_trace.lookup(("apply", ms, loop_i, align, Tz, Tref, seed), reference)
        except Exception as e:     # e.g. a start beyond the clip: whatever the reference raises, this build raises too
            with pytest.raises(type(e)):
                K.apply_mask_strategy(zb, refs, [ms], loop_i, align=align)
            return
        got = K.apply_mask_strategy(zb, refs, [ms], loop_i, align=align)
        assert torch.equal(za, zb) and torch.equal(got, want_masks), ms

    check()
    for v in range(0, 40):
        for p in (1, 3, 5):
            for m in (5, 15, 38):
                assert K.find_nearest_point(v, p, m) == ref_trace.lookup(("nearest", v, p, m), lambda: ref("find_nearest_point")(v, p, m))
    for n in (0, 5, 10, 35):
        assert K.dframe_to_frame(n) == ref_trace.lookup(("dframe", n), lambda: ref("dframe_to_frame")(n))
    with pytest.raises(AssertionError):
        K.dframe_to_frame(7)

    class Vae:
        def encode(self, v):
            return v[:, :4, :3] * 2

    vid = torch.arange(2 * 4 * 6 * 2 * 2, dtype=torch.float32).view(2, 4, 6, 2, 2)
    # (an entry without references is [] in the reference's flow — its `refs is None` branch dies on len(None) two lines later)
    ra, ma = ref_trace.value(lambda: ref("append_generated")(Vae(), vid, [[], [torch.zeros(4, 1, 2, 2)]], [None, "0"], 1, 5, 0.0))
    rb, mb = K.append_generated(Vae().encode, vid, [[], [torch.zeros(4, 1, 2, 2)]], [None, "0"], 1, 5, 0.0)
    assert ma == mb and len(ra) == len(rb) and all(len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y)) for x, y in zip(ra, rb))


def test_gemm_tile_raster_is_a_bijection_for_every_setting():
    """csrc/common.h gemm_raster (through the host probe vsys_gemm_raster_probe): whatever column-group width / panel-chunk height
    the measurement tools select, every tile of the grid is visited exactly once — so the raster can never change a result."""
    import ctypes

    from videosys_amd import _lib

    lib = _lib.load()
    bm, bn = ctypes.c_int64(), ctypes.c_int64()
    for nbm, nbn in ((152, 18), (152, 24), (152, 6), (19, 18), (7, 24), (1, 9), (3, 3), (37, 12)):
        for gw, ph in ((6, 0), (12, 0), (4, 0), (3, 0), (6, 6), (8, 4), (9, 2), (6, 1), (0, 0), (24, 3), (5, 7)):
            seen = set()
            for t in range(nbm * nbn):
                assert lib.vsys_gemm_raster_probe(t, nbm, nbn, gw, ph, ctypes.byref(bm), ctypes.byref(bn)) == 0
                assert 0 <= bm.value < nbm and 0 <= bn.value < nbn
                seen.add((bm.value, bn.value))
            assert len(seen) == nbm * nbn, (nbm, nbn, gw, ph)
    assert lib.vsys_gemm_raster_probe(152 * 18, 152, 18, 6, 0, ctypes.byref(bm), ctypes.byref(bn)) != 0
    # the default raster keeps the 32 tiles an XCD runs first inside 6 column tiles (one W slab)
    cols = set()
    for t in range(32):
        lib.vsys_gemm_raster_probe(t, 152, 18, 6, 0, ctypes.byref(bm), ctypes.byref(bn))
        cols.add(bn.value)
    assert cols == set(range(6))


def test_bench_plain_form_starts_its_own_ranks(monkeypatch):
    """``python bench.py --gpus N`` (N > 1) with no launcher in the environment re-executes itself under torch.distributed.run with
    one process per GPU on 127.0.0.1 and hands back the launcher's exit code; under a launcher (RANK set) it does not."""
    import subprocess
    import sys

    import bench

    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "2"])
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "5", "--warmup", "2"]
    assert os.path.basename(cmd[-7]) == "bench.py" and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    # under a launcher the same command line goes on to the measurement (which refuses a box without devices)
    seen.clear()
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "4")
    if not torch.cuda.is_available():
        with pytest.raises(AssertionError, match="needs MI355X"):
            bench.main()
        assert not seen


def test_bench_full_is_opt_in(monkeypatch):
    """A plain bench.py command line measures the headline figure only; --full (off by default) adds the other measurements and
    is handed on to the ranks a plain ``--gpus N`` starts."""
    import subprocess
    import sys

    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--full"])
    assert bench.parse().full is True
    seen = {}
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: seen.setdefault("cmd", cmd) and 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--full"])
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and seen["cmd"][-3:] == ["--gpus", "2", "--full"]


@pytest.mark.parametrize("B,T,S,P,chunks", [(2, 5, 12, 4, False), (1, 38, 36, 8, False), (2, 19, 10, 4, True), (1, 10, 7, 8, True),
                                            (2, 3, 9, 2, False)])
def test_p2p_plans_equal_pack_exchange_unpack(B, T, S, P, chunks):
    """The one-kernel peer-to-peer exchange (dsp.plan_p2p_to_*: one copy per peer, straight from the source tensor into the peer's
    destination tensor) moves exactly the elements of pack -> all_to_all_single -> unpack (plan_switch_to_*), for padded frames
    (T % P != 0), padded columns (S % P != 0: the last rank's shard is part padding, or all of it), and chunked switches.  Every
    destination starts as a sentinel: both paths must write the same positions with the same values (all_to_all_with_pad,
    comm.py:282-304)."""
    from videosys_amd import dsp

    C = 8
    Sl = (S + (P - S % P) % P) // P
    Tp = (T + (P - T % P) % P) // P
    g = torch.Generator().manual_seed(B * 100 + T * 10 + S + P)
    xs = [torch.randn(B, T, Sl, C, generator=g) for _ in range(P)]                       # every rank's S-shard at rest
    cks = [None] if not chunks else [(0, -(-Tp // 2)), (-(-Tp // 2), Tp)] if Tp >= 2 else [None]
    for ck in cks:
        # ---- to the temporal shard
        packs, recvs = [], []
        for r in range(P):
            pack, unpack, sshape, oshape = dsp.plan_switch_to_temporal_shard(B, T, Sl, S, C, P, ck)
            send = torch.full(sshape, 5.0)
            torch_copy_executor(xs[r], send, pack)
            packs.append(send)
        ref = []
        for r in range(P):
            recv = torch.stack([packs[src][r] for src in range(P)], 0)
            out = torch.full(oshape, 7.0)
            torch_copy_executor(recv, out, unpack)
            ref.append(out)
        got = [torch.full(oshape, 7.0) for _ in range(P)]
        for me in range(P):
            ops, osh = dsp.plan_p2p_to_temporal_shard(B, T, Sl, S, C, P, me, ck)
            assert osh == oshape and len(ops) == P
            for r, o in enumerate(ops):
                if o is not None:
                    torch_copy_executor(xs[me], got[r], [o])
        for r in range(P):
            assert torch.equal(got[r], ref[r]), ("to_temporal", r, ck)
        # ---- and back: every rank's [B, Tc, S, C] into the frames of the S-shards
        Tc = oshape[1]
        ys = [torch.randn(B, Tc, S, C, generator=g) for _ in range(P)]
        packs = []
        for r in range(P):
            pack, unpack_r, sshape, oshape2 = dsp.plan_switch_to_spatial_shard(B, Tp, T, S, Sl, C, P, ck)
            send = torch.full(sshape, 5.0)
            torch_copy_executor(ys[r], send, pack)
            packs.append(send)
        ref = []
        for r in range(P):
            recv = torch.stack([packs[src][r] for src in range(P)], 0)
            out = torch.full(oshape2, 7.0)
            torch_copy_executor(recv, out, unpack_r)
            ref.append(out)
        got = [torch.full(oshape2, 7.0) for _ in range(P)]
        for me in range(P):
            ops, osh = dsp.plan_p2p_to_spatial_shard(B, Tp, T, S, Sl, C, P, me, ck)
            assert osh == oshape2
            for r, o in enumerate(ops):
                if o is not None:
                    torch_copy_executor(ys[me], got[r], [o])
        for r in range(P):
            assert torch.equal(got[r], ref[r]), ("to_spatial", r, ck)


@pytest.mark.parametrize("B,Lt,Lv,heads,P", [(2, 3, 9, 8, 4), (1, 5, 45, 6, 2), (2, 2, 7, 8, 8), (1, 4, 16, 12, 4)])
def test_p2p_ulysses_plans_equal_pack_exchange_unpack(B, Lt, Lv, heads, P):
    """The Ulysses head <-> sequence exchange of CogVideoX as peer-to-peer copies (dsp.plan_p2p_heads_scatter / _gather: straight into the
    peers' destination tensors, two problems per peer on the way back) against pack -> all_to_all_single -> unpack (plan_heads_scatter /
    plan_heads_gather; cogvideox_transformer_3d.py:45-86,112-123,160-165): same written positions, same values — padded video shards
    (Lv % P != 0, a rank with no video row at all) included."""
    from videosys_amd import dsp

    hd = 8
    C = heads * hd
    hw = C // P
    Lvl = -(-Lv // P)
    Ll, L = Lt + Lvl, Lt + Lv
    g = torch.Generator().manual_seed(B + Lt * 10 + Lv * 100 + P)
    qkvs = [torch.randn(B, Ll, 3 * C, generator=g) for _ in range(P)]
    # ---- sequence -> heads
    sends, ref = [], []
    for r in range(P):
        pack, ul, ur, sshape, oshape = dsp.plan_heads_scatter(B, Lt, Lvl, Lv, C, P, r)
        send = torch.full(sshape, 5.0)
        torch_copy_executor(qkvs[r], send, pack)
        sends.append(send)
    for r in range(P):
        pack, ul, ur, sshape, oshape = dsp.plan_heads_scatter(B, Lt, Lvl, Lv, C, P, r)
        recv = torch.stack([sends[src][r] for src in range(P)], 0)
        out = torch.full(oshape, 7.0)
        torch_copy_executor(qkvs[r], out, ul)
        torch_copy_executor(recv, out, ur)
        ref.append(out)
    got = [torch.full(oshape, 7.0) for _ in range(P)]
    for me in range(P):
        ops, osh = dsp.plan_p2p_heads_scatter(B, Lt, Lvl, Lv, C, P, me)
        assert osh == oshape and len(ops) == P
        for r, mine in enumerate(ops):
            for o in (mine or []):
                torch_copy_executor(qkvs[me], got[r], [o])
    for r in range(P):
        assert torch.equal(got[r], ref[r]), ("scatter_heads", r)
    # ---- heads -> sequence
    aos = [torch.randn(B, L, hw, generator=g) for _ in range(P)]
    sends, ref = [], []
    for r in range(P):
        pack, unpack, sshape, oshape = dsp.plan_heads_gather(B, Lt, Lvl, Lv, C, P)
        send = torch.full(sshape, 5.0)
        torch_copy_executor(aos[r], send, pack)
        sends.append(send)
    for r in range(P):
        recv = torch.stack([sends[src][r] for src in range(P)], 0)
        out = torch.full(oshape, 7.0)
        torch_copy_executor(recv, out, unpack)
        ref.append(out)
    got = [torch.full(oshape, 7.0) for _ in range(P)]
    for me in range(P):
        ops, osh = dsp.plan_p2p_heads_gather(B, Lt, Lvl, Lv, C, P, me)
        assert osh == oshape and all(len(m) == 2 for m in ops)
        for r, mine in enumerate(ops):
            for o in mine:
                torch_copy_executor(aos[me], got[r], [o])
    for r in range(P):
        assert torch.equal(got[r], ref[r]), ("gather_heads", r)
