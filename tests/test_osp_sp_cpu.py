"""CPU: Open-Sora-Plan v1.2 sequence parallelism, everything that needs no GPU.

  * dsp.UlyssesParallel with no text rows (Lt = 0): the pack / unpack plans applied with a torch executor on CPU tensors over
    tools/local_group.LocalWorld, and the peer-to-peer plans applied peer by peer, against the reference's all_to_all_comm written
    out (open_sora_plan_v120_transformer_3d.py:916-941 through comm.py: tensor_split on the scatter dim, concatenate on the gather
    dim), both directions; no plan holds a zero-row text problem and a gather is one problem per peer;
  * the receive image of the image route, indexed with the row formula of vsys_attn_prep_kv96_img / vsys_flash_attn_d96_img, holds
    the same result, and the send image of the way back, filled by that formula, gathers to the same rows;
  * OpenSoraT2V.enable_parallel's validation, the N % P check of forward, OpenSoraPlanPipeline's num_gpus rule, and _set_parallel
    dropping the recorded programs;
  * vsys_attn_prep_kv96_img / vsys_flash_attn_d96_img: declared, exported, bound, outside the op table, and every refused call's
    error code (the base entry points' checks plus the slab rule)."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from op_table import assert_coded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3
HD = 96
CASES = [(72, 8, 2), (72, 8, 8), (140, 4, 4)]     # (N tokens, heads, P ranks), B = 2
B = 2


def torch_executor(src, dst, ops):
    """vsys_copy_4d's semantics on CPU tensors (zero fill outside n1_valid / n2_valid)."""
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


def all_to_all_comm(xs, scatter_dim, gather_dim):
    """The reference's exchange over the P tensors of the ranks: rank r receives piece r of every rank's tensor_split along
    scatter_dim and concatenates the pieces, in source order, along gather_dim."""
    P = len(xs)
    pieces = [torch.tensor_split(x, P, dim=scatter_dim) for x in xs]
    return [torch.cat([pieces[src][r] for src in range(P)], dim=gather_dim).contiguous() for r in range(P)]


def local_qkv(N, heads, P, seed):
    """Per rank: qkv [B, Nl, 3C] of its tokens, values that name (rank, row, column)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N // P, 3 * heads * HD, generator=g).to(torch.bfloat16) for _ in range(P)]


def scattered_want(qkvs, heads):
    """Per rank: [B, N, 3 hw] = q | k | v of its heads over the whole sequence, by all_to_all_comm (scatter heads, gather tokens)."""
    C = heads * HD
    parts = [all_to_all_comm([x[..., i * C:(i + 1) * C] for x in qkvs], 2, 1) for i in range(3)]
    return [torch.cat([parts[i][r] for i in range(3)], dim=2) for r in range(len(qkvs))]


def image_row(s, b, seg, slab):
    return (s // seg) * slab + b * seg + s % seg


@pytest.mark.parametrize("N,heads,P", CASES)
def test_pack_unpack_plans_without_text_rows_equal_all_to_all_comm(N, heads, P):
    from tools.local_group import LocalWorld
    from videosys_amd import dsp

    C, Nl, hw = heads * HD, N // P, heads * HD // P
    qkvs = local_qkv(N, heads, P, N + P)
    want_h = scattered_want(qkvs, heads)
    g = torch.Generator().manual_seed(7)
    aos = [torch.randn(B, N, hw, generator=g).to(torch.bfloat16) for _ in range(P)]        # attention outputs of the ranks' heads
    want_back = all_to_all_comm(aos, 1, 2)                                                  # scatter tokens, gather heads: [B, Nl, C]

    def rank_fn(r, group):
        up = dsp.UlyssesParallel(group, copy_executor=torch_executor, text_rows=False)
        assert up.p2p is None
        got_h = up.scatter_heads(qkvs[r].view(B * Nl, 3 * C), B, 0, N, C).clone()
        got_back = up.gather_heads(aos[r].view(B * N, hw), B, 0, N, C).clone()
        # the image route: the receive image as it lies, read by the kernels' row formula ...
        recv = up.scatter_heads_image(qkvs[r].view(B * Nl, 3 * C), B, N, C)
        assert tuple(recv.shape) == (P, B, Nl, 3, hw)
        img = recv.view(P * B * Nl, 3 * hw)
        rows = torch.tensor([image_row(s, b, Nl, B * Nl) for b in range(B) for s in range(N)])
        from_img = img[rows].clone()
        # ... and the send image of the way back, filled by the same formula, nothing packed
        send = up.heads_send_image(B, N, C, aos[r])
        assert tuple(send.shape) == (P, B, Nl, hw)
        send.fill_(float("nan"))
        send.view(P * B * Nl, hw)[rows] = aos[r].view(B * N, hw)
        got_img_back = up.gather_heads_image(send, B, N, C).clone()
        return got_h, got_back, from_img, got_img_back

    for r, (got_h, got_back, from_img, got_img_back) in enumerate(LocalWorld(P, timeout=60).run(rank_fn)):
        assert torch.equal(got_h.view(B, N, 3 * hw), want_h[r]), f"scatter, rank {r}"
        assert torch.equal(got_back.view(B, Nl, C), want_back[r]), f"gather, rank {r}"
        assert torch.equal(from_img.view(B, N, 3 * hw), want_h[r]), f"receive image by the row formula, rank {r}"
        assert torch.equal(got_img_back.view(B, Nl, C), want_back[r]), f"gather of a caller-filled send image, rank {r}"


@pytest.mark.parametrize("N,heads,P", CASES)
def test_peer_to_peer_plans_without_text_rows_equal_all_to_all_comm(N, heads, P):
    from videosys_amd import dsp

    C, Nl, hw = heads * HD, N // P, heads * HD // P
    qkvs = local_qkv(N, heads, P, N + P + 1)
    want_h = scattered_want(qkvs, heads)
    outs = [torch.full((B, N, 3 * hw), float("nan"), dtype=torch.bfloat16) for _ in range(P)]
    for rank in range(P):
        ops, shape = dsp.plan_p2p_heads_scatter(B, 0, Nl, N, C, P, rank)
        assert shape == (B, N, 3 * hw) and all(o is not None and len(o) == 1 for o in ops), "one problem per peer, none for text rows"
        for r in range(P):
            torch_executor(qkvs[rank], outs[r], ops[r])
    for r in range(P):
        assert torch.equal(outs[r], want_h[r]), f"p2p scatter, rank {r}"
    g = torch.Generator().manual_seed(8)
    aos = [torch.randn(B, N, hw, generator=g).to(torch.bfloat16) for _ in range(P)]
    want_back = all_to_all_comm(aos, 1, 2)
    backs = [torch.full((B, Nl, C), float("nan"), dtype=torch.bfloat16) for _ in range(P)]
    for rank in range(P):
        ops, shape = dsp.plan_p2p_heads_gather(B, 0, Nl, N, C, P, rank)
        assert shape == (B, Nl, C) and all(len(o) == 1 for o in ops), "a gather without text rows is one problem per peer"
        for r in range(P):
            torch_executor(aos[rank], backs[r], ops[r])
    for r in range(P):
        assert torch.equal(backs[r], want_back[r]), f"p2p gather, rank {r}"


def test_no_plan_holds_a_zero_row_problem_and_the_launch_limit_follows():
    from tools.local_group import StubGroup
    from videosys_amd import dsp

    for N, heads, P in CASES:
        C, Nl = heads * HD, N // P
        pack, local, recv, _, _ = dsp.plan_heads_scatter(B, 0, Nl, N, C, P, 1)
        gpack, gunpack, _, _ = dsp.plan_heads_gather(B, 0, Nl, N, C, P)
        assert local == [] and len(pack) == len(recv) == len(gpack) == len(gunpack) == P
        assert all(o.n0 * o.n1 * o.n2 > 0 for o in pack + recv + gpack + gunpack)
    # CogVideoX's plans (text rows) are what they were: one local text problem, two pack problems per peer
    pack, local, recv, _, _ = dsp.plan_heads_scatter(B, 5, 9, 72, 8 * HD, 8, 1)
    assert len(local) == 1 and local[0].n1 == 5 and len(dsp.plan_heads_gather(B, 5, 9, 72, 8 * HD, 8)[0]) == 16
    assert all(len(o) == 2 for o in dsp.plan_p2p_heads_gather(B, 5, 9, 72, 8 * HD, 8, 1)[0])
    # 16 ranks in one peer-to-peer launch without text rows, 8 with (in-process groups take the one-kernel exchange)
    assert dsp.UlyssesParallel(StubGroup(16, 0), text_rows=False).p2p is not None
    assert dsp.UlyssesParallel(StubGroup(16, 0)).p2p is None and dsp.UlyssesParallel(StubGroup(8, 0)).p2p is not None


# ------------------------------------------------------------------------------------------------ validation
def small_model(heads=8, **over):
    from videosys_amd.open_sora_plan import OpenSoraT2V

    kw = dict(num_attention_heads=heads, attention_head_dim=96, in_channels=4, out_channels=4, num_layers=2, cross_attention_dim=heads * 96,
              attention_bias=True, sample_size=(8, 12), sample_size_t=3, patch_size=2, patch_size_t=1, activation_fn="gelu-approximate",
              norm_type="ada_norm_single", norm_elementwise_affine=False, norm_eps=1e-6, caption_channels=32, use_rope=True,
              interpolation_scale_h=1.0, interpolation_scale_w=1.0, interpolation_scale_t=1.0)
    kw.update(over)
    return OpenSoraT2V(**kw, device="cpu")


def manager(group, P, r=0, cp=1):
    return SimpleNamespace(sp_size=P, cp_size=cp, dp_size=1, dp_rank=0, sp_rank=r, cp_rank=0, sp_group=group, cp_group=None)


def test_enable_parallel_validation():
    from tools.local_group import StubGroup

    m = small_model(heads=8)
    m.enable_parallel(1, 1, False)
    assert m._sp is None and m.parallel_manager.sp_size == 1
    with pytest.raises(NotImplementedError) as e:          # no process group of 2 ranks in this process
        m.enable_parallel(1, 2, False)
    assert isinstance(e.value, AssertionError), "the mesh mismatch is both a NotImplementedError and an AssertionError"
    with pytest.raises(NotImplementedError, match="enable_cp"):
        m.enable_parallel(1, 1, True)
    with pytest.raises(NotImplementedError, match="enable_cp"):
        m.enable_parallel(enable_cp=True, parallel_mgr=manager(StubGroup(2, 0), 2))
    with pytest.raises(NotImplementedError, match="cp_size"):
        m.enable_parallel(parallel_mgr=manager(StubGroup(2, 0), 2, cp=2))
    with pytest.raises(ValueError, match="heads"):
        m.enable_parallel(parallel_mgr=manager(StubGroup(3, 0), 3))
    assert m._sp is None, "a refused call left the model sharded"
    m.enable_parallel(parallel_mgr=manager(StubGroup(4, 1), 4, 1))
    assert (m._sp.P, m._sp.rank, m._sp.text_rows) == (4, 1, False) and m.parallel_manager.sp_size == 4
    m.attn_route = "bogus"
    m._sp.p2p = None
    with pytest.raises(ValueError, match="attn_route"):
        m._route()
    m.attn_route = None
    assert m._route() == type(m).DEFAULT_A2A_ROUTE and type(m).DEFAULT_A2A_ROUTE in ("rows", "image")
    m.enable_parallel(parallel_mgr=manager(None, 1))       # back to one rank
    assert m._sp is None


def test_forward_refuses_a_token_count_the_ranks_cannot_split():
    from tools.local_group import StubGroup

    m = small_model(heads=8, sample_size=(8, 10))
    m.enable_parallel(parallel_mgr=manager(StubGroup(8, 0), 8))
    x = torch.zeros(2, 4, 3, 8, 10)                        # 3 * 4 * 5 = 60 tokens over 8 ranks
    with pytest.raises(ValueError, match="60 video tokens"):
        m(x, timestep=torch.tensor([500, 500]), encoder_hidden_states=torch.zeros(2, 1, 8, 32))


def test_pipeline_num_gpus_must_be_the_world_size():
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanConfig, OpenSoraPlanPipeline

    with pytest.raises(NotImplementedError, match="num_gpus") as e:
        OpenSoraPlanPipeline(OpenSoraPlanConfig(num_gpus=2, transformer="/nonexistent: no component may be read before the check"))
    assert isinstance(e.value, AssertionError)


def test_set_parallel_drops_the_recorded_programs():
    from tools.local_group import StubGroup
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanPipeline
    from videosys_amd.program import StepCache

    p = OpenSoraPlanPipeline.__new__(OpenSoraPlanPipeline)
    p.transformer = small_model(heads=8)
    p._steps = StepCache()
    p._steps.entries = {"recorded under one rank": object()}
    p._set_parallel(parallel_mgr=manager(StubGroup(2, 0), 2))
    assert p._steps.entries == {} and p.transformer._sp is not None and p.transformer._sp.P == 2
    p._steps.entries = {"recorded under two ranks": object()}
    p._set_parallel()                                      # the process group of this process: one rank
    assert p._steps.entries == {} and p.transformer._sp is None


# ------------------------------------------------------------------------------------------------ C ABI of the image entry points
IMG = ("vsys_attn_prep_kv96_img", "vsys_flash_attn_d96_img")


def test_image_entry_points_declared_exported_bound_and_in_the_op_table():
    from videosys_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    lib = _lib.load()
    for n in IMG:
        assert re.search(rf"\nint {n}\(", hdr) and n in _lib.SIGNATURES and hasattr(lib, n)
    assert_coded(IMG)                                 # in the launch-program table, with the prototype's arity
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"attention96_img.hip"' in src and "attention96.h" in src


def test_image_entry_points_host_side_argument_checks():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # an aligned address that is never dereferenced: every call below is refused before any launch

    def prep(k=P, ks=192, v=P, vs=192, cos=None, sin=None, kp=P, vt=P, batch=2, heads=2, kv_len=72, kv_pad=128, seg=9, slab=18):
        return lib.vsys_attn_prep_kv96_img(k, ks, v, vs, cos, sin, kp, vt, batch, heads, kv_len, kv_pad, seg, slab, None)

    def flash(q=P, qs=192, cos=None, sin=None, kp=P, vt=P, lens=None, out=P, os_=192, batch=2, heads=2, q_len=72, kv_len=72, kv_pad=128,
              seg=9, qslab=18, oslab=18):
        return lib.vsys_flash_attn_d96_img(q, qs, cos, sin, kp, vt, lens, out, os_, batch, heads, q_len, kv_len, kv_pad, seg, qslab, oslab,
                                           None)

    # the slab rule: seg_len >= 1; with more than one slab a slab holds at least batch * seg_len rows; one slab ignores the stride
    assert prep(seg=0) == VSYS_ERR_SHAPE and prep(seg=-3) == VSYS_ERR_SHAPE and prep(slab=17) == VSYS_ERR_SHAPE
    assert prep(seg=1 << 40) == VSYS_ERR_SHAPE
    assert flash(seg=0) == VSYS_ERR_SHAPE and flash(qslab=17) == VSYS_ERR_SHAPE and flash(oslab=17) == VSYS_ERR_SHAPE
    # ... and behind it every check of the base entry points, with their codes
    assert prep(kv_pad=100) == VSYS_ERR_SHAPE and prep(kv_pad=64) == VSYS_ERR_SHAPE
    assert prep(ks=190) == VSYS_ERR_SHAPE and prep(vs=96) == VSYS_ERR_SHAPE
    assert prep(cos=P) == VSYS_ERR_ARG and prep(k=None) == VSYS_ERR_ARG and prep(vt=None) == VSYS_ERR_ARG
    assert prep(batch=1 << 40) == VSYS_ERR_SHAPE and prep(batch=40000, heads=2, slab=40000 * 9) == VSYS_ERR_SHAPE
    assert flash(kv_pad=96) == VSYS_ERR_SHAPE and flash(kv_len=0) == VSYS_ERR_SHAPE and flash(kv_len=200) == VSYS_ERR_SHAPE
    assert flash(qs=100) == VSYS_ERR_SHAPE and flash(os_=190) == VSYS_ERR_SHAPE and flash(os_=96) == VSYS_ERR_SHAPE
    assert flash(sin=P) == VSYS_ERR_ARG and flash(out=None) == VSYS_ERR_ARG and flash(q_len=-1) == VSYS_ERR_SHAPE
    assert prep(k=P + 8) == VSYS_ERR_ALIGN and prep(vt=P + 2) == VSYS_ERR_ALIGN and prep(cos=P + 4, sin=P) == VSYS_ERR_ALIGN
    assert flash(q=P + 8) == VSYS_ERR_ALIGN and flash(out=P + 4) == VSYS_ERR_ALIGN and flash(lens=P + 2) == VSYS_ERR_ALIGN
    assert prep(batch=0) == 0 and flash(q_len=0) == 0                                          # nothing to do: nothing is launched
    # one slab (seg_len >= len): the slab strides are unused, so a small one is no error — refused later only for what the base refuses
    assert prep(seg=72, slab=0, kv_pad=100) == VSYS_ERR_SHAPE and prep(seg=100, slab=0, k=P + 8) == VSYS_ERR_ALIGN
    assert flash(seg=72, qslab=0, oslab=0, q=P + 8) == VSYS_ERR_ALIGN
