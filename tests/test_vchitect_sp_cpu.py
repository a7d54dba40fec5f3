"""No GPU: Vchitect-2.0 sequence parallelism on the host side.

  * tests/vchitect_sp_ref.py (the sharded forward restated) against tests/vchitect_ref.py: P = 1 is the single-process forward
    bit for bit in float64; at depth 1, B = 1 and per-sample text every P gives the P = 1 result bit for bit (the cross keys of every
    rank are then the same rows, and no block follows in which the text rows could differ per frame) — where a rank holds ONE frame,
    (2, 2) and (3, 8), the P = 1 result with every `*temp*` weight zeroed, which is what the `cur_frame == 1` rule read on the local
    frame count makes of it; a poisoned padded frame's text reaches no output.
  * the exchange plans the layer uses (dsp.plan_switch_to_spatial_shard / _temporal_shard and their peer-to-peer forms, frames and
    tokens swapped with respect to STDiT3) applied with a torch executor, against all_to_all_with_pad written out as comm.py does it.
  * vsys_attn_temporal_d64_img: header, ctypes table, exports, the op table still at 60, every refused call's error code.
  * enable_parallel's three host-side answers."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import vchitect_ref as vr
import vchitect_sp_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSYS_ERR_SHAPE, VSYS_ERR_ALIGN, VSYS_ERR_ARG = -1, -2, -3
CFG = dict(num_layers=2, heads=3, patch=2, out_channels=16, sample_size=32, pos_embed_max_size=24)
JD = PD = 64


def inputs(F, B=1, L=7, depth=2, per_frame_text=True, seed=11, hw=(12, 20)):
    from videosys_amd.vchitect import synth_state_dict

    sd = {k: v.to(torch.bfloat16).float() for k, v in synth_state_dict(depth, 3, joint_attention_dim=JD, pooled_projection_dim=PD, seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 100 * F)
    x = torch.randn(B, F, 16, *hw, generator=g).to(torch.bfloat16).float()
    enc = torch.randn(B * F if per_frame_text else B, L, JD, generator=g).to(torch.bfloat16).float()
    if not per_frame_text:
        enc = enc[:, None].expand(B, F, L, JD).reshape(B * F, L, JD)
    pooled = torch.randn(B, PD, generator=g).to(torch.bfloat16).float()
    return sd, x, enc, pooled, dict(CFG, num_layers=depth)


def test_restatement_with_one_rank_is_the_single_process_forward():
    sd, x, enc, pooled, cfg = inputs(3, B=2, L=8, hw=(16, 16))
    ts = torch.tensor([500.0, 500.0])
    assert torch.equal(sr.model_forward(sd, cfg, x, enc, pooled, ts, 1), vr.model_forward(sd, cfg, x, enc, pooled, ts))


@pytest.mark.parametrize("F,P", [(5, 2), (5, 4), (3, 8), (2, 2)])
def test_restatement_depth_one_per_sample_text_does_not_depend_on_the_rank_count(F, P):
    sd, x, enc, pooled, cfg = inputs(F, depth=1, per_frame_text=False)
    ts = torch.tensor([500.0])
    one = sr.model_forward(sd, cfg, x, enc, pooled, ts, 1)
    many = sr.model_forward(sd, cfg, x, enc, pooled, ts, P)
    if -(-F // P) == 1:       # one frame per rank, (2, 2) and (3, 8): the temporal contributions are multiplied by zero (the rule reads the LOCAL count)
        zeroed = {k: (torch.zeros_like(v) if "temp" in k else v) for k, v in sd.items()}
        one = sr.model_forward(zeroed, cfg, x, enc, pooled, ts, 1)
    assert torch.equal(many, one)
    # what a padded frame's text rows hold reaches no output
    assert torch.equal(sr.model_forward(sd, cfg, x, enc, pooled, ts, P, pad_text=1e3), many)


def test_restatement_depth_two_differs_past_the_first_shard():
    """Rank r's cross keys are the text rows of frame r Fl, which differ per frame after the first block: frames [0, Fl) still
    equal the single-process run (rank 0's keys are frame 0), the others do not."""
    F, P = 5, 2
    sd, x, enc, pooled, cfg = inputs(F, depth=2, per_frame_text=False)
    ts = torch.tensor([500.0])
    one, two = sr.model_forward(sd, cfg, x, enc, pooled, ts, 1), sr.model_forward(sd, cfg, x, enc, pooled, ts, P)
    Fl = 3
    assert torch.equal(two[:Fl], one[:Fl]) and not torch.equal(two[Fl:], one[Fl:])


# ------------------------------------------------------------------------------------------------ plans
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


def exchange(sends):
    """all_to_all_single over P ranks: recv[dst][src] = send[src][dst]."""
    P = len(sends)
    return [torch.stack([sends[src][dst] for src in range(P)]) for dst in range(P)]


PLAN_CASES = [(5, 2, 6, 3), (5, 4, 6, 3), (2, 2, 5, 2), (5, 4, 60, 7), (3, 8, 60, 7)]


@pytest.mark.parametrize("F,P,S,L", PLAN_CASES)
def test_plans_equal_the_exchange_written_out(F, P, S, L):
    """Both tensors (video n = S, text n = L), both directions, both routes.  (5, 4): rank 3 holds only padding and rank 2 one real
    frame; (60, 7) at P = 8: Sl = 8, Ll = 1 and the last rank has no text token at all."""
    from videosys_amd import dsp

    B, C = 2, 8
    Fl = -(-F // P)
    g = torch.Generator().manual_seed(F * 100 + P)
    for n in (S, L):
        nl = -(-n // P)
        full = torch.randn(B, F, n, C, generator=g).to(torch.bfloat16)
        at_rest = [c.reshape(B, Fl, n, C) for c in sr.split_frames(full.reshape(B * F, n, C), B, P)]
        want = sr.all_to_all_with_pad(at_rest, 2, 1, scatter_pad=sr.pad_to(n, P), gather_pad=sr.pad_to(F, P))       # [B, F, nl, C] per rank
        dirty = [t.clone() for t in at_rest]
        for r in range(P):                                  # what a padded frame holds after a block: anything
            dirty[r][:, max(0, min(Fl, F - r * Fl)):] = float("nan")
        # ---- frames -> tokens, pack + all_to_all_single + unpack
        pack, unpack, sshape, oshape = dsp.plan_switch_to_spatial_shard(B, Fl, F, n, nl, C, P)
        assert oshape == (B, F, nl, C)
        sends = []
        for r in range(P):
            send = torch.full(sshape, 7.0, dtype=torch.bfloat16)
            torch_executor(dirty[r], send, pack)
            sends.append(send)
        got = []
        for r, recv in enumerate(exchange(sends)):
            out = torch.full(oshape, 7.0, dtype=torch.bfloat16)
            torch_executor(recv, out, unpack)
            assert torch.equal(out, want[r]), f"to the token shard, rank {r}"
            assert not torch.isnan(out).any()              # no real row reads a padded frame
            assert bool((out[:, :, max(0, min(nl, n - r * nl)):] == 0).all())      # padded tokens are zero rows, as the reference's
            got.append(out)
        # ---- the same in one copy per peer
        outs = [torch.full(oshape, 7.0, dtype=torch.bfloat16) for _ in range(P)]
        for r in range(P):
            ops_, _ = dsp.plan_p2p_to_spatial_shard(B, Fl, F, n, nl, C, P, r)
            for dst, o in enumerate(ops_):
                if o is not None:
                    torch_executor(dirty[r], outs[dst], [o])
        for r in range(P):
            assert torch.equal(outs[r], want[r]), f"peer to peer to the token shard, rank {r}"
        # ---- tokens -> frames
        back_want = sr.all_to_all_with_pad(want, 1, 2, scatter_pad=sr.pad_to(F, P), gather_pad=sr.pad_to(n, P))
        tok = [t.clone() for t in want]
        for r in range(P):                                  # the attention's output on a padded token: anything
            tok[r][:, :, max(0, min(nl, n - r * nl)):] = float("nan")
        pack, unpack, sshape, oshape = dsp.plan_switch_to_temporal_shard(B, F, nl, n, C, P)
        assert oshape == (B, Fl, n, C)
        sends = []
        for r in range(P):
            send = torch.full(sshape, 7.0, dtype=torch.bfloat16)
            torch_executor(tok[r], send, pack)
            sends.append(send)
        for r, recv in enumerate(exchange(sends)):
            out = torch.full(oshape, 7.0, dtype=torch.bfloat16)
            torch_executor(recv, out, unpack)
            assert torch.equal(out, back_want[r]) and torch.equal(out, at_rest[r]), f"back to the frame shard, rank {r}"
        outs = [torch.full(oshape, 7.0, dtype=torch.bfloat16) for _ in range(P)]
        for r in range(P):
            ops_, _ = dsp.plan_p2p_to_temporal_shard(B, F, nl, n, C, P, r)
            for dst, o in enumerate(ops_):
                if o is not None:
                    torch_executor(tok[r], outs[dst], [o])
        for r in range(P):
            assert torch.equal(outs[r], at_rest[r]), f"peer to peer back to the frame shard, rank {r}"


# ------------------------------------------------------------------------------------------------ the entry point
def test_image_entry_point_is_declared_bound_exported_and_outside_the_op_table():
    from videosys_amd import _lib, _opcodes

    name = "vsys_attn_temporal_d64_img"
    hdr = open(os.path.join(ROOT, "include", "videosys_amd.h")).read()
    m = re.search(rf"\nint {name}\(([^;]*?)\);", hdr, flags=re.S)
    assert m, "no prototype in the header"
    params = [x.strip() for x in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert params[-1] == "void* stream" and len(params) == len(_lib.SIGNATURES[name])
    for p, t in zip(params, _lib.SIGNATURES[name]):
        assert (t is _lib._ptr) == p.rsplit(" ", 1)[0].endswith("*"), p
    sib = _lib.SIGNATURES["vsys_attn_temporal_d64"]
    assert _lib.SIGNATURES[name] == sib[:20] + [_lib._i64] * 3 + sib[20:]       # the sibling's arguments with Tl and the two slab strides
    assert hasattr(_lib.load(), name)
    # the one launch entry point without a code: its integer / pointer arguments do not fit a command record
    n_int = sum(t is not _lib._f32 for t in _lib.SIGNATURES[name][:-1])
    cap = int(re.search(r"#define VSYS_CMD_MAX_INT (\d+)", hdr).group(1))
    assert n_int == len(params) - 1 == 26 and cap == 24 and n_int > cap
    assert name not in _opcodes.OPCODES and len(_opcodes.OPCODES) == 74
    assert int(re.search(r"#define VSYS_OP_COUNT (\d+)", hdr).group(1)) == 75
    gen = os.path.join(ROOT, "videosys_amd", "csrc", "gen", "program_gen.py")
    assert subprocess.run([sys.executable, gen, "--check"], capture_output=True).returncode == 0


def test_image_entry_point_argument_checks():
    from videosys_amd import _lib

    lib = _lib.load()
    P = 0x10000           # a 16-byte aligned address that is never dereferenced: every call below is refused before any launch

    def img(B=1, T=5, Tl=2, S=3, L=2, heads=2, ld=128, vid=P, txt=P, cos=P, sin=P, out=P, qp=None, slab_v=None, slab_t=None):
        q = vid if qp is None else qp
        sv = B * Tl * S if slab_v is None else slab_v
        st = B * Tl * L if slab_t is None else slab_t
        return lib.vsys_attn_temporal_d64_img(q, ld, vid, ld, vid, ld, txt, ld, txt, ld, txt, ld, cos, sin, out, ld, out if txt else None, ld,
                                              B, T, Tl, sv, st, S, L, heads, None)

    assert img(T=0) == VSYS_ERR_SHAPE
    assert img(heads=0) == VSYS_ERR_SHAPE
    assert img(S=0, L=0) == VSYS_ERR_SHAPE
    assert img(B=0) == VSYS_ERR_SHAPE
    assert img(ld=64) == VSYS_ERR_SHAPE                     # a row narrower than heads * 64
    assert img(ld=132) == VSYS_ERR_ALIGN                    # a stride that is no multiple of 8 elements
    assert img(qp=P + 2) == VSYS_ERR_ALIGN                  # a pointer off the 16-byte grid
    assert img(sin=None) == VSYS_ERR_ARG                    # one RoPE table without the other
    assert img(vid=None) == VSYS_ERR_ARG                    # S > 0 without video rows
    assert img(txt=None) == VSYS_ERR_ARG                    # L > 0 without text rows
    assert img(T=1 << 31) == VSYS_ERR_SHAPE
    assert img(Tl=0) == VSYS_ERR_SHAPE
    assert img(Tl=-3) == VSYS_ERR_SHAPE
    assert img(Tl=1 << 31) == VSYS_ERR_SHAPE
    assert img(slab_v=5) == VSYS_ERR_SHAPE                  # slabs that overlap: a slab holds B * Tl * S rows
    assert img(slab_t=3) == VSYS_ERR_SHAPE
    assert img(B=1 << 20, S=1 << 12, L=0, txt=None, heads=4) == VSYS_ERR_SHAPE      # a grid past 2^31 - 1 workgroups


# ------------------------------------------------------------------------------------------------ enable_parallel
def _model():
    from videosys_amd.vchitect import VchitectXLTransformerModel

    return VchitectXLTransformerModel(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=3,
                                      joint_attention_dim=JD, caption_projection_dim=192, pooled_projection_dim=PD, out_channels=16,
                                      pos_embed_max_size=24, device="cpu")


def _manager(P, r=0):
    from types import SimpleNamespace

    from tools.local_group import StubGroup

    return SimpleNamespace(sp_size=P, cp_size=1, dp_size=1, dp_rank=0, sp_rank=r, cp_rank=0, sp_group=StubGroup(P, r), cp_group=None)


def test_enable_parallel_without_a_group_of_that_size_raises():
    m = _model()
    for args in ((1, 2, False), (1, 4, True), (2, 1, False)):
        with pytest.raises(NotImplementedError, match="no process group of"):
            m.enable_parallel(*args)
        with pytest.raises(NotImplementedError):
            m.transformer_blocks[0].attn.enable_parallel(*args)
    m.enable_parallel(1, 1, False)
    m.enable_parallel(1, 1, True)
    assert m._sp is None and all(b.attn._sp is None for b in m.transformer_blocks)


def test_enable_parallel_with_an_injected_manager():
    m = _model()
    m.enable_parallel(parallel_mgr=_manager(1))
    assert m._sp is None and all(b.attn._sp is None for b in m.transformer_blocks)
    with pytest.raises(NotImplementedError, match="CFG split"):
        m.enable_parallel(1, 2, True, parallel_mgr=_manager(2))
    m.enable_parallel(parallel_mgr=_manager(2, 1))
    assert m._sp is not None and (m._sp.P, m._sp.rank) == (2, 1)
    assert all(b.attn._sp is m._sp for b in m.transformer_blocks)
    assert [b.attn._sp_tag for b in m.transformer_blocks] == ["0", "1"]
    assert m._local_frames(5) == (3, 3, 2)
    m.enable_parallel(1, 1, False)
    assert m._sp is None and all(b.attn._sp is None for b in m.transformer_blocks)
