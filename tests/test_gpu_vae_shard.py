"""-m gpu: the VAE decode shared by the ranks of a group — CausalVAEDecoder.decode(z, group=) (Open-Sora-Plan: the (sample, temporal
chunk, spatial tile) units of the tiled decode dealt over the ranks), AutoencoderKLSD3Decoder.decode_u8 / decode(group=) (Vchitect:
contiguous frame blocks) and the two pipelines' ``shard_vae_decode`` switch.  Ranks are threads of tools/local_group.LocalWorld on
the one GPU, each with its own staging buffers and stream, as in tests/test_gpu_osp_sp.py.

Exact: a tile's GroupNorm runs over the tile alone and the 2-D decoder is per frame, so whoever decodes a unit gets the unsharded
decode's bits; every comparison below is torch.equal.  Beside the bits the tests count the work: the ``_decode_tile`` calls (frames
through ``_decode_rows``) of a rank are its share of the deal, not the whole decode, and a decode issues ONE all-gather (none when
it does not tile, or when sharding is switched off)."""
import copy
import functools
import os
import threading

import numpy as np
import pytest
import torch

from test_vae_shard_cpu import Counted

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Forwarding(Counted):
    """Counted, for a group a transformer runs on as well: whatever else the group offers (the in-process exchange set-up) passes."""

    def __getattr__(self, name):
        return getattr(self._g, name)


def refusing_group(P):
    from tools.local_group import StubGroup

    class Refuses(StubGroup):
        def all_gather_into_tensor(self, out, x):
            raise AssertionError("a collective was issued")

        all_to_all_single = all_gather_into_tensor

    return Refuses(P, 0)


def own_buffers(dec):
    """The same weights with staging buffers of its own: what a rank holds."""
    mine = copy.copy(dec)
    mine._padded = {}
    return mine


def on_ranks(P, fn):
    """fn(rank, counted group) on P threads, each on a stream of its own; the per-rank results."""
    from tools.local_group import LocalWorld

    torch.cuda.synchronize()

    def body(r, group):
        torch.cuda.set_device(0)
        with torch.cuda.stream(torch.cuda.Stream()):
            out = fn(r, Counted(group))
            torch.cuda.current_stream().synchronize()
        return out

    return LocalWorld(P, timeout=120).run(body)


# ------------------------------------------------------------------------------------------------ Open-Sora-Plan decoder
@functools.lru_cache(maxsize=None)
def osp_decoder():
    """hidden_size 32 with the weights and the tiling of tools/mint_osp_vae.py: tiles of 4 latent pixels stepping 3, chunks of 2
    latent frames."""
    from tools.mint_osp_vae import HIDDEN, SEED, TILING
    from videosys_amd.vae_open_sora_plan import CausalVAEDecoder, synth_state_dict

    d = CausalVAEDecoder(synth_state_dict(SEED, hidden_size=HIDDEN), device=dev())
    for k, v in TILING.items():
        setattr(d, k, v)
    d.enable_tiling()
    return d


@functools.lru_cache(maxsize=None)
def osp_case(shape):
    """(latents on the device, the unsharded decode) — computed once per shape."""
    z = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))).to(torch.bfloat16).float().to(dev())
    want = osp_decoder().decode(z)
    torch.cuda.synchronize()
    return z, want


def counting_tiles(d):
    calls = []
    inner = d._decode_tile
    d._decode_tile = lambda zt, in_scale: (calls.append(tuple(zt.shape)), inner(zt, in_scale))[1]
    return calls


@pytest.mark.parametrize("shape,units,P", [((1, 4, 3, 6, 8), 12, 2), ((1, 4, 3, 6, 8), 12, 3), ((1, 4, 3, 6, 8), 12, 8),
                                           ((2, 4, 3, 6, 8), 24, 3), ((1, 4, 2, 6, 8), 6, 8)])
def test_osp_tiled_decode_over_ranks_is_the_unsharded_decode(shape, units, P):
    from videosys_amd.vae_blocks import deal_units

    z, want = osp_case(shape)
    assert tuple(want.shape) == (shape[0], 3, 4 * (shape[2] - 1) + 1, 8 * shape[3], 8 * shape[4])
    ulist, costs = osp_decoder().tile_units(shape[0], *shape[2:])
    assert len(ulist) == units
    owner, _, _ = deal_units(costs, P)

    def rank_fn(r, g):
        d = own_buffers(osp_decoder())
        calls = counting_tiles(d)
        out = d.decode(z, group=g)
        return bool(torch.equal(out, want)), float((out.float() - want.float()).abs().max()), len(calls), g.gathers, g.all_to_alls

    res = on_ranks(P, rank_fn)
    for r, (same, diff, ncalls, gathers, a2a) in enumerate(res):
        assert same, f"rank {r} of {P}: decode(z, group) differs from decode(z), max |diff| {diff}"
        assert ncalls == owner.count(r), f"rank {r} of {P} decoded {ncalls} units, its share of the deal is {owner.count(r)}"
        assert (gathers, a2a) == (1, 0), f"rank {r} of {P}: {gathers} all-gathers, {a2a} all-to-alls in one decode"
    assert sum(n for _, _, n, _, _ in res) == units, "the ranks together decoded every unit once"
    assert [n for _, _, n, _, _ in res].count(0) == max(0, P - units)


def test_osp_in_scale_and_wrapper_take_the_group():
    from videosys_amd.vae_open_sora_plan import SCALE, CausalVAEModelWrapper

    z, _ = osp_case((1, 4, 3, 6, 8))
    w = CausalVAEModelWrapper.__new__(CausalVAEModelWrapper)
    w.vae = osp_decoder()
    want = w.decode(z * SCALE)
    torch.cuda.synchronize()
    assert tuple(want.shape) == (1, 9, 3, 48, 64)

    def rank_fn(r, g):
        mine = CausalVAEModelWrapper.__new__(CausalVAEModelWrapper)
        mine.vae = own_buffers(osp_decoder())
        return bool(torch.equal(mine.decode(z * SCALE, group=g), want)), g.gathers

    assert on_ranks(2, rank_fn) == [(True, 1)] * 2


def test_osp_untiled_decode_and_group_of_one_issue_no_collective():
    d = own_buffers(osp_decoder())
    z, want = osp_case((1, 4, 3, 6, 8))
    calls = counting_tiles(d)
    assert torch.equal(d.decode(z, group=refusing_group(1)), want) and len(calls) == 12      # a group of one: today's path
    small, small_want = osp_case((1, 4, 2, 4, 4))                                           # one tile, one chunk: does not tile
    assert torch.equal(d.decode(small, group=refusing_group(4)), small_want) and len(calls) == 13
    d.disable_tiling()
    plain = d.decode(z)
    assert not torch.equal(plain, want), "tiling changed nothing"
    assert torch.equal(d.decode(z, group=refusing_group(4)), plain) and len(calls) == 15


# ------------------------------------------------------------------------------------------------ SD3 decoder
@functools.lru_cache(maxsize=None)
def sd3_case():
    """(decoder with synthetic weights, sampler-side latents [1, 5, 16, 6, 8], decoder-side latents [5, 16, 6, 8], decode_u8, decode)."""
    from videosys_amd import vae_sd3

    dec = vae_sd3.AutoencoderKLSD3Decoder(vae_sd3.synth_state_dict(5), device=dev())
    g = torch.Generator().manual_seed(12)
    lat = (torch.randn(1, 5, 16, 6, 8, generator=g) * 1.3 + 0.2).to(dev())
    z = torch.randn(5, 16, 6, 8, generator=g).to(torch.bfloat16).float().to(dev())
    u8, px = dec.decode_u8(lat).clone(), dec.decode(z)[0].clone()
    torch.cuda.synchronize()
    assert tuple(u8.shape) == (5, 48, 64, 3) and tuple(px.shape) == (5, 3, 48, 64) and float(u8.float().std()) > 0
    return dec, lat, z, u8, px


@pytest.mark.parametrize("P", [2, 3, 8])
def test_sd3_frames_over_ranks_are_the_unsharded_decode(P):
    from videosys_amd.vae_blocks import frame_shards

    dec, lat, z, u8, px = sd3_case()
    shards = frame_shards(5, P)

    def rank_fn(r, g):
        d = own_buffers(dec)
        frames = []
        inner = d._decode_rows
        d._decode_rows = lambda zz, s, b: (frames.append(zz.shape[0]), inner(zz, s, b))[1]
        a = d.decode_u8(lat, group=g)
        n_u8, gathers_u8 = sum(frames), g.gathers
        b = d.decode(z, group=g)[0]
        ns = d.decode(z, return_dict=True, group=g).sample
        return (bool(a.dtype == torch.uint8 and torch.equal(a, u8)), bool(torch.equal(b, px)), bool(torch.equal(ns, px)), n_u8, sum(frames),
                gathers_u8, g.gathers, g.all_to_alls)

    for r, (same_u8, same_px, same_ns, n_u8, n_all, g_u8, g_all, a2a) in enumerate(on_ranks(P, rank_fn)):
        mine = shards[r][1] - shards[r][0]
        assert same_u8 and same_px and same_ns, f"rank {r} of {P}: (decode_u8, decode, decode as namespace) equal the ungrouped: {(same_u8, same_px, same_ns)}"
        assert (n_u8, n_all) == (mine, 3 * mine), f"rank {r} of {P} decoded {n_u8} frames, frame_shards gives it {mine}"
        assert (g_u8, g_all, a2a) == (1, 3, 0), f"rank {r} of {P}: all-gathers after one / three decodes {(g_u8, g_all)}"
    assert [b - a for a, b in shards].count(0) == {2: 0, 3: 0, 8: 3}[P]


def test_sd3_group_of_one_issues_no_collective():
    dec, lat, z, u8, px = sd3_case()
    d = own_buffers(dec)
    assert torch.equal(d.decode_u8(lat, group=refusing_group(1)), u8) and torch.equal(d.decode(z, group=refusing_group(1))[0], px)


# ------------------------------------------------------------------------------------------------ pipelines
VARIANTS = ("sharded", "config off", "environment off")


def pipeline_variants(P, build, generate, count):
    """Per rank: one pipeline (``build(rank, group)``), then ``generate`` three times — sharding on, ``shard_vae_decode=False``,
    ``VSYS_VAE_SHARD=0`` -> [rank][variant] = (frames, units decoded, all-gathers during the decodes); ``count(pipe, group)`` starts
    the two counts of a run and returns the callable that reads them.  The environment is the
    process's: a rank sets it before its third run (its peers are at most one collective behind, inside a run that does not read it
    to any effect) and the caller clears it after every rank is through."""
    from tools.local_group import LocalWorld

    lock = threading.Lock()
    saved = os.environ.pop("VSYS_VAE_SHARD", None)

    def rank_fn(r, group):
        torch.cuda.set_device(0)
        g = Forwarding(group)
        with lock:                       # (construction touches module state: one rank at a time)
            pipe = build(r, g)
        out = []
        for v in VARIANTS:
            pipe._config.shard_vae_decode = v != "config off"
            if v == "environment off":
                os.environ["VSYS_VAE_SHARD"] = "0"
            read = count(pipe, g)
            frames = generate(pipe)
            out.append((frames,) + read())
        return out

    try:
        return LocalWorld(P, timeout=240).run(rank_fn)
    finally:
        os.environ.pop("VSYS_VAE_SHARD", None)
        if saved is not None:
            os.environ["VSYS_VAE_SHARD"] = saved


def gathers_during(pipe, method, g):
    """Wrap ``pipe.<method>``: box[0] += the all-gathers the group saw during each call."""
    box = [0]
    inner = getattr(type(pipe), method).__get__(pipe)

    def wrapped(*a, **kw):
        before = g.gathers
        out = inner(*a, **kw)
        box[0] += g.gathers - before
        return out

    setattr(pipe, method, wrapped)
    return box


def test_osp_pipeline_two_ranks_share_the_decode():
    """OpenSoraPlanPipeline at tests/test_gpu_osp_pipeline.py's geometry with the tiling of tools/mint_osp_vae.py (latent [1, 4, 3, 8, 12]:
    two chunks x 3 x 4 tiles = 24 units), 2 steps, 2 ranks with an injected manager."""
    import test_gpu_osp_pipeline as tp
    from test_gpu_osp_sp import manager
    from tools.mint_osp_vae import TILING
    from videosys_amd import pab
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanPipeline
    from videosys_amd.vae_blocks import deal_units

    P, steps = 2, 2
    pab.set_pab_manager(None)

    def make():
        pipe = OpenSoraPlanPipeline(tp.config(), device=dev())
        for k, v in TILING.items():
            setattr(pipe.vae.vae, k, v)
        return pipe

    single = make()
    pe, pm, ne, nm = tp.embeds(single, ["a red fox runs over the snow"])

    def generate(pipe):
        gen = torch.Generator(device=dev()).manual_seed(77)
        out = pipe.generate(prompt_embeds=pe, prompt_attention_mask=pm, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm,
                            negative_prompt=None, num_inference_steps=steps, guidance_scale=tp.GS, latents=tp.start().clone(), generator=gen,
                            verbose=False)
        torch.cuda.synchronize()
        return out.video.clone()

    want = generate(single)
    assert want.dtype == torch.uint8 and tuple(want.shape) == (1, 9, 64, 96, 3)
    ulist, costs = single.vae.vae.tile_units(1, 3, 8, 12)
    owner, _, _ = deal_units(costs, P)
    assert len(ulist) == 24

    def build(r, g):
        pipe = make()
        pipe._set_parallel(parallel_mgr=manager(g, P, r))
        pipe.transformer._sp.p2p = None
        assert pipe.transformer._sp.P == P and pipe._decode_group() is g
        return pipe

    def count(pipe, g):
        if "calls" not in pipe.__dict__:
            pipe.calls = counting_tiles(pipe.vae.vae)
            pipe.box = gathers_during(pipe, "decode_latents", g)
        del pipe.calls[:]
        pipe.box[0] = 0
        return lambda: (len(pipe.calls), pipe.box[0])

    res = pipeline_variants(P, build, generate, count)
    for r, runs in enumerate(res):
        for v, (frames, ncalls, gathers) in zip(VARIANTS, runs):
            assert torch.equal(frames, want), f"rank {r}, {v}: the frames differ from the single-rank run's"
            share = owner.count(r) if v == "sharded" else 24
            assert (ncalls, gathers) == (share, 1 if v == "sharded" else 0), f"rank {r}, {v}: {ncalls} units decoded (expected {share}), {gathers} all-gathers"
    assert sum(runs[0][1] for runs in res) == 24


def test_vchitect_pipeline_two_ranks_share_the_decode():
    """VchitectXLPipeline at tests/test_gpu_vchitect_sp.py's pipeline geometry (5 frames of 12 x 20 latent pixels), 2 steps, 2 ranks with
    an injected manager.  DEPTH ONE: with two layers the frame-sharded transformer is by construction not the single-process one
    (tests/test_gpu_vchitect_sp.py: cross keys = row 0 of the local shard), so only at depth one can the frames of a 2-rank run be
    held to the single-rank run's; the decode under test is the same."""
    import test_gpu_vchitect_pipeline as tp
    from test_gpu_vchitect_sp import HH, JD, L, PD, WW, manager
    from videosys_amd import VchitectConfig, VchitectXLPipeline, pab
    from videosys_amd.vae_blocks import frame_shards

    pab.set_pab_manager(None)
    F, P, steps = 5, 2, 2
    gen = torch.Generator().manual_seed(100 + F)
    bf = lambda *s: torch.randn(*s, generator=gen).to(torch.bfloat16).float()
    emb = dict(prompt_embeds=bf(1, L, JD), pooled_prompt_embeds=bf(1, PD), negative_prompt_embeds=bf(1, L, JD),
               negative_pooled_prompt_embeds=bf(1, PD))
    z0 = bf(1, F, 16, HH, WW)
    make = lambda: VchitectXLPipeline(VchitectConfig(f"synthetic:{tp.SEED}", transformer_config=dict(tp.TCFG, num_layers=1)))

    def generate(pipe):
        out = pipe.generate(height=8 * HH, width=8 * WW, frames=F, num_inference_steps=steps, guidance_scale=tp.GS, seed=0, latents=z0, **emb)
        torch.cuda.synchronize()
        pt = pipe.decode_frames(z0.to(dev()), "pt")              # the bf16 route of decode_frames ("np" is its copy to the host)
        torch.cuda.synchronize()
        return np.stack([np.asarray(f) for f in out.video[0]]), pt.float().cpu()

    single = make()
    want, want_pt = generate(single)
    assert want.shape == (F, 8 * HH, 8 * WW, 3) and want.dtype == np.uint8 and tuple(want_pt.shape) == (F, 3, 8 * HH, 8 * WW)
    shards = frame_shards(F, P)

    def build(r, g):
        pipe = make()
        pipe._set_parallel(parallel_mgr=manager(g, P, r))
        pipe.transformer._sp.p2p = None
        assert pipe.transformer._sp.P == P and pipe._decode_group() is g
        return pipe

    def count(pipe, g):
        if "frames" not in pipe.__dict__:
            pipe.frames = []
            inner = pipe.vae._decode_rows
            pipe.vae._decode_rows = lambda zz, s, b: (pipe.frames.append(zz.shape[0]), inner(zz, s, b))[1]
            pipe.box = gathers_during(pipe, "decode_frames", g)
        del pipe.frames[:]
        pipe.box[0] = 0
        return lambda: (sum(pipe.frames), pipe.box[0])

    res = pipeline_variants(P, build, generate, count)
    for r, runs in enumerate(res):
        for v, ((frames, pt), nframes, gathers) in zip(VARIANTS, runs):
            assert np.array_equal(frames, want), f"rank {r}, {v}: the frames differ from the single-rank run's"
            assert torch.equal(pt, want_pt), f"rank {r}, {v}: decode_frames(..., 'pt') differs from the single-rank run's"
            share = (shards[r][1] - shards[r][0]) if v == "sharded" else F
            # (generate() and the "pt" call decode once each)
            assert (nframes, gathers) == (2 * share, 2 if v == "sharded" else 0), f"rank {r}, {v}: {nframes} frames decoded (expected {2 * share}), {gathers} all-gathers"
