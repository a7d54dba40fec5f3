"""CPU: the host layer that shares one VAE decode among the ranks of a group (videosys_amd/vae_blocks.py deal_units / gather_units /
frame_shards), the balance it gives the Open-Sora-Plan v1.2 tilings, and the ``shard_vae_decode`` switch of the two pipelines.
Ranks are threads of tools/local_group.LocalWorld over CPU tensors."""
import os
from types import SimpleNamespace

import pytest
import torch

# total cost over the busiest rank's cost, derived from the deal: a 64-latent tile stepping 48, 8-frame chunks overlapping by one
BALANCE = {"29x480p": (1.80, 1.80, 1.80), "93x480p": (1.99, 3.92, 6.08), "29x720p": (1.97, 3.25, 5.38), "93x720p": (2.00, 3.94, 7.84)}
UNITS = {"29x480p": 4, "93x480p": 16, "29x720p": 8, "93x720p": 32}


def cogvideox_areas():
    """The inputs of tests/test_cogvideox_vae_cpu.py: 3 x 3 tiles of 30 x 45 latent pixels stepping 25 / 36 over 60 x 90."""
    return [min(30, 60 - i) * min(45, 90 - j) for i in (0, 25, 50) for j in (0, 36, 72)]


@pytest.mark.parametrize("P", [1, 2, 3, 4, 8, 11])
def test_deal_units_owns_every_unit_once_with_dense_slots(P):
    from videosys_amd.vae_blocks import deal_units

    for costs in (cogvideox_areas(), [5, 5, 5, 5, 5, 5], [7], []):
        owner, slot, per = deal_units(costs, P)
        assert len(owner) == len(slot) == len(costs) and all(0 <= o < P for o in owner)
        for r in range(P):
            assert sorted(s for o, s in zip(owner, slot) if o == r) == list(range(owner.count(r))), (P, r)
        assert per == max([owner.count(r) for r in range(P)], default=0)
        assert deal_units(costs, P) == (owner, slot, per), "not deterministic"
    # ties go to the lower index: equal units over more ranks than units land on ranks 0 .. n - 1, in order
    assert deal_units([3, 3, 3], 8)[0] == [0, 1, 2]
    # largest first, each to the least loaded: 9 | 5 + 3 (+ 1 to the rank that then has less: 8 < 9)
    assert deal_units([1, 3, 9, 5], 2)[0] == [1, 1, 0, 1]


def test_deal_units_is_the_cogvideox_deal():
    from videosys_amd.vae_blocks import deal_units
    from videosys_amd.vae_cogvideox import CogVideoXVAE

    areas = cogvideox_areas()
    for P in (1, 2, 3, 4, 8):
        assert CogVideoXVAE._deal_tiles(areas, P) == deal_units(areas, P)
    owner, slot, per = deal_units(areas, 4)
    loads = [sum(a for a, o in zip(areas, owner) if o == r) for r in range(4)]
    assert sum(areas) == 7560 and max(loads) == 1980 and per == 3 and owner[0] == 0


def osp_decoder_geometry():
    """A CausalVAEDecoder without weights or device (the constructor refuses a CPU), with the tiling OpenSoraPlanPipeline sets
    (pipeline_open_sora_plan.py:309-315 of the reference, tile_overlap_factor 0.25): the unit list needs nothing else."""
    from videosys_amd.vae_open_sora_plan import CausalVAEDecoder

    d = CausalVAEDecoder.__new__(CausalVAEDecoder)
    d.tile_overlap_factor, d.tile_sample_min_size, d.tile_latent_min_size = 0.25, 512, 64
    d.tile_sample_min_size_t, d.tile_latent_min_size_t = 29, 8
    return d


@pytest.mark.parametrize("name", sorted(BALANCE))
def test_balance_of_the_published_open_sora_plan_geometries(name):
    from videosys_amd.pipeline_open_sora_plan import _V120_GEOMETRY
    from videosys_amd.vae_blocks import deal_units

    geo = _V120_GEOMETRY[name]
    units, costs = osp_decoder_geometry().tile_units(1, geo["sample_size_t"], *geo["sample_size"])
    assert len(units) == len(costs) == UNITS[name]
    for P, want in zip((2, 4, 8), BALANCE[name]):
        owner, _, _ = deal_units(costs, P)
        busiest = max(sum(c for c, o in zip(costs, owner) if o == r) for r in range(P))
        assert round(sum(costs) / busiest, 2) == want, (name, P, sum(costs) / busiest)


def test_tile_units_cover_the_batch_in_decode_order():
    d = osp_decoder_geometry()
    d.tile_latent_min_size, d.tile_sample_min_size, d.tile_latent_min_size_t, d.tile_overlap_factor = 4, 32, 2, 0.25
    units, costs = d.tile_units(2, 3, 6, 8)
    assert len(units) == 24 and units[0] == (0, (0, 2), 0, 0) and units[6] == (0, (1, 3), 0, 0) and units[12][0] == 1
    assert costs[:6] == [2 * 4 * 4, 2 * 4 * 4, 2 * 4 * 2, 2 * 3 * 4, 2 * 3 * 4, 2 * 3 * 2]
    assert len(d.tile_units(1, 2, 6, 8)[0]) == 6


class Counted:
    """A LocalGroup that counts its collectives (dsp.py group protocol)."""

    def __init__(self, group):
        self._g, self.size, self.rank = group, group.size, group.rank
        self.gathers = self.all_to_alls = 0

    def all_gather_into_tensor(self, out, x):
        self.gathers += 1
        self._g.all_gather_into_tensor(out, x)

    def all_to_all_single(self, recv, send):
        self.all_to_alls += 1
        self._g.all_to_all_single(recv, send)


@pytest.mark.parametrize("P", [1, 2, 3, 8])
def test_gather_units_hands_every_rank_every_unit_after_one_all_gather(P):
    from tools.local_group import LocalWorld
    from videosys_amd.vae_blocks import deal_units, gather_units

    shapes = [(3, 1 + u % 2, 2 + u, 5 - u % 3) for u in range(6)]       # six units, two ranks of eight idle
    pad = (3, 2, 7, 5)
    costs = [s[1] * s[2] * s[3] for s in shapes]

    def fake(u):
        n = 3 * costs[u]
        return ((torch.arange(n) % 7) + 10 * (u + 1)).to(torch.bfloat16).view(shapes[u])

    owner, slot, per = deal_units(costs, P)

    def rank_fn(r, group):
        g = Counted(group)
        mine = {u: fake(u) for u in range(6) if owner[u] == r}
        out = gather_units(mine, owner, slot, per, pad, g, torch.device("cpu"), shapes)
        return out, g.gathers, g.all_to_alls, len(mine)

    results = LocalWorld(P, timeout=60).run(rank_fn)
    assert sum(n for _, _, _, n in results) == 6 and [n for _, _, _, n in results].count(0) == max(0, P - 6)
    for r, (out, gathers, a2a, _) in enumerate(results):
        assert (gathers, a2a) == (1, 0), f"rank {r} of {P}: {gathers} all-gathers, {a2a} all-to-alls"
        assert len(out) == 6
        for u in range(6):
            assert out[u].dtype == torch.bfloat16 and out[u].is_contiguous() and tuple(out[u].shape) == shapes[u]
            assert torch.equal(out[u], fake(u)), (P, r, u)


@pytest.mark.parametrize("F,P", [(5, 2), (5, 3), (5, 8), (40, 8)])
def test_frame_shards_are_contiguous_and_cover_the_frames(F, P):
    from videosys_amd.vae_blocks import frame_shards

    sh = frame_shards(F, P)
    per = -(-F // P)
    assert len(sh) == P and sh[0][0] == 0 and max(b for _, b in sh) == F
    for r, (a, b) in enumerate(sh):
        assert 0 <= b - a <= per and a == min(r * per, F)
        if r:
            assert a == sh[r - 1][1]
        if r * per >= F:
            assert (a, b) == (F, F), "a rank past the end has no frames"
    assert sum(b - a for a, b in sh) == F
    if (F, P) == (40, 8):
        assert all(b - a == 5 for a, b in sh)


def test_configs_take_shard_vae_decode_and_refuse_unknown_keywords():
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanConfig
    from videosys_amd.pipeline_vchitect import VchitectConfig

    for cls in (OpenSoraPlanConfig, VchitectConfig):
        assert cls().shard_vae_decode is True
        assert cls(shard_vae_decode=False).shard_vae_decode is False
        with pytest.raises(TypeError):
            cls(shard_vae_decoder=False)
        with pytest.raises(TypeError):
            cls(shard_vae_decode=True, no_such_keyword=1)


def test_decode_group_rule():
    """The transformer's group under sequence parallelism; None on one rank, with shard_vae_decode=False, with VSYS_VAE_SHARD=0."""
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanPipeline
    from videosys_amd.pipeline_vchitect import VchitectXLPipeline

    saved = os.environ.pop("VSYS_VAE_SHARD", None)
    try:
        for cls in (OpenSoraPlanPipeline, VchitectXLPipeline):
            pipe = lambda shard, sp: SimpleNamespace(_config=SimpleNamespace(shard_vae_decode=shard), transformer=SimpleNamespace(_sp=sp))
            two, one = SimpleNamespace(P=2, group="the group"), SimpleNamespace(P=1, group="alone")
            assert cls._decode_group(pipe(True, two)) == "the group"
            assert cls._decode_group(pipe(True, one)) is None and cls._decode_group(pipe(True, None)) is None
            assert cls._decode_group(pipe(False, two)) is None
            os.environ["VSYS_VAE_SHARD"] = "0"
            assert cls._decode_group(pipe(True, two)) is None
            os.environ["VSYS_VAE_SHARD"] = "1"
            assert cls._decode_group(pipe(True, two)) == "the group"
            del os.environ["VSYS_VAE_SHARD"]
    finally:
        os.environ.pop("VSYS_VAE_SHARD", None)
        if saved is not None:
            os.environ["VSYS_VAE_SHARD"] = saved
