"""-m gpu: Open-Sora-Plan v1.2 sequence parallelism (videosys_amd/open_sora_plan.py: tokens sharded at rest, the Ulysses head <->
sequence exchange around the head-dim-96 attention) with every rank of the group on the one GPU of the box: ranks are threads
(tools/local_group.LocalWorld), one test runs two gloo processes.

Exact everywhere: every op outside the self-attention works row by row on the local tokens, the attention of a head does not depend
on which rank computes it, and the image kernels give the base kernels' bits (tests/test_gpu_osp_attention_img.py) — so the sharded
model must give the single-process BITS on every rank, on every route (peer-to-peer + rows, all_to_all_single + rows,
all_to_all_single + image), recorded and replayed.

Model A: 8 heads x 96, 2 layers, patch 2, latent [2, 4, 3, 8, 12] = 72 tokens, 8 text keys with visible counts [8, 5]; P in {2, 4, 8}.
Model B: 4 heads, latent [2, 4, 5, 8, 14] = 140 tokens (two query blocks, three key tiles); P in {2, 4}."""
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

ROUTES = [(True, "rows"), (False, "rows"), (False, "image")]          # (peer-to-peer exchange, attention route)
MODELS = {"A": dict(heads=8, thw=(3, 8, 12)), "B": dict(heads=4, thw=(5, 8, 14))}
LK, CC, SEED = 8, 32, 1206
PAB_CFG = dict(spatial_broadcast=True, spatial_threshold=[100, 900], spatial_range=2, cross_broadcast=True, cross_threshold=[100, 900],
               cross_range=3)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def model(name):
    from videosys_amd.open_sora_plan import OpenSoraT2V, synth_state_dict

    heads, (T, Hh, Ww) = MODELS[name]["heads"], MODELS[name]["thw"]
    kw = dict(num_attention_heads=heads, attention_head_dim=96, in_channels=4, out_channels=4, num_layers=2, cross_attention_dim=heads * 96,
              attention_bias=True, sample_size=(Hh, Ww), sample_size_t=T, patch_size=2, patch_size_t=1, activation_fn="gelu-approximate",
              norm_type="ada_norm_single", norm_elementwise_affine=False, norm_eps=1e-6, caption_channels=CC, use_rope=True,
              interpolation_scale_h=1.0, interpolation_scale_w=1.0, interpolation_scale_t=1.0)
    sd = synth_state_dict(num_layers=2, num_heads=heads, caption_channels=CC, in_channels=4, out_channels=4, patch_size=2, seed=SEED)
    return OpenSoraT2V(**kw, device=dev()).load_state_dict(sd)


def inputs(name, step=0):
    g = torch.Generator().manual_seed(SEED + step)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()
    mask = torch.ones(2, 1, LK)
    mask[1, 0, 5:] = 0                                     # visible counts [8, 5]
    return bf(2, 4, *MODELS[name]["thw"]), bf(2, 1, LK, CC), mask


def run(m, x, enc, mask, t=500):
    return m(x, timestep=torch.tensor([t, t]), encoder_hidden_states=enc, encoder_attention_mask=mask).video


def manager(group, P, r):
    from types import SimpleNamespace

    return SimpleNamespace(sp_size=P, cp_size=1, dp_size=1, dp_rank=0, sp_rank=r, cp_rank=0, sp_group=group, cp_group=None)


def shard(m, group, P, r, p2p, route):
    m.enable_parallel(parallel_mgr=manager(group, P, r))
    assert m._sp.p2p is not None          # in-process groups run the one-kernel exchange by default
    if not p2p:
        m._sp.p2p = None
    m.attn_route = route
    return m


def record_and_replay(m, x, enc, mask):
    """One recorded call and its replay into the same buffer: (first output, replayed output)."""
    from videosys_amd import program

    run(m, x, enc, mask)                  # warm: text K / V, tables, workspace and exchange sites resident
    with program.Recorder() as rec:
        out = run(m, x, enc, mask)
    prog = rec.finish()
    assert prog is not None, rec.invalid
    torch.cuda.synchronize()
    first = out.clone()
    out.fill_(float("nan"))
    prog.run()
    torch.cuda.synchronize()
    return first, out.clone()


_WANT = {}


def single_process(name):
    """The single-process output, once per model (left unchanged)."""
    if name not in _WANT:
        from videosys_amd import pab

        pab.set_pab_manager(None)
        _WANT[name] = run(model(name), *inputs(name)).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(_WANT[name]).all()
    return _WANT[name]


@pytest.mark.parametrize("name,P", [("A", 2), ("A", 4), ("A", 8), ("B", 2), ("B", 4)])
def test_sharded_equals_single_process_on_every_rank_and_route(name, P):
    from tools.local_group import LocalWorld
    from videosys_amd import pab

    want = single_process(name)
    pab.set_pab_manager(None)
    x, enc, mask = inputs(name)

    def rank_fn(r, group):
        torch.cuda.set_device(0)
        m = model(name)
        res = []
        for p2p, route in ROUTES:
            shard(m, group, P, r, p2p, route)
            before = m._sp.p2p.launches if p2p else 0
            first, again = record_and_replay(m, x, enc, mask)
            if p2p:
                assert m._sp.p2p.launches > before
                m._sp.p2p.check()
            res.append((bool(torch.equal(first, want)), bool(torch.equal(again, want)), float((first - want).abs().max())))
        return res

    for r, res in enumerate(LocalWorld(P, timeout=120).run(rank_fn)):
        bad = [(v, got) for v, got in zip(ROUTES, res) if not (got[0] and got[1])]
        assert not bad, f"model {name}, rank {r} of {P}: (p2p, route) -> (recorded equal, replayed equal, max |diff|): {bad}"


def test_recorded_image_step_has_exactly_the_collectives_as_host_actions():
    """Model A on 2 ranks, the image route over all_to_all_single: the image attention launches are commands of the recorded step
    (they have op codes), so its host actions are the collectives and nothing else — two all-to-alls per block and the all-gather of
    the tail, as many collectives per replay — and the replay gives the single-process bits."""
    from tools.local_group import LocalWorld
    from videosys_amd import pab, program
    from videosys_amd._opcodes import OPCODES

    P, depth = 2, 2
    want = single_process("A")
    pab.set_pab_manager(None)
    x, enc, mask = inputs("A")

    def rank_fn(r, group):
        torch.cuda.set_device(0)
        calls = {"n": 0}
        a2a, gather = group.all_to_all_single, group.all_gather_into_tensor
        group.all_to_all_single = lambda recv, send: (calls.__setitem__("n", calls["n"] + 1), a2a(recv, send))[1]
        group.all_gather_into_tensor = lambda out, t: (calls.__setitem__("n", calls["n"] + 1), gather(out, t))[1]
        m = shard(model("A"), group, P, r, False, "image")
        run(m, x, enc, mask)                  # warm, as record_and_replay
        calls["n"] = 0
        with program.Recorder() as rec:
            out = run(m, x, enc, mask)
        prog = rec.finish()
        assert prog is not None, rec.invalid
        recorded = calls["n"]
        host = [k for k, seg in enumerate(prog.segments) if not isinstance(seg, tuple)]
        ops = [c.op for seg in prog.segments if isinstance(seg, tuple) for c in seg[0]]
        # no two host actions are neighbours: between two collectives lie the commands of the attention they frame
        apart = all(k > 0 and isinstance(prog.segments[k - 1], tuple) for k in host)
        out.fill_(float("nan"))
        calls["n"] = 0
        prog.run()
        torch.cuda.synchronize()
        return (recorded, len(host), apart, calls["n"], ops.count(OPCODES["vsys_attn_prep_kv96_img"]),
                ops.count(OPCODES["vsys_flash_attn_d96_img"]), len(ops) == prog.n_launches, bool(torch.equal(out, want)))

    for r, res in enumerate(LocalWorld(P, timeout=120).run(rank_fn)):
        n = 2 * depth + 1
        assert res == (n, n, True, n, depth, depth, True, True), \
            (f"rank {r}: (collectives while recording, host actions, commands between them, collectives per replay, image prep / "
             f"flash commands, every launch a command, replay equals single process) = {res}")


def test_pab_schedule_sharded_equals_single_process_and_broadcast_steps_exchange_nothing():
    """Four timesteps, ranges 2 (spatial) and 3 (cross), as tests/test_gpu_osp_model.py: every step on every rank equals the
    single-process step through the same schedule (the caches hold local rows), and a step exchanges twice per block that computes its
    self-attention, never for a broadcast one — on every rank alike — plus the one all-gather of the tail."""
    from tools.local_group import LocalWorld
    from videosys_amd import pab

    P, steps, depth = 4, [800, 700, 600, 500], 2
    data = [inputs("A", step=i) for i in range(len(steps))]
    try:
        pab.set_pab_manager(pab.PABConfig(**PAB_CFG))
        pab.update_steps(len(steps))
        cs = cc = 0
        want_dec = []
        for t in steps:
            bs, cs = pab.if_broadcast_spatial(t, cs)
            bc, cc = pab.if_broadcast_cross(t, cc)
            want_dec.append((bs, bc))
        assert want_dec[0] == (False, False) and any(w[0] for w in want_dec) and any(w[1] for w in want_dec)
        one = model("A")
        one.reset_pab_state()
        want = [run(one, *d, t=t).clone() for d, t in zip(data, steps)]
        torch.cuda.synchronize()

        def rank_fn(r, group):
            torch.cuda.set_device(0)
            calls = {"a2a": 0, "gather": 0}
            a2a, gather = group.all_to_all_single, group.all_gather_into_tensor
            group.all_to_all_single = lambda recv, send: (calls.__setitem__("a2a", calls["a2a"] + 1), a2a(recv, send))[1]
            group.all_gather_into_tensor = lambda out, t: (calls.__setitem__("gather", calls["gather"] + 1), gather(out, t))[1]
            m = shard(model("A"), group, P, r, False, "image")
            m.reset_pab_state()
            got, counts, same = [], [], []
            for i, (d, t) in enumerate(zip(data, steps)):
                calls.update(a2a=0, gather=0)
                out = run(m, *d, t=t)
                torch.cuda.synchronize()
                same.append(bool(torch.equal(out, want[i])))
                got.append(list(m.last_decisions))
                counts.append(dict(calls))
            local_rows = all(st.last_attn.shape[0] == 2 * 72 // P and st.last_cross.shape[0] == 2 * 72 // P for st in m.states)
            return got, counts, same, local_rows

        results = LocalWorld(P, timeout=120).run(rank_fn)
    finally:
        pab.set_pab_manager(None)
    for r, (got, counts, same, local_rows) in enumerate(results):
        assert got == [[w] * depth for w in want_dec], (r, got, want_dec)
        assert counts == [dict(a2a=0 if w[0] else 2 * depth, gather=1) for w in want_dec], (r, counts)
        assert same == [True] * len(steps), f"rank {r}: steps equal to the single-process schedule: {same}"
        assert local_rows, f"rank {r}: the PAB caches do not hold the local rows"


# ------------------------------------------------------------------------------------------------ two processes over gloo
def _worker(rank, world, port, outdir, p2p=False):
    import traceback

    import torch.distributed as dist

    try:
        os.environ["VSYS_DSP_P2P"] = "1" if p2p else "0"
        os.environ["VSYS_P2P_TIMEOUT_S"] = "5"
        from videosys_amd import pab

        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
        pab.set_pab_manager(None)
        x, enc, mask = inputs("A")
        m = model("A")
        want = run(m, x, enc, mask).clone()
        m.enable_parallel(1, world, False)
        assert m._sp is not None and (m._sp.P, m._sp.rank) == (world, rank)
        res = []
        for route in (("rows",) if p2p else ("rows", "image")):
            m.attn_route = route
            first, again = record_and_replay(m, x, enc, mask)
            res.append((route, bool(torch.equal(first, want)), bool(torch.equal(again, want)), float((first - want).abs().max())))
        if p2p:
            assert m._sp.p2p is not None and m._sp.p2p.launches > 0, "VSYS_DSP_P2P=1 did not take the peer-to-peer path"
            m._sp.p2p.check()
        else:
            assert m._sp.p2p is None
        bad = [v for v in res if not (v[1] and v[2])]
        with open(os.path.join(outdir, f"r{rank}.txt"), "w") as f:
            f.write("ok" if not bad else f"mismatch (route, recorded equal, replayed equal, max|diff|): {bad}")
    except Exception:
        with open(os.path.join(outdir, f"r{rank}.txt"), "w") as f:
            f.write(traceback.format_exc())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("p2p", [False, True], ids=["all_to_all", "peer_to_peer"])
def test_two_processes_over_gloo_equal_single_process(p2p):
    from test_gpu_sp import _run

    _run(_worker, (p2p,))


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_two_ranks_in_process():
    """OpenSoraPlanPipeline with synthetic components (tests/test_gpu_osp_pipeline.py's small geometry) on 2 ranks with an injected
    manager, 3 steps under PAB: the uint8 frames on both ranks equal the single-rank run's, and every rank recorded one program per
    PAB decision pattern and replayed the other steps."""
    import test_gpu_osp_pipeline as tp
    from tools.local_group import LocalWorld
    from videosys_amd import pab
    from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanPipeline, OpenSoraPlanV120PABConfig

    P, steps = 2, 3
    pcfg = OpenSoraPlanV120PABConfig(spatial_threshold=[100, 850], spatial_range=2, cross_threshold=[100, 850], cross_range=3)
    over = dict(enable_pab=True, pab_config=pcfg)
    lock = threading.Lock()

    def generate(pipe, e):
        pe, pm, ne, nm = e
        g = torch.Generator(device=dev()).manual_seed(77)
        out = pipe.generate(prompt_embeds=pe, prompt_attention_mask=pm, negative_prompt_embeds=ne, negative_prompt_attention_mask=nm,
                            negative_prompt=None, num_inference_steps=steps, guidance_scale=tp.GS, latents=tp.start().clone(), generator=g,
                            verbose=False)
        torch.cuda.synchronize()
        return out.video

    try:
        single = OpenSoraPlanPipeline(tp.config(**over), device=dev())
        e = tp.embeds(single, ["a red fox runs over the snow"])
        want = generate(single, e).clone()
        assert want.dtype == torch.uint8 and want.dim() == 5
        patterns = len({tuple(map(tuple, s)) for s in single.pab_trace})

        def rank_fn(r, group):
            torch.cuda.set_device(0)
            with lock:                       # (construction touches module state: one rank at a time)
                pipe = OpenSoraPlanPipeline(tp.config(**over), device=dev())
            pipe._set_parallel(parallel_mgr=manager(group, P, r))
            assert pipe.transformer._sp is not None and pipe.transformer._sp.P == P
            video = generate(pipe, e)
            return video.cpu(), dict(pipe.step_stats), [list(s) for s in pipe.pab_trace]

        results = LocalWorld(P, timeout=120).run(rank_fn)
    finally:
        pab.set_pab_manager(None)
    for r, (video, stats, trace) in enumerate(results):
        assert torch.equal(video, want.cpu()), f"rank {r}: the frames differ from the single-rank run's"
        assert trace == [list(s) for s in single.pab_trace]
        assert stats == {"recorded": patterns, "replayed": steps - patterns, "eager": 0}, (r, stats, patterns)
