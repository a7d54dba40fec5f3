#!/usr/bin/env python
"""Mint the Vchitect-2.0 fixtures: the reference's OWN VchitectXLTransformerModel and JointTransformerBlock
(vchitect_transformer_3d.py, attentions.py:321-949) run on the CPU at a small geometry, in float64, float32 and bfloat16, without and
with PAB.  Runs only where the reference tree is present (oracle.ref_loader.reference_available()); the fixtures hold data only —
inputs, outputs and plain metadata; the weights are regenerated from videosys_amd.vchitect.synth_state_dict(seed), rounded to bf16 —
and tests/test_vchitect_pinned_cpu.py / tests/test_gpu_vchitect_pinned.py pin tests/vchitect_ref.py, tests/vchitect_sp_ref.py and the
HIP model to them without the reference tree.

    python tools/mint_vchitect.py            write the fixtures
    python tools/mint_vchitect.py --check    rebuild in memory and compare with the committed files (exit 1 on any difference)

  tests/golden/vchitect_fwd_small.pt     the model in the PIPELINE's call form (B = 1, one text row), cases f3 / f1 / rect / b2f1
  tests/golden/vchitect_pab_small.pt     four sampler steps of two calls each (the rows of a CFG pair) with PAB, and the same calls without
  tests/golden/vchitect_layer_small.pt   one JointTransformerBlock, context_pre_only False and True, and the outputs of its attn module
  tests/golden/vchitect_sp_small.pt      the model with sp_size = 2: two gloo processes, the reference's ParallelManager and comm.py

The reference class imports over oracle/diffusers_stub.py; parallel_manager is a stand-in with sp_size = cp_size = 1 except in the
two-process run.  The mint asserts, on the reference alone, what makes the PAB fixture worth having: the first PAB call equals the
PAB-free call bit for bit, every branch broadcasts on some call, and on every call with a stale branch the PAB output is at least
4 x 1.5 x the bf16 floor away from the PAB-free output (so a model that recomputes, or mixes the wrong cache, cannot pass a 1.5 x floor
bound).  If a seed fails that, change the seed, not the factor."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FWD, PABF, LAYER, SPF = (os.path.join(GOLDEN, f"vchitect_{n}_small.pt") for n in ("fwd", "pab", "layer", "sp"))

SEED = 2024
JD = PD = 64
L = 8
KWARGS = dict(sample_size=32, patch_size=2, in_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=3,
              joint_attention_dim=JD, caption_projection_dim=192, pooled_projection_dim=PD, out_channels=16, pos_embed_max_size=24)
PAB = dict(spatial_broadcast=True, spatial_threshold=[100, 950], spatial_range=2, temporal_broadcast=True, temporal_threshold=[100, 950],
           temporal_range=3, cross_broadcast=True, cross_threshold=[100, 950], cross_range=4)
PAB_STEPS = [900, 700, 500, 300]
# name: (B, F, latent H, latent W, timestep)
CASES = {"f3": (1, 3, 16, 16, 500), "f1": (1, 1, 16, 16, 500), "rect": (1, 2, 16, 12, 500), "b2f1": (2, 1, 16, 16, 500)}
PAB_GEOMETRY = (3, 8, 8)        # F, latent H, latent W of the PAB calls
SP_CASE = dict(P=2, F=3, HW=16, L=7, t=500)


class SP1:
    sp_size, cp_size, sp_group = 1, 1, None


def rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


class Mesh:
    """colossalai.cluster.process_group_mesh.ProcessGroupMesh, the two members the reference's ParallelManager uses, restated from
    its published behaviour: ranks laid out row-major on the mesh; the group along an axis joins the ranks that differ only there."""

    def __init__(self, *size):
        import numpy as np
        import torch.distributed as dist

        assert int(np.prod(size)) == dist.get_world_size(), (size, dist.get_world_size())
        self._shape, self._coord = size, np.unravel_index(dist.get_rank(), size)

    def get_group_along_axis(self, axis):
        import numpy as np
        import torch.distributed as dist

        mine = None
        ranks = np.arange(int(np.prod(self._shape))).reshape(self._shape)
        for line in np.moveaxis(ranks, axis, -1).reshape(-1, self._shape[axis]):     # every rank creates every group, in one order
            group = dist.new_group([int(r) for r in line])
            if dist.get_rank() in line:
                mine = group
        return mine


def reference_modules():
    """The reference's vchitect_transformer_3d and pab_mgr modules.  Also fixes the thread count of this process: the host BLAS splits
    its sums by thread, so the fp32 and bf16 bits of the fixtures are those of 8 threads, whatever OMP_NUM_THREADS says (as
    oracle/make_golden.py does)."""
    from oracle import diffusers_stub as ds

    torch.set_num_threads(8)
    from oracle import ref_loader

    ref_loader.install_stubs()
    sys.modules["colossalai.cluster.process_group_mesh"].ProcessGroupMesh = Mesh
    for k in [k for k in sys.modules if k == "diffusers" or k.startswith("diffusers.")]:
        del sys.modules[k]
    ds.install()
    m = importlib.import_module("videosys.models.transformers.vchitect_transformer_3d")
    return m, importlib.import_module("videosys.core.pab.pab_mgr")


def weights():
    from videosys_amd.vchitect import synth_state_dict

    sd = synth_state_dict(KWARGS["num_layers"], KWARGS["num_attention_heads"], joint_attention_dim=JD, pooled_projection_dim=PD, seed=SEED)
    return {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


def build(m, sd, dtype, manager=None):
    model = m.VchitectXLTransformerModel(**KWARGS)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and missing == ["pos_embed.pos_embed"], (missing, unexpected)
    model.parallel_manager = manager or SP1()
    for _, mod in model.named_modules():
        if hasattr(mod, "parallel_manager"):
            mod.parallel_manager = model.parallel_manager
    return model.eval().to(dtype)


def call(model, dtype, x, enc, pooled, t):
    B = x.shape[0]
    with torch.no_grad():
        return model(x.to(dtype), encoder_hidden_states=enc.to(dtype), pooled_projections=pooled.to(dtype),
                     timestep=torch.tensor([float(t)] * B), return_dict=False)[0].clone()


def reset_pab(m, model):
    for mod in model.modules():
        if isinstance(mod, m.VchitectAttention):
            mod.spatial_count = mod.temporal_count = mod.cross_count = 0
            mod.last_spatial = mod.last_temporal = mod.last_cross = None


def inputs():
    """bf16-exact inputs of every call, from one seeded generator (stored as bf16: half the bytes, the same values)."""
    g = torch.Generator().manual_seed(SEED + 1)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    cases = {n: dict(x=bf(B, F, 16, H, W), encoder_hidden_states=bf(B, L, JD), pooled=bf(B, PD), t=t) for n, (B, F, H, W, t) in CASES.items()}
    F, H, W = PAB_GEOMETRY
    # one latent per step, both rows of the CFG pair read it (torch.cat([latents] * 2)); the rows differ in text and pooled text
    pab = dict(x=bf(len(PAB_STEPS), F, 16, H, W), encoder_hidden_states=bf(2, L, JD), pooled=bf(2, PD), timesteps=list(PAB_STEPS), config=dict(PAB))
    return cases, pab


def decisions(pab_mgr):
    """(temporal, cross, spatial) of the eight calls from the reference's own functions, counters advancing once per CALL."""
    ct = cc = cs = 0
    out = []
    for t in PAB_STEPS:
        for _ in range(2):
            bt, ct = pab_mgr.if_broadcast_temporal(t, ct)
            bc, cc = pab_mgr.if_broadcast_cross(t, cc)
            bs, cs = pab_mgr.if_broadcast_spatial(t, cs)
            out.append((bt, bc, bs))
    return out


def mint_model(m, pab_mgr, sd):
    cases, pab = inputs()
    fwd = dict(meta=dict(seed=SEED, kwargs=dict(KWARGS), floor_bf16={}, floor_f32={}), cases=cases)
    pabf = dict(meta=dict(seed=SEED, kwargs=dict(KWARGS), floor_bf16=[], floor_f32=[]), **pab)
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32"), (torch.bfloat16, "bf16")):
        model = build(m, sd, dtype)
        if tag == "f64":
            fwd["meta"]["state_dict_shapes"] = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        if tag == "f32":
            fwd["pos_embed"] = model.state_dict()["pos_embed.pos_embed"].clone()       # the persistent buffer as a checkpoint holds it
        pab_mgr.PAB_MANAGER = None
        for n, c in cases.items():
            c["ref_" + tag] = call(model, dtype, c["x"], c["encoder_hidden_states"], c["pooled"], c["t"])
        rows = [(s, r) for s in range(len(PAB_STEPS)) for r in range(2)]
        one = lambda s, r: call(model, dtype, pab["x"][s:s + 1], pab["encoder_hidden_states"][r:r + 1], pab["pooled"][r:r + 1], PAB_STEPS[s])
        pabf["free_" + tag] = [one(s, r) for s, r in rows]
        pab_mgr.set_pab_manager(pab_mgr.PABConfig(**PAB))
        pab_mgr.update_steps(len(PAB_STEPS))           # what the pipeline sets: the counters of its 2 x steps calls wrap at `steps`
        if tag == "f64":
            pabf["decisions"] = decisions(pab_mgr)
        reset_pab(m, model)
        pabf["pab_" + tag] = [one(s, r) for s, r in rows]
        pab_mgr.PAB_MANAGER = None
        assert torch.equal(pabf["pab_" + tag][0], pabf["free_" + tag][0]), "the first PAB call differs from the PAB-free call"
    for n, c in cases.items():
        fwd["meta"]["floor_bf16"][n], fwd["meta"]["floor_f32"][n] = rms(c["ref_bf16"], c["ref_f64"]), rms(c["ref_f32"], c["ref_f64"])
    dec = pabf["decisions"]
    assert dec[0] == (False, False, False) and all(any(d[i] for d in dec) for i in range(3)), dec
    for i, d in enumerate(dec):
        fl = rms(pabf["pab_bf16"][i], pabf["pab_f64"][i])
        pabf["meta"]["floor_bf16"].append(fl)
        pabf["meta"]["floor_f32"].append(rms(pabf["pab_f32"][i], pabf["pab_f64"][i]))
        gap = rms(pabf["pab_f64"][i], pabf["free_f64"][i])
        print(f"[pab call {i}] decisions {d}, |pab - free| rms {gap:.4e}, bf16 floor {fl:.4e}, ratio {gap / fl:.1f}")
        if any(d):
            assert gap >= 4 * 1.5 * fl, f"call {i}: a stale branch moves the output by {gap:.3e} < 6 x the bf16 floor {fl:.3e}: change SEED"
        else:
            assert gap == 0.0
    for n in cases:
        print(f"[{n}] bf16 floor {fwd['meta']['floor_bf16'][n]:.4e}, f32 floor {fwd['meta']['floor_f32'][n]:.4e}")
    return fwd, pabf


def mint_layer(m, sd):
    """One reference JointTransformerBlock at B = 1, F = 3, S = 16, L = 4 on the inputs of vchitect_ref.layer_inputs(SEED); weights: the
    block-0 (context_pre_only False) and block-1 (True) entries of the model's state dict."""
    import vchitect_ref as vr

    hs, enc, temb = vr.layer_inputs(SEED)
    F = hs.shape[0]
    freqs = m.VchitectXLTransformerModel.precompute_freqs_cis(64, 64, theta=1e6)
    out = dict(meta=dict(seed=SEED, floor_bf16={}, floor_f32={}))
    for i, cpo in enumerate((False, True)):
        pre = f"transformer_blocks.{i}."
        bsd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        res = {}
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32"), (torch.bfloat16, "bf16")):
            blk = m.JointTransformerBlock(dim=192, num_attention_heads=3, attention_head_dim=192, context_pre_only=cpo)
            blk.load_state_dict(bsd, strict=True)
            blk.attn.parallel_manager = SP1()
            blk = blk.eval().to(dtype)
            seen = []
            blk.attn.register_forward_hook(lambda mod, a, o: seen.append(o))
            with torch.no_grad():
                y, x = blk(hidden_states=hs.to(dtype), encoder_hidden_states=enc.to(dtype), temb=temb.to(dtype), freqs_cis=freqs, full_seqlen=F,
                           Frame=F, timestep=None)
            assert (y is None) == cpo
            res["x_" + tag] = x.clone()
            if y is not None:
                res["y_" + tag] = y.clone()
            if tag != "bf16":
                res["attn_x_" + tag], res["attn_y_" + tag] = seen[0][0].clone(), seen[0][1].clone()
        for t in ("x", "y", "attn_x", "attn_y"):
            if t + "_f64" in res:
                res[t + "_f32_floor"] = rms(res.pop(t + "_f32"), res[t + "_f64"])       # only the floor of the fp32 run is kept
                if t + "_bf16" in res:
                    res[t + "_bf16_floor"] = rms(res[t + "_bf16"], res[t + "_f64"])
        out["context_pre_only" if cpo else "joint"] = res
    return out


# ------------------------------------------------------------------------------------------------ sp_size = 2 over gloo
def sp_inputs():
    g = torch.Generator().manual_seed(SEED + 3)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    c = SP_CASE
    return dict(x=bf(1, c["F"], 16, c["HW"], c["HW"]), encoder_hidden_states=bf(1, c["L"], JD), pooled=bf(1, PD), t=c["t"])


def _sp_worker(rank, world, port, ret):
    try:
        import torch.distributed as dist

        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)

        def list_all_to_all(outs, ins, group=None):     # gloo has no list all-to-all: the one collective of _all_to_all_func
            send = torch.stack(ins)
            recv = torch.empty_like(send)
            dist.all_to_all_single(recv, send, group=group)
            for o, r in zip(outs, recv.unbind(0)):
                o.copy_(r)

        dist.all_to_all = list_all_to_all
        m, pab_mgr = reference_modules()
        pab_mgr.PAB_MANAGER = None
        # the reference's all-gather asserts a CUDA tensor (comm.py:181).  Only the FINAL gather of the local frames goes through it
        # (:561-562, after the last block): it is served by this project's function of the same signature, which tests/test_host_cpu.py
        # holds equal to the reference's on recorded traces; the ranks' local outputs are stored beside it, untouched by the swap
        from videosys_amd import comm as own_comm

        importlib.import_module("videosys.core.distributed.comm")._gather_sequence_func = own_comm._gather_sequence_func
        pm = importlib.import_module("videosys.core.distributed.parallel_mgr")
        c, sd, got = sp_inputs(), weights(), {}
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32"), (torch.bfloat16, "bf16")):
            model = build(m, sd, dtype)
            model.enable_parallel(1, world, False)
            assert isinstance(model.parallel_manager, pm.ParallelManager) and model.parallel_manager.sp_size == world
            seen = []
            model.transformer_blocks[-1].register_forward_hook(lambda mod, a, o: seen.append(o[1].clone()))
            got["ref_" + tag] = call(model, dtype, c["x"], c["encoder_hidden_states"], c["pooled"], c["t"])
            got["local_" + tag] = seen[0]
        ret.put((rank, "ok", got))
        dist.barrier()
    except Exception:  # noqa
        import traceback

        ret.put((rank, traceback.format_exc(), None))
    finally:
        import torch.distributed as dist

        if dist.is_initialized():
            dist.destroy_process_group()


def mint_sp(m, sd):
    """The reference with sp_size = 2 in two gloo processes (its ParallelManager, set_pad / split_from_second_dim, all_to_all_with_pad),
    float64: F = 3 (temporal pad 1), S + L = 64 + 7 = 71 (spatial pad 1).  Stored: every rank's local hidden states after the last block
    (frames [r Fl, (r + 1) Fl), the padded frame included), the gathered prediction in float64 and bfloat16 (asserted equal on both
    ranks; the floors are the sharded class's own: bf16 and fp32 runs of the same two processes), and the float64 prediction of the same
    call with sp_size = 1 (the two differ: a rank's cross keys are row 0 of ITS shard)."""
    import socket

    import torch.multiprocessing as mp

    P = SP_CASE["P"]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    procs = [ctx.Process(target=_sp_worker, args=(r, P, port, ret)) for r in range(P)]
    for p in procs:
        p.start()
    res = sorted((ret.get(timeout=120) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for rank, status, _ in res:
        assert status == "ok", f"rank {rank}: {status}"
    got = [{k: v.clone() for k, v in r[2].items()} for r in res]
    for tag in ("f64", "f32", "bf16"):
        assert all(torch.equal(got[0]["ref_" + tag], g["ref_" + tag]) for g in got[1:]), "the ranks' gathered predictions differ"
    c = sp_inputs()
    fx = dict(meta=dict(seed=SEED, kwargs=dict(KWARGS), **SP_CASE), **c, ref_f64=got[0]["ref_f64"], ref_bf16=got[0]["ref_bf16"],
              local_hidden_f64=[g["local_f64"] for g in got])
    fx["single_f64"] = call(build(m, sd, torch.float64), torch.float64, c["x"], c["encoder_hidden_states"], c["pooled"], c["t"])
    fx["meta"]["floor_bf16"], fx["meta"]["floor_f32"] = rms(fx["ref_bf16"], fx["ref_f64"]), rms(got[0]["ref_f32"], fx["ref_f64"])
    print(f"[sp] sharded vs single f64 rms {rms(fx['ref_f64'], fx['single_f64']):.4e}, bf16 floor {fx['meta']['floor_bf16']:.4e}, "
          f"f32 floor {fx['meta']['floor_f32']:.4e}")
    return fx


def mint(parts=("fwd", "pab", "layer", "sp")):
    m, pab_mgr = reference_modules()
    sd = weights()
    out = {}
    if "fwd" in parts or "pab" in parts:
        out[FWD], out[PABF] = mint_model(m, pab_mgr, sd)
    if "layer" in parts:
        out[LAYER] = mint_layer(m, sd)
    if "sp" in parts:
        out[SPF] = mint_sp(m, sd)
    return out


def same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    return a == b


def main():
    fxs = mint()
    if "--check" in sys.argv:
        stale = [p for p, fx in fxs.items() if not same(fx, torch.load(p, weights_only=True))]
        if stale:
            print("stale:", *stale)
            sys.exit(1)
        print("fixture matches")
        return
    for p, fx in fxs.items():
        torch.save(fx, p)
        print("wrote", os.path.relpath(p, ROOT), os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
