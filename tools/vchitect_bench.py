#!/usr/bin/env python
"""Time the two halves of a Vchitect-2.0 video at the pipeline's defaults (288 x 480, 40 frames -> latent 36 x 60) on random weights:

  decode   AutoencoderKLSD3Decoder.decode_u8 of 40 frames (vae_sd3.py: the two end kernels + the 2-D decoder)
  step     one denoise step at the 2B geometry (18 layers, 18 heads x 64, L = 77 + 256 text tokens): the recorded pair of model calls
           (uncond, text) + the guidance / Euler launch, as VchitectXLPipeline issues it

    python tools/vchitect_bench.py [--reps 5] [--out FILE.json] [--skip-step] [--skip-decode]

Prints one JSON line; device time from HIP events around ``reps`` repetitions after one warm-up.

    python tools/vchitect_bench.py --ranks 8 [--reps 20] [--out FILE.json]

times the same step as ONE rank (rank 0) of an N-way sequence-parallel group with the wire stubbed (tools/local_group.StubGroup: a
collective is a device copy of the rank's own send buffer, so the results are meaningless and the time is the rank's own work):
the recorded step of every route — "rows" (unpack, old kernel, pack) and "image" (vsys_attn_temporal_d64_img on the exchange image)
over all_to_all_single, "p2p_rows" over the one-kernel exchange — and of the single-rank model in the same run, replayed in turn;
per route the median of ``reps`` replays, each timed on the host between two stream synchronisations, and the launch count.

    python tools/vchitect_bench.py --shard-decode 2 4 8 [--reps 7] [--out profiles/vchitect_decode_shard_timing.json]

times rank 0's share of ``decode_u8(latents, group=)`` for every P (its ceil(F / P) frames + the zeroed piece, the all-gather stubbed
by StubGroup — one device copy of the piece per rank — and the trim), the same frames decoded WITHOUT a group (what is left is the
replicated tail) and the unsharded decode, in turn in one process; medians of ``reps`` repetitions on the host clock between stream
synchronisations.  No multi-GPU run: the wire is not in these numbers."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--ranks", type=int, default=0, help="time one rank of an N-way sequence-parallel group, wire stubbed")
    ap.add_argument("--shard-decode", type=int, nargs="+", default=None, metavar="P",
                    help="time rank 0's share of the VAE decode sharded over P ranks (gather stubbed) against the unsharded decode")
    args = ap.parse_args()
    if args.ranks:
        return ranks_main(args)
    if args.shard_decode:
        return shard_decode_main(args)
    dev = torch.device("cuda:0")
    F, h, w = 40, 36, 60
    res = {"device": torch.cuda.get_device_name(0), "frames": F, "latent": [h, w], "reps": args.reps}
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, F, 16, h, w, generator=g).to(dev)
    if not args.skip_decode:
        from videosys_amd import vae_sd3

        dec = vae_sd3.AutoencoderKLSD3Decoder(vae_sd3.synth_state_dict(0), device=dev)
        res["decode_ms_40f_288x480"] = round(timed(lambda: dec.decode_u8(lat), args.reps), 3)
        res["frames_per_launch"] = dec.frames_per_launch
        del dec
        torch.cuda.empty_cache()
    if not args.skip_step:
        from videosys_amd import VchitectConfig, VchitectXLPipeline, pab

        pipe = VchitectXLPipeline(VchitectConfig("Vchitect/Vchitect-2.0-2B", transformer_config=dict(
            num_layers=18, num_attention_heads=18, attention_head_dim=64, caption_projection_dim=1152, joint_attention_dim=4096,
            pooled_projection_dim=2048)), vae=None)
        pab.set_pab_manager(None)
        L = 77 + 256
        emb = torch.randn(2, L, 4096, generator=g).to(torch.bfloat16)
        pooled = torch.randn(2, 2048, generator=g).to(torch.bfloat16)
        z, enc, pl, pred = pipe._step_buffers(lat, emb, pooled)

        def step():
            pipe._issue_pair(z, enc, pl, pred, 500.0)
            from videosys_amd import ops

            ops.cfg_euler_step(z, pred, 4.0, -1e-4)

        res["step_ms_2b_40f_36x60"] = round(timed(step, args.reps), 3)
        res["step_stats"] = dict(pipe.step_stats)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def ranks_main(args):
    import statistics
    import time
    from types import SimpleNamespace

    from tools.local_group import StubGroup
    from videosys_amd import VchitectConfig, VchitectXLPipeline, ops, pab

    dev, P = torch.device("cuda:0"), args.ranks
    F, h, w, L = 40, 36, 60, 77 + 256
    reps = max(args.reps, 20)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, F, 16, h, w, generator=g).to(dev)
    pipe = VchitectXLPipeline(VchitectConfig("Vchitect/Vchitect-2.0-2B", transformer_config=dict(
        num_layers=18, num_attention_heads=18, attention_head_dim=64, caption_projection_dim=1152, joint_attention_dim=4096,
        pooled_projection_dim=2048)), vae=None)
    pab.set_pab_manager(None)
    emb = torch.randn(2, L, 4096, generator=g).to(torch.bfloat16)
    pooled = torch.randn(2, 2048, generator=g).to(torch.bfloat16)
    z, enc, pl, pred = pipe._step_buffers(lat, emb, pooled)
    tr = pipe.transformer

    def step():
        pipe._issue_pair(z, enc, pl, pred, 500.0)
        ops.cfg_euler_step(z, pred, 4.0, -1e-4)

    mgr = SimpleNamespace(sp_size=P, cp_size=1, dp_size=1, dp_rank=0, sp_rank=0, cp_rank=0, sp_group=StubGroup(P, 0), cp_group=None)
    programs, info = {}, {}
    for name in ("single", "rows", "image", "p2p_rows"):
        if name == "single":
            tr.enable_parallel(1, 1, False)
        else:
            pipe._set_parallel(parallel_mgr=mgr)
            if name != "p2p_rows":
                tr._sp.p2p = None
            for b in tr.transformer_blocks:
                b.attn.attn_route = "image" if name == "image" else "rows"
        pipe._steps.clear()
        step()                                  # records the pair of model calls
        step()                                  # first replay
        torch.cuda.synchronize()
        programs[name] = pipe._steps.entries    # (clear() starts a new table: this one keeps its program)
        assert len(pipe._steps) == 1, f"the {name} step was not recordable"
        (prog, _), = pipe._steps.entries.values()
        # launches: the recorded ones + the guidance / Euler launch + what host actions launch themselves (the image route's attention,
        # one per block and model call, has no op code and is issued by the closure of the collective it feeds)
        closure_launches = 2 * len(tr.transformer_blocks) if name == "image" else 0
        info[name] = {"launches_per_step": prog.n_launches + 1 + closure_launches,
                      "of_which_issued_by_host_actions": closure_launches,
                      "host_actions_per_step": sum(1 for seg in prog.segments if not isinstance(seg, tuple))}
    times = {name: [] for name in programs}
    for _ in range(reps):                       # the routes in turn, so that drift hits them alike
        for name, ent in programs.items():
            pipe._steps.entries = ent
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    res = {"device": torch.cuda.get_device_name(0), "ranks": P, "rank": 0, "frames": F, "latent": [h, w], "text_tokens": L, "replays": reps,
           "what": "wire stubbed, random weights; per-rank step (two model calls + guidance) in ms, median of the replays; a collective of the "
                   "stub is one device copy and is not counted as a launch"}
    for name, ts in times.items():
        info[name].update(step_ms_median=round(statistics.median(ts), 3), step_ms_min=round(min(ts), 3), step_ms_max=round(max(ts), 3))
    res["routes"] = info
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def shard_decode_main(args):
    import statistics
    import time

    from tools.local_group import StubGroup
    from videosys_amd import vae_sd3
    from videosys_amd.vae_blocks import frame_shards

    dev = torch.device("cuda:0")
    F, h, w = 40, 36, 60
    reps = max(args.reps, 5)
    lat = torch.randn(1, F, 16, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    dec = vae_sd3.AutoencoderKLSD3Decoder(vae_sd3.synth_state_dict(0), device=dev)
    cases = {"unsharded": lambda: dec.decode_u8(lat)}
    for P in args.shard_decode:
        f0, f1 = frame_shards(F, P)[0]
        grp, mine = StubGroup(P, 0), lat[:, f0:f1].contiguous()
        cases[f"rank0_of_{P}"] = lambda grp=grp: dec.decode_u8(lat, group=grp)
        cases[f"frames_of_rank0_of_{P}"] = lambda mine=mine: dec.decode_u8(mine)
    times = {k: [] for k in cases}
    for fn in cases.values():
        fn()
    for _ in range(reps):                       # in turn, so that drift hits them alike
        for k, fn in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"device": torch.cuda.get_device_name(0), "frames": F, "latent": [h, w], "frames_per_launch": dec.frames_per_launch, "reps": reps,
           "what": "AutoencoderKLSD3Decoder.decode_u8, random weights; rank 0 of P with the all-gather STUBBED (tools/local_group.StubGroup: "
                   "a device copy of the rank's own piece per rank; no multi-GPU run exists, the wire is not in these numbers); ms, median "
                   "(min, max) of the repetitions, host clock between stream synchronisations, the cases in turn in one process",
           "unsharded_ms": [round(med["unsharded"], 3), round(min(times["unsharded"]), 3), round(max(times["unsharded"]), 3)], "ranks": {}}
    for P in args.shard_decode:
        t, own = times[f"rank0_of_{P}"], med[f"frames_of_rank0_of_{P}"]
        per = -(-F // P)
        res["ranks"][str(P)] = {"frames_of_rank0": per, "rank0_ms": [round(med[f"rank0_of_{P}"], 3), round(min(t), 3), round(max(t), 3)],
                                "its_frames_alone_ms": round(own, 3), "expected_ms_unsharded_x_share": round(med["unsharded"] * per / F, 3),
                                "unsharded_over_rank0": round(med["unsharded"] / med[f"rank0_of_{P}"], 3), "ideal_ratio": round(F / per, 3),
                                "tail_ms": round(med[f"rank0_of_{P}"] - own, 3),
                                "tail_share_of_rank0": round((med[f"rank0_of_{P}"] - own) / med[f"rank0_of_{P}"], 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
