#!/usr/bin/env python
"""Time the pieces of an Open-Sora-Plan v1.2 video that this build adds around the transformer, at the 29x480p geometry (29 frames of
480 x 640 -> latent 8 x 60 x 80) on random weights:

  decode     CausalVAEModelWrapper.decode of the latent at hidden_size 128: tiled as the pipeline sets it up (tile_latent_min_size 64,
             tile_latent_min_size_t 8, overlap 0.25: four spatial tiles, one temporal chunk) and untiled
  step       one denoise step: the recorded CFG model call (32 layers, 24 heads x 96, 512 text tokens) + the ancestral launch, as
             OpenSoraPlanPipeline issues it
  upsample   vsys_upsample_trilinear2x at the decoder's two call sites of the untiled decode (C = 512: 8 x 60 x 80 -> 15 x 120 x 160,
             then 15 x 120 x 160 -> 29 x 240 x 320), with vsys_regrid(up=1) moving the SAME destination bytes in the same run as the
             yardstick (a nearest 2x copy into the same padded grid), alternating; the ratio per destination byte is recorded

    python tools/osp_pipeline_bench.py [--reps 7] [--out profiles/osp_pipeline_timing.json] [--skip-step] [--skip-decode]

Prints one JSON line.  Every figure is the median of ``reps`` repetitions, each timed on the host between two stream
synchronisations, after one warm-up of the same shape.

    python tools/osp_pipeline_bench.py --shard 2 4 8 [--reps 5] [--out profiles/osp_decode_shard_timing.json]

times, at 29x480p and 93x480p, OpenSoraPlanPipeline.decode_latents (tiled decode + the uint8 pass + the copy to the host) as rank 0 of
a P-way group for every P — its units of the deal, the zeroed gather buffer, the all-gather stubbed by tools/local_group.StubGroup (one
device copy of the buffer per rank), crop, stitch, uint8 — against the unsharded decode_latents and against rank 0's units decoded
alone (what is left of rank 0's time is the replicated tail), in turn in one process.  No multi-GPU run: the wire is not in these
numbers."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)


def upsample_sites(dev, reps):
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd import ops
    from videosys_amd.ops import VaeGrid

    out = []
    for C, T, H, W in ((512, 8, 60, 80), (512, 15, 120, 160)):
        gs = VaeGrid(1, T, H, W, 1, 0)
        gd = VaeGrid(1, 2 * T - 1, 2 * H, 2 * W, 1, 2)
        gn = VaeGrid(1, 2 * T - 1, H, W, 1, 0)           # the regrid yardstick: as many source frames as destination frames
        x = torch.randn(gs.rows, C, device=dev).to(torch.bfloat16)
        xn = torch.randn(gn.rows, C, device=dev).to(torch.bfloat16)
        y = gd.alloc(C, dev, zero=True)[1]
        tri, reg = [], []
        oops.upsample_trilinear2x(x, gs, y, gd, C)
        ops.regrid(xn, gn, y, gd, C, up=1)
        for _ in range(reps):                            # alternating, so that drift hits both alike
            for fn, acc in ((lambda: oops.upsample_trilinear2x(x, gs, y, gd, C), tri), (lambda: ops.regrid(xn, gn, y, gd, C, up=1), reg)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        dst_bytes = (2 * T - 1) * 4 * H * W * C * 2
        a, b = statistics.median(tri), statistics.median(reg)
        out.append({"C": C, "source": [T, H, W], "destination_bytes": dst_bytes, "trilinear_ms": round(a, 3), "regrid_up1_ms": round(b, 3),
                    "trilinear_gb_per_s_of_destination": round(dst_bytes / a / 1e6, 1), "ratio_per_destination_byte": round(a / b, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--shard", type=int, nargs="+", default=None, metavar="P",
                    help="time rank 0's share of the tiled decode sharded over P ranks (gather stubbed) against the unsharded decode")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    if args.shard:
        return shard_main(args, dev)
    T, h, w = 8, 60, 80
    res = {"device": torch.cuda.get_device_name(0), "geometry": "29x480p", "latent": [T, h, w], "reps": args.reps,
           "what": "random weights; median (min, max) of the repetitions in ms, host clock between stream synchronisations"}
    g = torch.Generator().manual_seed(0)
    lat = (torch.randn(1, 4, T, h, w, generator=g) * 0.18215).to(dev)
    res["upsample_trilinear2x"] = upsample_sites(dev, max(args.reps, 11))
    if not args.skip_decode:
        from videosys_amd.vae_open_sora_plan import CausalVAEModelWrapper

        vae = CausalVAEModelWrapper("synthetic:0", device=dev, hidden_size=128)
        res["decode_untiled_ms_29f_480x640"] = median_ms(lambda: vae.decode(lat), args.reps)
        v = vae.vae                                      # the pipeline's setting (OpenSoraPlanPipeline.__init__)
        v.enable_tiling()
        v.tile_overlap_factor, v.tile_sample_min_size, v.tile_latent_min_size = 0.25, 512, 64
        v.tile_sample_min_size_t, v.tile_latent_min_size_t = 29, 8
        res["decode_tiled_ms_29f_480x640"] = median_ms(lambda: vae.decode(lat), args.reps)
        res["decoded_shape"] = list(vae.decode(lat).shape)
        del vae
        torch.cuda.empty_cache()
    if not args.skip_step:
        from videosys_amd import open_sora_plan_ops as oops
        from videosys_amd import pab
        from videosys_amd.pipeline_open_sora_plan import OpenSoraPlanConfig, OpenSoraPlanPipeline

        from tools.osp_bench import random_state_dict
        from videosys_amd.open_sora_plan import OpenSoraT2V
        from videosys_amd.pipeline_open_sora_plan import _V120_GEOMETRY

        model = OpenSoraT2V(**_V120_GEOMETRY["29x480p"], device=dev)     # (weights drawn on the device: 2.7 G values)
        model.load_state_dict(random_state_dict(model, dev))
        pipe = OpenSoraPlanPipeline(OpenSoraPlanConfig(transformer_type="29x480p"), transformer=model, device=dev)
        pab.set_pab_manager(None)
        L = 512
        enc = torch.randn(2, 1, L, 4096, generator=g).to(torch.bfloat16).to(dev)
        mask = torch.zeros(2, 1, L, dtype=torch.int64)
        mask[0, 0, :1], mask[1, 0, :40] = 1, 1
        b = pipe._buffers(lat * 100.0, enc, mask.to(dev))
        pipe.transformer._encode_text(b["enc"], b["mask"])
        b["model_in"].copy_((b["z"] * 0.01).to(torch.bfloat16).repeat(2, 1, 1, 1, 1))
        noise = torch.randn(b["z"].shape, device=dev)

        def step():
            b["xin"].copy_(b["model_in"])
            pred = pipe._issue_model(b["xin"], 500.0, b["enc"], b["mask"])
            oops.cfg_ancestral_step(b["z"], pred, noise, b["model_in"], 7.5, -1e-3, 1e-3, 0.01)

        res["step_ms_29x480p_512_text_tokens"] = median_ms(step, args.reps)
        res["step_stats"] = dict(pipe.step_stats)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def shard_main(args, dev):
    from types import SimpleNamespace

    from tools.local_group import StubGroup
    from videosys_amd.pipeline_open_sora_plan import _V120_GEOMETRY, OpenSoraPlanPipeline
    from videosys_amd.vae_blocks import deal_units
    from videosys_amd.vae_open_sora_plan import SCALE, CausalVAEModelWrapper

    vae = CausalVAEModelWrapper("synthetic:0", device=dev, hidden_size=128)
    v = vae.vae                                          # the pipeline's setting (OpenSoraPlanPipeline.__init__)
    v.enable_tiling()
    v.tile_overlap_factor, v.tile_sample_min_size, v.tile_latent_min_size = 0.25, 512, 64
    v.tile_sample_min_size_t, v.tile_latent_min_size_t = 29, 8
    lat_t = v.tile_latent_min_size

    def pipeline(group):
        """decode_latents as a rank of ``group`` runs it: the method of the pipeline class on the parts it reads."""
        p = OpenSoraPlanPipeline.__new__(OpenSoraPlanPipeline)
        p.vae, p._config = vae, SimpleNamespace(shard_vae_decode=True)
        p.transformer = SimpleNamespace(_sp=None if group is None else SimpleNamespace(P=group.size, group=group))
        return p

    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "geometries": {},
           "what": "OpenSoraPlanPipeline.decode_latents (tiled CausalVAE decode at hidden_size 128 + uint8 pass + copy to the host), random "
                   "weights; rank 0 of P with the all-gather STUBBED (tools/local_group.StubGroup: a device copy of the rank's own buffer "
                   "per rank; no multi-GPU run exists, the wire is not in these numbers); ms, median (min, max) of the repetitions, host "
                   "clock between stream synchronisations, the cases in turn in one process"}
    for name in ("29x480p", "93x480p"):
        geo = _V120_GEOMETRY[name]
        T, (h, w) = geo["sample_size_t"], geo["sample_size"]
        lat = (torch.randn(1, 4, T, h, w, generator=torch.Generator().manual_seed(0)) * SCALE).to(dev)
        zb = lat[0].to(torch.bfloat16)
        units, costs = v.tile_units(1, T, h, w)
        cases = {"unsharded": lambda p=pipeline(None): p.decode_latents(lat)}
        balance = {}
        for P in args.shard:
            owner, _, _ = deal_units(costs, P)
            mine = [units[u] for u in range(len(units)) if owner[u] == 0]
            balance[P] = sum(costs) / max(sum(c for c, o in zip(costs, owner) if o == r) for r in range(P))
            cases[f"rank0_of_{P}"] = lambda p=pipeline(StubGroup(P, 0)): p.decode_latents(lat)
            cases[f"units_of_rank0_of_{P}"] = lambda mine=mine: [
                v._decode_tile(zb[:, t0:t1, i:i + lat_t, j:j + lat_t].contiguous(), 1.0 / SCALE) for _, (t0, t1), i, j in mine]
        times = {k: [] for k in cases}
        for fn in cases.values():
            fn()
        for _ in range(args.reps):                       # in turn, so that drift hits them alike
            for k, fn in cases.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(ts) for k, ts in times.items()}
        tri = lambda k: [round(med[k], 3), round(min(times[k]), 3), round(max(times[k]), 3)]
        out = {"latent": [T, h, w], "units": len(units), "unsharded_ms": tri("unsharded"), "ranks": {}}
        for P in args.shard:
            r0, own = med[f"rank0_of_{P}"], med[f"units_of_rank0_of_{P}"]
            out["ranks"][str(P)] = {"rank0_ms": tri(f"rank0_of_{P}"), "its_units_alone_ms": round(own, 3),
                                    "balance_of_the_deal": round(balance[P], 2), "expected_ms_unsharded_over_balance": round(med["unsharded"] / balance[P], 3),
                                    "unsharded_over_rank0": round(med["unsharded"] / r0, 3), "tail_ms": round(r0 - own, 3),
                                    "tail_share_of_rank0": round((r0 - own) / r0, 4)}
        res["geometries"][name] = out
        v.clear_cache()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
