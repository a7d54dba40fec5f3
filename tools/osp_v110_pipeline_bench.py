#!/usr/bin/env python
"""Time the pieces of an Open-Sora-Plan v1.1 video that this build adds around the transformer, at the 65x512x512 geometry (65 frames of
512 x 512 -> latent 17 x 64 x 64) on random weights:

  step       one sampler call as OpenSoraPlanV110Pipeline issues it — the replayed CFG model call (28 + 28 blocks, 16 heads x 72, 300
             text keys, the geometry of tools/osp_v110_bench.py) + the copy of the bf16 model input + ONE vsys_cfg_pndm_step launch in
             its multistep form — the replayed model call alone, and the bare transformer call recorded and replayed the way
             tools/osp_v110_bench.py does it (the parent's yardstick), in turn in one run
  decode     CausalVAEModelWrapper.decode (v1.1: SpatialUpsample2x + TimeUpsampleRes2x) of the latent at hidden_size 128, untiled and
             tiled as the pipeline sets it up (tile_latent_min_size 64, tile_latent_min_size_t 8, overlap 0.25)
  pndm       vsys_cfg_pndm_step in its multistep form (reads the two CFG halves, the sample and three history entries; writes the
             history slot, the sample and both bf16 halves) beside vsys_cfg_ancestral_step at the same element count, alternating in one
             run: a single launch between two synchronisations (launch + synchronise latency, not the kernel), and 200 launches back
             to back divided by 200 with the bytes/s of each over ITS OWN traffic (an upper bound of the kernel's time: the host's
             issue rate still bounds it, and the few MB of operands stay in the last-level cache)
  time2x     vsys_upsample_time2x with the residual destination at the decoder's two call sites (C = 512: 17 x 128 x 128 -> 33, then
             33 x 256 x 256 -> 65 frames) beside a plain vsys_regrid copy into the SAME destination grid, alternating; per destination
             byte (time2x also writes the residual destination: its own bytes/s counts both)

    python tools/osp_v110_pipeline_bench.py [--reps 7] [--out profiles/osp_v110_pipeline_timing.json] [--skip-step] [--skip-decode]

Prints one JSON line.  Every figure is the median (min, max) of its section's repetitions (``--reps`` for the step, at most 3 for the
decode, at least 21 / 11 for the two kernels; each section records its own), each timed on the host between two stream
synchronisations, after one warm-up of the same shape."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


BATCH = 200


def in_turn(fns, reps):
    """{name: [median, min, max] ms}: one warm-up each, then the functions in turn ``reps`` times, so that drift hits them alike."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}


def pndm_vs_ancestral(dev, reps, shape=(1, 4, 17, 64, 64)):
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd.pipeline_open_sora_plan_v110 import PNDMScheduler

    s = PNDMScheduler()
    s.set_timesteps(50)
    k = s.step_coeffs(12)
    r = lambda *sh: torch.randn(*sh, device=dev)
    n = 1
    for v in shape:
        n *= v
    two = (2 * shape[0], 2 * shape[1]) + shape[2:]
    mo, z, h, e, noise = r(*two), r(*shape), [r(*shape) for _ in range(3)], r(*shape), r(*shape)
    mi = torch.empty((2 * shape[0],) + shape[1:], dtype=torch.bfloat16, device=dev)
    pndm = lambda: vops.cfg_pndm_step(mo, mi, z, 7.5, 1.0, [1e-3 * c for c in k["cz"]], None, base=z, srcs=h, e_out=e)
    anc = lambda: oops.cfg_ancestral_step(z, mo, noise, mi, 7.5, -1e-3, 1e-3, 0.5)
    # ONE launch between two synchronisations is launch + synchronise latency, not the kernel; BATCH launches back to back on the
    # stream between two synchronisations, divided by BATCH, approach the kernel's own time (the launches queue behind each other)
    batch = lambda fn: (lambda: [fn() for _ in range(BATCH)])
    t = in_turn({"pndm": pndm, "ancestral": anc}, reps)
    tb = in_turn({"pndm": batch(pndm), "ancestral": batch(anc)}, reps)
    bytes_pndm = n * (4 * (2 + 1 + 3) + 4 * 2 + 2 * 2)        # reads: two halves, z, three history; writes: e, z, two bf16 halves
    bytes_anc = n * (4 * (2 + 1 + 1) + 4 + 2 * 2)             # reads: two halves, z, noise; writes: z, two bf16 halves
    per = lambda v: [round(x / BATCH, 5) for x in v]
    return {"elements": n, "reps": reps, "single_launch_pndm_plms_ms": t["pndm"], "single_launch_ancestral_ms": t["ancestral"],
            "single_launch_note": "one launch between two synchronisations: launch + synchronise latency, NOT the kernel's rate",
            "batch": BATCH, "per_launch_in_batch_pndm_plms_ms": per(tb["pndm"]), "per_launch_in_batch_ancestral_ms": per(tb["ancestral"]),
            "pndm_bytes": bytes_pndm, "ancestral_bytes": bytes_anc,
            "pndm_gb_per_s_in_batch": round(bytes_pndm / (tb["pndm"][0] / BATCH) / 1e6, 1),
            "ancestral_gb_per_s_in_batch": round(bytes_anc / (tb["ancestral"][0] / BATCH) / 1e6, 1),
            "batch_note": "back-to-back launches: still bounded below by the host's issue rate per launch (ctypes call), so an upper bound "
                          "of the kernel's time; the operands (10 MB / 6.7 MB) stay in the 256 MB last-level cache between launches"}


def time2x_sites(dev, reps):
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd import ops
    from videosys_amd.ops import VaeGrid

    out = []
    for C, T, H, W in ((512, 17, 128, 128), (512, 33, 256, 256)):
        T2 = 2 * T - 1
        gs, gd, gr = VaeGrid(1, T, H, W, 1, 0), VaeGrid(1, T2, H, W, 1, 2), VaeGrid(1, T2, H, W, 1, 0)
        gn = VaeGrid(1, T2, H, W, 1, 0)                  # the regrid yardstick: a plain copy of as many frames as it writes
        x = torch.randn(gs.rows, C, device=dev).to(torch.bfloat16)
        y = gd.alloc(C, dev, zero=True)[1]
        y2 = torch.empty(gr.rows, C, dtype=torch.bfloat16, device=dev)
        xn = torch.randn(gn.rows, C, device=dev).to(torch.bfloat16)
        t = in_turn({"time2x_res": lambda: vops.upsample_time2x(x, gs, y, gd, C, y2, gr, 0.8),
                     "time2x": lambda: vops.upsample_time2x(x, gs, y, gd, C),
                     "regrid": lambda: ops.regrid(xn, gn, y, gd, C, up=0, tmode=0)}, reps)
        dst = T2 * H * W * C * 2
        out.append({"C": C, "source": [T, H, W], "reps": reps, "destination_bytes": dst, "time2x_res_ms": t["time2x_res"], "time2x_ms": t["time2x"],
                    "regrid_copy_ms": t["regrid"], "time2x_gb_per_s_of_destination": round(dst / t["time2x"][0] / 1e6, 1),
                    "time2x_res_gb_per_s_of_both_destinations": round(2 * dst / t["time2x_res"][0] / 1e6, 1),
                    "regrid_gb_per_s_of_destination": round(dst / t["regrid"][0] / 1e6, 1),
                    "ratio_per_destination_byte": round(t["time2x"][0] / t["regrid"][0], 3),
                    "ratio_per_destination_byte_with_residual": round(t["time2x_res"][0] / 2 / t["regrid"][0], 3)})
        del x, y, y2, xn
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-decode", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda:0")
    T, h, w = 17, 64, 64
    import socket

    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "geometry": "65x512x512", "latent": [T, h, w],
           "reps": f"{args.reps} for the step; each other section states its own",
           "what": "random weights; [median, min, max] of the repetitions in ms, host clock between stream synchronisations, cases in turn"}
    g = torch.Generator().manual_seed(0)
    lat = (torch.randn(1, 4, T, h, w, generator=g) * 0.18215).to(dev)
    res["cfg_pndm_step"] = pndm_vs_ancestral(dev, max(args.reps, 21))
    res["upsample_time2x"] = time2x_sites(dev, max(args.reps, 11))

    def flush():
        line = json.dumps(res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return line

    flush()
    if not args.skip_decode:
        from videosys_amd.vae_open_sora_plan_v110 import CausalVAEModelWrapper

        vae = CausalVAEModelWrapper("synthetic:0", device=dev, hidden_size=128)
        res["decode_reps"] = min(args.reps, 3)
        res["decode_untiled_ms_65f_512x512"] = in_turn({"d": lambda: vae.decode(lat)}, min(args.reps, 3))["d"]
        v = vae.vae                                      # the pipeline's setting (OpenSoraPlanV110Pipeline.__init__)
        v.enable_tiling()
        v.tile_overlap_factor, v.tile_sample_min_size, v.tile_latent_min_size = 0.25, 512, 64
        v.tile_sample_min_size_t, v.tile_latent_min_size_t = 29, 8
        res["decode_tiled_ms_65f_512x512"] = in_turn({"d": lambda: vae.decode(lat)}, min(args.reps, 3))["d"]
        res["decoded_shape"] = list(vae.decode(lat).shape)
        del vae
        torch.cuda.empty_cache()
        flush()
    if not args.skip_step:
        from osp_v110_bench import random_state_dict
        from videosys_amd import open_sora_plan_v110_ops as vops
        from videosys_amd import pab
        from videosys_amd.open_sora_plan_v110 import LatteT2V
        from videosys_amd.pipeline_open_sora_plan_v110 import _V110_GEOMETRY, OpenSoraPlanV110Config, OpenSoraPlanV110Pipeline

        model = LatteT2V(**_V110_GEOMETRY["65x512x512"], device=dev)
        model.load_state_dict(random_state_dict(model, 4096, dev))
        pipe = OpenSoraPlanV110Pipeline(OpenSoraPlanV110Config(), transformer=model, device=dev)
        pab.set_pab_manager(None)
        enc = torch.randn(2, 1, 300, 4096, generator=g).to(torch.bfloat16).to(dev)
        b = pipe._buffers(lat / 0.18215, enc)
        z = b["z"][0]
        b["model_in"].copy_(z.to(torch.bfloat16).repeat(2, 1, 1, 1, 1))
        pipe.scheduler.set_timesteps(50)
        k = pipe.scheduler.step_coeffs(12)
        ts = pipe.scheduler.timesteps

        def model_only():
            return pipe._issue_model(b["xin"], 500, b["enc"], ts)

        def step():
            b["xin"].copy_(b["model_in"])
            pred = model_only()
            vops.cfg_pndm_step(pred, b["model_in"], z, 7.5, 1.0, [1e-3 * c for c in k["cz"]], None, base=z, srcs=b["hist"][:3], e_out=b["hist"][3])

        for hbuf in b["hist"]:
            hbuf.normal_()
        model_only()                                     # records (the text K / V are made resident first, outside the recording)
        res["recorded_launches"] = next(iter(pipe._steps.entries.values()))[0].n_launches
        # the yardstick of tools/osp_v110_bench.py on the SAME model in the SAME run: the bare transformer call, recorded after one eager
        # call and replayed — what profiles/osp_v110_timing.json holds from another run
        from videosys_amd import program

        x = torch.randn(2, 4, T, h, w, generator=g).to(dev)
        tsv = torch.tensor([500, 500])
        bare_call = lambda: model(x, timestep=tsv, encoder_hidden_states=b["enc"], encoder_attention_mask=None)
        bare_call()
        with program.Recorder() as rec:
            bare_call()
        bare = rec.finish()
        res["bare_model_recorded_launches"] = bare.n_launches
        t = in_turn({"step": step, "model": model_only, "bare": bare.run}, args.reps)
        res["step_ms_65x512x512_300_text_keys"] = t["step"]
        res["model_alone_ms_same_run"] = t["model"]
        res["bare_model_program_ms_same_run"] = t["bare"]
        res["step_stats"] = dict(pipe.step_stats)
        try:
            with open(os.path.join(ROOT, "profiles", "osp_v110_timing.json")) as fh:
                res["parent_model_step_ms_profiles_osp_v110_timing"] = json.load(fh)["step_65x512x512"]["median_ms"]
        except Exception as e:
            res["parent_model_step_ms_profiles_osp_v110_timing"] = f"not read: {e!r}"
    print(flush())


if __name__ == "__main__":
    main()
