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
synchronisations, after one warm-up of the same shape."""
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
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    dev = torch.device("cuda:0")
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


if __name__ == "__main__":
    main()
