#!/usr/bin/env python
"""Time the two halves of a Vchitect-2.0 video at the pipeline's defaults (288 x 480, 40 frames -> latent 36 x 60) on random weights:

  decode   AutoencoderKLSD3Decoder.decode_u8 of 40 frames (vae_sd3.py: the two end kernels + the 2-D decoder)
  step     one denoise step at the 2B geometry (18 layers, 18 heads x 64, L = 77 + 256 text tokens): the recorded pair of model calls
           (uncond, text) + the guidance / Euler launch, as VchitectXLPipeline issues it

    python tools/vchitect_bench.py [--reps 5] [--out FILE.json] [--skip-step] [--skip-decode]

Prints one JSON line; device time from HIP events around ``reps`` repetitions after one warm-up."""
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
    args = ap.parse_args()
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


if __name__ == "__main__":
    main()
