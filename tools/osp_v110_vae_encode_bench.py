#!/usr/bin/env python
"""Timing of the Open-Sora-Plan v1.1 CausalVAE encode (65 x 512 x 512, hidden size 128, random weights) on one MI355X, written to
profiles/osp_v110_vae_encode_timing.json.  TIMING ONLY: one box, one run, medians; the parent has no v1.1 encode, so the whole-encode
time has no before / after and nothing here is a threshold.

  * the two TimeDownsampleRes2x launches alone (vsys_conv_time_down2_bf16) at the channel counts and frame sizes of that encode: 256
    channels, 33 -> 17 frames of 128 x 128, and 512 channels, 17 -> 9 frames of 64 x 64 (the 65-frame encode itself runs them on 65 and
    33 frames), in ms and TFLOP/s (2 M N K over the median, K = 27 C; the pooled residual is not counted);
  * at each site the COMPOSED route the kernels before this one allow, timed in the same run and ALTERNATED with the fused launch
    window by window: vsys_regrid into a padded grid with two front frames + the front-frame copy (vsys_regrid, tmode 1), vsys_conv_bf16
    at stride 1 over all T frames with the (1 - alpha) weights, vsys_subsample of every second frame, then the pool and the mix as
    torch element-wise expressions (there was no HIP pool);
  * the TimeDownsample2x mode (no weights) at the same two sites, in ms and GB/s of the bytes it must move;
  * the whole encode.

Times are host clocks around a window of ``--inner`` launches that ends in a stream synchronise; every shape is warmed up first.

    python tools/osp_v110_vae_encode_bench.py [--frames 65 --size 512 --site-frames 33 --reps 7 --inner 10 --encode-reps 3]"""
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
OUT = os.path.join(ROOT, "profiles", "osp_v110_vae_encode_timing.json")


def window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def alternated(fns, reps, inner):
    """{name: [median, min, max] ms per call}, the windows of the routes taking turns."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, inner))
    return {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--site-frames", type=int, default=33, help="source frames of the first launch timed alone (the second gets its output's)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--encode-reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on a HIP device"
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd import ops
    from videosys_amd.ops import VaeGrid
    from videosys_amd.vae_open_sora_plan_v110 import CausalVAEModel, synth_state_dict

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    sites = []
    for C, div, alpha, T in ((256, 4, 0.58, a.site_frames), (512, 8, 0.81, (a.site_frames - 1) // 2 + 1)):
        H = W = a.size // div
        g = VaeGrid(1, T, H, W, 0, 0)                                          # the dense rows the spatial downsampler leaves
        og = vops.time_down2_grid(g)
        x = torch.randn(g.rows, C, dtype=torch.bfloat16, device=dev)
        w = (torch.randn(C, 27 * C, generator=gen) / (27 * C) ** 0.5 * (1 - alpha)).to(torch.bfloat16).to(dev)
        b = (0.1 * torch.randn(C, generator=gen)).to(torch.bfloat16).to(dev)
        out = torch.empty(og.rows, C, dtype=torch.bfloat16, device=dev)
        pooled = torch.empty_like(out)
        gp = VaeGrid(1, T, H, W, 1, 2)
        _, xp = gp.alloc(C, dev, zero=True)
        gc = gp.conv_out()
        full = torch.empty(gc.rows, C, dtype=torch.bfloat16, device=dev)
        half = torch.empty(og.rows, C, dtype=torch.bfloat16, device=dev)

        def composed():
            ops.regrid(x, g, xp[2 * gp.plane:], VaeGrid(1, T, H, W, 1, 0), C)                               # the padded copy ...
            ops.regrid(xp[2 * gp.plane:3 * gp.plane], VaeGrid(1, 1, H, W, 1, 0), xp[:2 * gp.plane], VaeGrid(1, 2, H, W, 1, 0), C, tmode=1)
            ops.conv(xp, gp, w, b, C, 3, 3, out=full)                                                       # ... every frame ...
            ops.subsample(full, gc, half, og, C, t_stride=2)                                                # ... half thrown away
            v = x.view(T, H * W, C)
            f0 = torch.cat([v[:1], v[:2 * og.T - 3:2]]) if og.T > 1 else v[:1]
            f1 = torch.cat([v[:1], v[1:2 * og.T - 2:2]]) if og.T > 1 else v[:1]
            pool = ((f0.float() + f1.float()) + v[:2 * og.T - 1:2].float()) * (alpha / 3.0)                 # pool and mix
            return (half.view(og.T, H * W, C).float() + pool).to(torch.bfloat16)

        fused = lambda: vops.conv_time_down2(x, g, w, b, C, alpha / 3.0, out=out)
        ms = alternated(dict(fused=fused, composed=composed, pool_only=lambda: vops.conv_time_down2(x, g, None, None, C, 1 / 3, out=pooled)),
                        a.reps, a.inner)
        diff = float((composed().reshape(-1, C).float() - out.float()).abs().max())
        flop = 2.0 * og.rows * C * 27 * C
        moved = 2.0 * C * ((2 * og.T - 1) * H * W + og.rows)
        sites.append(dict(C=C, source=[T, H, W], output=[og.T, H, W], fused_ms=ms["fused"], fused_tflops=round(flop / ms["fused"][0] * 1e-9, 1),
                          composed_ms=ms["composed"], composed_over_fused=round(ms["composed"][0] / ms["fused"][0], 2),
                          max_abs_diff_composed_vs_fused=diff, pool_only_ms=ms["pool_only"],
                          pool_only_gb_per_s=round(moved / ms["pool_only"][0] * 1e-6, 1)))
        print(sites[-1], flush=True)
        del x, xp, full, half, out, pooled
        torch.cuda.empty_cache()
    vae = CausalVAEModel(synth_state_dict(0, 128, encoder=True), device=dev)
    clip = torch.randn(1, 3, a.frames, a.size, a.size, generator=gen).clamp(-1, 1).to(torch.bfloat16).to(dev)
    post = vae.encode(clip)                                                    # warm-up: staging buffers, code objects
    torch.cuda.synchronize()
    enc = [window(lambda: vae.encoder.moments(clip), 1) for _ in range(a.encode_reps)]
    res = dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), reps=a.reps, inner=a.inner,
               what="TIMING ONLY, one box, one run: random weights; median (min, max) of the repetitions in ms per call, host clock around "
                    "a window that ends in a stream synchronise; fused / composed / pool-only windows alternate",
               time_down2_launches=sites,
               **{f"encode_ms_{a.frames}f_{a.size}x{a.size}": [round(statistics.median(enc), 1), round(min(enc), 1), round(max(enc), 1)]},
               encode_reps=a.encode_reps, moments_shape=list(post.parameters.shape),
               moments_finite=bool(torch.isfinite(post.parameters.float()).all()),
               peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2**30, 2),
               parent="none: the v1.1 CausalVAEModel had no encode before this kernel", box="one MI355X (gfx950), one process",
               note="tflops = 2 M N K / median with K = 27 C.  composed = padded copy with two front frames (two vsys_regrid), vsys_conv_bf16 "
                    "at stride 1 over every frame, vsys_subsample (t_stride 2), pool and mix as torch element-wise expressions; its output "
                    "differs from the fused one by the extra bf16 rounding of the convolution.  Recorded, not gated.")
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
