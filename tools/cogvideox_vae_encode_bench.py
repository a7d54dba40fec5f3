#!/usr/bin/env python
"""Timing of the CogVideoX VAE encode at the published size (49 x 480 x 720, random weights) on one MI355X, written to
profiles/cogvideox_vae_encode_timing.json.  TIMING ONLY: one box, one run, medians; the parent has no encode, so there is no before /
after and no threshold.

  * the two launches of vsys_conv_pool_down2_bf16 (after down blocks 0 and 1) in ms and TFLOP/s (2 M N K over the median), and beside
    them vsys_conv_down2_bf16 in its spatial mode at the SAME output shapes (the same M, N, K: one source frame per output frame
    instead of two), for orientation;
  * at both sites the pooled launch against conv_down2 on a pooled copy made by torch (bf16 (a + b) / 2): the same products in the
    same order, so the outputs are expected to be equal bit for bit;
  * the whole encode.

Times are host clocks around work that ends in a stream synchronise: a window of ``--inner`` launches per repetition for the kernels,
one encode per repetition for the model; every shape is warmed up first.

    python tools/cogvideox_vae_encode_bench.py [--frames 49 --height 480 --width 720 --reps 7 --inner 20 --encode-reps 3]"""
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
OUT = os.path.join(ROOT, "profiles", "cogvideox_vae_encode_timing.json")


def timed(fn, reps, inner):
    """[median, min, max] ms per call of ``fn`` over ``reps`` windows of ``inner`` calls."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=49)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--encode-reps", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on a HIP device"
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd import vae_blocks as vb
    from videosys_amd.ops import VaeGrid
    from videosys_amd.vae_cogvideox import CogVideoXVAE, synth_state_dict

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    sites, T, H, W = [], a.frames, a.height, a.width
    for C in (128, 256):
        g = VaeGrid(1, T, H, W, 1, 0)                                        # the rows a resnet's last conv leaves: bordered
        og = vb.pool_down2_grid(g)
        x = torch.randn(g.rows, C, dtype=torch.bfloat16, device=dev)
        w = (torch.randn(C, 9 * C, generator=gen) / (9 * C) ** 0.5).to(torch.bfloat16).to(dev)
        b = (0.1 * torch.randn(C, generator=gen)).to(torch.bfloat16).to(dev)
        wh = vb.half_weights(w)
        out = torch.empty(og.rows, C, dtype=torch.bfloat16, device=dev)
        pool_ms = timed(lambda: vb.conv_pool_down2(x, g, wh, b, C, out=out), a.reps, a.inner)
        v = x.view(T, g.Hp, g.Wp, C)
        odd = T % 2
        pooled = torch.cat([v[:odd], (v[odd::2] + v[odd + 1::2]) / 2], dim=0).reshape(-1, C).contiguous()   # the copy the kernel avoids
        gs = VaeGrid(1, og.T, H, W, 1, 0)
        ref = torch.empty_like(out)
        down_ms = timed(lambda: oops.conv_down2(pooled, gs, w, b, C, 1, out=ref), a.reps, a.inner)
        flop = 2.0 * og.rows * C * 9 * C
        sites.append(dict(source=[T, H, W], C=C, output=[og.T, og.H, og.W], pool_down2_ms=pool_ms,
                          pool_down2_tflops=round(flop / pool_ms[0] * 1e-9, 1), conv_down2_spatial_same_output_ms=down_ms,
                          conv_down2_spatial_tflops=round(flop / down_ms[0] * 1e-9, 1),
                          equal_bits_vs_conv_down2_on_torch_pooled_copy=bool(torch.equal(out, ref)),
                          max_abs_diff_vs_that=float((out.float() - ref.float()).abs().max())))
        print(sites[-1], flush=True)
        del x, pooled, out, ref, v
        torch.cuda.empty_cache()
        T, H, W = og.T, og.H, og.W
    vae = CogVideoXVAE(synth_state_dict(0, encoder=True), device=dev)
    clip = torch.randn(1, 3, a.frames, a.height, a.width, generator=gen).clamp(-1, 1).to(torch.bfloat16).to(dev)
    post = vae.encode(clip).latent_dist                                      # warm-up: staging buffers, code objects
    torch.cuda.synchronize()
    enc_ms = timed(lambda: vae.moments(clip), a.encode_reps, 1)
    res = dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), reps=a.reps, inner=a.inner,
               what="TIMING ONLY, one box, one run: random weights; median (min, max) of the repetitions in ms per call, host clock "
                    "around a window that ends in a stream synchronise",
               pool_down2_launches=sites, **{f"encode_ms_{a.frames}f_{a.height}x{a.width}": enc_ms}, encode_reps=a.encode_reps,
               moments_shape=list(post.parameters.shape), moments_finite=bool(torch.isfinite(post.parameters.float()).all()),
               peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2**30, 2),
               parent="none: CogVideoXVAE had no encode before this kernel", box="one MI355X (gfx950), one process",
               note="tflops = 2 M N K / median with K = 9 C.  conv_down2_spatial_* is vsys_conv_down2_bf16 (kt = 1) at the same output "
                    "shape on a pooled copy of the source made by torch for this comparison only: it reads one frame per output frame, the "
                    "pooled kernel two, and sums them in registers.  Recorded, not gated.")
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
