#!/usr/bin/env python
"""Timing of the VAE mid-block attention (vae_blocks.attention_core) on its two paths: the materialised one (three batched GEMMs
around vsys_softmax_rows) and the flash kernel vsys_vae_flash_attn (csrc/attention_vae.hip), alternated in ONE process with random
weights; median and spread over the rounds (cuda events around the whole core: q / k / V^T projections and the out-projection
included in the time, the 4 L^2 C n flop of the two attention products alone in the TFLOP/s).

    python tools/vae_flash_bench.py [--rounds 7] [--out profiles/vae_flash_attn_timing.json]
    python tools/vae_flash_bench.py --smoke      one untiled CausalVAEModel.encode of a 720 x 1280 clip and one OpenSoraVAE.decode
                                                  at 720p (14 400 keys per frame: neither ran before the flash path), random weights
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videosys_amd import vae_blocks  # noqa: E402


def weights(C, dev):
    g = torch.Generator().manual_seed(0)
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    lin = lambda: bf(torch.randn(C, C, generator=g) / math.sqrt(C))
    vec = lambda: bf(0.02 * torch.randn(C, generator=g))
    return vae_blocks.AttnWeights(None, lin(), vec(), lin(), vec(), lin(), vec(), lin(), vec().float())


def time_core(n, L, C, paths, rounds, dev):
    Lp = (L + 127) // 128 * 128
    w = weights(C, dev)
    hn, xd = (torch.zeros(n, Lp, C, dtype=torch.bfloat16, device=dev) for _ in range(2))
    hn[:, :L], xd[:, :L] = torch.randn(n, L, C, device=dev).to(torch.bfloat16), torch.randn(n, L, C, device=dev).to(torch.bfloat16)
    hn, xd = hn.view(n * Lp, C), xd.view(n * Lp, C)
    ms = {p: [] for p in paths}
    for r in range(rounds + 1):                       # round 0 warms up
        for p in paths:
            vae_blocks.FORCE_FLASH = p == "flash"
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            vae_blocks.attention_core(hn, xd, n, L, Lp, C, w)
            b.record()
            torch.cuda.synchronize()
            if r:
                ms[p].append(a.elapsed_time(b))
    vae_blocks.FORCE_FLASH = False
    flop = 4.0 * L * L * C * n
    return {p: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), tflops=flop / statistics.median(v) / 1e9) for p, v in ms.items()}


def smoke(dev):
    from videosys_amd import vae_open_sora as vos
    from videosys_amd import vae_open_sora_plan as osp

    vae = osp.CausalVAEModel(osp.synth_state_dict(0, 128, encoder=True), device=dev)
    x = torch.randn(1, 3, 5, 720, 1280, device=dev).clamp(-1, 1)
    t0 = time.time()
    post = vae.encode(x)
    torch.cuda.synchronize()
    print(f"[smoke] CausalVAEModel.encode 5 x 720 x 1280 untiled: {type(post).__name__}, {time.time() - t0:.2f} s (first call)", flush=True)
    del vae, post
    dec = vos.OpenSoraVAE(vos.synth_state_dict(0), device=dev)
    z = torch.randn(1, 4, 5, 90, 160, device=dev)
    t0 = time.time()
    y = dec.decode(z, 17)
    torch.cuda.synchronize()
    print(f"[smoke] OpenSoraVAE.decode latents 5 x 90 x 160 (17 frames of 720 x 1280) -> {tuple(y.shape)}, finite {bool(torch.isfinite(y.float()).all())}, "
          f"{time.time() - t0:.2f} s (first call)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--smoke", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.smoke:
        return smoke(dev)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "rounds": args.rounds,
           "what": "vae_blocks.attention_core, C = 512, random weights, paths alternated in one process; time = whole core "
                   "(projections included), tflops = 4 L^2 C n / median",
           "decode_512_64f_64x64": time_core(64, 4096, 512, ("materialised", "flash"), args.rounds, dev),
           "decode_720p_8f_90x160": time_core(8, 14400, 512, ("flash",), args.rounds, dev),
           "note_720p": "14 400 keys per frame: the materialised path cannot run (vsys_softmax_rows takes 8192), so this row has no "
                        "parent to compare with"}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
