#!/usr/bin/env python
"""Timing of the Open-Sora v1.2 VAE encode (one 17-frame 512 x 512 micro batch, random weights) on one MI355X, written to
profiles/opensora_vae_encode_timing.json.  TIMING ONLY: one box, one run, medians; nothing here is a threshold.

  * the five strided layers alone, at the shapes of that encode — the three Downsample2D layers of the 2-D encoder on a micro batch of 4
    frames (128 channels at 512 x 512, 256 at 256 x 256, 512 at 128 x 128) and the two stride-(2, 1, 1) CausalConv3d layers of the temporal
    encoder (256 channels, 20 -> 10 and 10 -> 5 frames of 64 x 64) — each on the STRIDED route (one launch of vsys_conv_down2_bf16 kt = 1 /
    vsys_conv_causal_tdown2_bf16) and on the COMPOSED route (vsys_regrid into a zero-bordered copy, vsys_conv_bf16 at stride 1,
    vsys_subsample), the two ALTERNATED window by window in the same run, through OpenSoraVAE's own two methods; ms, and TFLOP/s of the
    strided launch (2 M N K over the median, M the output voxels); then the temporal layer at other latent sizes (4 x 6 to 128 x 128);
  * the whole ``encode`` of the clip, VSYS_VAE_ENCODE_STRIDED=1 and =0 alternated the same way.

Times are host clocks around a window of ``--inner`` calls that ends in a stream synchronise; every shape is warmed up first.

    python tools/opensora_vae_encode_bench.py [--frames 17 --size 512 --reps 7 --inner 100 --encode-reps 5]"""
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
OUT = os.path.join(ROOT, "profiles", "opensora_vae_encode_timing.json")


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
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--encode-reps", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on a HIP device"
    from videosys_amd.ops import VaeGrid
    from videosys_amd.vae_open_sora import OpenSoraVAE_V1_2

    dev = torch.device("cuda:0")
    vae = OpenSoraVAE_V1_2(from_pretrained="synthetic-full:0", device=dev)
    S, lat, mb = a.size, a.size // 8, vae.micro_batch_size
    Tp = a.frames + (-a.frames) % 4
    #        layer                      weights          source grid (dense rows)       strides
    sites = [("spatial down 0", vae.e_down[0][1], VaeGrid(mb, 1, S, S, 0, 0), (1, 2)),
             ("spatial down 1", vae.e_down[1][1], VaeGrid(mb, 1, S // 2, S // 2, 0, 0), (1, 2)),
             ("spatial down 2", vae.e_down[2][1], VaeGrid(mb, 1, S // 4, S // 4, 0, 0), (1, 2)),
             ("temporal down 1", vae.te_down[1], VaeGrid(1, Tp, lat, lat, 0, 0), (2, 1)),
             ("temporal down 2", vae.te_down[2], VaeGrid(1, Tp // 2, lat, lat, 0, 0), (2, 1))]
    # the same temporal layer over other latent sizes: where the launch no longer fills the machine (tiles = row tiles of 256 output
    # voxels x column tiles of 128 channels, on 256 CUs) the time of either route is the latency of ONE tile's k-loop
    sites += [(f"temporal sweep T={T}", vae.te_down[1], VaeGrid(1, T, h, w, 0, 0), (2, 1))
              for h, w in ((4, 6), (16, 16), (32, 32), (48, 48), (80, 80), (96, 96), (128, 128)) for T in (Tp, Tp // 2)]
    layers = []
    for name, cv, g, (ts, ss) in sites:
        x = torch.randn(g.rows, cv.cin, dtype=torch.bfloat16, device=dev)
        ms = alternated(dict(strided=lambda: vae._strided_conv_tile(x, g, cv, ts, ss), composed=lambda: vae._strided_conv_composed(x, g, cv, ts, ss)),
                        a.reps, a.inner)
        (y1, g1), (y0, g0) = vae._strided_conv_tile(x, g, cv, ts, ss), vae._strided_conv_composed(x, g, cv, ts, ss)
        assert (g1.n, g1.T, g1.H, g1.W) == (g0.n, g0.T, g0.H, g0.W)
        flop = 2.0 * g1.rows * cv.cout * cv.w.shape[1]
        layers.append(dict(layer=name, cin=cv.cin, cout=cv.cout, source=[g.n, g.T, g.H, g.W], output=[g1.n, g1.T, g1.H, g1.W],
                           tiles=g1.n * -(-g1.sample_rows // 256) * (cv.cout // 128),
                           strided_ms=ms["strided"], composed_ms=ms["composed"], composed_over_strided=round(ms["composed"][0] / ms["strided"][0], 2),
                           strided_tflops=round(flop / ms["strided"][0] * 1e-9, 1), equal_bits=bool(torch.equal(y1.view(torch.int16), y0.view(torch.int16))),
                           max_abs_diff=float((y1.float() - y0.float()).abs().max())))
        print(layers[-1], flush=True)
        del x, y1, y0
        torch.cuda.empty_cache()
    clip = torch.randn(1, 3, a.frames, S, S, generator=torch.Generator().manual_seed(3)).clamp(-1, 1).to(torch.bfloat16).to(dev)

    def encode(route):
        os.environ["VSYS_VAE_ENCODE_STRIDED"] = route
        torch.manual_seed(0)
        return vae.encode(clip)

    enc = alternated({"strided": lambda: encode("1"), "composed": lambda: encode("0")}, a.encode_reps, 1)
    z1, z0 = encode("1"), encode("0")
    os.environ.pop("VSYS_VAE_ENCODE_STRIDED")
    res = dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), reps=a.reps, inner=a.inner, encode_reps=a.encode_reps,
               what="TIMING ONLY, one box, one run: random weights; median (min, max) of the repetitions in ms per call, host clock around a "
                    "window that ends in a stream synchronise; strided / composed windows alternate",
               box="one MI355X (gfx950), one process", strided_layers=layers,
               slower_on_strided=[f"{l['layer']} {l['source']}" for l in layers if l["strided_ms"][0] > l["composed_ms"][0]],
               **{f"encode_ms_{a.frames}f_{S}x{S}": enc}, encode_composed_over_strided=round(enc["composed"][0] / enc["strided"][0], 3),
               encode_latents_equal=bool(torch.equal(z1, z0)), encode_latents_finite=bool(torch.isfinite(z1).all()), latents_shape=list(z1.shape),
               peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2**30, 2),
               note="tflops = 2 M N K / median of the strided launch, M = output voxels, K = taps * cin.  composed = vsys_regrid into the "
                    "zero-bordered copy, vsys_conv_bf16 at stride 1 over every position, vsys_subsample.  Both routes allocate their output "
                    "per call, as encode does.  Recorded, not gated.")
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
