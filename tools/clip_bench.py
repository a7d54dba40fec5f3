"""Time the two CLIP text encoders of Vchitect-2.0 (clip.CLIPTextEncoder at the CLIP-L and CLIP-bigG geometries) on one prompt of 77
tokens, random weights generated on the device, and write profiles/clip_encoder_timing.json.

    python tools/clip_bench.py [--iters 30] [--warmup 5] [--out profiles/clip_encoder_timing.json]

Per encoder: the median (and the spread) of ``iters`` encodes, each between two stream synchronisations on a host clock, after
``warmup`` untimed encodes; the launch count of one encode; and, for context only, the time the weights alone would take at the
6.2 TB/s this project measured for streaming reads — an encode reads every weight once, so that is its floor.  There
is NO threshold and nothing to compare against: the parent commit cannot run this path at all.  Needs a HIP device; no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TB_S = 6.2   # measured streaming-read rate of this project's weight-streaming linears


def time_encoder(name, geometry, iters, warmup, batch=1, tokens=77):
    from videosys_amd.clip import CLIPTextEncoder

    enc = CLIPTextEncoder(device="cuda:0", **geometry).init_random_(0)
    ids = torch.randint(0, geometry["vocab_size"], (batch, tokens))
    ids[:, -1] = geometry["vocab_size"] - 1
    for _ in range(warmup):
        out = enc(ids, output_hidden_states=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.text_embeds.float()).all()) and bool(torch.isfinite(out.hidden_states[-2].float()).all())
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc(ids, output_hidden_states=True)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    streamed = sum(v.numel() for k, v in enc.w.items() if k not in ("tok", "pos")) * 2     # every linear / norm weight, once
    return {"encoder": name, "batch": batch, "tokens": tokens, "layers": geometry["num_hidden_layers"],
            "hidden_size": geometry["hidden_size"], "median_ms": round(statistics.median(ts) * 1e3, 4),
            "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4), "iters": iters, "warmup": warmup,
            "kernel_launches": enc.launches, "streamed_weight_bytes": streamed,
            "weight_stream_floor_ms_at_6.2TBs": round(streamed / (HBM_TB_S * 1e12) * 1e3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_encoder_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_bench.py needs a HIP device: a timing taken anywhere else says nothing about the MI355X")
    from videosys_amd.clip import CLIP_BIGG, CLIP_L

    rows = [time_encoder("CLIP-L", CLIP_L, args.iters, args.warmup), time_encoder("CLIP-bigG", CLIP_BIGG, args.iters, args.warmup)]
    doc = {"what": "clip.CLIPTextEncoder, one prompt (B = 1, L = 77), random weights, output_hidden_states=True: host clock between "
                   "two stream synchronisations around one encode, median of `iters` after `warmup` untimed encodes",
           "device": torch.cuda.get_device_name(0),
           "comparison": "none: the parent commit cannot run this path (its pipeline raises 'the CLIP encoders ... are not built'), so "
                         "there is no earlier time and no threshold; weight_stream_floor_ms is context, not a target",
           "encoders": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
