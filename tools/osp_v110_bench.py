#!/usr/bin/env python
"""Time the Open-Sora-Plan v1.1 transformer at the 65 x 512 x 512 geometry (28 + 28 blocks, 16 heads x 72; latent 17 x 64 x 64 at patch
2 = 17 frames of 1 024 tokens; CFG batch 2; 300 text keys) on RANDOM weights, and each roped head-dim-72 kernel beside its plain
counterpart at the shape of that step's spatial attention (34 (sample, frame) pairs x 16 heads x 1 024^2).

    python tools/osp_v110_bench.py [--reps 20] [--layers 28] [--out profiles/osp_v110_timing.json] [--skip-step] [--skip-kernels]

  step     one denoise step of open_sora_plan_v110.LatteT2V with use_rope, recorded once (program.Recorder) and replayed; if the step
           cannot be recorded the eager call is timed instead and the record says so ("mode")
  kernels  open_sora_plan_v110_ops.flash_attn_rope beside ops.flash_attn (no q norm), and attn_prep_kv_rope beside ops.attn_prep_kv (no k
           norm), each pair alternating in one process so that drift hits both alike

Every figure is the median of ``reps`` (>= 20) repetitions, each timed on the host between two stream synchronisations, after a
warm-up.  Writes one JSON record: box (host name), device, date, and the measurements.  A measurement to record, not a gate."""
import argparse
import datetime
import json
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": len(ts)}


def in_turn(fns, reps, warm=3):
    """name -> stats of ``reps`` calls of every function, the functions called in turn."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ts.items()}


def random_state_dict(model, caption_channels, dev, seed=0):
    """bf16 weights with the reference's names, drawn on the device (a CPU draw of 0.8 G values takes a while)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    C, p = model.C, model.patch_size

    def shape(k):
        if k == "pos_embed.proj.weight":
            return (C, model.in_channels, p, p)
        if k.endswith("scale_shift_table"):
            return (2, C) if k == "scale_shift_table" else (6, C)
        n_out, n_in = C, C
        if "timestep_embedder.linear_1" in k:
            n_in = 256
        elif "adaln_single.linear" in k:
            n_out = 6 * C
        elif "caption_projection.linear_1" in k:
            n_in = caption_channels
        elif "ff.net.0.proj" in k:
            n_out = 4 * C
        elif "ff.net.2" in k:
            n_in = 4 * C
        elif k.startswith("proj_out"):
            n_out = p * p * model.out_channels
        return (n_out,) if k.endswith(".bias") else (n_out, n_in)

    sd = {}
    for k in model.expected_keys():
        s = shape(k)
        scale = 0.02 if k.endswith(".bias") else (s[-1]**-0.5 if len(s) == 2 and "scale_shift" not in k else 0.05)
        sd[k] = (torch.randn(*s, generator=g, device=dev) * scale).to(torch.bfloat16)
    return sd


def step_time(args, dev):
    from videosys_amd import pab, program
    from videosys_amd.open_sora_plan_v110 import LatteT2V

    pab.set_pab_manager(None)
    T, HW, Lk = 17, 64, 300
    model = LatteT2V(num_attention_heads=16, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=args.layers,
                     cross_attention_dim=1152, sample_size=(HW, HW), patch_size=2, caption_channels=4096, video_length=T, use_rope=True,
                     model_max_length=Lk, device=dev)
    model.load_state_dict(random_state_dict(model, 4096, dev))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, T, HW, HW, generator=g).to(dev)
    enc = torch.randn(2, 1, Lk, 4096, generator=g).to(torch.bfloat16).to(dev)
    ts = torch.tensor([500, 500])
    call = lambda: model(x, timestep=ts, encoder_hidden_states=enc, encoder_attention_mask=None)
    call()
    mode, run, extra = "eager", call, {}
    try:
        with program.Recorder() as rec:
            call()
        prog = rec.finish()
        if prog is not None:
            mode, run = "replayed", prog.run
            extra = dict(recorded_launches=prog.n_launches, host_actions=sum(1 for s in prog.segments if not isinstance(s, tuple)))
        else:
            extra = dict(not_recorded=str(rec.invalid))
    except Exception as e:      # the figure is still worth having
        extra = dict(not_recorded=repr(e))
    res = in_turn({"step": run}, args.reps)["step"]
    res.update(mode=mode, layers=f"{model.L} + {model.L}", heads=16, head_dim=72, frames=T, tokens_per_frame=(HW // 2)**2, batch=2, text_keys=Lk,
               **extra)
    return res


def kernel_times(args, dev):
    from videosys_amd import open_sora_plan_v110 as m
    from videosys_amd import open_sora_plan_v110_ops as vops
    from videosys_amd import ops

    B, H, L = 34, 16, 1024
    C = H * 72
    g = torch.Generator(device=dev).manual_seed(2)
    qkv = torch.randn(B * L, 3 * C, generator=g, device=dev).to(torch.bfloat16)
    cos, sin = (t.to(dev) for t in m.rope_tables_2d(32, 32, 1.0))
    o = torch.empty(B * L, C, dtype=torch.bfloat16, device=dev)
    kp, vt = ops.alloc_kv_buffers(B, H, L, dev)
    k, v, q = qkv[:, C:2 * C], qkv[:, 2 * C:], qkv[:, :C]
    ops.attn_prep_kv(k, v, None, kp, vt, B, H, L)
    out = {"shape": {"batch": B, "heads": H, "q_len": L, "kv_len": L}}
    fl = in_turn({"flash_plain": lambda: ops.flash_attn(q, None, kp, vt, o, B, H, L, L),
                  "flash_rope": lambda: vops.flash_attn_rope(q, cos, sin, kp, vt, o, B, H, L, L)}, args.reps)
    flops = 4.0 * B * H * L * L * 72
    for r in fl.values():
        r["tflops"] = round(flops / (r["median_ms"] * 1e-3) / 1e12, 1)
    out.update(fl)
    out["flash_rope_over_plain_time"] = round(fl["flash_rope"]["median_ms"] / fl["flash_plain"]["median_ms"], 4)
    pr = in_turn({"prep_plain": lambda: ops.attn_prep_kv(k, v, None, kp, vt, B, H, L),
                  "prep_rope": lambda: vops.attn_prep_kv_rope(k, v, cos, sin, kp, vt, B, H, L)}, args.reps)
    out.update(pr)
    out["prep_rope_over_plain_time"] = round(pr["prep_rope"]["median_ms"] / pr["prep_plain"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    args = ap.parse_args()
    args.reps = max(args.reps, 20)
    dev = torch.device("cuda:0")
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "note": "random weights (no checkpoint offline): times are valid, outputs are not a video; median of host-timed repetitions "
                   "between two stream synchronisations, after warm-up; the kernel pairs alternate in one process"}
    if not args.skip_kernels:
        res["attention_kernels_34x16x1024"] = kernel_times(args, dev)
    if not args.skip_step:
        res["step_65x512x512"] = step_time(args, dev)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
