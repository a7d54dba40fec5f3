#!/usr/bin/env python
"""Time the Open-Sora-Plan v1.2 transformer at the 29x480p geometry (32 layers, 24 heads x 96; latent 8 x 60 x 80 at patch 2 = 9 600
tokens; CFG batch 2; 512 text keys) on RANDOM weights, and the head-dim-96 flash kernel beside the head-dim-64 one.

    python tools/osp_bench.py [--reps 30] [--layers 32] [--out profiles/osp_v120_timing.json] [--skip-step] [--skip-kernels]
    python tools/osp_bench.py --ranks 4 --ranks 8 [--out profiles/osp_sp_timing.json]      one rank of a sequence-parallel group

  step     one denoise step of OpenSoraT2V, recorded once (program.Recorder) and replayed
  kernels  vsys_flash_attn_d96 and, in the same process and in turn, vsys_flash_attn_d64 at batch 2, 24 heads, 9 600 x 9 600 keys, no
           rotation tables: TFLOP/s on the algorithmic 4 * batch * heads * Lq * Lk * head_dim flops

  --ranks  the recorded step of ONE rank (rank 0) of a P-way Ulysses group with the wire stubbed (tools/local_group.StubGroup: a collective
           is a device copy of the same bytes, the one-kernel exchange writes into the rank's own tensors): per P the three routes —
           peer-to-peer + rows, all_to_all_single + rows, all_to_all_single + image — recorded once each and replayed IN TURN, 20
           replays each, median and min..max, launches and host actions per step; and the single-rank step of the same run beside
           them.  What a rank computes and launches is real; what the wire costs is NOT measured (no multi-GPU run exists).

Every figure is the median of ``reps`` (>= 30) repetitions, each timed on the host between two stream synchronisations, after a
warm-up.  Writes one JSON record: box (host name), device, date, and the measurements."""
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


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": reps}


def random_state_dict(model, dev, seed=0):
    """bf16 weights of the model's own shapes, drawn on the device (a CPU draw of 2.7 G values takes minutes)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for k, s in model.expected_shapes().items():
        scale = 0.02 if k.endswith(".bias") else (s[-1]**-0.5 if len(s) == 2 and "scale_shift" not in k else 0.05)
        sd[k] = (torch.randn(*s, generator=g, device=dev) * scale).to(torch.bfloat16)
    return sd


def build_step(args, dev):
    """(model, call): the 29x480p transformer on random weights and one CFG-pair forward of it."""
    from videosys_amd import pab
    from videosys_amd.open_sora_plan import OpenSoraT2V, OpenSoraT2V_ROPE_L_122

    pab.set_pab_manager(None)
    T, H, W, Lk = 8, 60, 80, 512
    kw = dict(in_channels=4, out_channels=8, attention_bias=True, sample_size=(H, W), sample_size_t=T, activation_fn="gelu-approximate",
              norm_elementwise_affine=False, norm_eps=1e-6, use_rope=True, interpolation_scale_t=1.0, device=dev)
    if args.layers == 32:
        model = OpenSoraT2V_ROPE_L_122(**kw)
    else:       # a shallower stack of the same blocks (a quick look; the recorded figure is the 32-layer one)
        model = OpenSoraT2V(num_layers=args.layers, attention_head_dim=96, num_attention_heads=24, patch_size_t=1, patch_size=2,
                            norm_type="ada_norm_single", caption_channels=4096, cross_attention_dim=2304, **kw)
    model.load_state_dict(random_state_dict(model, dev))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, T, H, W, generator=g).to(dev)
    enc = torch.randn(2, 1, Lk, 4096, generator=g).to(torch.bfloat16).to(dev)
    mask = torch.ones(2, 1, Lk)
    mask[1, 0, 300:] = 0
    call = lambda: model(x, timestep=torch.tensor([500, 500]), encoder_hidden_states=enc, encoder_attention_mask=mask)
    shape = dict(layers=model.L, heads=model.H, head_dim=96, tokens=T * (H // 2) * (W // 2), batch=2, text_keys=Lk, visible=[Lk, 300])
    return model, call, shape


def record(call):
    from videosys_amd import program

    call()
    with program.Recorder() as rec:
        call()
    prog = rec.finish()
    assert prog is not None, rec.invalid
    return prog


def counts(prog):
    return dict(recorded_launches=prog.n_launches, host_actions=sum(1 for s in prog.segments if not isinstance(s, tuple)))


def step_time(args, dev):
    model, call, shape = build_step(args, dev)
    prog = record(call)
    res = median_ms(prog.run, args.reps)
    res.update(shape, **counts(prog))
    return res


def in_turn(progs, reps, warm=3):
    """name -> {median, min, max} of ``reps`` replays of every program, the programs replayed in turn so that drift hits them alike."""
    for prog in progs.values():
        for _ in range(warm):
            prog.run()
    ts = {k: [] for k in progs}
    for _ in range(reps):
        for k, prog in progs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            prog.run()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), reps=reps, **counts(progs[k]))
            for k, v in ts.items()}


def sp_step_times(args, dev, reps=20):
    """The per-rank step of a P-way group, wire stubbed, for every P of --ranks, and the single-rank step of the same run."""
    from types import SimpleNamespace

    from tools.local_group import StubGroup

    model, call, shape = build_step(args, dev)
    out = dict(shape, single_rank=in_turn({"step": record(call)}, reps)["step"], ranks={})
    for P in args.ranks:
        progs = {}
        for name, p2p, route in (("p2p_rows", True, "rows"), ("a2a_rows", False, "rows"), ("a2a_image", False, "image")):
            mgr = SimpleNamespace(sp_size=P, cp_size=1, dp_size=1, dp_rank=0, sp_rank=0, cp_rank=0, sp_group=StubGroup(P, 0), cp_group=None)
            model.enable_parallel(parallel_mgr=mgr)
            if not p2p:
                model._sp.p2p = None
            model.attn_route = route
            progs[name] = record(call)
        res = in_turn(progs, reps)
        rows, img = res["a2a_rows"], res["a2a_image"]
        res["image_beats_rows"] = bool(img["median_ms"] < rows["median_ms"] and img["max_ms"] < rows["min_ms"])   # the default's rule
        res["local_tokens"] = shape["tokens"] // P
        out["ranks"][str(P)] = res
    model.enable_parallel(parallel_mgr=SimpleNamespace(sp_size=1, cp_size=1))
    return out


def kernel_times(args, dev):
    from videosys_amd import open_sora_plan_ops as oops
    from videosys_amd import ops

    B, H, L = 2, 24, 9600
    g = torch.Generator(device=dev).manual_seed(2)
    out = {}
    bufs = {}
    for D in (96, 64):
        C = H * D
        qkv = torch.randn(B * L, 3 * C, generator=g, device=dev).to(torch.bfloat16)
        o = torch.empty(B * L, C, dtype=torch.bfloat16, device=dev)
        if D == 96:
            kp, vt = oops.alloc_kv_buffers96(B, H, L, dev)
            oops.attn_prep_kv96(qkv[:, C:2 * C], qkv[:, 2 * C:], None, None, kp, vt, B, H, L)
            fn = lambda qkv=qkv, kp=kp, vt=vt, o=o, C=C: oops.flash_attn96(qkv[:, :C], None, None, kp, vt, None, o, B, H, L, L)
        else:
            kp, vt = ops.alloc_kv_buffers64(B, H, L, dev)
            ops.attn_prep_kv64(qkv[:, C:2 * C], qkv[:, 2 * C:], None, None, None, None, 0, kp, vt, B, H, L)
            fn = lambda qkv=qkv, kp=kp, vt=vt, o=o, C=C: ops.flash_attn64(qkv[:, :C], None, None, None, None, 0, kp, vt, o, B, H, L, L)
        bufs[D] = fn
    times = {D: [] for D in bufs}
    for D, fn in bufs.items():
        for _ in range(3):
            fn()
    for _ in range(args.reps):               # the two kernels in turn, so that drift hits them alike
        for D, fn in bufs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[D].append((time.perf_counter() - t0) * 1e3)
    for D, ts in times.items():
        ms = statistics.median(ts)
        flops = 4.0 * B * H * L * L * D
        out[f"flash_d{D}"] = {"median_ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": len(ts),
                              "tflops": round(flops / (ms * 1e-3) / 1e12, 1)}
    out["shape"] = {"batch": B, "heads": H, "q_len": L, "kv_len": L}
    out["d96_over_d64_tflops"] = round(out["flash_d96"]["tflops"] / out["flash_d64"]["tflops"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--ranks", type=int, action="append", default=None,
                    help="time one rank of a sequence-parallel group of this size, wire stubbed (repeatable); nothing else is timed then")
    args = ap.parse_args()
    args.reps = max(args.reps, 30)
    dev = torch.device("cuda:0")
    res = {"box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "note": "random weights (no checkpoint offline): times are valid, outputs are not a video; median of host-timed repetitions "
                   "between two stream synchronisations, after warm-up"}
    if args.ranks:
        res["note"] += "; --ranks: ONE rank of the group with the wire stubbed (a collective is a device copy of the same bytes): the wire is " \
                       "unmeasured, no multi-GPU run exists"
        res["sequence_parallel_step_29x480p"] = sp_step_times(args, dev)
    else:
        if not args.skip_kernels:
            res["attention_kernels"] = kernel_times(args, dev)
        if not args.skip_step:
            res["replayed_step_29x480p"] = step_time(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
