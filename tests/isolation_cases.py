"""The case table of the guard-band tests (tests/isolation.py): which kernel call, at which shapes, in which operand form.  DATA plus
one builder per operation; imported by tests/test_gpu_isolation_*.py (which run the rows) and by tests/test_isolation_cpu.py (which
checks that every kernel-launching function of videosys_amd/ops.py is named here or in NOT_COVERED).

A row is ``Case(family, ops, name, builder, params, gemm_variants, flash_variants)``.  ``builder(ops, dev, **params)`` returns
``(fn, operands, outputs, inplace)`` for isolation.check_isolated: ``fn(t)`` makes ONE call through videosys_amd.ops on the dict
``t`` of tensors (tight copies or arena views) and may return a dict of tensors the op allocated itself (compared bit for bit between
the two runs; an op that allocates its own result cannot have it placed in the arena, its INPUTS still are).  That holds for
patch_embed, patch_embed_shard, final_layer, final_layer_tokens, unpatchify_tokens, im2col_patch, unpatchify_cvx, timestep_embedding,
vae_first_im2col and gather_rows: for them these tests see an over-READ that reaches the result and a modified input, NOT an
over-write behind the result.  add_rows / add_bcast_rows take contiguous tensors only, so there is no row gap a wide store could hit;
their guard is the band behind the last element.

Operand forms used (the ones the model really passes): x / q / k / v as column slices of a wider buffer, ``out`` row-strided with
live guard columns on both sides, ``out`` aliasing ``res`` (in place), the gate as one column block of a [samples, 6 C] table with
gate_stride = 6 C, statistics as a row slice ``buf[:, r0:r1]`` with the parent's leading dimension, a rows_per_sample that puts a
sample boundary inside a tile.

What is guard INSIDE Kp / Vt depends on the entry point:
  * flash_attn default and k_norm_bound forms mask keys >= kv_len ("masked"): every Kp row and every Vt column (rows 0-72 and 76)
    at key index >= kv_len is poisoned, in buffers allocated for a longer kv_pad too — with the LARGEST FINITE value under both runs
    (``interior_fills=("max",)``; bands and gaps keep the run's fill).  Reason, measured on the device: with NaN in the Vt pad
    columns every output element is NaN (a masked key has probability 0 and still goes through the PV MFMA: 0 x NaN); with NaN in
    the Kp pad rows ALONE (Vt pads finite) every output element is NaN as well, at every ragged kv_len (1 .. 3600) and every kernel,
    although the logit of a pad key is overwritten (attention.hip, the ``masked`` branch) — so a pad row's content reaches a VALID
    key's logit with weight 0; with the huge finite value in both, the bits are those of zeros there.  "Finite behind kv_len" is
    therefore part of these entry points' contract (include/videosys_amd.h, vsys_flash_attn_d72; ops.flash_attn); attn_prep_kv
    writes zeros there, Latte's shorter kv_len inside a longer prepared buffer leaves real K / V values;
  * keys_exact / varlen carry the caller's promise of ZEROS there, so those positions hold the zeros attn_prep_kv wrote and the guard
    starts behind kv_pad ("exact");
  * Vt rows 73-75 and 77-95 hold zeros in every case (the caller's part of the contract, ops.alloc_kv_buffers).
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from isolation import Operand
from test_gpu_numerics_gemm import branch_cases       # the dispatch-boundary table of the GEMM numerics tests (a pure function)

Case = namedtuple("Case", "family ops name builder params gemm_variants flash_variants")
CASES = []

HD, VT_ROWS = 72, 96


def case(family, ops_named, name, builder, gemm_variants=(0,), flash_variants=(0,), **params):
    CASES.append(Case(family, tuple(ops_named), name, builder, params, tuple(gemm_variants), tuple(flash_variants)))


def family(name):
    return [c for c in CASES if c.family == name]


def rnd(dev, shape, seed, scale=1.0, offset=0.0, dtype=torch.bfloat16):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev) * scale + offset).to(dtype)


def strided(data, pad_l=8, pad_r=8):
    """``data`` [rows, cols] as the column slice [pad_l, pad_l + cols) of a buffer pad_l + cols + pad_r wide."""
    return Operand(data, parent=(data.shape[0], pad_l + data.shape[1] + pad_r), at=(0, pad_l))


def gate_table(dev, samples, N, seed, block=2):
    """The gate as column block ``block`` of a [samples, 6 N] modulation table: fn passes t['gate'][0] with the view's row stride
    as gate_stride (6 N in the arena; the other five column blocks are guard)."""
    return Operand(rnd(dev, (samples, N), seed, 0.7), parent=(samples, 6 * N), at=(0, block * N))


# ================================================================================================ GEMM family
def _rps(M):
    rps = max(1, M // 3 + 5)             # three samples, boundaries inside tiles (as tests/test_gpu_numerics_gemm.py)
    return rps, -(-M // rps)


def b_gemm(ops, dev, M, N, K, form):
    if isinstance(M, tuple):                                      # ("branch", i): row i of branch_cases(cu) — cu is the device's
        _, M, N, K, _ = branch_cases(torch.cuda.get_device_properties(0).multi_processor_count)[M[1]]
    x = Operand(rnd(dev, (M, K), 1), parent=(M, K + 128), at=(0, 64))
    w, b = rnd(dev, (N, K), 2, 1.0 / math.sqrt(K)), rnd(dev, (N,), 3, 0.1)
    o = {"x": x, "w": Operand(w), "bias": Operand(b)}
    rps, ns = _rps(M)
    if form in ("bias", "gelu"):
        o["out"] = strided(torch.zeros(M, N, dtype=torch.bfloat16, device=dev))
        epi = ops.EPI_BIAS if form == "bias" else ops.EPI_BIAS_GELU
        return (lambda t: ops.gemm(t["x"], t["w"], t["bias"], epilogue=epi, out=t["out"])), o, ["out"], []
    o["xr"] = strided(rnd(dev, (M, N), 4))                       # out aliases res: in place, as the model calls proj / fc2
    o["gate"] = gate_table(dev, ns, N, 5)
    outs = ["xr"]
    if form == "gate_res_aux":
        o["aux"] = strided(torch.zeros(M, N, dtype=torch.bfloat16, device=dev), 16, 0)
        outs.append("aux")

    def fn(t):
        ops.gemm(t["x"], t["w"], t["bias"], epilogue=ops.EPI_GATE_RES, gate=t["gate"][0], gate_stride=t["gate"].stride(0), rows_per_sample=rps,
                 res=t["xr"], aux=t.get("aux"), out=t["xr"])
    return fn, o, outs, ["xr"]


def _stats_slice(dev, nblk, M, data=None):
    """Statistics of M rows as the row slice buf[:, 16:16 + M] of a [nblk, M + 40, 2] buffer."""
    d = torch.zeros(nblk, M, 2, dtype=torch.float32, device=dev) if data is None else data
    return Operand(d, parent=(nblk, M + 40, 2), at=(0, 16, 0))


def b_gemm_stats(ops, dev, M, N, K):
    rps, ns = _rps(M)
    o = {"x": Operand(rnd(dev, (M, K), 11), parent=(M, K + 64), at=(0, 64)), "w": Operand(rnd(dev, (N, K), 12, 1.0 / math.sqrt(K))),
         "bias": Operand(rnd(dev, (N,), 13, 0.1)), "xr": strided(rnd(dev, (M, N), 14)), "gate": gate_table(dev, ns, N, 15, 5),
         "stats": _stats_slice(dev, N // 96, M)}

    def fn(t):
        ops.gemm_stats(t["x"], t["w"], t["bias"], t["stats"], gate=t["gate"][0], gate_stride=t["gate"].stride(0), rows_per_sample=rps, res=t["xr"],
                       out=t["xr"])
    return fn, o, ["xr", "stats"], ["xr"]


def b_gemm_ln(ops, dev, M, N, K, gelu):
    x = (rnd(dev, (M, K), 21).float() * 1.5 + rnd(dev, (M, 1), 22, 2.0).float()).to(torch.bfloat16)
    st = ops.ln_stats_buffer(M, K, dev)
    ops.ln_row_stats(x, st)
    wp = rnd(dev, (N, K), 23, 1.0 / math.sqrt(K))
    o = {"x": Operand(x, parent=(M, K + 64), at=(0, 0)), "wp": Operand(wp), "cs": Operand(wp.float().sum(1)),
         "cv": Operand(rnd(dev, (N,), 24, 0.1, dtype=torch.float32)), "stats": _stats_slice(dev, K // 96, M, st),
         "out": strided(torch.zeros(M, N, dtype=torch.bfloat16, device=dev))}
    return (lambda t: ops.gemm_ln(t["x"], t["wp"], t["cs"], t["cv"], t["stats"], gelu=gelu, out=t["out"])), o, ["out"], []


def b_gemm_gate_res_add(ops, dev, M, N, K, nadds, aux, stats):
    rps, ns = _rps(M)
    o = {"x": Operand(rnd(dev, (M, K), 31), parent=(M, K + 64), at=(0, 0)), "w": Operand(rnd(dev, (N, K), 32, 1.0 / math.sqrt(K))),
         "bias": Operand(rnd(dev, (N,), 33, 0.1)), "xr": strided(rnd(dev, (M, N), 34)), "gate": gate_table(dev, ns, N, 35)}
    outs = ["xr"]
    for i in range(nadds):
        o[f"add{i}"] = strided(rnd(dev, (M, N), 36 + i, 0.5))     # same strides as res, as the entry point requires
    if aux:
        o["aux"] = strided(torch.zeros(M, N, dtype=torch.bfloat16, device=dev))
        outs.append("aux")
    if stats:
        o["stats"] = Operand(torch.zeros(N // 96, M, 2, dtype=torch.float32, device=dev))   # this entry point wants it contiguous
        outs.append("stats")

    def fn(t):
        ops.gemm_gate_res_add(t["x"], t["w"], t["bias"], res=t["xr"], gate=t["gate"][0], gate_stride=t["gate"].stride(0), rows_per_sample=rps,
                              aux=t.get("aux"), adds=[t[f"add{i}"] for i in range(nadds)], stats=t.get("stats"), out=t["xr"])
    return fn, o, outs, ["xr"]


def b_gemm_gate2(ops, dev, B, Lt, Lv, N, K):
    L = Lt + Lv
    M = B * L
    o = {"x": Operand(rnd(dev, (M, K), 41), parent=(M, K + 64), at=(0, 64)), "w": Operand(rnd(dev, (N, K), 42, 1.0 / math.sqrt(K))),
         "bias": Operand(rnd(dev, (N,), 43, 0.1)), "xr": strided(rnd(dev, (M, N), 44)),
         "mod": Operand(rnd(dev, (B, 6 * N), 45, 0.7))}        # gate = block 2, text gate 3 N further on (block 5)

    def fn(t):
        ops.gemm_gate2(t["x"], t["w"], t["bias"], t["mod"][0, 2 * N:3 * N], 6 * N, L, Lt, 3 * N, res=t["xr"], out=t["xr"])
    return fn, o, ["xr"], ["xr"]


def b_gate_add_rows(ops, dev, B, Lt, Lv, C):
    L = Lt + Lv
    o = {"x": Operand(rnd(dev, (B * L, C), 51)), "y": Operand(rnd(dev, (B * L, C), 52)), "mod": Operand(rnd(dev, (B, 6 * C), 53, 0.7))}
    return (lambda t: ops.gate_add_rows(t["x"], t["y"], t["mod"][0, 2 * C:3 * C], L, 6 * C, Lt, 3 * C)), o, ["x"], ["x"]


def b_gemm128(ops, dev, form):
    if form == "bias_res":
        M, N, K = 700, 384, 160
        o = {"a": Operand(rnd(dev, (M, K), 61), parent=(M, K + 32), at=(0, 0)), "w": Operand(rnd(dev, (N, K), 62, 1.0 / math.sqrt(K))),
             "b": Operand(rnd(dev, (N,), 63)), "res": Operand(rnd(dev, (M, N), 64)),
             "out": strided(torch.zeros(M, N, dtype=torch.bfloat16, device=dev))}
        return (lambda t: ops.gemm128(t["a"], t["w"], t["b"], res=t["res"], out=t["out"])), o, ["out"], []
    nb, L, C = 3, 256, 64
    o = {"q": Operand(rnd(dev, (nb, L, C), 65)), "k": Operand(rnd(dev, (nb, L, C), 66)),
         "s": Operand(torch.zeros(nb, L, L, dtype=torch.float32, device=dev))}
    return (lambda t: ops.gemm128(t["q"], t["k"], out_f32=t["s"], out_scale=0.125, batch=nb, batch_a=L * C, batch_w=L * C,
                                  batch_o=L * L, M=L)), o, ["s"], []


def b_linear_small(ops, dev, M, N, K):
    o = {"x": Operand(rnd(dev, (M, K), 71), parent=(M, K + 16), at=(0, 8)), "w": Operand(rnd(dev, (N, K), 72, 1.0 / math.sqrt(K))),
         "b": Operand(rnd(dev, (N,), 73)), "out": strided(torch.zeros(M, N, dtype=torch.bfloat16, device=dev))}
    return (lambda t: ops.linear_small(t["x"], t["w"], t["b"], ops.ACT_SILU, ops.ACT_GELU_TANH, out=t["out"])), o, ["out"], []


def b_linear_skinny(ops, dev, M, N, K, pad, nsplit):
    Mp = -(-M // pad) * pad
    x = rnd(dev, (Mp, K), 81)
    dead = torch.zeros(Mp, K, dtype=torch.bool, device=dev)
    dead[M:] = True                                               # rows >= M: multiplied, never stored
    o = {"x": Operand(x, interior=dead), "w": Operand(rnd(dev, (N, K), 82, 1.0 / math.sqrt(K))),
         "r": Operand(rnd(dev, (M, N), 83), parent=(M, N + 16), at=(0, 8))}     # in place on the residual stream, M rows only
    split = ops.skinny_split(N, Mp, K) if nsplit is None else nsplit
    o["part"] = Operand(torch.zeros(split * N * Mp, dtype=torch.float32, device=dev), scratch=True)

    def fn(t):
        ops.linear_skinny(t["x"], M, t["w"], res=t["r"], out=t["r"], nsplit=nsplit, part=t["part"])
    # the fp32 partials are a workspace: their content is not compared (rows >= M hold whatever the dead rows give), their guard is
    return fn, o, ["r", "part"], ["r", "part"]


def b_gemm_ln_qkv_kv(ops, dev, M, S, heads, K):
    """The spatial qkv site with the K/V epilogue.  Any wp / cs / cv are valid operands (the column order only decides which feature
    lands where); the statistics are the real ones of x.  Vt rows 72-95 are the caller's (kv_set_constant_rows), q is row-strided."""
    C, N = HD * heads, 216 * heads
    x = (rnd(dev, (M, K), 21).float() * 1.5 + rnd(dev, (M, 1), 22, 2.0).float()).to(torch.bfloat16)
    st = ops.ln_stats_buffer(M, K, dev)
    ops.ln_row_stats(x, st)
    wp = rnd(dev, (N, K), 23, 1.0 / math.sqrt(K))
    vt0 = torch.zeros(M // S, heads, VT_ROWS, S, dtype=torch.bfloat16, device=dev)
    ops.kv_set_constant_rows(vt0)
    mine = torch.zeros_like(vt0, dtype=torch.bool)
    mine[:, :, HD:] = True
    g = _kv_guard(M // S, heads)
    o = {"x": Operand(x, parent=(M, K + 64), at=(0, 64)), "wp": Operand(wp), "cs": Operand(wp.float().sum(1)),
         "cv": Operand(rnd(dev, (N,), 24, 0.1, dtype=torch.float32)), "stats": _stats_slice(dev, K // 96, M, st),
         "kw": Operand(rnd(dev, (HD,), 7, 0.5, 1.0)), "q": strided(torch.zeros(M, C, dtype=torch.bfloat16, device=dev)),
         "kp": Operand(torch.zeros(M // S, heads, S, HD, dtype=torch.bfloat16, device=dev), guard_elems=g["kp"]),
         "vt": Operand(vt0, callers=mine, guard_elems=g["vt"])}

    def fn(t):
        ops.gemm_ln_qkv_kv(t["x"], t["wp"], t["cs"], t["cv"], t["stats"], t["kw"], t["q"], t["kp"], t["vt"], S, heads)
    return fn, o, ["q", "kp", "vt"], []


def _grid_rows(ops, dev, grid, C, seed, border="zero"):
    """Storage [guard + rows + guard, C] of a VaeGrid with random interior; border / front-frame cells zero (conv input) or random."""
    buf = torch.zeros(grid.rows + 2 * grid.guard, C, dtype=torch.bfloat16, device=dev)
    rows = buf[grid.guard:grid.guard + grid.rows]
    full = rnd(dev, (grid.n, grid.T + grid.tf, grid.Hp, grid.Wp, C), seed)
    if border == "zero":
        keep = torch.zeros(grid.n, grid.T + grid.tf, grid.Hp, grid.Wp, 1, dtype=torch.bool, device=dev)
        keep[:, grid.tf:, grid.pad:grid.pad + grid.H, grid.pad:grid.pad + grid.W] = True
        full = full * keep
    rows.view(grid.n, grid.sample_rows, C)[:, :(grid.T + grid.tf) * grid.plane] = full.reshape(grid.n, -1, C)
    return buf


def b_conv(ops, dev, n, T, H, W, cin, cout, kt, res):
    grid = ops.VaeGrid(n, T, H, W, 1, kt - 1)
    og = grid.conv_out()
    o = {"a": Operand(_grid_rows(ops, dev, grid, cin, 91)),      # the grid's whole storage: border and slack rows are read by design
         "w": Operand(rnd(dev, (cout, cin * kt * 9), 92, 1.0 / math.sqrt(cin * kt * 9))), "b": Operand(rnd(dev, (cout,), 93, 0.1)),
         "out": strided(torch.zeros(og.rows, cout, dtype=torch.bfloat16, device=dev))}
    if res:
        o["res"] = Operand(rnd(dev, (og.rows, cout), 94))

    def fn(t):
        ops.conv(t["a"][grid.guard:grid.guard + grid.rows], grid, t["w"], t["b"], cin, kt, 3, out=t["out"], res=t.get("res"))
    return fn, o, ["out"], []


C0 = 1152
for _v in ((0, 8),):
    for _form in ("bias", "gelu", "gate_res", "gate_res_aux"):
        for _M in (1, 17, 127, 129, 897):
            case("gemm", ["gemm"], f"gemm {_form} M={_M}", b_gemm, _v, M=_M, N=192 if _M < 200 else C0, K=C0, form=_form)
    # both sides of every dispatch boundary: tests/test_gpu_numerics_gemm.py branch_cases(cu); cu is known on the device only
    for _i, _row in enumerate(branch_cases(256)):         # (which rows exist does not depend on the CU count; their M does)
        if _row[0].startswith("M = "):
            continue                                      # M = 1 / 17 / 127 / 129 are rows of their own above, in every form
        for _form in ("bias", "gate_res"):
            case("gemm", ["gemm"], f"gemm {_form} dispatch boundary {_i}", b_gemm, _v, M=("branch", _i), N=0, K=0, form=_form)
    case("gemm", ["gemm"], "gemm gate_res M=4864 K=4608", b_gemm, _v, M=4864, N=C0, K=4 * C0, form="gate_res")
    case("gemm", ["gemm"], "gemm bias M=4864", b_gemm, _v, M=4864, N=C0, K=C0, form="bias")
    case("gemm", ["gemm"], "gemm gate_res_aux M=38912 (config 2)", b_gemm, (0,), M=38912, N=C0, K=C0, form="gate_res_aux")
    for _M in (1, 127, 129, 897, 4864):
        case("gemm", ["gemm_stats"], f"gemm_stats M={_M}", b_gemm_stats, _v, M=_M, N=C0, K=C0 if _M != 4864 else 4 * C0)
        for _g in (False, True):
            case("gemm", ["gemm_ln"], f"gemm_ln gelu={_g} M={_M}", b_gemm_ln, _v, M=_M, N=3 * C0 if not _g else 4 * C0, K=C0, gelu=_g)
    for _n, _a, _s in ((0, False, False), (1, True, False), (2, True, True), (2, False, True)):
        for _M in (129, 897):
            case("gemm", ["gemm_gate_res_add"], f"gemm_gate_res_add adds={_n} aux={_a} stats={_s} M={_M}", b_gemm_gate_res_add, _v,
                 M=_M, N=C0, K=C0, nadds=_n, aux=_a, stats=_s)
for _M, _S, _h, _K in ((6208, 64, 16, 1152), (2048, 1024, 16, 1152), (1280, 256, 8, 576)):    # tests/test_gpu_fused_kv.py
    case("gemm", ["gemm_ln_qkv_kv"], f"gemm_ln_qkv_kv M={_M} S={_S} heads={_h}", b_gemm_ln_qkv_kv, M=_M, S=_S, heads=_h, K=_K)
case("gemm", ["gemm_gate2"], "gemm_gate2 text 226 + video 1350", b_gemm_gate2, (0, 8), B=2, Lt=226, Lv=1350, N=1920, K=1920)
case("gemm", ["gate_add_rows"], "gate_add_rows text 226 + video 131", b_gate_add_rows, B=2, Lt=226, Lv=131, C=1920)
case("gemm", ["gemm128"], "gemm128 bias + res", b_gemm128, form="bias_res")
case("gemm", ["gemm128"], "gemm128 batched fp32", b_gemm128, form="batched_f32")
for _M in (1, 2, 17):
    case("gemm", ["linear_small"], f"linear_small M={_M}", b_linear_small, M=_M, N=1152, K=256)
case("gemm", ["linear_small"], "linear_small odd N", b_linear_small, M=3, N=100, K=72)
for _M, _N, _K, _pad, _ns in ((300, 512, 2048, 384, None), (77, 256, 4096, 128, 8), (600, 1024, 512, 128, 2), (200, 512, 1056, 384, 5)):
    case("gemm", ["linear_skinny"], f"linear_skinny {_M}x{_N}x{_K} pad {_pad}", b_linear_skinny, M=_M, N=_N, K=_K, pad=_pad, nsplit=_ns)
for _p in ((1, 3, 6, 5, 128, 256, 3, True), (3, 1, 9, 7, 256, 128, 1, False), (2, 1, 16, 16, 128, 128, 1, True)):
    case("gemm", ["conv"], f"conv {_p}", b_conv, **dict(zip(("n", "T", "H", "W", "cin", "cout", "kt", "res"), _p)))


# ================================================================================================ K/V preparation and flash, head_dim 72
def _kv_guard(batch, heads):
    return dict(kp=batch * heads * 64 * HD, vt=batch * heads * VT_ROWS * 64)    # one 64-key tile of every (batch, head) image


def _vt_callers(vt):
    m = torch.zeros_like(vt, dtype=torch.bool)
    m[:, :, 73:76] = True
    m[:, :, 77:] = True
    return m


def b_prep_kv(ops, dev, batch, heads, kv_len, norm, extra_pad=0):
    C = heads * HD
    rows = batch * kv_len
    qkv = rnd(dev, (rows, 3 * C), kv_len + heads, 1.0, 0.3)
    kv_pad = ops.kv_pad_len(kv_len) + extra_pad
    g = _kv_guard(batch, heads)
    vt0 = torch.zeros(batch, heads, VT_ROWS, kv_pad, dtype=torch.bfloat16, device=dev)
    o = {"k": Operand(qkv[:, C:2 * C].contiguous(), parent=(rows, 3 * C), at=(0, C)),      # the q columns are guard
         "v": Operand(qkv[:, 2 * C:].contiguous(), parent=(rows, 3 * C), at=(0, 2 * C)),
         "kp": Operand(torch.zeros(batch, heads, kv_pad, HD, dtype=torch.bfloat16, device=dev), guard_elems=g["kp"]),
         "vt": Operand(vt0, callers=_vt_callers(vt0), guard_elems=g["vt"])}
    if norm:
        o["w"] = Operand(rnd(dev, (HD,), 7, 0.5, 1.0))
    return (lambda t: ops.attn_prep_kv(t["k"], t["v"], t.get("w"), t["kp"], t["vt"], batch, heads, kv_len)), o, ["kp", "vt"], []


def b_prep_kv_varlen(ops, dev, lens, heads, norm):
    C, total, batch = heads * HD, sum(lens), len(lens)
    kv = rnd(dev, (total, 2 * C), total, 1.0, 0.3)
    kv_pad = ops.kv_pad_len(max(lens))
    g = _kv_guard(batch, heads)
    vt0 = torch.zeros(batch, heads, VT_ROWS, kv_pad, dtype=torch.bfloat16, device=dev)
    keys0 = ops.VarlenKeys(lens, dev)
    o = {"k": Operand(kv[:, :C].contiguous(), parent=(total, 2 * C), at=(0, 0)),           # packed rows behind sum(lens) are guard
         "v": Operand(kv[:, C:].contiguous(), parent=(total, 2 * C), at=(0, C)),
         "cu": Operand(keys0.cu_seqlens, int_guard=[0]),         # a misread offset 0 is a valid row, and a different one
         "kp": Operand(torch.zeros(batch, heads, kv_pad, HD, dtype=torch.bfloat16, device=dev), guard_elems=g["kp"]),
         "vt": Operand(vt0, callers=_vt_callers(vt0), guard_elems=g["vt"])}
    if norm:
        o["w"] = Operand(rnd(dev, (HD,), 7, 0.5, 1.0))

    def fn(t):
        keys = ops.VarlenKeys(lens, dev)
        keys.cu_seqlens = t["cu"]
        ops.attn_prep_kv_varlen(t["k"], t["v"], t.get("w"), keys, t["kp"], t["vt"], heads)
    return fn, o, ["kp", "vt"], []


def _prepared(ops, dev, batch, heads, kv_len, kv_pad, norm_w, seed, lens=None):
    C = heads * HD
    kp = torch.zeros(batch, heads, kv_pad, HD, dtype=torch.bfloat16, device=dev)
    vt = torch.zeros(batch, heads, VT_ROWS, kv_pad, dtype=torch.bfloat16, device=dev)
    if lens is None:
        kv = rnd(dev, (batch * kv_len, 2 * C), seed)
        ops.attn_prep_kv(kv[:, :C], kv[:, C:], norm_w, kp, vt, batch, heads, kv_len)
    else:
        kv = rnd(dev, (sum(lens), 2 * C), seed)
        ops.attn_prep_kv_varlen(kv[:, :C], kv[:, C:], norm_w, ops.VarlenKeys(lens, dev), kp, vt, heads)
    torch.cuda.synchronize()
    return kp, vt


def b_flash(ops, dev, batch, heads, q_len, kv_len, entry, extra_pad=0):
    """entry: 'masked' (flash_attn), 'kb' (k_norm_bound), 'exact' (keys_exact)."""
    C = heads * HD
    norm = entry == "kb"
    qw = rnd(dev, (HD,), 5, 0.1, 1.0) if norm else None
    kw = rnd(dev, (HD,), 6, 0.1, 1.0) if norm else None
    kv_pad = ops.kv_pad_len(kv_len) + (0 if entry == "exact" else extra_pad)
    kp, vt = _prepared(ops, dev, batch, heads, kv_len, kv_pad, kw, q_len + kv_len)
    g = _kv_guard(batch, heads)
    ki = vi = None
    if entry != "exact":                                            # masked entry points: pad keys are poisoned
        ki = torch.zeros_like(kp, dtype=torch.bool)
        ki[:, :, kv_len:] = True
        vi = torch.zeros_like(vt, dtype=torch.bool)
        vi[:, :, :73, kv_len:] = True
        vi[:, :, 76, kv_len:] = True
    rows = batch * q_len
    o = {"q": Operand(rnd(dev, (rows, C), q_len), parent=(rows, 3 * C), at=(0, 0)),       # k / v columns of the qkv buffer are guard
         "kp": Operand(kp, interior=ki, guard_elems=g["kp"], interior_fills=("max",)),           # module docstring: the contract
         "vt": Operand(vt, interior=vi, guard_elems=g["vt"], interior_fills=("max",)),           # says finite behind kv_len
         "out": strided(torch.zeros(rows, C, dtype=torch.bfloat16, device=dev))}
    if norm:
        o["qw"] = Operand(qw)
    bound = ops.rms_key_bound(qw, kw) if norm else None
    assert not norm or bound

    def fn(t):
        ops.flash_attn(t["q"], t.get("qw"), t["kp"], t["vt"], t["out"], batch, heads, q_len, kv_len, k_norm_bound=bound,
                       keys_exact=entry == "exact")
    return fn, o, ["out"], []


def b_flash_varlen(ops, dev, heads, q_len, lens):
    C, batch = heads * HD, len(lens)
    kv_pad = ops.kv_pad_len(max(lens))
    kp, vt = _prepared(ops, dev, batch, heads, 0, kv_pad, None, q_len + sum(lens), lens=lens)
    g = _kv_guard(batch, heads)
    rows = batch * q_len
    keys0 = ops.VarlenKeys(lens, dev)
    o = {"q": Operand(rnd(dev, (rows, C), q_len), parent=(rows, 3 * C), at=(0, 0)), "kp": Operand(kp, guard_elems=g["kp"]),
         "vt": Operand(vt, guard_elems=g["vt"]), "lens": Operand(keys0.kv_lens, int_guard=[1]),   # 1 key: valid for every buffer
         "out": strided(torch.zeros(rows, C, dtype=torch.bfloat16, device=dev))}

    def fn(t):
        keys = ops.VarlenKeys(lens, dev)
        keys.kv_lens = t["lens"]
        ops.flash_attn_varlen(t["q"], None, t["kp"], t["vt"], keys, t["out"], heads, q_len)
    return fn, o, ["out"], []


KV_LENS = (1, 44, 63, 64, 65, 300, 320, 1024, 3600)
Q_LENS = (100, 257, 700, 1000)
FLASH_VARIANTS = (0, 8, 10, 23, 15, 14, 16, 17, 18)
for _kv in KV_LENS:
    case("flash72", ["attn_prep_kv"], f"attn_prep_kv kv_len={_kv}", b_prep_kv, batch=2, heads=8, kv_len=_kv, norm=_kv != 300)
    case("flash72", ["attn_prep_kv"], f"attn_prep_kv kv_len={_kv} in a longer buffer", b_prep_kv, batch=2, heads=8, kv_len=_kv, norm=True,
         extra_pad=64)
    for _q in Q_LENS:
        for _e in ("masked", "kb", "exact"):
            case("flash72", ["flash_attn"], f"flash_attn {_e} q_len={_q} kv_len={_kv}", b_flash, flash_variants=FLASH_VARIANTS,
                 batch=2, heads=8, q_len=_q, kv_len=_kv, entry=_e, extra_pad=64 if _q == 257 else 0)
case("flash72", ["flash_attn"], "flash_attn masked q_len=19456 kv_len=300 (cross attention of config 2)", b_flash,
     batch=2, heads=16, q_len=19456, kv_len=300, entry="masked")
case("flash72", ["flash_attn"], "flash_attn kb q_len=19456 kv_len=1024", b_flash, batch=1, heads=16, q_len=19456, kv_len=1024, entry="kb")
for _lens in ((300, 1, 64, 129), (17, 320)):
    for _n in (False, True):
        case("flash72", ["attn_prep_kv_varlen"], f"attn_prep_kv_varlen lens={_lens} norm={_n}", b_prep_kv_varlen, lens=_lens, heads=8, norm=_n)
    for _q in Q_LENS:
        case("flash72", ["flash_attn_varlen"], f"flash_attn_varlen lens={_lens} q_len={_q}", b_flash_varlen, flash_variants=(0, 10),
             heads=8, q_len=_q, lens=_lens)
case("flash72", ["flash_attn_varlen"], "flash_attn_varlen q_len=19456 (config 2)", b_flash_varlen, heads=16, q_len=19456, lens=(300, 41, 128, 7))


# ================================================================================================ temporal attention
def b_temporal(ops, dev, B, T, S, heads, norm_rope):
    C = heads * HD
    rows = B * T * S
    o = {"qkv": Operand(rnd(dev, (rows, 3 * C), T * 100 + S)),   # the rows behind B T S are guard: the frame clamp of attention_t3.hip
         "out": strided(torch.zeros(rows, C, dtype=torch.bfloat16, device=dev))}
    if norm_rope:
        o["qw"], o["kw"] = Operand(rnd(dev, (HD,), 1, 0.2, 1.0)), Operand(rnd(dev, (HD,), 2, 0.2, 1.0))
        ang = torch.rand(T, HD // 2, generator=torch.Generator().manual_seed(T)) * 6.0
        o["cos"] = Operand(ang.cos().repeat_interleave(2, -1).contiguous().to(dev))
        o["sin"] = Operand(ang.sin().repeat_interleave(2, -1).contiguous().to(dev))

    def fn(t):
        ops.attn_temporal(t["qkv"], C, t.get("qw"), t.get("kw"), t.get("cos"), t.get("sin"), t["out"], B, T, S, heads)
    return fn, o, ["out"], []


for _T in (1, 19, 32, 33, 38, 64):
    for _S in (9, 37, 1024):
        for _nr in (True, False):
            case("temporal", ["attn_temporal"], f"attn_temporal T={_T} S={_S} norm+rope={_nr}", b_temporal, flash_variants=(0, 22, 21, 4, 9),
                 B=1 if _S == 1024 else 2, T=_T, S=_S, heads=2, norm_rope=_nr)


# ================================================================================================ head_dim 64 path
def b_prep_kv64(ops, dev, B, H, Lt, Lv):
    D, L = 64, Lt + Lv
    C = H * D
    kv_pad = ops.kv_pad_len(L)
    qkv = rnd(dev, (B * L, 3 * C), L)
    ang = torch.rand(Lv, D // 2, generator=torch.Generator().manual_seed(L)) * 6.0
    o = {"k": Operand(qkv[:, C:2 * C].contiguous(), parent=(B * L, 3 * C), at=(0, C)),
         "v": Operand(qkv[:, 2 * C:].contiguous(), parent=(B * L, 3 * C), at=(0, 2 * C)),
         "lw": Operand(rnd(dev, (D,), 1, 0.2, 1.0)), "lb": Operand(rnd(dev, (D,), 2, 0.1)),
         "cos": Operand(ang.cos().repeat_interleave(2, -1).contiguous().to(dev)), "sin": Operand(ang.sin().repeat_interleave(2, -1).contiguous().to(dev)),
         # the buffers keep what the caller put behind kv_len only where the kernel writes nothing: compared as in-place operands
         "kp": Operand(torch.zeros(B, H, kv_pad, D, dtype=torch.bfloat16, device=dev), guard_elems=B * H * 64 * D),
         "vt": Operand(torch.zeros(B, H, D, kv_pad, dtype=torch.bfloat16, device=dev), guard_elems=B * H * 64 * D)}

    def fn(t):
        ops.attn_prep_kv64(t["k"], t["v"], t["lw"], t["lb"], t["cos"], t["sin"], Lt, t["kp"], t["vt"], B, H, L)
    return fn, o, ["kp", "vt"], ["kp", "vt"]


def b_flash64(ops, dev, B, H, Lt, Lv, kb):
    D, L = 64, Lt + Lv
    C = H * D
    qkv = rnd(dev, (B * L, 3 * C), L)
    qw, qb, kw, kb_ = rnd(dev, (D,), 1, 0.1, 1.0), rnd(dev, (D,), 2, 0.05), rnd(dev, (D,), 3, 0.1, 1.0), rnd(dev, (D,), 4, 0.05)
    ang = torch.rand(Lv, D // 2, generator=torch.Generator().manual_seed(L)) * 6.0
    cos, sin = ang.cos().repeat_interleave(2, -1).contiguous().to(dev), ang.sin().repeat_interleave(2, -1).contiguous().to(dev)
    kp, vt = ops.alloc_kv_buffers64(B, H, L, dev)
    ops.attn_prep_kv64(qkv[:, C:2 * C], qkv[:, 2 * C:], kw, kb_, cos, sin, Lt, kp, vt, B, H, L)
    torch.cuda.synchronize()
    bound = ops.ln_key_bound(qw, qb, kw, kb_) if kb else None
    assert not kb or bound
    o = {"q": Operand(qkv[:, :C].contiguous(), parent=(B * L, 3 * C), at=(0, 0)), "qw": Operand(qw), "qb": Operand(qb),
         "cos": Operand(cos), "sin": Operand(sin), "kp": Operand(kp, guard_elems=B * H * 64 * D), "vt": Operand(vt, guard_elems=B * H * 64 * D),
         "out": strided(torch.zeros(B * L, C, dtype=torch.bfloat16, device=dev))}

    def fn(t):
        ops.flash_attn64(t["q"], t["qw"], t["qb"], t["cos"], t["sin"], Lt, t["kp"], t["vt"], t["out"], B, H, L, L, k_norm_bound=bound)
    return fn, o, ["out"], []


def b_ln_modulate(ops, dev, B, Lt, Lv, C):
    L = Lt + Lv
    o = {"x": Operand(rnd(dev, (B * L, C), 1, 1.0, 0.3)), "w": Operand(rnd(dev, (C,), 2, 0.1, 1.0)), "b": Operand(rnd(dev, (C,), 3, 0.1)),
         "mod": Operand(rnd(dev, (B, 6 * C), 4, 0.3)), "out": Operand(torch.zeros(B * L, C, dtype=torch.bfloat16, device=dev))}

    def fn(t):
        ops.ln_modulate(t["x"], t["w"], t["b"], t["mod"][0, 0:C], t["mod"][0, C:2 * C], L, mod_stride=6 * C, seg_split=Lt, mod_alt=3 * C,
                        out=t["out"])
    return fn, o, ["out"], []


def b_im2col_patch(ops, dev, F, H, W):
    o = {"z": Operand(rnd(dev, (1, F, 16, H, W), 1, dtype=torch.float32))}
    return (lambda t: {"cols": ops.im2col_patch(t["z"], 2, 2)}), o, [], []


def b_unpatchify_cvx(ops, dev, B, F, Hp, Wp):
    o = {"x": Operand(rnd(dev, (B * F * Hp * Wp, 64), 1), parent=(B * F * Hp * Wp, 128), at=(0, 0))}
    return (lambda t: {"pix": ops.unpatchify_cvx(t["x"], B, F, Hp, Wp, 16, 2)}), o, [], []


for _p in ((2, 6, 20, 300), (1, 3, 226, 130), (1, 2, 30, 1000), (1, 3, 226, 2100)):
    _kw = dict(zip(("B", "H", "Lt", "Lv"), _p))
    case("d64", ["attn_prep_kv64"], f"attn_prep_kv64 {_p}", b_prep_kv64, **_kw)
    case("d64", ["flash_attn64"], f"flash_attn64 {_p}", b_flash64, flash_variants=(0, 12, 14, 15), kb=False, **_kw)
    case("d64", ["flash_attn64"], f"flash_attn64 key bound {_p}", b_flash64, flash_variants=(0, 17), kb=True, **_kw)
case("d64", ["ln_modulate"], "ln_modulate text 226 + video 131", b_ln_modulate, B=2, Lt=226, Lv=131, C=1920)
case("d64", ["im2col_patch"], "im2col_patch 3 x 30 x 46", b_im2col_patch, F=3, H=30, W=46)
case("d64", ["unpatchify_cvx"], "unpatchify_cvx 2 x 3 x 15 x 23", b_unpatchify_cvx, B=2, F=3, Hp=15, Wp=23)


# ================================================================================================ row-wise and layout kernels
LATENTS = [(19, 64, 64), (3, 90, 160), (2, 45, 77)]     # tests/test_gpu_numerics_attn_io.py
ROWS = (1, 255, 257)


def b_ln_row_stats(ops, dev, rows, C):
    o = {"x": Operand(rnd(dev, (rows, C), rows, 1.0, 0.5)), "stats": Operand(torch.zeros(C // 96, rows + 7, 2, dtype=torch.float32, device=dev))}
    keep = torch.zeros(C // 96, rows + 7, 2, dtype=torch.bool, device=dev)
    keep[:, rows:] = True                                         # rows of the buffer behind ``rows`` are not the kernel's
    o["stats"].interior = keep
    return (lambda t: ops.ln_row_stats(t["x"], t["stats"])), o, ["stats"], []


def b_adaln_modulate(ops, dev, rows, C):
    rps = max(1, rows // 2 + 1)
    ns = -(-rows // rps)
    o = {"x": Operand(rnd(dev, (rows, C), rows, 1.0, 0.5)), "mod": Operand(rnd(dev, (ns, 6 * C), 2, 0.3)),
         "out": Operand(torch.zeros(rows, C, dtype=torch.bfloat16, device=dev))}
    return (lambda t: ops.adaln_modulate(t["x"], t["mod"][0, :C], t["mod"][0, C:2 * C], rps, 6 * C, out=t["out"])), o, ["out"], []


def b_adaln_prescale(ops, dev, nsites, N, K):
    """Several sites in one launch.  The site table holds addresses, so it is built inside fn from the tensors of the run; its guard
    repeats site 0 with shift and scale exchanged — valid for the kernel, different from every real site."""
    o = {"mod": Operand(rnd(dev, (2 * K * nsites,), 9, 0.3))}
    for s in range(nsites):
        o[f"W{s}"], o[f"b{s}"] = Operand(rnd(dev, (N, K), 10 + s, 1.0 / math.sqrt(K))), Operand(rnd(dev, (N,), 20 + s, 0.1))
        o[f"Wp{s}"] = Operand(torch.zeros(N, K, dtype=torch.bfloat16, device=dev))
        o[f"cs{s}"], o[f"cv{s}"] = (Operand(torch.zeros(N, dtype=torch.float32, device=dev)) for _ in range(2))
    outs = [f"{n}{s}" for s in range(nsites) for n in ("Wp", "cs", "cv")]
    nb = -(-N // 4)

    def fn(t):
        rows = [[t[f"W{s}"].data_ptr(), t[f"b{s}"].data_ptr(), t[f"Wp{s}"].data_ptr(), t[f"cs{s}"].data_ptr(), t[f"cv{s}"].data_ptr(),
                 2 * K * s, 2 * K * s + K, N, K, nb * s] for s in range(nsites)]
        decoy = list(rows[0])
        decoy[5], decoy[6] = decoy[6], decoy[5]
        from isolation import Arena
        so = {"sites": Operand(torch.tensor(rows, dtype=torch.int64, device=dev), int_guard=decoy)}
        a = Arena(so, [], [], "nan")
        ops.adaln_prescale(a.views["sites"], nb * nsites, t["mod"])
        torch.cuda.synchronize()
        assert not a.damages("sites")
    return fn, o, outs, []


def b_mod_table(ops, dev, nblk, B, C):
    o = {"table": Operand(rnd(dev, (nblk, 6 * C), 1)), "t": Operand(rnd(dev, (B, 6 * C), 2)),
         "out": Operand(torch.zeros(nblk, B, 6 * C, dtype=torch.bfloat16, device=dev))}
    return (lambda t: ops.mod_table(t["table"], t["t"], out=t["out"])), o, ["out"], []


def b_timestep_embedding(ops, dev, B):
    o = {"t": Operand(torch.linspace(1.0, 999.0, B, device=dev))}
    return (lambda t: {"emb": ops.timestep_embedding(t["t"])}), o, [], []


def _pe_params(dev, Hp, Wp):
    return {"w": Operand(rnd(dev, (C0, 16), 1, 0.2)), "b": Operand(rnd(dev, (C0,), 2, 0.05)), "pos": Operand(rnd(dev, (Hp * Wp, C0), 3))}


def b_patch_embed(ops, dev, T, H, W, shard):
    Hp, Wp = -(-H // 2), -(-W // 2)
    o = dict(_pe_params(dev, Hp, Wp), z=Operand(rnd(dev, (1, 4, T, H, W), 4, dtype=torch.float32)))
    if shard is None:
        return (lambda t: {"x": ops.patch_embed(t["z"], t["w"], t["b"], t["pos"], 2, (1, 2, 2), C0)}), o, [], []
    Sl = -(-(Hp * Wp) // 8)
    return (lambda t: {"x": ops.patch_embed_shard(t["z"], t["w"], t["b"], t["pos"], 2, (1, 2, 2), C0, shard * Sl, Sl)}), o, [], []


def _fl_params(dev):
    return {"table": Operand(rnd(dev, (2, C0), 1, 1.0 / math.sqrt(C0))), "tv": Operand(rnd(dev, (2, C0), 2, 0.3)),
            "w": Operand(rnd(dev, (32, C0), 3, 1.0 / math.sqrt(C0))), "b": Operand(rnd(dev, (32,), 4, 0.05))}


def b_final_layer(ops, dev, T, H, W):
    Hp, Wp = -(-H // 2), -(-W // 2)
    o = dict(_fl_params(dev), x=Operand(rnd(dev, (2 * T * Hp * Wp, C0), 5, 1.0, 0.2)))
    return (lambda t: {"pix": ops.final_layer(t["x"], t["table"], t["tv"], t["w"], t["b"], 2, T, Hp, Wp, H, W, (1, 2, 2), 8)}), o, [], []


def b_final_layer_tokens(ops, dev, T, Sl):
    o = dict(_fl_params(dev), x=Operand(rnd(dev, (2 * T * Sl, C0), 5, 1.0, 0.2)))
    return (lambda t: {"tok": ops.final_layer_tokens(t["x"], t["table"], t["tv"], t["w"], t["b"], 2, T, Sl)}), o, [], []


def b_unpatchify_tokens(ops, dev, T, H, W):
    Hp, Wp = -(-H // 2), -(-W // 2)
    Sl = -(-(Hp * Wp) // 8)
    o = {"tok": Operand(rnd(dev, (8, 2, T, Sl, 32), 1, dtype=torch.float32))}
    return (lambda t: {"pix": ops.unpatchify_tokens(t["tok"], 8, 2, T, Sl, Hp, Wp, H, W, (1, 2, 2), 8)}), o, [], []


def b_add_rows(ops, dev, rows, C):
    o = {"x": Operand(rnd(dev, (rows, C), 1)), "y": Operand(rnd(dev, (rows, C), 2))}
    return (lambda t: ops.add_rows(t["x"], t["y"])), o, ["x"], ["x"]


def b_add_bcast_rows(ops, dev, rows, C):
    o = {"x": Operand(rnd(dev, (rows, C), 1)), "e": Operand(rnd(dev, (3, C), 2))}
    return (lambda t: ops.add_bcast_rows(t["x"], t["e"], 2, 3)), o, ["x"], ["x"]


def b_copy_4d(ops, dev, batch):
    """[n0, n1, n2, C] rows out of a padded source into a padded destination, with zero fill outside (n1_valid, n2_valid).  The
    descriptors of copy_4d_batch are HOST memory (validated by the entry point), so there is nothing of them to guard on the device."""
    n0, n1, n2, C = 2, 5, 7, 72
    src = Operand(rnd(dev, (n0, n1 - 1, n2 - 2, C), 1), parent=(n0, n1 + 1, n2 + 1, C + 8), at=(0, 1, 0, 0))
    dst = Operand(torch.zeros(n0, n1, n2, C, dtype=torch.bfloat16, device=dev), parent=(n0, n1, n2 + 3, C + 16), at=(0, 0, 1, 8))
    if not batch:      # the strides are those of the tensors of the run (tight or arena view)
        return ((lambda t: ops.copy_4d(t["src"], t["dst"], n0, n1, n2, C, t["src"].stride()[:3], t["dst"].stride()[:3], n1 - 1, n2 - 2)),
                {"src": src, "dst": dst}, ["dst"], [])

    def fn(t):
        ss, ds = t["src"].stride()[:3], t["dst"].stride()[:3]
        ops.copy_4d_batch(t["src"], t["dst"], [(0, 0, 1, n1, n2, C, *ss, *ds, n1 - 1, n2 - 2), (ss[0], ds[0], 1, n1, n2, C, *ss, *ds, n1 - 1, n2 - 2)])
    return fn, {"src": src, "dst": dst}, ["dst"], []


def b_cfg_step(ops, dev, T, H, W, linear):
    o = {"z": Operand(rnd(dev, (1, 4, T, H, W), 1, dtype=torch.float32)), "m": Operand(rnd(dev, (2, 8, T, H, W), 2, dtype=torch.float32))}
    if linear:
        return (lambda t: ops.cfg_linear_step(t["z"], t["m"], 7.0, 0.98, -0.03, True)), o, ["z"], ["z"]
    return (lambda t: ops.cfg_euler_step(t["z"], t["m"], 7.0, -0.033)), o, ["z"], ["z"]


for _r in ROWS:
    case("rowwise", ["ln_row_stats"], f"ln_row_stats rows={_r}", b_ln_row_stats, rows=_r, C=C0)
    case("rowwise", ["adaln_modulate"], f"adaln_modulate rows={_r}", b_adaln_modulate, rows=_r, C=C0)
    case("rowwise", ["add_rows"], f"add_rows rows={_r}", b_add_rows, rows=_r, C=C0)
    case("rowwise", ["add_rows"], f"add_rows rows={_r} width 104", b_add_rows, rows=_r, C=104)   # 13 16-byte stores: no whole wave, no whole block
    case("rowwise", ["add_bcast_rows"], f"add_bcast_rows rows={_r}", b_add_bcast_rows, rows=_r, C=C0)
    case("rowwise", ["final_layer_tokens"], f"final_layer_tokens Sl={_r}", b_final_layer_tokens, T=2, Sl=_r)
case("rowwise", ["adaln_prescale"], "adaln_prescale three sites in one launch", b_adaln_prescale, nsites=3, N=384, K=1152)
case("rowwise", ["mod_table"], "mod_table 28 blocks", b_mod_table, nblk=28, B=2, C=C0)
case("rowwise", ["timestep_embedding"], "timestep_embedding B=3", b_timestep_embedding, B=3)
for _T, _H, _W in LATENTS:
    case("rowwise", ["patch_embed"], f"patch_embed {_T}x{_H}x{_W}", b_patch_embed, T=_T, H=_H, W=_W, shard=None)
    case("rowwise", ["patch_embed_shard"], f"patch_embed_shard {_T}x{_H}x{_W} last shard", b_patch_embed, T=_T, H=_H, W=_W, shard=7)
    case("rowwise", ["final_layer"], f"final_layer {_T}x{_H}x{_W}", b_final_layer, T=_T, H=_H, W=_W)
    case("rowwise", ["unpatchify_tokens"], f"unpatchify_tokens {_T}x{_H}x{_W}", b_unpatchify_tokens, T=_T, H=_H, W=_W)
    case("rowwise", ["cfg_euler_step"], f"cfg_euler_step {_T}x{_H}x{_W}", b_cfg_step, T=_T, H=_H, W=_W, linear=False)
    case("rowwise", ["cfg_linear_step"], f"cfg_linear_step {_T}x{_H}x{_W}", b_cfg_step, T=_T, H=_H, W=_W, linear=True)
case("rowwise", ["copy_4d"], "copy_4d padded source and destination", b_copy_4d, batch=False)
case("rowwise", ["copy_4d_batch"], "copy_4d_batch two problems", b_copy_4d, batch=True)


# ================================================================================================ VAE and T5 kernels
def _grid_operand(ops, dev, grid, C, seed, border="random"):
    """A VaeGrid's storage as ONE operand: the border and front-frame cells belong to it (read by design), the guard is what lies
    outside the storage.  fn passes the grid's row view of it."""
    return Operand(_grid_rows(ops, dev, grid, C, seed, border))


def _grid_dst(ops, dev, grid, C):
    """A destination grid's storage as a pure output: the kernels write the interior cells only, so the border, the front frames,
    the slack rows of every sample and the rows around the grid are guard (``interior`` of the operand)."""
    buf = torch.zeros(grid.rows + 2 * grid.guard, C, dtype=torch.bfloat16, device=dev)
    dead = torch.ones(grid.rows + 2 * grid.guard, C, dtype=torch.bool, device=dev)
    cells = dead[grid.guard:grid.guard + grid.rows].view(grid.n, grid.sample_rows, C)[:, :(grid.T + grid.tf) * grid.plane]
    cells.view(grid.n, grid.T + grid.tf, grid.Hp, grid.Wp, C)[:, grid.tf:, grid.pad:grid.pad + grid.H, grid.pad:grid.pad + grid.W] = False
    return Operand(buf, interior=dead)


def _rows_of(t, grid):
    return t[grid.guard:grid.guard + grid.rows]


def b_group_norm(ops, dev, n, T, H, W, C, silu, spatial):
    gs, gd = ops.VaeGrid(n, T, H, W, 1, 0), ops.VaeGrid(n, T, H, W, 1, 2)
    o = {"x": _grid_operand(ops, dev, gs, C, 1), "y": _grid_dst(ops, dev, gd, C),
         "gamma": Operand(rnd(dev, (C,), 3, 0.1, 1.0)), "beta": Operand(rnd(dev, (C,), 4, 0.1))}
    if spatial:
        zd = (T, H // 2, W // 2)
        o["yb"] = Operand(rnd(dev, (n * zd[0] * zd[1] * zd[2], 2 * C), 5, 0.3, 0.5))
        return (lambda t: ops.spatial_norm_silu(_rows_of(t["x"], gs), gs, _rows_of(t["y"], gd), gd, C, t["gamma"], t["beta"], t["yb"], zd)), o, ["y"], []
    return (lambda t: ops.group_norm(_rows_of(t["x"], gs), gs, _rows_of(t["y"], gd), gd, C, t["gamma"], t["beta"], 1e-6, silu)), o, ["y"], []


def b_grid_move(ops, dev, kind):
    n, T, H, W, C = 2, 3, 5, 6, 128
    if kind == "regrid":
        gs, gd = ops.VaeGrid(n, T, H, W, 1, 0), ops.VaeGrid(n, T, 2 * H, 2 * W, 1, 0)
        call = lambda x, y: ops.regrid(x, gs, y, gd, C, up=1)
    elif kind == "subsample":
        gs, gd = ops.VaeGrid(n, T, 2 * H, 2 * W, 1, 0), ops.VaeGrid(n, T, H - 1, W - 1, 1, 0)
        call = lambda x, y: ops.subsample(x, gs, y, gd, C, 1, 2, 0, 1)
    else:
        gs, gd = ops.VaeGrid(n, T, H, W, 1, 0), ops.VaeGrid(n, 2 * T, H, W, 1, 0)
        call = lambda x, y: ops.d2s_time(x, gs, y, gd, C)
    o = {"x": _grid_operand(ops, dev, gs, 2 * C if kind == "d2s_time" else C, 1), "y": _grid_dst(ops, dev, gd, C)}
    return (lambda t: call(_rows_of(t["x"], gs), _rows_of(t["y"], gd))), o, ["y"], []


def b_blend_edge(ops, dev, axis):
    o = {"a": Operand(rnd(dev, (3, 20, 24), 1)), "b": Operand(rnd(dev, (3, 18, 24) if axis == 0 else (3, 20, 22), 2))}
    return (lambda t: ops.blend_edge(t["a"], t["b"], 6 if axis == 0 else 5, axis)), o, ["b"], ["b"]


def b_vae_first_im2col(ops, dev, kt, kcols):
    o = {"z": Operand(rnd(dev, (4, 3, 4, 5), 1))}
    params = [3.85, 2.32, 2.33, 3.06, -0.10, 0.34, 0.27, 0.98] + [0.1 * i - 0.7 for i in range(16)] + [0.01, -0.02, 0.03, 0.04]
    return (lambda t: {"cols": ops.vae_first_im2col(t["z"], kt, kcols, params)}), o, [], []


def b_extract_planar(ops, dev):
    g = ops.VaeGrid(1, 4, 5, 6, 1, 0)
    dead = torch.ones(4, 6, 5, 6, dtype=torch.bool, device=dev)
    dead[:, 2:5] = False                                          # frames 1-3 of the grid go to frames 2-4 of out; the others are not its
    o = {"x": _grid_operand(ops, dev, g, 128, 1), "out": Operand(torch.zeros(4, 6, 5, 6, dtype=torch.bfloat16, device=dev), interior=dead)}
    return (lambda t: ops.extract_planar(_rows_of(t["x"], g), g, 4, 1, t["out"], 2)), o, ["out"], []


def b_softmax_rows(ops, dev, rows, n, ld):
    s = rnd(dev, (rows, ld), 1, 3.0, dtype=torch.float32)
    dead = torch.zeros(rows, ld, dtype=torch.bool, device=dev)
    dead[:, n:] = True                                            # columns n .. ld of the scores are padding
    o = {"s": Operand(s, interior=dead), "p": Operand(torch.zeros(rows, ld, dtype=torch.bfloat16, device=dev))}
    return (lambda t: ops.softmax_rows(t["s"], n=n, out=t["p"])), o, ["p"], []


def b_t5_attention(ops, dev, B, L, H, lens, mfma):
    inner = H * 64
    o = {"qkv": Operand(rnd(dev, (B * L, 3 * inner), L)), "out": strided(torch.zeros(B * L, inner, dtype=torch.bfloat16, device=dev))}
    rel = rnd(dev, (H, 2 * L - 1), 2, dtype=torch.float32)
    if not mfma:
        o["rel"] = Operand(rel)
        o["klen"] = Operand(torch.tensor(lens, dtype=torch.int32, device=dev), int_guard=[1])
        return (lambda t: ops.t5_attention(t["qkv"], t["rel"], t["klen"], B, L, H, out=t["out"])), o, ["out"], []
    center = (L + 127) // 128 * 128 - 1
    tab = torch.zeros(H, center + (L + 63) // 64 * 64, device=dev)
    tab[:, center - (L - 1):center + L] = rel * math.log2(math.e)
    kv_pad = (L + 63) // 64 * 64
    o["tab"] = Operand(tab)
    o["wk"], o["wv"] = (Operand(torch.zeros(H * kv_pad * 64, dtype=torch.bfloat16, device=dev), scratch=True) for _ in range(2))
    # (the K / V^T workspaces: their guard is checked, their content belongs to the kernel pair)
    return ((lambda t: ops.t5_attention_mfma(t["qkv"], t["tab"], center, lens, B, L, H, out=t["out"], ws=(t["wk"], t["wv"]))), o,
            ["out", "wk", "wv"], ["wk", "wv"])


def b_t5_rows(ops, dev, kind):
    if kind == "gather_rows":
        o = {"table": Operand(rnd(dev, (100, 512), 1)), "ids": Operand(torch.tensor([5, 99, 0, 17, 5, 42, 1], dtype=torch.int64, device=dev), int_guard=[3])}
        return (lambda t: {"rows": ops.gather_rows(t["table"], t["ids"])}), o, [], []
    if kind == "rms_norm_rows":
        o = {"x": Operand(rnd(dev, (77, 1024), 1)), "w": Operand(rnd(dev, (1024,), 2, 0.1, 1.0)),
             "out": Operand(torch.zeros(77, 1024, dtype=torch.bfloat16, device=dev))}
        return (lambda t: ops.rms_norm_rows(t["x"], t["w"], out=t["out"])), o, ["out"], []
    o = {"h": Operand(rnd(dev, (77, 1024), 1)), "out": Operand(torch.zeros(77, 512, dtype=torch.bfloat16, device=dev))}
    return (lambda t: ops.geglu(t["h"], out=t["out"])), o, ["out"], []


for _p in ((2, 1, 10, 6, 128, True), (1, 3, 6, 6, 1024, True), (3, 1, 8, 8, 256, False)):
    case("vae_t5", ["group_norm"], f"group_norm {_p}", b_group_norm, spatial=False, **dict(zip(("n", "T", "H", "W", "C", "silu"), _p)))
case("vae_t5", ["spatial_norm_silu"], "spatial_norm_silu 2 x 2 x 6 x 8 x 128", b_group_norm, n=2, T=2, H=6, W=8, C=128, silu=True, spatial=True)
for _k in ("regrid", "subsample", "d2s_time"):
    case("vae_t5", [_k], _k, b_grid_move, kind=_k)
for _a in (0, 1):
    case("vae_t5", ["blend_edge"], f"blend_edge axis {_a}", b_blend_edge, axis=_a)
for _kt, _kc in ((3, 128), (1, 64)):
    case("vae_t5", ["vae_first_im2col"], f"vae_first_im2col kt={_kt}", b_vae_first_im2col, kt=_kt, kcols=_kc)
case("vae_t5", ["extract_planar"], "extract_planar with a frame skip", b_extract_planar)
case("vae_t5", ["softmax_rows"], "softmax_rows 37 x 200 of 256", b_softmax_rows, rows=37, n=200, ld=256)
for _p in ((2, 150, 4, (150, 97)), (1, 300, 8, (120,)), (2, 77, 2, (1, 77))):
    for _m in (False, True):
        case("vae_t5", ["t5_attention_mfma" if _m else "t5_attention"], f"t5_attention{'_mfma' if _m else ''} {_p}", b_t5_attention,
             mfma=_m, **dict(zip(("B", "L", "H", "lens"), _p)))
for _k in ("gather_rows", "rms_norm_rows", "geglu"):
    case("vae_t5", [_k], _k, b_t5_rows, kind=_k)


# ================================================================================================ what has no case, and why
NOT_COVERED = {
    # host-side helpers: no kernel is launched
    "ln_stats_buffer": "allocator (host side)",
    "kv_pad_len": "host arithmetic",
    "alloc_kv_buffers": "allocator (host side)",
    "alloc_kv_buffers64": "allocator (host side)",
    "qkv_kv_column_order": "host-side index table",
    "gemm_ln_qkv_kv_dispatched": "host-side dispatch query, no launch",
    "kv_set_constant_rows": "torch fills at set-up time, no kernel of the library",
    "rms_key_bound": "host arithmetic on two weight vectors",
    "ln_key_bound": "host arithmetic on the norm weights",
    "static_max_allowed": "reads the VSYS_FLASH_STATIC switch (host side), no launch",
    "skinny_split": "host arithmetic",
    # out of scope of the guard-band tests
    "p2p_exchange": "peer-to-peer exchange: writes into other processes' memory by design, needs several ranks",
    "collectives": "collectives run outside the library's kernels (torch.distributed)",
    "recorded_programs": "a recorded program replays the same entry points with the same arguments: covered call by call",
}


def covered_ops():
    return {name for c in CASES for name in c.ops}
