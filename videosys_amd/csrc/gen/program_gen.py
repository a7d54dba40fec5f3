#!/usr/bin/env python
"""Generate the launch-program dispatch (csrc/program_ops.inc), the VSYS_OP_* block of include/videosys_amd.h and the host mirror
(videosys_amd/_opcodes.py: op codes + the argument / return kinds of EVERY entry point, which videosys_amd/_lib.py turns into the
ctypes table) from the prototypes of include/videosys_amd.h and include/videosys_amd_lab.h.

Every extern "C" entry point whose last parameter is ``void* stream`` gets an op code: existing codes are kept (they are ABI), new
entry points are numbered after the highest one.  A command carries the entry point's integer / pointer arguments in declaration
order in a[] and its float arguments in f[] (include/videosys_amd.h "Launch programs"); the generated switch casts them back to the
prototype's parameter types, so vsys_program_run — and with it torch.ops.vsys.launch / program_run (csrc/torch_binding.cpp) — reaches
EVERY kernel of the library through the same functions a direct caller binds.

    python videosys_amd/csrc/gen/program_gen.py          rewrites the three outputs in place (idempotent)
    python videosys_amd/csrc/gen/program_gen.py --check  exit 1 if any output is stale (tests/test_host_cpu.py)
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
HDR = os.path.join(ROOT, "include", "videosys_amd.h")
LAB_HDR = os.path.join(ROOT, "include", "videosys_amd_lab.h")
INC = os.path.join(ROOT, "videosys_amd", "csrc", "program_ops.inc")
PYM = os.path.join(ROOT, "videosys_amd", "_opcodes.py")
# entry points with a stream that stay OUT of the op table: they run once per video outside the denoise step, so nothing records them,
# and the table's size is pinned where it was when the Vchitect transformer was added (tests/test_vchitect_cpu.py)
# (vsys_attn_temporal_d64_img: a recorded sequence-parallel step issues it from the host closure of the collective it feeds;
#  vsys_attn_prep_kv96 / vsys_flash_attn_d96: a recorded Open-Sora-Plan step replays them from host closures, open_sora_plan_ops.py;
#  vsys_attn_prep_kv96_img / vsys_flash_attn_d96_img: the same, on the exchange image of a sequence-parallel step;
#  vsys_attn_prep_kv_rope / vsys_flash_attn_d72_rope: the same for Open-Sora-Plan v1.1, open_sora_plan_v110_ops.py;
#  vsys_cfg_ancestral_step: the Open-Sora-Plan sampler launches it from the host after each replay, its scalars change every step;
#  vsys_cfg_pndm_step: the same for the v1.1 sampler, whose pointers rotate as well; vsys_upsample_time2x: the v1.1 VAE decode)
NO_OP = {"vsys_vae_first_im2col_nc", "vsys_pixels_to_u8", "vsys_clip_attention_d64", "vsys_splitk_reduce_bias_act",
         "vsys_attn_temporal_d64_img", "vsys_attn_prep_kv96", "vsys_flash_attn_d96", "vsys_upsample_trilinear2x",
         "vsys_cfg_ancestral_step", "vsys_pixels_to_u8_trunc", "vsys_attn_prep_kv96_img", "vsys_flash_attn_d96_img",
         "vsys_attn_prep_kv_rope", "vsys_flash_attn_d72_rope", "vsys_upsample_time2x", "vsys_cfg_pndm_step"}
BEGIN, END = "/* >>> VSYS_OP codes (generated: csrc/gen/program_gen.py) */", "/* <<< VSYS_OP codes */"


def parse(h):
    """Every extern "C" prototype of a header, in declaration order: (name, [(kind, C type), ...], return kind, launches).  Kinds:
    p pointer, l int64_t, i int, f float, s const char* (return only).  ``launches``: the last parameter is ``void* stream`` (it is
    part of the kind list like any other parameter)."""
    out = []
    for ret, name, args in re.findall(r"\n(int|const char\*) (vsys_\w+)\(([^;]*?)\);", h, flags=re.S):
        params = [x.strip() for x in re.sub(r"\s+", " ", args).split(",")]
        kinds = []
        for p in ([] if params == ["void"] else params):
            ty = p.rsplit(" ", 1)[0].strip()
            kind = "f" if ty == "float" else "p" if ty.endswith("*") else {"int64_t": "l", "int": "i"}.get(ty)
            if kind is None:
                raise SystemExit(f"{name}: parameter type {ty!r} has no vsys_cmd / ctypes representation")
            kinds.append((kind, ty))
        out.append((name, kinds, "i" if ret == "int" else "s", params[-1] == "void* stream"))
    return out


def ops_of(protos):
    """The prototypes that get an op code: last parameter ``void* stream`` and not in NO_OP; (name, kinds without the stream)."""
    return [(name, kinds[:-1]) for name, kinds, _, launches in protos if launches and name not in NO_OP]


def build():
    h = open(HDR).read()
    protos, lab_protos = parse(h), parse(open(LAB_HDR).read())
    entries = ops_of(protos)
    old = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VSYS_OP_(\w+)\s+(\d+)", h) if m.group(1) != "COUNT"}
    codes, nxt = {}, max(old.values(), default=0) + 1
    for name, _ in entries:
        key = name[len("vsys_"):].upper()
        if key in old:
            codes[name] = old[key]
    for name, _ in entries:
        if name not in codes:
            codes[name] = nxt
            nxt += 1
    count = max(codes.values()) + 1
    by_code = sorted(entries, key=lambda e: codes[e[0]])
    max_i = max(sum(1 for k, _ in kinds if k != "f") for _, kinds in entries)
    max_f = max(sum(1 for k, _ in kinds if k == "f") for _, kinds in entries)
    # ---- header block
    lines = [BEGIN]
    for name, _ in by_code:
        lines.append(f"#define VSYS_OP_{name[5:].upper():28s} {codes[name]}")
    lines += [f"#define VSYS_OP_COUNT {count}", END]
    block = "\n".join(lines)
    if BEGIN in h:
        h2 = h[:h.index(BEGIN)] + block + h[h.index(END) + len(END):]
    else:   # first run: replace the hand-written run of defines
        m = list(re.finditer(r"#define VSYS_OP_\w+[^\n]*\n", h))
        h2 = h[:m[0].start()] + block + "\n" + h[m[-1].end():]
    # ---- dispatch
    inc = ["// GENERATED by csrc/gen/program_gen.py from include/videosys_amd.h — do not edit.",
           f"static_assert(VSYS_CMD_MAX_INT >= {max_i} && VSYS_CMD_MAX_FLOAT >= {max_f}, \"vsys_cmd is too small for the widest entry point\");",
           "#ifdef VSYS_PROGRAM_TABLE", "constexpr OpInfo kOps[VSYS_OP_COUNT] = {", "    {0, 0},"]
    table = {codes[n]: (sum(1 for k, _ in ks if k != "f"), sum(1 for k, _ in ks if k == "f"), n) for n, ks in entries}
    for c in range(1, count):
        ni, nf, n = table.get(c, (0, 0, "(unused)"))
        inc.append(f"    {{{ni}, {nf}}},   // {c} {n}")
    inc += ["};", "#endif", "#ifdef VSYS_PROGRAM_CASES"]
    for name, kinds in by_code:
        args, ii, fi = [], 0, 0
        for k, ty in kinds:
            if k == "f":
                args.append(f"c.f[{fi}]")
                fi += 1
            elif k == "p":
                args.append(f"reinterpret_cast<{ty}>(c.a[{ii}])")
                ii += 1
            else:
                args.append(f"static_cast<{ty}>(c.a[{ii}])")
                ii += 1
        inc.append(f"        case VSYS_OP_{name[5:].upper()}: rc = {name}({', '.join(args + ['st'])}); break;")
    inc += ["#endif", ""]
    py = ['"""GENERATED by csrc/gen/program_gen.py from include/videosys_amd.h and include/videosys_amd_lab.h — do not edit."""',
          "# entry point -> VSYS_OP code", "OPCODES = {"]
    for name, _ in by_code:
        py.append(f'    "{name}": {codes[name]},')
    py += ["}", f"N_INT, N_FLOAT = {max(max_i, 20)}, {max(max_f, 2)}   # minimum capacity of a vsys_cmd (VSYS_CMD_MAX_INT / _FLOAT)"]
    for var, ps, what in (("ENTRY_POINTS", protos, "videosys_amd.h"), ("LAB_ENTRY_POINTS", lab_protos, "videosys_amd_lab.h (-DVSYS_LAB builds)")):
        py += [f"# every prototype of include/{what}: entry point -> (parameter kinds, return kind); p pointer, l int64_t, i int, f float,",
               "# s const char*; a trailing stream is the last p", f"{var} = {{"]
        py += [f'    "{name}": ("{"".join(k for k, _ in kinds)}", "{ret}"),' for name, kinds, ret, _ in ps]
        py.append("}")
    py.append("")
    return {HDR: h2, INC: "\n".join(inc), PYM: "\n".join(py)}, max_i, max_f


def main():
    outs, max_i, max_f = build()
    stale = [p for p, t in outs.items() if not os.path.exists(p) or open(p).read() != t]
    if "--check" in sys.argv:
        if stale:
            print("stale:", stale)
            sys.exit(1)
        return
    for p in stale:
        with open(p, "w") as fh:
            fh.write(outs[p])
        print("wrote", os.path.relpath(p, ROOT))
    print(f"widest entry point: {max_i} integer / {max_f} float arguments")


if __name__ == "__main__":
    main()
