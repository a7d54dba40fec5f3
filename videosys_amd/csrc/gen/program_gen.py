#!/usr/bin/env python
"""Generate the launch-program dispatch (csrc/program_ops.inc), the VSYS_OP_* block of include/videosys_amd.h and the host mirror
(videosys_amd/_opcodes.py: op codes + the argument / return kinds of EVERY entry point, which videosys_amd/_lib.py turns into the
ctypes table) from the prototypes of include/videosys_amd.h and include/videosys_amd_lab.h.

The rule: every extern "C" entry point whose last parameter is ``void* stream`` and whose arguments fit a vsys_cmd (VSYS_CMD_MAX_INT
integer / pointer, VSYS_CMD_MAX_FLOAT float) gets an op code; the only exception is vsys_attn_temporal_d64_img with 26 integer /
pointer arguments (NO_OP below, checked against the header on every run).  Existing codes are kept (they are ABI), new entry points
are numbered after the highest one.  A command carries the entry point's integer / pointer arguments in declaration order in a[] and
its float arguments in f[] (include/videosys_amd.h "Launch programs"); the generated switch casts them back to the prototype's
parameter types, so vsys_program_run — and with it torch.ops.vsys.launch / program_run (csrc/torch_binding.cpp) — reaches every such
kernel through the same functions a direct caller binds.

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
# the launch entry points that do NOT fit a command record and so have no op code (checked in ops_of).  vsys_attn_temporal_d64_img: 26
# integer / pointer arguments against VSYS_CMD_MAX_INT = 24, and growing the record is an ABI change; a recorded sequence-parallel
# Vchitect step issues it from the host action of the collective it feeds (vchitect_ops.attn_temporal64_img)
NO_OP = {"vsys_attn_temporal_d64_img"}
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


def counts(kinds):
    """(integer / pointer arguments, float arguments) of a kind list: the a[] and f[] slots a command needs."""
    nf = sum(1 for k, _ in kinds if k == "f")
    return len(kinds) - nf, nf


def ops_of(protos, cap_i, cap_f):
    """The prototypes that get an op code, as (name, kinds without the stream): last parameter ``void* stream`` and at most cap_i
    integer / pointer and cap_f float arguments.  The ones left out must be exactly NO_OP."""
    launch = [(name, kinds[:-1]) for name, kinds, _, launches in protos if launches]
    wide = {name: counts(kinds) for name, kinds in launch if counts(kinds)[0] > cap_i or counts(kinds)[1] > cap_f}
    if set(wide) != NO_OP:
        raise SystemExit(f"NO_OP = {sorted(NO_OP)}, but the launch entry points that do not fit a vsys_cmd ({cap_i} integer / {cap_f} float "
                         f"arguments) are {wide}: every entry point that fits gets a code, one that does not is named there with the reason")
    return [e for e in launch if e[0] not in wide]


def build():
    h = open(HDR).read()
    protos, lab_protos = parse(h), parse(open(LAB_HDR).read())
    cap_i, cap_f = (int(re.search(rf"#define VSYS_CMD_MAX_{w}\s+(\d+)", h).group(1)) for w in ("INT", "FLOAT"))
    entries = ops_of(protos, cap_i, cap_f)
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
    max_i, max_f = (max(counts(kinds)[w] for _, kinds in entries) for w in (0, 1))
    # ---- header block
    lines = [BEGIN]
    for name, _ in by_code:
        lines.append(f"#define VSYS_OP_{name[5:].upper():28s} {codes[name]}")
    lines += [f"#define VSYS_OP_COUNT {count}", END]
    block = "\n".join(lines)
    h2 = h[:h.index(BEGIN)] + block + h[h.index(END) + len(END):]
    # ---- dispatch
    inc = ["// GENERATED by csrc/gen/program_gen.py from include/videosys_amd.h — do not edit.",
           f"static_assert(VSYS_CMD_MAX_INT >= {max_i} && VSYS_CMD_MAX_FLOAT >= {max_f}, \"vsys_cmd is too small for the widest entry point\");",
           "#ifdef VSYS_PROGRAM_TABLE", "constexpr OpInfo kOps[VSYS_OP_COUNT] = {", "    {0, 0},"]
    table = {codes[n]: counts(ks) + (n,) for n, ks in entries}
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
