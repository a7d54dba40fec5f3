#!/usr/bin/env python
"""Are two device assemblies (hipcc -S --cuda-device-only) the same code?  CPU only, compares text.

    python tools/isa_same.py A.s B.s [--json OUT]

Per kernel symbol it reports
  1. whether the symbol exists in both files;
  2. the resource metadata (.vgpr_count, .agpr_count, .sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size,
     .sgpr_spill_count, .vgpr_spill_count) of both and whether it is equal;
  3. whether the inline-asm statements (the text between ;;#ASMSTART and ;;#ASMEND) are equal, statement by statement in order;
  4. whether the compiler-generated instructions around them have the same mnemonic sequence; lines whose mnemonics agree and
     whose operands differ are counted, apart those that only swap sources (same destination, same multiset of sources — what
     a commutative instruction may do), which are allowed.
Exit status 0 when 1-4 hold for every kernel, 1 otherwise."""
import argparse
import json
import re
import sys

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".sgpr_spill_count", ".vgpr_spill_count")


def parse(path):
    """{kernel: {"meta": {...}, "asm": [statement text, ...], "code": [(mnemonic, [operand, ...]), ...]}}"""
    with open(path) as fh:
        lines = fh.read().split("\n")
    kernels = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    out = {k: {"meta": {}, "asm": [], "code": []} for k in kernels}
    cur, stmt = None, None
    for ln in lines:
        m = re.match(r"(\S+):", ln)
        if m and m.group(1) in out:
            cur = out[m.group(1)]
            continue
        t = ln.strip()
        if cur is None or not t:
            continue
        if t.startswith(".amdhsa_kernel") or t.startswith(".Lfunc_end"):
            cur = None
        elif "#ASMSTART" in t:
            stmt = []
        elif "#ASMEND" in t:
            cur["asm"].append("\n".join(stmt))
            stmt = None
        elif stmt is not None:
            stmt.append(t)
        elif not t.startswith((".", ";")) and not re.match(r"\S+:\s*(;.*)?$", t):
            code = t.split(";")[0].split(None, 1)
            cur["code"].append((code[0], [o.strip() for o in code[1].split(",")] if len(code) > 1 else []))
    # the amdhsa.kernels metadata: one "  - .key: value" block per kernel
    block = {}
    for ln in lines + ["  - "]:
        if ln.startswith("  - "):
            if block.get(".name") in out:
                out[block[".name"]]["meta"] = {k: block.get(k) for k in META_KEYS}
            block = {}
        m = re.match(r"\s+(?:- )?(\.\w+):\s*(\S+)\s*$", ln)
        if m:
            block[m.group(1)] = m.group(2)
    return out


def compare(a, b):
    res = {}
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            res[k] = {"in_both": False, "same": False}
            continue
        ka, kb = a[k], b[k]
        ca, cb = ka["code"], kb["code"]
        mnem_same = [x[0] for x in ca] == [x[0] for x in cb]
        swapped = other = 0
        if mnem_same:
            for (_, oa), (_, ob) in zip(ca, cb):
                if oa != ob:
                    if oa[:1] == ob[:1] and sorted(oa[1:]) == sorted(ob[1:]):
                        swapped += 1
                    else:
                        other += 1
        r = {"in_both": True,
             "meta_a": ka["meta"], "meta_same": ka["meta"] == kb["meta"] and None not in ka["meta"].values(),
             "asm_statements": [len(ka["asm"]), len(kb["asm"])], "asm_same": ka["asm"] == kb["asm"],
             "instructions": [len(ca), len(cb)], "mnemonics_same": mnem_same,
             "operands_swapped_sources": swapped, "operands_other": other}
        if not r["meta_same"]:
            r["meta_b"] = kb["meta"]
        r["same"] = r["meta_same"] and r["asm_same"] and mnem_same and other == 0
        res[k] = r
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--json", help="write the per-kernel summary here")
    args = ap.parse_args()
    res = compare(parse(args.a), parse(args.b))
    for k, r in res.items():
        if not r["in_both"]:
            print(f"DIFF {k}: in one file only")
            continue
        what = [n for n, ok in (("metadata", r["meta_same"]), ("asm statements", r["asm_same"]), ("mnemonics", r["mnemonics_same"]),
                                ("operands", r["operands_other"] == 0)) if not ok]
        print(f"{'same' if r['same'] else 'DIFF'} {k}: {r['instructions'][0]} instructions, {r['asm_statements'][0]} asm statements, "
              f"{r['operands_swapped_sources']} swapped-source lines" + (": " + ", ".join(what) + " differ" if what else ""))
    ok = bool(res) and all(r["same"] for r in res.values())
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"a": args.a, "b": args.b, "all_same": ok, "kernels": res}, fh, indent=1)
            fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
