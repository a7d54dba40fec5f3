"""Static instruction mix of a GEMM kernel's K loop and of everything behind it (the epilogue) — no GPU needed.

    python tools/epilogue_mix.py videosys_amd/csrc/gemm_bf16.hip videosys_amd/csrc/gemm2_bf16.hip [--kernel SUBSTRING ...] [--out FILE.json]

Each source is cross-compiled to gfx950 assembly (hipcc -S, the flags of the build).  For every named kernel (default: the gate +
residual kernels of the N = 1152 launches and the two-workgroup kernels of qkv / cross-q / fc1): the K loop = the innermost
backward-branch loop that holds the most v_mfma instructions, and "after" = every instruction between that loop's backward branch
and the end of the kernel.  Instructions are classed by PREFIX only (first match): v_mfma, transcendental, v_pk_, v_cvt, other v_,
ds_, buffer_ / global_, s_waitcnt, the rest.  Counts are per wave as the compiler laid the code out; "after" holds every store
phase the kernel has (full tile, ragged tile, PAB operands), so it is an upper bound on what one launch executes.
tools/isa_mix.py reads a built object and reports the hot loop only; this one reads the source's assembly and reports both sides."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videosys_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]

CLASSES = [
    ("v_mfma", r"^v_mfma|^v_smfmac"),
    ("transcendental", r"^v_(exp|log|rcp|rsq|sqrt|sin|cos)_"),
    ("v_pk_", r"^v_pk_"),
    ("v_cvt", r"^v_cvt"),
    ("other v_", r"^v_"),
    ("ds_", r"^ds_"),
    ("buffer_ / global_", r"^buffer_|^global_"),
    ("s_waitcnt", r"^s_waitcnt"),
    ("rest", r"."),
]
DEFAULT_KERNELS = {
    "gemm_bf16.hip": ["gemm_kernel<2, 8, 256, 1, 0, 1, 0>", "gemm_kernel<5, 8, 256, 1, 0, 1, 0>"],
    "gemm2_bf16.hip": ["gemm2_kernel<0, 2, 0, 1>", "gemm2_kernel<3, 2, 0, 1>", "gemm2_kernel<4, 2, 0, 1>"],
}


def _tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def assembly(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([os.environ.get("HIPCC") or _tool("hipcc")] + FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.abspath(src)],
                       check=True, capture_output=True, cwd=os.path.dirname(os.path.abspath(src)))
        with open(out) as fh:
            return fh.read()


def functions(asm):
    """{mangled name: [(label or None, mnemonic or None, operands)]} for every kernel body between its label and .Lfunc_end."""
    out, cur = collections.OrderedDict(), None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            cur.append((m.group(1), None, ""))
            continue
        code = line.split(";")[0].strip()
        if not code or code.startswith("."):
            continue
        parts = code.split(None, 1)
        cur.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def demangle(names):
    """name<integer template arguments> of a kernel symbol (``...11gemm_kernelILi5ELi8E...EEv...`` -> ``gemm_kernel<5, 8, ...>``); the
    symbol itself where it has another form.  (No c++filt needed: the kernels here take integers and booleans only.)"""
    out = {}
    for sym in names:
        out[sym] = sym
        for m in re.finditer(r"\d+", sym):
            for p in range(m.start(), m.end()):      # a digit run may end a nested name and begin the length prefix
                n = int(sym[p:m.end()])
                t = re.match(r"I((?:L[a-z]n?\d+E)+)E", sym[m.end() + n:])
                if out[sym] == sym and t and re.fullmatch(r"[A-Za-z_]\w*", sym[m.end():m.end() + n] or "0"):
                    args = [("-" if a[1] else "") + a[2] for a in re.findall(r"L([a-z])(n?)(\d+)E", t.group(1))]
                    out[sym] = f"{sym[m.end():m.end() + n]}<{', '.join(args)}>"
    return out


def k_loop(body):
    """(first index, index of the backward branch) of the innermost loop with the most MFMAs."""
    label_at = {lab: i for i, (lab, _, _) in enumerate(body) if lab}
    loops = []
    for i, (_, op, args) in enumerate(body):
        if op and op.startswith(("s_cbranch", "s_branch")):
            t = label_at.get(args.strip())
            if t is not None and t <= i:
                loops.append((t, i))

    def mfma(s, e):
        return sum(1 for _, op, _ in body[s:e + 1] if op and op.startswith("v_mfma"))

    best = None
    for s, e in loops:
        n = mfma(s, e)
        inner = not any((s2, e2) != (s, e) and s <= s2 and e2 <= e and mfma(s2, e2) >= max(1, n // 2) for s2, e2 in loops)
        if n and inner and (best is None or (n, s - e) > best[0]):
            best = ((n, s - e), s, e)
    return None if best is None else best[1:]


def classify(op):
    for name, pat in CLASSES:
        if re.search(pat, op):
            return name
    return "rest"


def mix(ins):
    ops = [op for _, op, _ in ins if op]
    cls = collections.Counter(classify(op) for op in ops)
    v = collections.Counter(op for op in ops if op.startswith("v_") and not op.startswith(("v_mfma", "v_smfmac")))
    return {"classes": {name: cls[name] for name, _ in CLASSES if cls[name]},
            "valu_non_mfma": sum(v.values()),
            "top_v": [[op, n] for op, n in v.most_common(12)]}


def report(src, wanted):
    fns = functions(assembly(src))
    names = demangle(list(fns))
    out = collections.OrderedDict()
    for want in wanted:
        hits = [m for m in fns if want in names[m] or want in m]
        if not hits:
            raise SystemExit(f"{src}: no kernel matches {want!r}")
        for m in hits:
            body = fns[m]
            loop = k_loop(body)
            if loop is None:
                raise SystemExit(f"{names[m]}: no loop with MFMAs")
            s, e = loop
            out[names[m]] = {"k_loop": mix(body[s:e + 1]), "after": mix(body[e + 1:])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--kernel", action="append", default=None, help="substring of a demangled kernel name (default: the hot GEMM kernels)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = collections.OrderedDict()
    for src in a.sources:
        res[os.path.basename(src)] = report(src, a.kernel or DEFAULT_KERNELS.get(os.path.basename(src), []))
    for src, ks in res.items():
        for k, r in ks.items():
            print(f"== {src}: {k}")
            for side in ("k_loop", "after"):
                c = r[side]["classes"]
                print(f"   {side:7s} non-MFMA VALU {r[side]['valu_non_mfma']:5d} | " + ", ".join(f"{n} {c[n]}" for n in c))
            print("   after, most frequent v_*: " + ", ".join(f"{o} x{n}" for o, n in r["after"]["top_v"]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
