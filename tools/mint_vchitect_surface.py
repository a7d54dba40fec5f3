#!/usr/bin/env python
"""Mint tests/golden/vchitect_pipeline_surface.json: parameter names and defaults of the reference's VchitectPABConfig.__init__,
VchitectConfig.__init__, VchitectXLPipeline.__init__ and VchitectXLPipeline.generate, read from the reference's source with ``ast``
(the module itself needs diffusers to import).  A default that is a Python literal is stored as its value, any other as its source
text (``torch.device('cuda')``, ``torch.bfloat16``, ``VchitectPABConfig()``).

    python tools/mint_vchitect_surface.py <reference>/videosys/pipelines/vchitect/pipeline_vchitect.py
"""
import ast
import json
import os
import sys

WANT = {("VchitectPABConfig", "__init__"), ("VchitectConfig", "__init__"), ("VchitectXLPipeline", "__init__"), ("VchitectXLPipeline", "generate")}


def params(fn: ast.FunctionDef):
    args = fn.args.args[1:]          # without self
    defaults = [None] * (len(args) - len(fn.args.defaults)) + list(fn.args.defaults)
    out = []
    for a, d in zip(args, defaults):
        if d is None:
            out.append({"name": a.arg, "required": True})
            continue
        try:
            out.append({"name": a.arg, "default": ast.literal_eval(d)})
        except ValueError:
            out.append({"name": a.arg, "default_source": ast.unparse(d)})
    return out


def main():
    tree = ast.parse(open(sys.argv[1]).read())
    out = {}
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef):
            for fn in cls.body:
                if isinstance(fn, ast.FunctionDef) and (cls.name, fn.name) in WANT:
                    out[f"{cls.name}.{fn.name}"] = params(fn)
    assert len(out) == len(WANT), sorted(out)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "vchitect_pipeline_surface.json")
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
