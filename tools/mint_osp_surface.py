#!/usr/bin/env python
"""Mint tests/golden/osp_pipeline_surface.json: parameter names and defaults of the reference's OpenSoraPlanV120PABConfig.__init__,
OpenSoraPlanConfig.__init__, OpenSoraPlanPipeline.__init__, .generate, .encode_prompt_v120 and .prepare_latents, and the names of the
public methods of OpenSoraPlanPipeline, read from the reference's source with ``ast`` as tools/mint_vchitect_surface.py does.

    python tools/mint_osp_surface.py <reference>/videosys/pipelines/open_sora_plan/pipeline_open_sora_plan.py
"""
import ast
import json
import os
import sys

from mint_vchitect_surface import params

WANT = {("OpenSoraPlanV120PABConfig", "__init__"), ("OpenSoraPlanConfig", "__init__"), ("OpenSoraPlanPipeline", "__init__"),
        ("OpenSoraPlanPipeline", "generate"), ("OpenSoraPlanPipeline", "encode_prompt_v120"), ("OpenSoraPlanPipeline", "prepare_latents")}


def main():
    tree = ast.parse(open(sys.argv[1]).read())
    out = {}
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef):
            for fn in cls.body:
                if isinstance(fn, ast.FunctionDef) and (cls.name, fn.name) in WANT:
                    out[f"{cls.name}.{fn.name}"] = params(fn)
            if cls.name == "OpenSoraPlanPipeline":
                out["OpenSoraPlanPipeline.methods"] = [fn.name for fn in cls.body if isinstance(fn, ast.FunctionDef) and not fn.name.startswith("__")]
    assert len(out) == len(WANT) + 1, sorted(out)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "osp_pipeline_surface.json")
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
