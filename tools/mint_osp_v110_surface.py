#!/usr/bin/env python
"""Mint tests/golden/osp_v110_pipeline_surface.json: parameter names and defaults of the reference's OpenSoraPlanV110PABConfig.__init__
(both MLP tables included), OpenSoraPlanConfig.__init__, OpenSoraPlanPipeline.__init__, .encode_prompt (the v1.1 text path) and
.generate, read from the reference's source with ``ast`` as tools/mint_osp_surface.py does.  Data only.

    python tools/mint_osp_v110_surface.py <reference>/videosys/pipelines/open_sora_plan/pipeline_open_sora_plan.py [--check]
"""
import ast
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mint_vchitect_surface import params  # noqa: E402

WANT = {("OpenSoraPlanV110PABConfig", "__init__"), ("OpenSoraPlanConfig", "__init__"), ("OpenSoraPlanPipeline", "__init__"),
        ("OpenSoraPlanPipeline", "generate"), ("OpenSoraPlanPipeline", "encode_prompt")}
DST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "osp_v110_pipeline_surface.json")


def mint(path):
    tree = ast.parse(open(path).read())
    out = {}
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef):
            for fn in cls.body:
                if isinstance(fn, ast.FunctionDef) and (cls.name, fn.name) in WANT:
                    out[f"{cls.name}.{fn.name}"] = params(fn)
    assert len(out) == len(WANT), sorted(out)
    return json.loads(json.dumps(out))       # (dict keys as JSON holds them: the timesteps of the MLP tables become strings)


def main():
    out = mint(sys.argv[1])
    if "--check" in sys.argv:
        with open(DST) as fh:
            if json.load(fh) != out:
                print("stale:", DST)
                sys.exit(1)
        print("fixture matches")
        return
    with open(DST, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", DST)


if __name__ == "__main__":
    main()
