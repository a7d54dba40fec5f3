"""TEST INFRASTRUCTURE ONLY — mints tests/golden/ref_traces/ from the REAL reference (needs the reference tree at
oracle/ref_loader.REFERENCE_ROOT, VSYS_REFERENCE_ROOT overrides it):

    python oracle/make_golden_ref_traces.py

The CPU tests that compare this build against the reference's own code (its classes, functions, sources and example scripts) wrap
every piece that touches the reference in ``ref_trace.value(...)`` / ``.lookup(...)`` (tests/ref_trace.py).  This script runs
exactly those tests with VSYS_REF_RECORD=1: the pieces run live and what they return is written as plain data, one file per test.
A normal test run replays the files and reads nothing outside the repository.  The minting run must pass; it fails otherwise.
"""
from __future__ import annotations

import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TESTS = [
    "tests/test_cogvideox_cpu.py::test_oracle_vs_live_reference",
    "tests/test_cogvideox_cpu.py::test_dpm_scheduler_matches_the_reference_class",
    "tests/test_cogvideox_vae_cpu.py::test_cogvideox_vae_param_inventory_matches_reference",
    "tests/test_cogvideox_vae_cpu.py::test_cogvideox_vae_oracle_matches_live_reference_class",
    "tests/test_host_cpu.py::test_comm_operators_equal_the_reference_functions_over_gloo",
    "tests/test_host_cpu.py::test_timestep_transform_bitwise_equals_reference_function",
    "tests/test_host_cpu.py::test_timestep_transform_bf16_geometry_equals_reference_function",
    "tests/test_host_cpu.py::test_open_sora_geometry_vocabulary_matches_reference_tables",
    "tests/test_host_cpu.py::test_reference_module_paths_resolve_to_this_build",
    "tests/test_host_cpu.py::test_reference_example_scripts_run_against_this_build",
    "tests/test_host_cpu.py::test_generate_accepts_every_keyword_of_the_reference",
    "tests/test_host_cpu.py::test_pipelines_and_engine_have_every_method_of_the_reference_classes",
    "tests/test_host_cpu.py::test_pipeline_constructors_take_the_reference_components",
    "tests/test_host_cpu.py::test_caption_cleaner_equals_the_reference_on_generated_text",
    "tests/test_host_cpu.py::test_mask_strategy_helpers_equal_the_reference_on_generated_cases",
    "tests/test_latte_cpu.py::test_latte_oracle_vs_live_reference",
    "tests/test_oracle_vs_golden.py::test_live_reference_forward",
    "tests/test_pab_cpu.py::test_pab_decisions_match_reference_module",
    "tests/test_stdit3_hostflow_cpu.py::test_pipeline_adopts_the_reference_transformer_module",
    "tests/test_vae_cpu.py::test_decoder_param_inventory_matches_reference",
    "tests/test_vae_cpu.py::test_vae_oracle_matches_live_reference_class",
    "tests/test_vae_cpu.py::test_encoder_param_inventory_matches_reference",
    "tests/test_vae_cpu.py::test_vae_encode_oracle_matches_live_reference_class",
]


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_loader

    assert ref_loader.reference_available(), f"no reference tree at {ref_loader.REFERENCE_ROOT}"
    env = dict(os.environ, VSYS_REF_RECORD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
