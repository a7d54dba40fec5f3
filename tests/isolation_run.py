"""Runs one row of tests/isolation_cases.py on the device (TEST INFRASTRUCTURE, shared by tests/test_gpu_isolation_*.py): builds the
operands once, then isolation.check_isolated under every GEMM / flash variant the row lists.  A variant is forced with
vsys_tune_gemm_variant / vsys_tune_flash_variant inside try / finally; an id the build does not accept is passed over (the row says
"wherever the library accepts it"), and so is a forced id that the ENTRY POINT refuses for the shape with its host-side "unsupported
shape" / "bad argument" status on a trial call on tight operands (nothing is launched then).  Id 0 — the shipped dispatch — always
runs.  RAN counts what really executed, per family and (gemm id, flash id); REFUSED what was passed over: the last test of every
family file asserts on them."""
import collections

import torch

import isolation as iso

RAN = collections.defaultdict(collections.Counter)        # family -> {(gemm variant, flash variant): check_isolated calls that ran}
REFUSED = collections.defaultdict(collections.Counter)    # family -> {(gv, fv): passed over}; "tune" = the id is not in the build
HOST_REFUSALS = ("unsupported shape", "bad argument")


def run_case(row):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from videosys_amd import _lib, ops

    dev = torch.device("cuda:0")
    lib = _lib.load()
    params = dict(row.params)
    fills = params.pop("fills", iso.FILLS)         # a row that runs under one fill only says why in tests/isolation_cases.py
    fn, operands, outputs, inplace = row.builder(ops, dev, **params)
    torch.cuda.synchronize()
    ran = 0
    for gv in row.gemm_variants:
        for fv in row.flash_variants:
            try:
                if lib.vsys_tune_gemm_variant(gv) != 0 or lib.vsys_tune_flash_variant(fv) != 0:
                    assert gv or fv, "the default selection was rejected"
                    REFUSED[row.family][("tune", gv, fv)] += 1
                    continue
                if gv or fv:
                    try:
                        fn({n: op.tight() for n, op in operands.items()})
                        torch.cuda.synchronize()
                    except _lib.VsysError as e:
                        if not any(w in str(e) for w in HOST_REFUSALS):
                            raise
                        REFUSED[row.family][(gv, fv)] += 1
                        continue
                iso.check_isolated(fn, operands, outputs, inplace, fills=fills, what=f"{row.name} [gemm variant {gv}, flash variant {fv}]")
                RAN[row.family][(gv, fv)] += 1
                ran += 1
            finally:
                lib.vsys_tune_gemm_variant(0)
                lib.vsys_tune_flash_variant(0)
    assert ran, "no variant ran"


def check_counts(fam, rows):
    """Every row ran under the shipped dispatch, and every forced id some row lists ran at least once in the family unless the build
    does not contain it (then vsys_tune_* refused it for every row).  Prints the table, so a run's log says what executed."""
    ran, refused = RAN[fam], REFUSED[fam]
    print(f"\n[isolation {fam}] ran: {dict(sorted(ran.items()))}\n[isolation {fam}] passed over: {dict(sorted(refused.items(), key=str))}")
    assert ran[(0, 0)] == len(rows), f"{ran[(0, 0)]} of {len(rows)} rows ran under the shipped dispatch"
    listed = {(gv, fv) for r in rows for gv in r.gemm_variants for fv in r.flash_variants}
    for gv, fv in sorted(listed):
        in_build = refused[("tune", gv, fv)] == 0
        assert ran[(gv, fv)] > 0 or not in_build, f"variant (gemm {gv}, flash {fv}) is in the build and ran for no row of the family"
