"""Element-wise error bounds for kernels checked against a float64 reference.  TEST INFRASTRUCTURE: imported by the numerics tests
(tests/test_gpu_numerics_*.py, tests/test_numerics_cpu.py) the way tests/fulldepth_util.py is.

Method.  The reference is computed in float64 from the bf16-exact inputs the kernel received.  Every output element gets its own
bound, assembled by the test from the rounding chain of the operation's contract (the reference model run in bf16):
  * ``rnd(v)``      = 2^-8 |v| for every intermediate v the contract rounds to bf16 (unit roundoff of an 8-bit significand),
                      carried through the operations that follow it (a rounding before a multiply by g counts |g| times);
  * ``acc(K, s)``   = K 2^-24 s for an fp32 accumulation of K products whose absolute values sum to s (s = sum_k |a_k b_k|);
  * ``FLOOR``       = a tiny absolute floor (exact zeros, values far below the data's scale).
Each term is a worst case, so an implementation that rounds once fewer than the contract passes as well; what fails is an error
larger than every rounding of the chain together: a wrong element, a wrong operand, a tile left unwritten, partial sums held in
bf16, or an extra rounding where the contract keeps full precision.

A failure names the number of elements outside the bound, the worst one, its tile (256- and 128-row, 192-column: the GEMM
geometries) and the ratio of its error to its bound.
"""
from __future__ import annotations

import torch

U_BF16 = 2.0**-8
U_F32 = 2.0**-24
FLOOR = 2.0**-24


def rnd(v: torch.Tensor) -> torch.Tensor:
    """Worst-case error of rounding ``v`` to bf16."""
    return U_BF16 * v.abs()


def acc(K: int, abs_sum: torch.Tensor) -> torch.Tensor:
    """Worst-case error of an fp32 sum of K products whose absolute values add up to ``abs_sum``."""
    return (K * U_F32) * abs_sum


def bf16_exact(t: torch.Tensor) -> torch.Tensor:
    """``t`` rounded to bf16 and widened to float64 (the value a bf16 tensor holds)."""
    return t.to(torch.bfloat16).double()


def row_chunks(M: int, chunk: int):
    for r0 in range(0, M, chunk):
        yield r0, min(M, r0 + chunk)


def matmul_ref(a: torch.Tensor, w: torch.Tensor):
    """(a @ w^T, |a| @ |w|^T) in float64: the exact product of the bf16 operands and the sum of |a_k w_k| of each element."""
    a64, w64 = a.double(), w.double()
    return a64 @ w64.t(), a64.abs() @ w64.abs().t()


def tile_of(row: int, col: int) -> str:
    return f"256-row tile {row // 256}, 128-row tile {row // 128}, 192-col tile {col // 192}"


class Bound:
    """Accumulates the element-wise check over row chunks of one output (``add``), then ``check()`` raises with the worst element.

    Non-finite outputs violate every bound."""

    def __init__(self, what: str):
        self.what = what
        self.total = 0
        self.bad = 0
        self.worst = None   # (ratio, row, col, out, ref, bound)

    def add(self, out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, row0: int = 0) -> "Bound":
        out = out.double().reshape(ref.shape[0], -1)
        ref = ref.reshape(out.shape)
        bound = (bound.reshape(out.shape) + FLOOR)
        ratio = (out - ref).abs() / bound
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
        self.total += ratio.numel()
        self.bad += int((ratio > 1.0).sum())
        i = int(ratio.argmax())
        r, c = divmod(i, ratio.shape[1])
        q = float(ratio[r, c])
        if self.worst is None or q > self.worst[0]:
            self.worst = (q, row0 + r, c, float(out[r, c]), float(ref[r, c]), float(bound[r, c]))
        return self

    def message(self) -> str:
        q, r, c, o, f, b = self.worst
        return (f"{self.what}: {self.bad} of {self.total} elements outside the bound; worst at (row {r}, col {c}) [{tile_of(r, c)}]: "
                f"out {o:.6g}, ref {f:.6g}, bound {b:.3g}, |err| / bound = {q:.3g}")

    def check(self) -> None:
        assert self.total > 0, f"{self.what}: nothing was checked"
        assert self.bad == 0, self.message()


def check_elementwise(out, ref, bound, what: str) -> None:
    """One-shot form of Bound for outputs small enough to compare at once (any shape; rows = the first dimension)."""
    Bound(what).add(out, ref, bound).check()
