"""Guard bands around kernel operands: does a kernel read and write only what it was given?  TEST INFRASTRUCTURE, imported by
tests/test_isolation_cpu.py and tests/test_gpu_isolation_*.py the way tests/numerics.py is; the cases are data in
tests/isolation_cases.py.

Method.  Every tensor operand of ONE kernel call is placed inside ONE larger allocation (the arena), as a view with the shape and
strides the case asks for.  An operand is described by its tight ``data`` and, optionally, a ``parent`` shape with the offset of
the view inside it: a column slice of a wider buffer, a row slice ``buf[:, r0:r1]`` of a statistics buffer, one column block of
a modulation table.  Everything of the parent that is not the view (the GAP), a band IN FRONT of the parent and a band BEHIND it
are guard.  Elements inside the operand that the kernel must not let reach a result, or must not write (``interior``: pad keys of
Kp / Vt), are guard as well; the tight copy holds zeros there.

Guard size.  A band is at least as long as the furthest a plausible tail bug reaches, so an over-read or an over-write lands inside
the arena and never in unmapped memory: 256 rows of the operand's row stride (one full tile of the widest GEMM geometry) for operands
with rows, whatever the case adds (``guard_elems``: one 64-key tile of every (batch, head) image for Kp / Vt), and never less than
64 KiB.  The tests OBSERVE an overreach, they do not provoke a fault: every operand handed to a kernel is valid and every count
and offset is in range.

Guard contents.  Floating-point operands: every case runs under two fills, ``nan`` (a quiet NaN with a recognisable payload) and
``max`` (the largest finite value of the type) — max-style instructions drop a NaN operand, and a huge finite value times a masked
zero stays zero where a NaN does not, so the pair separates "was read and used" from "was read and properly discarded".  Integer
operands: ``int_guard``, values that are VALID for the kernel but differ from the real ones (a misread changes the answer, it never
sends the kernel out of bounds).

``check_isolated(fn, operands, outputs, inplace=...)`` does, for each fill:
  1. fn on tight, freshly allocated copies of the operands -> ``want`` (what the value tests already judge);
  2. fn on the arena views (pure outputs pre-filled with the guard pattern, so an unwritten element shows);
  3. every output view equals ``want`` bit for bit (integer views: NaN != NaN hides nothing) and holds no NaN / Inf ``want`` lacks;
  4. every guard element of every operand still holds its pattern;
  5. every input not declared in place is unchanged bit for bit.
A failure names the operand, the side (in front / behind / gap / interior), the first and last damaged offset in elements and as
(row, column) of the operand's geometry, and the number of bytes that differ.
"""
from __future__ import annotations

import math

import torch

MIN_GUARD_BYTES = 64 * 1024
GUARD_ROWS = 256
ALIGN = 256                      # bytes: every parent starts on a 256-byte boundary of the arena (kernels ask for 16)
FILLS = ("nan", "max")

_INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NAN_BITS = {torch.bfloat16: 0x7FA5, torch.float16: 0x7E5A, torch.float32: 0x7FC0A5A5, torch.float64: 0x7FF80000A5A5A5A5}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The integer view of ``t`` (same shape): what every comparison here is made on."""
    return t if not t.dtype.is_floating_point else t.view(_INT_VIEW[t.element_size()])


def fill_bits(dtype: torch.dtype, fill: str) -> int:
    """The bit pattern of a floating-point guard element, as the signed integer of the same width."""
    if fill == "nan":
        v = _NAN_BITS[dtype]
    elif fill == "max":
        v = int(bits(torch.tensor([torch.finfo(dtype).max], dtype=dtype))[0])
    else:
        raise ValueError(fill)
    n = 8 * torch.empty((), dtype=dtype).element_size()
    return v - (1 << n) if v >= (1 << (n - 1)) else v


class Operand:
    """One tensor operand of a kernel call.

    data         the tight tensor (values of the view; initial content of an output in the tight run)
    parent, at   shape of the buffer the view is cut out of and the view's start in it (same rank as data); None = tight
    interior     bool mask over data: guard elements INSIDE the operand (arena: the fill pattern, tight copy: zeros)
    callers      bool mask over data: elements of a pure output that belong to the caller (arena: data, not the pattern)
    guard_elems  extra lower limit for the bands in front and behind (elements)
    int_guard    integer operands: 1-D pattern of valid-but-different values the guard repeats (period = its length)
    scratch      a workspace of the call: its guard is checked, its content belongs to the kernel and is not compared
    interior_fills  the fills the INTERIOR guard of this operand may hold (default: every fill).  Under a fill that is not listed the
                 interior holds interior_fills[0] instead; the bands and gaps always hold the fill of the run.  For a documented
                 contract only (Vt pad columns of the masked flash entry points must be finite): the case table gives the reason.
    """

    def __init__(self, data, *, parent=None, at=None, interior=None, callers=None, guard_elems=0, int_guard=None, scratch=False,
                 interior_fills=None):
        self.data, self.scratch, self.interior_fills = data, scratch, interior_fills
        self.parent = tuple(parent) if parent is not None else tuple(data.shape)
        self.at = tuple(at) if at is not None else (0,) * data.dim()
        assert len(self.parent) == data.dim() == len(self.at), "parent / at must have the rank of data"
        for n, p, a in zip(data.shape, self.parent, self.at):
            assert 0 <= a and a + n <= p, f"view {tuple(data.shape)} at {self.at} does not fit parent {self.parent}"
        self.interior, self.callers = interior, callers
        assert interior is None or (interior.shape == data.shape and interior.dtype == torch.bool)
        assert callers is None or (callers.shape == data.shape and callers.dtype == torch.bool)
        if not data.dtype.is_floating_point:
            assert int_guard is not None, "an integer operand needs int_guard: valid values that differ from the real ones"
        self.int_guard = int_guard
        self.row_stride = self.parent[-1] if data.dim() else 1
        self.parent_numel = math.prod(self.parent)
        esz = data.element_size()
        band = max(-(-MIN_GUARD_BYTES // esz), GUARD_ROWS * self.row_stride if data.dim() >= 2 else 0, int(guard_elems))
        self.band = -(-band * esz // ALIGN) * ALIGN // esz

    def tight(self):
        t = self.data.clone().contiguous()
        if self.interior is not None:
            t[self.interior] = 0
        return t

    def slices(self):
        return tuple(slice(a, a + n) for a, n in zip(self.at, self.data.shape))


class Damage:
    def __init__(self, operand, side, first, last, nbytes, geometry):
        self.operand, self.side, self.first, self.last, self.nbytes, self.geometry = operand, side, first, last, nbytes, geometry

    def __str__(self):
        return (f"operand '{self.operand}': {self.side}: {self.nbytes} bytes differ, first at element {self.first[0]} "
                f"(row {self.first[1]}, col {self.first[2]}), last at element {self.last[0]} (row {self.last[1]}, col {self.last[2]}) "
                f"[{self.geometry}]")


class IsolationError(AssertionError):
    def __init__(self, what, damages):
        self.damages = damages
        super().__init__(f"{what}: " + "; ".join(str(d) for d in damages))


class Arena:
    """One allocation holding every operand of a call with its guard bands (module docstring)."""

    def __init__(self, operands: dict, outputs, inplace, fill: str):
        self.ops, self.fill = operands, fill
        self.outputs, self.inplace = tuple(outputs), set(inplace)
        dev = next(iter(operands.values())).data.device
        off, self.where = 0, {}
        for name, op in operands.items():
            esz = op.data.element_size()
            nbytes = (2 * op.band + op.parent_numel) * esz
            self.where[name] = off
            off += -(-nbytes // ALIGN) * ALIGN
        self.raw = torch.empty(off + ALIGN, dtype=torch.uint8, device=dev)
        base = (-self.raw.data_ptr()) % ALIGN
        self.seg, self.views, self.guard = {}, {}, {}
        for name, op in operands.items():
            esz = op.data.element_size()
            n = 2 * op.band + op.parent_numel
            seg = self.raw[base + self.where[name]: base + self.where[name] + n * esz].view(op.data.dtype)
            self._paint(seg, op)
            parent = seg[op.band: op.band + op.parent_numel].view(op.parent)
            view = parent[op.slices()]
            is_guard = torch.ones(n, dtype=torch.bool, device=dev)
            g_view = is_guard[op.band: op.band + op.parent_numel].view(op.parent)[op.slices()]
            g_view[...] = False
            pure_out = name in self.outputs and name not in self.inplace
            if pure_out:
                keep = op.callers if op.callers is not None else None
                if keep is not None:
                    view[keep] = op.data[keep]
                assert op.data.dtype.is_floating_point, "a pure integer output is not supported"
            else:
                if op.interior is not None:
                    keep = ~op.interior
                    view[keep] = op.data[keep]
                else:
                    view.copy_(op.data)
            if op.interior is not None:
                g_view[op.interior] = True
                if self._ifill(op) != fill:
                    bits(view)[op.interior] = fill_bits(op.data.dtype, self._ifill(op))
            self.seg[name], self.views[name], self.guard[name] = seg, view, is_guard

    def _ifill(self, op):
        return self.fill if op.interior_fills is None or self.fill in op.interior_fills else op.interior_fills[0]

    def _expected(self, op, n):
        """Guard pattern of a floating-point segment: a scalar, or a tensor where the interior holds another fill."""
        base = fill_bits(op.data.dtype, self.fill)
        if op.interior is None or self._ifill(op) == self.fill:
            return base
        e = torch.full((n,), base, dtype=_INT_VIEW[op.data.element_size()], device=op.data.device)
        e[op.band: op.band + op.parent_numel].view(op.parent)[op.slices()][op.interior] = fill_bits(op.data.dtype, self._ifill(op))
        return e

    def _pattern(self, op, n):
        """The guard pattern of a whole segment of n elements, as integers."""
        dev = op.data.device
        if op.data.dtype.is_floating_point:
            return None
        pat = torch.as_tensor(op.int_guard, dtype=op.data.dtype).to(dev).reshape(-1)
        idx = (torch.arange(n, device=dev) - op.band) % pat.numel()
        return pat[idx]

    def _paint(self, seg, op):
        if op.data.dtype.is_floating_point:
            bits(seg).fill_(fill_bits(op.data.dtype, self.fill))
        else:
            seg.copy_(self._pattern(op, seg.numel()))

    # ------------------------------------------------------------------------------------------------ checks
    def _geometry(self, op):
        return f"view {tuple(op.data.shape)} at {op.at} of parent {op.parent}, row stride {op.row_stride}, band {op.band} elements"

    def _locate(self, op, idx):
        """Segment index -> (offset in elements, row, column), all relative to the first element of the view."""
        origin, stride = 0, 1
        for a, p in zip(reversed(op.at), reversed(op.parent)):
            origin += a * stride
            stride *= p
        rel = int(idx) - op.band
        return rel - origin, rel // op.row_stride - origin // op.row_stride, rel % op.row_stride - origin % op.row_stride

    def damages(self, name):
        op, seg = self.ops[name], self.seg[name]
        n = seg.numel()
        if op.data.dtype.is_floating_point:
            expect = self._expected(op, n)
            bad = bits(seg) != expect
        else:
            bad = seg != self._pattern(op, n)
        bad &= self.guard[name]
        if not bool(bad.any()):
            return []
        out, esz = [], op.data.element_size()
        inside = torch.zeros(n, dtype=torch.bool, device=seg.device)
        if op.interior is not None:
            inside[op.band: op.band + op.parent_numel].view(op.parent)[op.slices()][op.interior] = True
        pos = torch.arange(n, device=seg.device)
        sides = (("in front of the operand", pos < op.band), ("behind the operand", pos >= op.band + op.parent_numel),
                 ("interior guard (elements of the operand the kernel must leave alone)", inside),
                 ("gap (columns / rows of the parent outside the view)", (pos >= op.band) & (pos < op.band + op.parent_numel) & ~inside))
        for side, where in sides:
            hit = torch.nonzero(bad & where).reshape(-1)
            if hit.numel():
                if op.data.dtype.is_floating_point:
                    x = bits(seg)[hit] ^ (expect[hit] if torch.is_tensor(expect) else expect)
                else:
                    x = seg[hit] ^ self._pattern(op, n)[hit]
                nbytes = sum(int(((x >> (8 * b)) & 0xFF).ne(0).sum()) for b in range(esz))
                out.append(Damage(name, side, self._locate(op, hit[0]), self._locate(op, hit[-1]), nbytes, self._geometry(op)))
        return out

    def differences(self, name, want, side):
        """Bitwise comparison of a view with ``want`` outside the interior guard."""
        op, view = self.ops[name], self.views[name]
        if op.scratch:
            return []
        got = view.contiguous()
        diff = bits(got) != bits(want.contiguous())
        if op.interior is not None:
            diff &= ~op.interior
        if not bool(diff.any()):
            return []
        hit = torch.nonzero(diff.reshape(-1)).reshape(-1)
        cols = op.data.shape[-1] if op.data.dim() else 1
        loc = lambda i: (int(i), int(i) // cols, int(i) % cols)
        x = bits(got).reshape(-1)[hit] ^ bits(want.contiguous()).reshape(-1)[hit]
        nbytes = sum(int(((x >> (8 * b)) & 0xFF).ne(0).sum()) for b in range(op.data.element_size()))
        extra = ""
        if op.data.dtype.is_floating_point:
            nf = (~torch.isfinite(got.float() if got.dtype != torch.float64 else got)) & torch.isfinite(want.float() if want.dtype != torch.float64 else want)
            if op.interior is not None:
                nf &= ~op.interior
            extra = f"; {int(nf.sum())} NaN / Inf the tight run does not hold"
            i0 = int(hit[0])
            extra += f"; first: got {float(got.reshape(-1)[i0])!r}, want {float(want.reshape(-1)[i0])!r}"
        return [Damage(name, side + extra, loc(hit[0]), loc(hit[-1]), nbytes, f"tight shape {tuple(op.data.shape)}")]


def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def run_isolated(fn, operands: dict, outputs, inplace=(), fill="nan"):
    """Steps 1-5 of the module docstring for one fill; returns the list of Damage (empty = isolated)."""
    outputs, inplace = tuple(outputs), set(inplace)
    assert set(outputs) <= set(operands) and inplace <= set(outputs), "outputs / inplace name operands; in-place operands are outputs"
    any_t = next(iter(operands.values())).data
    tight = {n: op.tight() for n, op in operands.items()}
    own_want = fn(tight)
    own_want = own_want if isinstance(own_want, dict) else {}
    _sync(any_t)
    arena = Arena(operands, outputs, inplace, fill)
    try:
        own = fn(arena.views)
        _sync(any_t)
        found = []
        for n, want in own_want.items():       # results the op allocated itself: no arena around them, same bits all the same
            d = bits(own[n].contiguous()) != bits(want.contiguous())
            if bool(d.any()):
                hit = torch.nonzero(d.reshape(-1)).reshape(-1)
                cols = want.shape[-1]
                found.append(Damage(n, "result allocated by the op differs from the tight run", (int(hit[0]), int(hit[0]) // cols, int(hit[0]) % cols),
                                    (int(hit[-1]), int(hit[-1]) // cols, int(hit[-1]) % cols), int(d.sum()) * want.element_size(),
                                    f"shape {tuple(want.shape)}"))
        for n in outputs:
            found += arena.differences(n, tight[n], "output differs from the tight run")
        for n in operands:
            found += arena.damages(n)
        for n, op in operands.items():
            if n not in outputs:
                found += arena.differences(n, op.tight(), "input modified (not declared in place)")
        return found
    finally:
        del arena


def check_isolated(fn, operands: dict, outputs, inplace=(), fills=FILLS, what="kernel"):
    """Assert that ``fn`` (one kernel call on a dict name -> tensor) is isolated under every fill (module docstring)."""
    failed = []
    for fill in fills:
        found = run_isolated(fn, operands, outputs, inplace, fill)
        if found:
            failed.append((fill, found))
    if failed:        # both fills are reported: which of them shows a leak tells "used" from "read and discarded" (module docstring)
        raise IsolationError(" | ".join(f"{what} [guard fill '{fill}']" for fill, _ in failed), [d for _, f in failed for d in f])
