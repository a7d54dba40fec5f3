"""Reference-derived values for the CPU tests that compare against the reference's own code, stored under tests/golden/ref_traces/.

A test wraps every piece of code that touches the reference tree in ``tr.value(fn)`` (``tr`` = the ``ref_trace`` fixture, or a
``Trace`` made by hand in a worker process).  A normal run REPLAYS what those pieces returned when the trace was minted, in call
order, and never reads anything outside the repository.  ``python oracle/make_golden_ref_traces.py`` mints the traces where the
reference tree exists: it runs the same tests with VSYS_REF_RECORD=1, so that ``fn`` runs live and its result is recorded.

Values are plain data only (tensors, numbers, strings, None and lists / tuples / dicts / sets of them): nothing of the reference's
code is stored.  An exception raised by ``fn`` is recorded by type and message and raised again on replay.  A result that is only
ever compared bit for bit and is too large to keep is recorded as its ``tensor_digest``."""
from __future__ import annotations

import builtins
import hashlib
import os
import re

import pytest
import torch

TRACE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_traces")
RECORD = os.environ.get("VSYS_REF_RECORD") == "1"


def _plain(v, where="value"):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().clone()
    if v is None or isinstance(v, (bool, int, float, str, bytes, torch.dtype, torch.Size)):
        return v
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(x, where) for x in v)
    if isinstance(v, (set, frozenset)):
        return type(v)(_plain(x, where) for x in v)
    if isinstance(v, dict):
        return {_plain(k, where): _plain(x, where) for k, x in v.items()}
    raise TypeError(f"{where}: a reference trace holds plain data only, not {type(v).__name__}")


def tensor_digest(t, samples=4096, seed=0):
    """Exact fingerprint of a tensor: shape, dtype, SHA-256 of its bytes, and a fixed seeded sample of its values (so that a
    mismatch can say where and by how much).  Two tensors of one dtype are bit-identical iff their digests are equal."""
    t = t.detach().cpu().contiguous()
    idx = torch.randint(0, t.numel(), (min(samples, t.numel()),), generator=torch.Generator().manual_seed(seed))
    return {"shape": tuple(t.shape), "dtype": str(t.dtype), "sha256": hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest(),
            "idx": idx, "values": t.reshape(-1)[idx].clone()}


def assert_digest_equal(got, want):
    """Bit-for-bit equality of two tensor_digest()s; the sample is compared first for a readable failure."""
    assert (got["shape"], got["dtype"]) == (want["shape"], want["dtype"]), (got["shape"], got["dtype"], want["shape"], want["dtype"])
    assert torch.equal(got["idx"], want["idx"])
    d = (got["values"].double() - want["values"].double()).abs()
    assert torch.equal(got["values"], want["values"]), f"sampled values differ: max |diff| {d.max().item():.3e} at flat index {int(got['idx'][d.argmax()])}"
    assert got["sha256"] == want["sha256"], "sampled values agree but the tensors differ elsewhere"


class Trace:
    def __init__(self, name: str):
        self.name = re.sub(r"[^A-Za-z0-9_.-]+", "_", name)
        self.path = os.path.join(TRACE_DIR, self.name + ".pt")
        self.values, self.pos, self.tables = [], 0, {}
        if not RECORD:
            if not os.path.exists(self.path):
                raise FileNotFoundError(f"reference trace {self.path} missing: mint it with oracle/make_golden_ref_traces.py")
            saved = torch.load(self.path, weights_only=False)
            self.values, self.tables = saved["values"], saved["tables"]

    @staticmethod
    def _live(fn, where):
        try:
            r = fn()
        except Exception as e:   # the reference's own exception is part of what it does (kept as its nearest built-in class)
            return ("raise", next(c.__name__ for c in type(e).__mro__ if getattr(builtins, c.__name__, None) is c), str(e))
        return ("ok", _plain(r, where))

    @staticmethod
    def _result(v):
        if v[0] == "raise":
            raise getattr(builtins, v[1])(v[2])
        return v[1]

    def value(self, fn):
        """``fn()`` (live, recorded) while minting; the recorded result of the same call otherwise."""
        if RECORD:
            v = self._live(fn, f"{self.name}[{len(self.values)}]")
            self.values.append(v)
        else:
            assert self.pos < len(self.values), f"{self.name}: more reference calls than the trace holds (re-mint it)"
            v = self.values[self.pos]
            self.pos += 1
        return self._result(v)

    def lookup(self, key, fn):
        """Like value(), keyed by ``key`` (plain, hashable) instead of call order: for property tests, whose examples are drawn
        deterministically but may be visited in another order."""
        if RECORD:
            if key not in self.tables:
                self.tables[key] = self._live(fn, f"{self.name}[{key!r}]")
        else:
            assert key in self.tables, f"{self.name}: no recorded reference result for {key!r} (re-mint it)"
        return self._result(self.tables[key])

    def close(self):
        if RECORD:
            os.makedirs(TRACE_DIR, exist_ok=True)
            torch.save({"values": self.values, "tables": self.tables}, self.path)
        else:
            assert self.pos == len(self.values), f"{self.name}: {len(self.values) - self.pos} recorded reference calls not made (re-mint it)"


@pytest.fixture
def ref_trace(request):
    tr = Trace(request.node.nodeid.split("::", 1)[0].rsplit("/", 1)[-1].replace(".py", "") + "__" + request.node.name)
    yield tr
    tr.close()
