"""The resident scratch memory of one model: a dict (``model._ws``) whose entries are reused from step to step, so a step allocates
nothing once it is warm and a recorded launch program (program.py) keeps replaying onto the same addresses.

It stays a plain dict on purpose: utils.HostOffload skips the attribute by name and releases it with ``clear()``, and the entries are
what they always were — ``name`` -> the flat allocation behind ``buf(name, ...)``, a tuple key -> what ``once`` made for it,
``"mlp_slab_pool"`` -> the list of free PAB slabs."""
from __future__ import annotations

import math

import torch


class Workspace(dict):
    def __init__(self, device, dtype=torch.bfloat16):
        super().__init__()
        self.device, self.dtype = torch.device(device), dtype

    def buf(self, name, shape, dtype=None):
        """A ``shape`` view of the one flat allocation kept under ``name``: grow-only (reallocated, never zeroed, only when the request
        outgrows it), so views handed out earlier under the same name alias it until then.  A name keeps the dtype it was first asked
        with (default: the workspace's)."""
        dtype = dtype or self.dtype
        n = math.prod(shape)
        b = self.get(name)
        if b is not None and b.dtype != dtype:
            raise ValueError(f"workspace buffer {name!r} holds {b.dtype}, asked for as {dtype}")
        if b is None or b.numel() < n:
            b = torch.empty(n, dtype=dtype, device=self.device)
            self[name] = b
        return b[:n].view(*shape)

    def once(self, key, make):
        """``self[key]``, made by ``make()`` on first use (K/V layouts, statistics buffers, decisions: one per geometry)."""
        if key not in self:
            self[key] = make()
        return self[key]

    def take_slab(self, like):
        """A slab for a PAB MLP-broadcast window: taken from the pool of slabs that closed windows handed back (a window's stored
        output lives until its last timestep, pab_mgr.py:148-174), so a generate() allocates at most as many 90 MB slabs as
        windows are open at once instead of one per window opening."""
        pool = self.setdefault("mlp_slab_pool", [])
        for k, b in enumerate(pool):
            if b.shape == like.shape:
                return pool.pop(k)
        return torch.empty_like(like)

    def give_slab(self, t):
        """Hand the slab of a closed window back (the caller orders it behind the slab's last reader on the stream)."""
        self.setdefault("mlp_slab_pool", []).append(t)
