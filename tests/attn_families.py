"""Input families of the attention numerics tests (tests/test_numerics_cpu.py, tests/test_gpu_numerics_attention.py).  TEST
INFRASTRUCTURE, imported like tests/numerics.py.

Every family builds ONE (batch, head) slice: q [q_len, 72], k, v [kv_len, 72] as bf16 plus what the test asserts on the float64
REFERENCE (never on the kernel) before it trusts the case: ``targets`` [q_len, n] — the key indices that must carry the row — and
``expect`` [q_len, 72] — the value the output then has to within about one bf16 ulp.

  diffuse    randn q, k; v = randn + 0.5 (output not centred on 0).  Every key matters a little: catches what changes many weights.
  retrieval  query i is (a multiple of) key t(i): its logit leads by tens of binades, the output is v[t(i)].  t walks key 0, every
             multiple of 64 with its two neighbours and kv_len - 1 first, then all other keys: a dropped, shifted or mispaired key
             changes a whole output row.
  two_key    every key of the last (ragged) tile is a copy of a key in an earlier tile; query i points at one such pair: the output is
             (v_a + v_b) / 2, so the two tiles' contributions must be weighted alike across the running-max bookkeeping.
  ramps      one dominant key per 64-key tile whose logit (exp2 domain) walks a given ladder from tile to tile; rows come in blocks of
             64 of one kind (the rescale decision is taken per wave):
               step8    6, 14.1, 9, 6, 6          ONE rescale, 8.1 above, and nothing larger afterwards: a rescale that is skipped or
                                                  wrong stays in the result (in "rising" the last step of 20 shrinks it to 2^-20)
               step20   6, 6, 26, 9, 6            the same with a jump of 20, not in the tile after the first
               rising   6, 9, 16.9, 25, 45        steps +3, +7.9, +8.1, +20
               falling  45, 25, 16.9, 9, 6        the same steps downward (only the first tile sets the maximum)
               below    6, 13.9, 13.9, 9, 6       never more than 7.9 above the adopted maximum: no rescale, P up to 2^7.9
               above    6, 14.1, 22, 42, 6        8.1 above (rescale), 7.9 above the new one (none), 20 above (rescale)
             No norm: the logits are products of two stored bf16 numbers each.
"""
from __future__ import annotations

import math

import torch

HD = 72
KSCALE = HD**-0.5 * math.log2(math.e)       # what attn_prep_kv folds into Kp
LADDERS = {"step8": (6.0, 14.1, 9.0, 6.0, 6.0), "rising": (6.0, 9.0, 16.9, 25.0, 45.0), "falling": (45.0, 25.0, 16.9, 9.0, 6.0),
           "below": (6.0, 13.9, 13.9, 9.0, 6.0), "step20": (6.0, 6.0, 26.0, 9.0, 6.0), "above": (6.0, 14.1, 22.0, 42.0, 6.0)}
LADDER_ORDER = ("step8", "rising", "falling", "below", "step20", "above")
MIN_WEIGHT = 1 - 2.0**-12


def _randn(shape, g):
    return torch.randn(shape, generator=g)


def target_order(kv_len: int) -> torch.Tensor:
    """All key indices, the edges first: 0, kv_len - 1, every multiple of 64 and its neighbours."""
    first = [0, kv_len - 1]
    for m in range(64, kv_len + 64, 64):
        first += [m - 1, m, m + 1]
    seen, order = set(), []
    for j in first + list(range(kv_len)):
        if 0 <= j < kv_len and j not in seen:
            seen.add(j)
            order.append(j)
    return torch.tensor(order, dtype=torch.int64)


def diffuse(q_len, kv_len, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = _randn((q_len, HD), g), _randn((kv_len, HD), g), _randn((kv_len, HD), g) + 0.5
    return dict(q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v.to(torch.bfloat16), targets=None, expect=None)


def _unit_rows(x):
    return x * (HD**0.5 / x.norm(dim=-1, keepdim=True))


def retrieval(q_len, kv_len, seed, gain=6.0):
    """Keys of norm sqrt(72); q_i = gain k_t(i).  Without norm the target's logit is gain 72 KSCALE = 73 (gain 6) against |others| <~ 40;
    with RMS norm the gain drops out and norm weights of about 2 give 4 * 72 KSCALE = 49 against <~ 27."""
    g = torch.Generator().manual_seed(seed)
    k = _unit_rows(_randn((kv_len, HD), g)).to(torch.bfloat16)
    v = (_randn((kv_len, HD), g) + 0.5).to(torch.bfloat16)
    t = target_order(kv_len)[torch.arange(q_len) % kv_len]
    q = (gain * k[t].float()).to(torch.bfloat16)
    return dict(q=q, k=k, v=v, targets=t[:, None], expect=v[t].double())


def two_key(q_len, kv_len, seed, gain=6.0):
    assert kv_len > 64
    g = torch.Generator().manual_seed(seed)
    k = _unit_rows(_randn((kv_len, HD), g)).to(torch.bfloat16)
    v = (_randn((kv_len, HD), g) + 0.5).to(torch.bfloat16)
    n0 = (kv_len - 1) // 64 * 64                       # first key of the last tile
    b = torch.arange(n0, kv_len)
    a = (b * 37 + 11) % n0
    assert a.unique().numel() == a.numel()
    k[b] = k[a]
    i = torch.arange(q_len) % b.numel()
    q = (gain * k[b[i]].float()).to(torch.bfloat16)
    return dict(q=q, k=k, v=v, targets=torch.stack([a[i], b[i]], dim=1), expect=(v[a[i]].double() + v[b[i]].double()) / 2)


def ramp_kind(row: int) -> str:
    return LADDER_ORDER[(row // 64) % len(LADDER_ORDER)]


def ramp_key(t: int) -> int:
    return 64 * t + (13 * t + 5) % 64


def ramps(q_len, kv_len, seed):
    """``levels`` [q_len, 5]: the ladder each row was built for (the test compares the reference's tile maxima with it)."""
    assert kv_len >= 320
    g = torch.Generator().manual_seed(seed)
    k = _randn((kv_len, HD), g)
    k[:, :16] = 0
    # dominant key of tile t: 4.0 in dim t (coarse) and 0.25 in dim 8 + t (fine): q's coarse part is level / kappa rounded to bf16, the
    # fine part carries what that rounding lost, so the ladder is met to ~10^-3 although a bf16 near 64 resolves only 0.25
    kappa = float(torch.tensor(4.0 * KSCALE).to(torch.bfloat16))
    kappa2 = float(torch.tensor(0.25 * KSCALE).to(torch.bfloat16))
    for t in range(5):
        k[ramp_key(t)] = 0
        k[ramp_key(t), t] = 4.0
        k[ramp_key(t), 8 + t] = 0.25
    q = 0.1 * _randn((q_len, HD), g)
    q[:, :16] = 0
    levels = torch.tensor([LADDERS[ramp_kind(i)] for i in range(q_len)], dtype=torch.float64)
    coarse = (levels / kappa).to(torch.bfloat16)
    q[:, :5] = coarse.float()
    q[:, 8:13] = ((levels - coarse.double() * kappa) / kappa2).float()
    v = (_randn((kv_len, HD), g) + 0.5).to(torch.bfloat16)
    return dict(q=q.to(torch.bfloat16), k=k.to(torch.bfloat16), v=v, targets=None, expect=None, levels=levels)


FAMILIES = {"diffuse": diffuse, "retrieval": retrieval, "two_key": two_key, "ramps": ramps}


def prep_k(k, w=None, eps=1e-6):
    """Kp as attn_prep_kv writes it (float32 arithmetic, bf16 result): bf16(bf16(k rstd) w KSCALE), w None: bf16(k KSCALE)."""
    kf = k.float()
    if w is None:
        return (kf * KSCALE).to(torch.bfloat16)
    n = (kf * torch.rsqrt((kf * kf).mean(dim=-1, keepdim=True) + eps)).to(torch.bfloat16).float()
    return (n * (w.float() * KSCALE)).to(torch.bfloat16)


def check_ladders(logits, levels, what=""):
    """The reference's tile maxima of a ramps case sit within 0.09 of the ladder (so 7.9 stays below 8 and 8.1 above)."""
    tiles = torch.stack([logits[..., 64 * t:64 * t + 64].amax(dim=-1) for t in range(5)], dim=-1)
    err = (tiles - levels.to(tiles.device)).abs().max().item()
    assert err < 0.09, f"{what}: the ramp ladder is off by {err:.3f} in the reference"
    rest = logits[..., 320:]
    assert rest.numel() == 0 or rest.max().item() < 3.0, f"{what}: a key past the fifth tile competes with the ladder"


def check_targets(ref, case, what=""):
    """The retrieval / two-key condition on the REFERENCE: joint weight >= 1 - 2^-12 on the targets, output = expect within 2^-7."""
    w = ref.weight.min().item()
    assert w >= MIN_WEIGHT, f"{what}: the reference puts only {w:.6f} on the target keys (construction too weak)"
    exp = case["expect"].to(ref.out.device)
    err = ((ref.out - exp).abs() / (exp.abs() + 2.0**-6)).max().item()
    assert err <= 2.0**-7, f"{what}: the reference output is {err:.3g} (relative) from the targets' v"
