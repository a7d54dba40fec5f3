"""The host plumbing the four transformers share: workspace.Workspace (resident scratch buffers, made-once entries, the PAB slab
pool), pab.BlockState / pab.reset_states, modules.sincos_1d, ops.static_max_allowed, utils.load_weights.  No GPU: device="cpu"."""
import numpy as np
import pytest
import torch

from videosys_amd import ops, pab
from videosys_amd.modules import sincos_1d
from videosys_amd.utils import load_weights
from videosys_amd.workspace import Workspace


@pytest.fixture
def ws():
    return Workspace("cpu", torch.bfloat16)


def test_buf_is_a_view_of_one_allocation_per_name(ws):
    a = ws.buf("x", (4, 6))
    assert a.shape == (4, 6) and a.dtype == torch.bfloat16 and a.is_contiguous()
    for shape in ((4, 6), (3, 5), (2, 2, 2), (24,)):       # smaller or equal: the same storage, from its start
        b = ws.buf("x", shape)
        assert b.data_ptr() == a.data_ptr() and tuple(b.shape) == shape and b.dtype == torch.bfloat16
    assert ws["x"].dim() == 1 and ws["x"].numel() == 24 and ws["x"].data_ptr() == a.data_ptr()   # the entry is the flat allocation
    assert ws.buf("x", torch.Size((2, 3))).shape == (2, 3)   # a tensor's .shape is a shape


def test_buf_grows_only_when_the_request_is_larger(ws):
    a = ws.buf("x", (4, 6))
    flat = ws["x"]
    big = ws.buf("x", (5, 5))
    assert ws["x"] is not flat and ws["x"].numel() == 25 and big.shape == (5, 5)
    assert big.data_ptr() != a.data_ptr()                  # (a is still alive here, so the address cannot have been recycled)
    assert ws.buf("x", (4, 6)).data_ptr() == big.data_ptr()   # and does not shrink back


def test_two_names_never_alias(ws):
    a, b = ws.buf("a", (8,)), ws.buf("b", (8,))
    a.fill_(1.0)
    b.fill_(2.0)
    assert a.data_ptr() != b.data_ptr() and bool((a == 1.0).all()) and bool((b == 2.0).all())


def test_buf_dtype_default_explicit_and_clash(ws):
    f = ws.buf("t", (3,), torch.float32)
    assert f.dtype == torch.float32 and f.shape == (3,)
    assert ws.buf("t", (2,), torch.float32).data_ptr() == f.data_ptr()
    with pytest.raises(ValueError):
        ws.buf("t", (3,))                                  # bound as fp32, asked for in the workspace's bf16
    ws.buf("u", (3,))
    with pytest.raises(ValueError):
        ws.buf("u", (1,), torch.float32)
    assert ws["t"].dtype == torch.float32 and ws["u"].dtype == torch.bfloat16   # a refused request changes nothing
    assert Workspace("cpu", torch.float16).buf("h", (2,)).dtype == torch.float16


def test_once_makes_each_key_once(ws):
    calls = []

    def make(tag):
        calls.append(tag)
        return (tag, object())

    first = ws.once(("kv", 2, 64), lambda: make("a"))
    assert ws.once(("kv", 2, 64), lambda: make("a")) is first and ws[("kv", 2, 64)] is first
    other = ws.once(("kv", 2, 128), lambda: make("b"))
    assert other is not first and calls == ["a", "b"]


def test_slab_pool(ws):
    x, y = torch.empty(4, 6, dtype=torch.bfloat16), torch.empty(2, 6, dtype=torch.bfloat16)
    fresh = ws.take_slab(x)
    assert fresh is not x and fresh.shape == x.shape and fresh.dtype == x.dtype       # an empty pool: empty_like
    ws.give_slab(fresh)
    assert ws["mlp_slab_pool"] == [fresh]
    other = ws.take_slab(y)                                # no slab of this shape in the pool: a fresh one, the pool untouched
    assert other is not fresh and other.shape == y.shape and len(ws["mlp_slab_pool"]) == 1
    assert ws.take_slab(x) is fresh and ws["mlp_slab_pool"] == []   # the same object comes back, and leaves the pool
    assert ws.take_slab(x) is not fresh


def test_clear_empties_everything(ws):
    ws.buf("x", (4,))
    ws.once(("kv", 1), lambda: (1, 2))
    ws.give_slab(torch.empty(3))
    assert isinstance(ws, dict) and len(ws) == 3
    ws.clear()
    assert len(ws) == 0 and ws.get("mlp_slab_pool", []) == []
    assert ws.take_slab(torch.empty(3)) is not None and ws.buf("x", (2,)).shape == (2,)   # and it goes on working


def _touched_states():
    states = [pab.BlockState(i // 2, bool(i % 2)) for i in range(4)]
    for st in states:
        st.attn_count, st.cross_count, st.mlp_count = 3, 2, 1
        st.attn_valid = st.cross_valid = True
    return states


def _assert_reset(states):
    for i, st in enumerate(states):
        assert (st.attn_count, st.cross_count, st.mlp_count) == (0, 0, 0)
        assert st.attn_valid is False and st.cross_valid is False
        assert (st.block_idx, st.temporal) == (i // 2, bool(i % 2))


def test_reset_states_with_and_without_a_manager():
    st = pab.BlockState(5, True)
    assert (st.block_idx, st.temporal, st.attn_count, st.cross_count, st.mlp_count) == (5, True, 0, 0, 0)
    assert st.attn_valid is False and st.cross_valid is False and st.last_attn is None and st.last_cross is None
    before = pab.PAB_MANAGER
    try:
        pab.set_pab_manager(pab.PABConfig(spatial_broadcast=True, spatial_threshold=[100, 900], spatial_range=2, mlp_broadcast=True))
        cfg = pab.PAB_MANAGER.config
        cfg.mlp_spatial_outputs[(900, 0)] = object()
        cfg.mlp_temporal_outputs[(900, 1)] = object()
        states = _touched_states()
        pab.reset_states(states)
        _assert_reset(states)
        assert cfg.mlp_spatial_outputs == {} and cfg.mlp_temporal_outputs == {}

        pab.set_pab_manager(None)                          # no manager: the stores of the one that was set are not reached
        cfg.mlp_spatial_outputs[(900, 0)] = 1
        cfg.mlp_temporal_outputs[(900, 1)] = 2
        states = _touched_states()
        pab.reset_states(states)
        _assert_reset(states)
        assert cfg.mlp_spatial_outputs == {(900, 0): 1} and cfg.mlp_temporal_outputs == {(900, 1): 2}
    finally:
        pab.PAB_MANAGER = before


@pytest.mark.parametrize("embed_dim", [8, 16])
def test_sincos_1d_is_the_float64_formula(embed_dim):
    pos = np.arange(5)
    got = sincos_1d(embed_dim, pos)
    omega = 1.0 / 10000 ** (np.arange(embed_dim // 2, dtype=np.float64) / (embed_dim / 2.0))    # float64 frequencies
    angle = pos.astype(np.float64)[:, None] * omega[None, :]
    want = np.concatenate([np.sin(angle), np.cos(angle)], axis=1)                               # [sin | cos]
    assert got.dtype == np.float64 and got.shape == (5, embed_dim)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], np.r_[np.zeros(embed_dim // 2), np.ones(embed_dim // 2)])     # position 0: sin 0 | cos 0
    assert np.array_equal(sincos_1d(embed_dim, pos.reshape(5, 1).astype(np.float32)), got)   # any grid shape / dtype is flattened


def test_static_max_allowed_reads_the_environment_every_call(monkeypatch):
    monkeypatch.delenv("VSYS_FLASH_STATIC", raising=False)
    assert ops.static_max_allowed() is True
    monkeypatch.setenv("VSYS_FLASH_STATIC", "0")
    assert ops.static_max_allowed() is False
    monkeypatch.setenv("VSYS_FLASH_STATIC", "1")
    assert ops.static_max_allowed() is True


def test_load_weights():
    sd = {"a.weight": torch.arange(24.0).reshape(2, 3, 2, 2).permute(0, 1, 3, 2), "a.bias": torch.ones(2, dtype=torch.float64)}
    dst = {}
    load_weights(dst, sd, ["a.weight", "a.bias"], device="cpu", dtype=torch.bfloat16, strict=True, reshape=("a.weight",))
    assert dst["a.weight"].shape == (2, 12) and dst["a.weight"].is_contiguous() and dst["a.weight"].dtype == torch.bfloat16
    assert torch.equal(dst["a.weight"], sd["a.weight"].reshape(2, -1).to(torch.bfloat16))
    assert dst["a.bias"].dtype == torch.bfloat16 and dst["a.bias"].shape == (2,)
    keys = ["a.weight"] + [f"m{i}" for i in range(10)]
    with pytest.raises(KeyError) as e:
        load_weights({}, sd, keys, device="cpu", dtype=torch.bfloat16, strict=True)
    assert e.value.args[0] == f"missing keys: {[f'm{i}' for i in range(8)]}..."
    with pytest.raises(KeyError) as e:
        load_weights({}, sd, ["a.bias", "m0"], device="cpu", dtype=torch.bfloat16, strict=True)
    assert e.value.args[0] == "missing keys: ['m0']"
    dst = {}
    load_weights(dst, sd, keys, device="cpu", dtype=torch.float32, strict=False, reshape=None)   # not strict: what is there is loaded
    assert list(dst) == ["a.weight"] and dst["a.weight"].shape == (2, 3, 2, 2) and dst["a.weight"].is_contiguous()
