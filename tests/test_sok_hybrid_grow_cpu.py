"""CPU: growth of the hybrid table (init_capacity -> max_capacity): the sequential oracle
(tests/lru_grow_oracle.py) has the properties the semantics promise, and the surface -- keywords,
the two new C symbols and their argument checks -- is there without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

from lru_grow_oracle import GrowFilterLruTable, GrowLruTable, checked_calls
from lru_oracle import EMPTY, LruTable, murmur3


def _map(t: LruTable):
    """key -> (score, row, states)"""
    return {k: (int(t.scores[s]), t.rows[s].tobytes(), tuple(st[s].tobytes() for st in t.states))
            for k, s in t.where.items()}


def _consistent(t: LruTable):
    occ = np.nonzero(t.keys != np.uint64(EMPTY))[0]
    assert len(occ) == len(t.where)
    for s in occ:
        k = int(t.keys[s])
        assert t.where[k] == s and murmur3(k, t.key_bytes) % t.nb == s // t.S


def test_a_doubling_moves_keys_in_slot_order_and_loses_nothing():
    rng = np.random.default_rng(3)
    t = GrowLruTable(256, 1024, 4, "", 64, seed=2, num_state=1, max_load_factor=1.0)
    keys = rng.choice(1 << 40, size=200, replace=False)
    t.lookup(keys, True)
    assert t.doublings == 0 and t.size() == 200 and t.rejected == 0
    t.states[0][:] = rng.random(t.states[0].shape, dtype=np.float32)
    before, where, nb, S = _map(t), dict(t.where), t.nb, t.S
    t.double()
    assert (t.C, t.nb, t.doublings) == (512, 2 * nb, 1)
    _consistent(t)
    assert _map(t) == before                                   # score, row, state went along
    moved = dict(t.last_moves)
    assert 0 < len(moved) < 200
    for k, s in where.items():
        if s in moved:
            assert moved[s] // S == s // S + nb
        else:
            assert t.where[k] == s                             # a key that stays keeps its slot
    for b in range(nb):
        src = [s for s, _ in t.last_moves if s // S == b]
        dst = [d for s, d in t.last_moves if s // S == b]
        assert src == sorted(src)                              # ascending old-slot order
        assert dst == list(range((b + nb) * S, (b + nb) * S + len(dst)))
    assert all(t.keys[s] == np.uint64(EMPTY) for s in moved)   # the slot it left is empty


def test_the_load_rule_counts_the_calls_own_new_keys():
    t = GrowLruTable(128, 1024, 2, "1", 64)
    t.lookup(np.arange(64), True)                # 0 + 64 > 0.5 * 128 is false
    assert (t.C, t.doublings) == (128, 0)
    t.lookup(np.arange(65), True)                # 64 + 1 > 64
    assert (t.C, t.doublings) == (256, 1)
    t.lookup(np.arange(1000, 1500), False)       # read-only calls never grow
    t.lookup([], True)                           # nor does the empty call
    assert (t.C, t.t) == (256, 3)
    t.lookup(np.r_[np.arange(65), np.arange(65), -1], True)   # hits, repeats, the reserved key
    assert t.C == 256
    t.lookup(np.arange(2000, 2448), True)        # 65 + 448 > 256: two doublings, decided once
    assert (t.C, t.doublings) == (1024, 3)


def test_a_first_call_beyond_the_largest_capacity_doubles_then_rejects():
    t = GrowLruTable(128, 512, 2, "1", 64)
    t.lookup(np.arange(2000) * 7919 + 1, True)
    assert (t.C, t.doublings, t.size(), t.rejected) == (512, 2, 512, 1488)


@pytest.mark.parametrize("S,c0,cmax,size,fullest", [(64, 128, 1024, 675, 57),
                                                    (128, 256, 2048, 1225, 93)])
def test_grown_equals_created_at_max_capacity(S, c0, cmax, size, fullest):
    """without eviction or rejection a key's score, row and state do not depend on its slot"""
    from oracle import pyoracle as orc
    g = GrowLruTable(c0, cmax, 4, "", S, seed=1, num_state=1)
    f = LruTable(cmax, 4, "", S, seed=1, num_state=1)
    calls = checked_calls(24 if S == 64 else 48)
    rng = np.random.default_rng(1)
    o = orc.OptParamsC()
    o.optimizer, o.update_type, o.lr, o.epsilon, o.scaler, o.times = orc.OPT_ADAGRAD, 0, 0.1, \
        1e-7, 1.0, 1
    evicted = 0
    for keys, train in calls:
        a, b = g.lookup(keys, train), f.lookup(keys, train)
        assert np.array_equal(a[0], b[0])
        evicted += a[2].size + b[2].size
        if train:
            grad = rng.standard_normal((keys.size, 4)).astype(np.float32)
            for t in (g, f):
                orc.update_params(np.arange(keys.size + 1), t.find(keys).astype(np.uint64),
                                  grad.copy(), o, t.rows, t.states[0], None)
        _consistent(g)
        assert _map(g) == _map(f)
    # the precondition, and the figures the input was chosen by
    assert evicted == 0 and g.rejected == 0 and f.rejected == 0
    assert g.doublings == 3 and g.C == cmax
    if S == 64:
        assert g.size() == size
        assert max(int((g.keys[b * S:(b + 1) * S] != np.uint64(EMPTY)).sum())
                   for b in range(g.nb)) == fullest


def test_filtered_growth_counts_admitted_keys_only():
    t = GrowFilterLruTable(128, 1024, 2, "1", 64, seed=4)
    keys = np.arange(5000, 5400)
    out = t.lookup(keys, True, admit=0.25)
    admitted = int((~out[4]).sum())
    assert t.filtered == 400 - admitted and t.size() == admitted
    want = 128
    while want < 1024 and admitted > 0.5 * want:
        want *= 2
    assert t.C == want and 128 < want < 1024


def test_capacities_must_be_a_power_of_two_apart():
    with pytest.raises(ValueError):
        GrowLruTable(384, 1024, 2, "", 128)
    with pytest.raises(ValueError):
        GrowLruTable(128, 1024, 2, "", 64, max_load_factor=0.0)
    assert GrowLruTable(100, 1000, 2, "", 128).Cmax == 1024     # 128 -> 1024 in whole buckets


def test_dynamic_variable_signature():
    from hugectr_amd import sok
    from hugectr_amd.hybrid_table import HybridTable
    sig = inspect.signature(sok.DynamicVariable)
    sig.bind(8, "", var_type="hybrid", init_capacity=128, max_capacity=1024, max_load_factor=0.75)
    assert list(sig.parameters)[:7] == ["dimension", "initializer", "key_type", "init_capacity",
                                        "mode", "seed", "name"]
    assert sig.parameters["init_capacity"].default is None
    hs = inspect.signature(HybridTable)
    assert hs.parameters["init_capacity"].kind is inspect.Parameter.KEYWORD_ONLY
    assert hs.parameters["init_capacity"].default is None
    assert hs.parameters["max_load_factor"].default == 0.5
    for name in ("current_capacity", "doublings", "hbm_slots", "tiered"):
        assert isinstance(getattr(HybridTable, name), property), name


@pytest.mark.parametrize("kw", [dict(init_capacity=2048), dict(max_load_factor=0),
                                dict(max_load_factor=1.5), dict(max_load_factor="0.5"),
                                dict(max_load_factor=True), dict(max_load_factor=float("nan"))])
def test_growth_keywords_are_validated_before_a_device_is_touched(kw):
    from hugectr_amd import sok
    with pytest.raises(ValueError, match="|".join(kw)):
        sok.DynamicVariable(8, "", var_type="hybrid", max_capacity=1024, **kw)


def test_growth_symbols_exported_and_arguments_checked_without_a_gpu():
    from hugectr_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hctr_lru_create_growing", "hctr_lru_growth"):
        assert hasattr(so, name), name
    L = _lib.lib
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert L.hctr_lru_create_growing(384, 1024, 0.5, 128, 8, _lib.KEY_I64, b"", 0, 1 << 40,
                                     out) == -1
    assert "384" in _lib.last_error() and "1024" in _lib.last_error()
    assert L.hctr_lru_create_growing(2048, 1024, 0.5, 128, 8, _lib.KEY_I64, b"", 0, 1 << 40,
                                     out) == -1
    assert "2048" in _lib.last_error() and "1024" in _lib.last_error()
    for load in (0.0, 1.5, float("nan")):
        assert L.hctr_lru_create_growing(128, 1024, load, 128, 8, _lib.KEY_I64, b"", 0, 1 << 40,
                                         out) == -1
        assert "max_load_factor" in _lib.last_error()
    assert L.hctr_lru_create_growing(128, 1024, 0.5, 100, 8, _lib.KEY_I64, b"", 0, 1 << 40,
                                     out) == -1
    assert "bucket_size" in _lib.last_error()
    assert L.hctr_lru_create_growing(128, 1024, 0.5, 128, 8, _lib.KEY_I64, b"", 0, 100, out) == -1
    assert "hbm_slots" in _lib.last_error()
    a, b, d = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    assert L.hctr_lru_growth(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(d)) == -1
    assert not h.value
