"""CPU: the hybrid (bounded, LRU-evicting) DynamicVariable -- known answers of the sequential oracle
(tests/lru_oracle.py) worked by hand, and the surface: keywords, sparse_read_and_evict, C ABI."""
import ctypes
import inspect

import numpy as np
import pytest

from lru_oracle import LruTable, murmur3


def _one_bucket():
    # 4 slots, one bucket: every key lands in bucket 0
    return LruTable(4, 2, "11", bucket_size=4)


def test_oracle_fill_lru_victim_tie_and_rejection():
    t = _one_bucket()
    _, slots, ek, _ = t.lookup([5, 3], insert=True)          # call 1: ascending key order
    assert slots.tolist() == [1, 0] and ek.size == 0
    _, slots, ek, _ = t.lookup([7, 9, 3], insert=True)       # call 2: 3 hit, 7 / 9 fill
    assert slots.tolist() == [2, 3, 0] and t.scores.tolist() == [2, 1, 2, 2]
    t.rows[1] = 4.0                                           # (a trained row)
    _, slots, ek, er = t.lookup([11], insert=True)            # call 3: LRU = slot 1 (score 1)
    assert slots.tolist() == [1] and ek.tolist() == [5] and er.tolist() == [[4.0, 4.0]]
    assert t.rows[1].tolist() == [11.0, 11.0]
    _, slots, ek, _ = t.lookup([13], insert=True)             # call 4: score tie 2 -> lowest slot 0
    assert slots.tolist() == [0] and ek.tolist() == [3]
    v, slots, ek, _ = t.lookup([24, 20, 21, 22, 23], insert=True)  # call 5: 5 keys, 4 slots
    # victims by (score, slot): (2, 2), (2, 3), (3, 1), (4, 0); the largest key is rejected
    assert slots.tolist() == [-1, 2, 3, 1, 0]
    assert ek.tolist() == [7, 9, 11, 13]
    assert t.rejected == 1 and t.size() == 4 and v[0].tolist() == [11.0, 11.0]
    assert t.scores.tolist() == [5, 5, 5, 5]
    v, slots, ek, _ = t.lookup([20, 99], insert=False)        # read only: nothing changes
    assert slots.tolist() == [2, -1] and ek.size == 0 and v[1].tolist() == [11.0, 11.0]
    assert t.t == 5 and t.scores.tolist() == [5, 5, 5, 5]


def test_oracle_hash_is_the_libraries():
    """the oracle's bucket hash = MurmurHash3_32 of the key bytes, seed 0, as the CPU oracle's C
    code computes it (and hctr_hash_keys on the device)"""
    from oracle import pyoracle as orc
    for k in [0, 1, 2, 12345, -7, 2**40 + 3, 2**63 - 1]:
        assert murmur3(k) == orc.murmur3_32(np.int64(k).tobytes())
    for k in [0, 9, 2**32 - 2]:
        assert murmur3(k, 4) == orc.murmur3_32(np.uint32(k).tobytes())


def test_uniform_initializer_depends_on_the_key_only():
    a = LruTable(8, 4, "", bucket_size=4, seed=3)
    b = LruTable(64, 4, "", bucket_size=4, seed=3)
    a.lookup([1, 2, 3, 4, 5], insert=True)
    b.lookup([5, 4], insert=True)
    va, _, _, _ = a.lookup([4, 5], insert=False)
    vb, _, _, _ = b.lookup([4, 5], insert=False)
    assert np.array_equal(va, vb) and (va > 0).all() and (va <= 1).all()


def test_dynamic_variable_takes_the_hybrid_keywords():
    from hugectr_amd import sok
    sig = inspect.signature(sok.DynamicVariable)
    sig.bind(16, "11", var_type="hybrid", max_capacity=16384)
    sig.bind(16, "11", var_type="hybrid", max_capacity=1024, max_bucket_size=128,
             evict_strategy="kLru", max_hbm_for_vectors=1, max_load_factor=0.5)
    assert sig.parameters["var_type"].kind is inspect.Parameter.KEYWORD_ONLY
    # the positional order is unchanged
    assert list(sig.parameters)[:7] == ["dimension", "initializer", "key_type", "init_capacity",
                                        "mode", "seed", "name"]


def test_sparse_read_and_evict_needs_a_hybrid_variable():
    import torch
    from hugectr_amd import sok
    import sparse_operation_kit as sok_pkg
    assert sok_pkg.sparse_read_and_evict is sok.sparse_read_and_evict
    hbm = sok.DynamicVariable.__new__(sok.DynamicVariable)    # (no device needed to be refused)
    hbm._var_type = "hbm"
    with pytest.raises(TypeError):
        sok.sparse_read_and_evict(hbm, torch.arange(4))
    with pytest.raises(TypeError):
        sok.sparse_read_and_evict(object(), torch.arange(4))


def test_lru_symbols_exported_and_arguments_checked_without_a_gpu():
    from hugectr_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hctr_lru_create", "hctr_lru_destroy", "hctr_lru_lookup_index", "hctr_lru_find",
                 "hctr_lru_rows", "hctr_lru_state", "hctr_lru_export", "hctr_lru_size",
                 "hctr_lru_rejected_count", "hctr_lru_capacity"):
        assert hasattr(so, name), name
    L = _lib.lib
    h = ctypes.c_void_p()
    assert L.hctr_lru_create(1024, 100, 16, _lib.KEY_I64, b"11", 0, ctypes.byref(h)) == -1
    assert "bucket_size" in _lib.last_error()
    assert L.hctr_lru_create(0, 128, 16, _lib.KEY_I64, b"11", 0, ctypes.byref(h)) == -1
    assert L.hctr_lru_lookup_index(None, None, 4, 1, None, None, None, None, None) == -1
    assert "null handle" in _lib.last_error()
