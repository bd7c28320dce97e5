"""CPU: the hybrid DynamicVariable's low-frequency admission filter and incremental dump -- known
answers of the sequential oracle (tests/lru_filter_oracle.py) worked by hand, the threshold -> call
mapping, and the surface: keywords, argument checks, C ABI."""
import ctypes
import datetime as dt
import inspect

import numpy as np
import pytest

from lru_filter_oracle import FilterLruTable, admit_below, admit_draw
from lru_oracle import LruTable


def test_admission_draws_written_out():
    """u(seed, key, t) = splitmix64(seed ^ splitmix64(key ^ splitmix64(t))) >> 32"""
    cases = [((0, 0, 1), 2978611956), ((0, 1, 1), 1467295306), ((7, 12345, 3), 3990433697),
             ((5, 2**40 + 3, 2), 1481293771), ((0, -7, 9), 91337075)]
    for (seed, key, t), u in cases:
        assert int(admit_draw(seed, [key], t)[0]) == u, (seed, key, t)
    assert admit_below(0.0) == 0 and admit_below(1.0) == 1 << 32 and admit_below(0.5) == 1 << 31
    assert admit_below(0.3) == 1288490189          # ceil(0.3 * 2^32)
    from hugectr_amd.hybrid_table import admit_below as lib_admit_below
    for p in (0.0, 0.3, 0.5, 0.999, 1.0):
        assert lib_admit_below(p) == admit_below(p)


def test_p0_keeps_stored_keys_and_admits_nothing():
    t = FilterLruTable(8, 2, "3", bucket_size=4)
    t.lookup([1, 2], insert=True)                                  # call 1: 1, 2 stored
    vec, slots, ek, _, filt = t.lookup([2, 5, 1, 5, 9], insert=True, admit=0.0)   # call 2
    assert filt.tolist() == [False, True, False, True, True]
    assert t.filtered == 3 and t.rejected == 0 and t.size() == 2
    assert (slots[filt] == -1).all() and (slots[~filt] >= 0).all() and ek.size == 0
    assert (vec[filt] == 0).all() and (vec[~filt] == 3).all()
    # the hits got score 2, nothing else changed
    occ = t.keys != np.uint64((1 << 64) - 1)
    assert sorted(t.scores[occ].tolist()) == [2, 2] and t.t == 2


def test_p1_equals_the_unfiltered_oracle():
    rng = np.random.default_rng(3)
    a = FilterLruTable(128, 4, "", bucket_size=64, seed=2)
    b = LruTable(128, 4, "", bucket_size=64, seed=2)
    for _ in range(6):
        keys = rng.integers(0, 800, size=300)
        va, sa, ka, ra, filt = a.lookup(keys, insert=True, admit=1.0)
        vb, sb, kb, rb = b.lookup(keys, insert=True)
        assert not filt.any()
        assert np.array_equal(va, vb) and np.array_equal(sa, sb) and np.array_equal(ka, kb)
        assert np.array_equal(ra, rb)
    assert np.array_equal(a.keys, b.keys) and np.array_equal(a.scores, b.scores)
    assert a.rejected == b.rejected > 0 and a.filtered == 0


def test_refused_key_is_admitted_in_a_later_call():
    # key 0, seed 0: u = 2978611956 >= 2^31 in call 1, 425127121 < 2^31 in call 2
    t = FilterLruTable(8, 2, "1", bucket_size=4)
    _, slots, _, _, filt = t.lookup([0, 0], insert=True, admit=0.5)
    assert filt.tolist() == [True, True] and t.size() == 0 and t.filtered == 2
    _, slots, _, _, filt = t.lookup([0], insert=True, admit=0.5)
    assert not filt.any() and slots[0] >= 0 and t.size() == 1 and t.filtered == 2


def test_export_if_selects_by_score():
    t = FilterLruTable(8, 1, "1", bucket_size=4)
    t.lookup([1, 2], insert=True)     # call 1
    t.lookup([3], insert=True)        # call 2
    t.lookup([1], insert=True)        # call 3: 1 -> score 3
    k, s, sc, r = t.export_if(0)
    assert sorted(k.tolist()) == [1, 2, 3]
    k, s, sc, r = t.export_if(2)
    assert sorted(k.tolist()) == [1, 3] and sorted(sc.tolist()) == [2, 3]
    assert t.export_if(4)[0].size == 0


def test_threshold_to_first_call():
    from hugectr_amd import sok
    from hugectr_amd.hybrid_table import first_call_since
    call_ns = [10_000_000_000, 20_000_000_000, 20_000_000_000, 35_000_000_000]
    assert first_call_since(call_ns, 0) == 1
    assert first_call_since(call_ns, 10_000_000_001) == 2
    assert first_call_since(call_ns, 20_000_000_000) == 2          # a tie: the call counts
    assert first_call_since(call_ns, 35_000_000_000) == 4
    assert first_call_since(call_ns, 35_000_000_001) is None       # after the last call
    assert first_call_since([], 0) is None
    utc = dt.timezone.utc
    assert sok._threshold_ns(dt.datetime.fromtimestamp(20, tz=utc)) == 20_000_000_000


def test_lookup_sparse_takes_the_filter_flag():
    from hugectr_amd import sok
    sig = inspect.signature(sok.lookup_sparse)
    assert list(sig.parameters)[:6] == ["params", "sp_ids", "sp_weights", "combiners", "training",
                                        "use_low_frequency_filter"]
    assert sig.parameters["use_low_frequency_filter"].default is False
    assert sig.parameters["training"].default is True
    import torch
    hbm = sok.DynamicVariable.__new__(sok.DynamicVariable)
    hbm._var_type = "hbm"
    ids = sok.Ragged(torch.arange(4), torch.tensor([2, 2]))
    with pytest.raises(TypeError):
        sok.lookup_sparse(hbm, ids, use_low_frequency_filter=True)
    static = sok.DistributedVariable.__new__(sok.DistributedVariable)
    with pytest.raises(TypeError):
        sok.lookup_sparse(static, ids, use_low_frequency_filter=True)


@pytest.mark.parametrize("ratio", [-0.1, 1.5, "0.5", float("nan"), True])
def test_filter_ratio_out_of_range_raises(ratio):
    from hugectr_amd import sok
    with pytest.raises(ValueError):
        sok.DynamicVariable(8, "1", var_type="hybrid", max_capacity=1024, filter_ratio=ratio)


def test_incremental_model_dump_argument_checks():
    from hugectr_amd import sok
    import sparse_operation_kit as sok_pkg
    assert sok_pkg.incremental_model_dump is sok.incremental_model_dump
    assert list(inspect.signature(sok.incremental_model_dump).parameters) == \
        ["sok_vars", "time_threshold", "sess"]
    now = dt.datetime.now(dt.timezone.utc)
    hbm = sok.DynamicVariable.__new__(sok.DynamicVariable)
    hbm._var_type = "hbm"
    hyb = sok.DynamicVariable.__new__(sok.DynamicVariable)
    hyb._var_type = "hybrid"
    static = sok.DistributedVariable.__new__(sok.DistributedVariable)
    with pytest.raises(Exception, match="not hkv backend"):
        sok.incremental_model_dump([hbm], now)
    with pytest.raises(Exception, match="not a sok.DynamicVariable"):
        sok.incremental_model_dump(static, now)
    with pytest.raises(Exception, match="length of time_threshold"):
        sok.incremental_model_dump([hyb, hyb, hyb], [now, now])
    with pytest.raises(Exception, match="sess"):
        sok.incremental_model_dump([hyb], now, sess=object())


def test_filter_symbols_exported_and_arguments_checked_without_a_gpu():
    from hugectr_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hctr_lru_lookup_index_filtered", "hctr_lru_filtered_count", "hctr_lru_compact",
                 "hctr_lru_export_if"):
        assert hasattr(so, name), name
    L = _lib.lib
    assert L.hctr_lru_lookup_index_filtered(None, None, 4, 1 << 31, None, None, None, None,
                                            None) == -1
    assert "null handle" in _lib.last_error()
    assert L.hctr_lru_filtered_count(None, None, None) == -1
    assert "null argument" in _lib.last_error()
    assert L.hctr_lru_compact(None, 2, 4, None, None, None, None, None, None, None, None, None,
                              None) == -1
    assert "null handle" in _lib.last_error()
    assert L.hctr_lru_export_if(None, 3, None, None, None, None, 0, None, None, None) == -1
    assert "null argument" in _lib.last_error()
