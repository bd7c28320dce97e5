"""CPU: the host-memory tier of hybrid DynamicVariables (max_hbm_for_vectors) -- the C ABI's new
symbols and their argument checks, worked examples of the HBM-slot formula, and the validation of
the budget."""
import ctypes
import inspect
import math

import pytest


def test_tier_symbols_exported_and_arguments_checked_without_a_gpu():
    from hugectr_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hctr_lru_create_tiered", "hctr_lru_placement", "hctr_lru_host_part",
                 "hctr_lru_gather_slots", "hctr_lru_scatter_slots", "hctr_lru_apply_update"):
        assert hasattr(so, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    L = _lib.lib
    h = ctypes.c_void_p()
    # hbm_slots must be a whole number of buckets (checked before anything is allocated)
    assert L.hctr_lru_create_tiered(1024, 128, 16, _lib.KEY_I64, b"11", 0, 100,
                                    ctypes.byref(h)) == -1
    assert "hbm_slots" in _lib.last_error()
    assert L.hctr_lru_create_tiered(1024, 100, 16, _lib.KEY_I64, b"11", 0, 512,
                                    ctypes.byref(h)) == -1
    assert "bucket_size" in _lib.last_error()
    assert L.hctr_lru_create_tiered(1024, 128, 16, _lib.KEY_I64, b"11", 0, 0, None) == -1
    a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert L.hctr_lru_placement(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert L.hctr_lru_gather_slots(None, 0, None, 4, None, None) == -1
    assert "null handle" in _lib.last_error()
    assert L.hctr_lru_scatter_slots(None, 0, None, 4, None, 0, None) == -1
    assert "null handle" in _lib.last_error()
    assert L.hctr_lru_apply_update(None, None, 4, 4, None, None, None, _lib.F32, _lib.OPT_SGD,
                                   0.1, 0.9, 0.999, 1e-7, 0.0, 1.0, 1, None) == -1
    assert "null handle" in _lib.last_error()


@pytest.mark.parametrize("g, dim, cap, S, want", [
    # 1 MiB at D = 16: 16384 rows = 128 buckets of 128 -- fits 2^16 slots in part
    (1 / 1024, 16, 1 << 16, 128, 16384),
    # 1000 B of budget rounds down to no whole bucket
    (1000 / 2**30, 4, 4096, 64, 0),
    # rounding down to a bucket: 0.001 GiB / 64 B = 16777.216 rows -> 131 buckets of 128
    (0.001, 16, 1 << 20, 128, 131 * 128),
    # clamped to C (capacity rounded up to whole buckets: 1000 -> 1024)
    (16, 128, 1000, 128, 1024),
    (1, 16, 1 << 24, 128, 1 << 24),       # exactly C: untiered
    (0, 128, 1 << 20, 128, 0),            # all values in host memory
    (0.0, 8, 256, 128, 0),
    (0.125, 128, 1 << 22, 128, 1 << 18),  # 128 MiB of D = 128 rows
    (float("inf"), 8, 256, 128, 256),
])
def test_hbm_slots_formula(g, dim, cap, S, want):
    from hugectr_amd.hybrid_table import hbm_slots_for
    got = hbm_slots_for(g, dim, cap, S)
    assert got == want
    assert got % S == 0
    C = -(-cap // S) * S
    if not math.isinf(g):
        assert got == min(C, math.floor(g * 2**30 / (dim * 4) / S) * S)


@pytest.mark.parametrize("bad", [-1, -0.5, float("nan"), True, False, "1", None, [1], 1j])
def test_max_hbm_for_vectors_is_validated(bad):
    from hugectr_amd import sok
    from hugectr_amd.hybrid_table import check_hbm_budget, hbm_slots_for
    with pytest.raises(ValueError):
        check_hbm_budget(bad)
    with pytest.raises(ValueError):
        hbm_slots_for(bad, 16, 1024, 128)
    if bad is None:
        return  # (None is the keyword left out: an all-HBM variable, which needs a device)
    # refused before anything touches a device
    with pytest.raises(ValueError, match="max_hbm_for_vectors"):
        sok.DynamicVariable(16, "11", var_type="hybrid", max_capacity=1024,
                            max_hbm_for_vectors=bad)


@pytest.mark.parametrize("good", [0, 1, 16, 0.5, 1e-4, 2**40])
def test_max_hbm_for_vectors_accepts_numbers(good):
    from hugectr_amd.hybrid_table import check_hbm_budget
    assert check_hbm_budget(good) == float(good)


def test_the_hybrid_keywords_still_bind():
    from hugectr_amd import sok
    sig = inspect.signature(sok.DynamicVariable)
    sig.bind(16, "11", var_type="hybrid", max_capacity=1024, max_hbm_for_vectors=0.25)
    sig.bind(16, "11", var_type="hybrid", max_capacity=1024, max_bucket_size=128,
             evict_strategy="kLru", max_hbm_for_vectors=1, max_load_factor=0.5)


def test_hybrid_table_takes_hbm_slots():
    from hugectr_amd.hybrid_table import HybridTable
    sig = inspect.signature(HybridTable)
    assert sig.parameters["hbm_slots"].default is None
    for name in ("gather_slots", "scatter_slots", "apply_update", "placement"):
        assert callable(getattr(HybridTable, name)), name
    assert isinstance(HybridTable.tiered, property)
