"""CPU: the C ABI and the configuration side of CompressionStrategy.Unique on several GPUs (no
compute calls here; tests/test_ebc_unique_gpu.py holds the parity tests)."""
import re
import types

import numpy as np
import pytest

import ebc_unique_oracle as uo

NEW = ["hctr_ebc_uniq_plan_workspace_bytes", "hctr_ebc_uniq_plan", "hctr_ebc_uniq_gather_rows",
       "hctr_ebc_uniq_network_forward", "hctr_ebc_uniq_backward_workspace_bytes",
       "hctr_ebc_uniq_network_backward"]


def test_header_exports_and_binding_name_the_new_entries():
    import ctypes
    import os
    from hugectr_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hugectr_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hctr_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTED_SYMBOLS)


def test_new_entries_validate_before_touching_the_device():
    from hugectr_amd import _lib
    L = _lib.lib
    assert L.hctr_ebc_uniq_plan_workspace_bytes(1000) > 9 * 4 * 1000
    assert L.hctr_ebc_uniq_plan(8, 0, 4, None, None, 10, None, None, None, None, 0, None) == -1
    assert "world" in _lib.last_error()
    assert L.hctr_ebc_uniq_plan(8, 2, 4, None, None, 2**32 - 1, None, None, None, None, 0, None) == -1
    assert "2^32 - 16" in _lib.last_error()
    assert L.hctr_ebc_uniq_plan(8, 2, 4, None, None, 10, None, None, None, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    assert L.hctr_ebc_uniq_gather_rows(4, 0, None, None, 10, None, 0, None) == -1
    assert "ev_size" in _lib.last_error()
    assert L.hctr_ebc_uniq_gather_rows(4, 16, None, None, 10, None, 7, None) == -1
    assert "out_dtype" in _lib.last_error()
    assert L.hctr_ebc_uniq_gather_rows(4, 16, None, None, 10, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    assert L.hctr_ebc_uniq_network_forward(8, 3, 16, 0, None, None, None, 0, None, None, None, None,
                                           None, None, None, 0, None) == -1
    assert "max_shards" in _lib.last_error()
    assert L.hctr_ebc_uniq_network_forward(8, 3, 16, 2, None, None, None, 0, None, None, None, None,
                                           None, None, None, 9, None) == -1
    assert "dtype" in _lib.last_error()
    assert L.hctr_ebc_uniq_network_forward(8, 3, 16, 2, None, None, None, 0, None, None, None, None,
                                           None, None, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    assert L.hctr_ebc_uniq_backward_workspace_bytes(1000, 8, 3, 16) > 6 * 4 * 1000
    assert L.hctr_ebc_uniq_network_backward(None, 8, 3, 16, 4, None, None, None, None, 0, 0, None,
                                            None, None, 10, 5, None, 0, None, None, 0, None) == -1
    assert "null handle" in _lib.last_error()


def test_plan_oracle_states_the_contract():
    # two peers, two buckets each; peer 0 repeats row 7, peer 1 holds one key
    urow, peer_off, ridx = uo.plan([0, 2, 3, 3, 4], [7, 3, 7, 7], 2, 2)
    assert urow.tolist() == [3, 7, 7] and peer_off.tolist() == [0, 2, 3]
    assert ridx.tolist() == [1, 0, 1, 0]
    acc = uo.pool([np.array([[1.0, 2.0], [3.0, 4.0]], np.float32), np.zeros((0, 2), np.float32)], 2, True)
    assert acc.tolist() == [2.0, 3.0]


def test_split_keeps_every_tables_strategy():
    """hugectr.Model splits a config by (placement, vector size, strategy); every sub-config names
    the strategy of its tables (on one GPU nothing is split by strategy)"""
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd.embedding_collection import EmbeddingCollectionConfig, EmbeddingTableConfig
    S = hugectr.CompressionStrategy
    tabs = [EmbeddingTableConfig("u16", 100, 16), EmbeddingTableConfig("r16", 100, 16),
            EmbeddingTableConfig("u4", 100, 4), EmbeddingTableConfig("r4", 100, 4),
            EmbeddingTableConfig("dp16", 10, 16), EmbeddingTableConfig("u16b", 50, 16)]
    names = [t.name for t in tabs]
    mp = ["u16", "r16", "u4", "r4", "u16b"]

    def config(world):
        c = EmbeddingCollectionConfig()
        c.embedding_lookup(tabs, [f"in{i}" for i in range(6)], [f"out{i}" for i in range(6)],
                           ["sum"] * 6)
        return c.shard([names] * world, [("mp", mp), ("dp", ["dp16"])],
                       [(S.Unique, ["u16", "u4", "u16b"]), (S.Reduction, ["r16", "r4"])])
    cfg = config(2)
    subs = hugectr.Model._split_by_ev_size(types.SimpleNamespace(world=2), cfg)
    got = {}
    for sub, ids in subs:
        key = (sub.shard_strategy if sub.shard_strategy == "dp" else "mp",
               sub.lookups[0][0].ev_size, tuple(sorted(set(sub.compression.values()))))
        got[key] = [cfg.lookups[l][0].name for l in ids]
        for t, _, _, _ in sub.lookups:  # nothing dropped, nothing invented
            assert sub.compression.get(t.name) == cfg.compression.get(t.name)
    assert got == {("dp", 16, ()): ["dp16"],
                   ("mp", 4, ("reduction",)): ["r4"], ("mp", 4, ("unique",)): ["u4"],
                   ("mp", 16, ("reduction",)): ["r16"], ("mp", 16, ("unique",)): ["u16", "u16b"]}
    assert sorted(l for _, ids in subs for l in ids) == list(range(6))
    one = hugectr.Model._split_by_ev_size(types.SimpleNamespace(world=1), config(1))
    assert len(one) == 3  # dp, ev 4, ev 16


def test_mixed_strategies_in_one_collection_are_refused_by_name():
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    from hugectr_amd.embedding_collection import (EmbeddingCollection, EmbeddingCollectionConfig,
                                                  EmbeddingTableConfig)
    tabs = [EmbeddingTableConfig(f"t{i}", 100, 8) for i in range(2)]
    cfg = EmbeddingCollectionConfig()
    cfg.embedding_lookup(tabs, ["a", "b"], "emb", ["sum"] * 2)
    cfg.shard([["t0", "t1"]] * 2, [("mp", ["t0", "t1"])],
              [(hugectr.CompressionStrategy.Reduction, ["t0"]),
               (hugectr.CompressionStrategy.Unique, ["t1"])])
    with pytest.raises(_lib.HugeCTRAmdError) as ex:
        EmbeddingCollection.for_rank(0, 2, cfg, 64)
    msg = str(ex.value)
    assert "CompressionStrategy.Unique" in msg and "separate collections" in msg
    assert "hugectr.Model splits" in msg
