"""No device: the hybrid options of EmbeddingTableConfig (every violation raises RuntimeError when
the object is made) and hugectr.Model._split_by_ev_size on a config mixing static, dynamic and
hybrid tables of two vector sizes."""
import types

import pytest


def _cfg(**kw):
    import hugectr_amd as ha
    base = dict(var_type="hybrid", max_capacity=1024)
    base.update(kw)
    return ha.EmbeddingTableConfig("t", base.pop("vocab", -1), 16, **base)


def test_hybrid_options_are_keyword_only_and_default_like_sok():
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    assert hugectr.EmbeddingTableConfig is ha.EmbeddingTableConfig
    t = ha.EmbeddingTableConfig("t", 100, 8, None, None)     # the positional signature
    assert (t.var_type, t.max_capacity, t.init_capacity, t.max_hbm_for_vectors) == (None,) * 4
    assert (t.max_load_factor, t.max_bucket_size, t.initializer) == (0.5, 128, "")
    with pytest.raises(TypeError):
        ha.EmbeddingTableConfig("t", -1, 8, None, None, "hybrid")
    h = _cfg(init_capacity=128, max_load_factor=1, max_bucket_size=64, max_hbm_for_vectors=0.5,
             initializer="ones")
    assert h.hybrid and h.max_capacity == 1024 and not t.hybrid
    assert ha.EmbeddingTableConfig("d", -1, 8, var_type="hbm").hybrid is False


@pytest.mark.parametrize("kw,match", [
    (dict(var_type="host"), "var_type"),
    (dict(vocab=100), "max_vocabulary_size must be < 0"),
    (dict(vocab=0), "max_vocabulary_size must be < 0"),
    (dict(max_capacity=None), "needs max_capacity"),
    (dict(max_capacity=0), "max_capacity must be a positive int"),
    (dict(max_capacity=10.5), "max_capacity must be a positive int"),
    (dict(max_capacity=True), "max_capacity must be a positive int"),
    (dict(init_capacity=0), "init_capacity must be a positive int"),
    (dict(init_capacity=2048), "above max_capacity"),
    (dict(init_capacity=384), "power of two"),
    (dict(max_load_factor=0.0), "max_load_factor"),
    (dict(max_load_factor=1.5), "max_load_factor"),
    (dict(max_load_factor="half"), "max_load_factor"),
    (dict(max_load_factor=True), "max_load_factor"),
    (dict(max_bucket_size=100), "max_bucket_size"),
    (dict(max_hbm_for_vectors=-1), "max_hbm_for_vectors"),
    (dict(max_hbm_for_vectors=float("nan")), "max_hbm_for_vectors"),
    (dict(max_hbm_for_vectors=True), "max_hbm_for_vectors"),
    (dict(max_hbm_for_vectors="1"), "max_hbm_for_vectors"),
    (dict(initializer=None), "initializer"),
])
def test_hybrid_option_violations(kw, match):
    with pytest.raises(RuntimeError, match=match):
        _cfg(**kw)


@pytest.mark.parametrize("var_type", [None, "hbm"])
@pytest.mark.parametrize("kw", [dict(max_capacity=1024), dict(init_capacity=64),
                                dict(max_load_factor=0.75), dict(max_bucket_size=64),
                                dict(max_hbm_for_vectors=1.0), dict(initializer="ones")])
def test_hybrid_options_on_another_table_kind(var_type, kw):
    import hugectr_amd as ha
    with pytest.raises(RuntimeError, match=f'{next(iter(kw))}.*var_type="hybrid"'):
        ha.EmbeddingTableConfig("t", -1, 16, var_type=var_type, **kw)


def test_the_budget_formula_is_the_hybrid_variables():
    """hbm_slots_for / check_hbm_budget are reused, not restated"""
    from hugectr_amd import embedding_collection as ec, hybrid_table
    assert ec.hbm_slots_for is hybrid_table.hbm_slots_for
    assert ec.check_hbm_budget is hybrid_table.check_hbm_budget


def test_setup_checks_come_before_any_device_call(monkeypatch):
    """mixed kinds in one collection, an unsupported optimizer, Unique on two GPUs, 2^24 keys: all
    raised by _setup before it asks for a device"""
    import torch
    import hugectr_amd as ha
    from hugectr_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("a device call")
    monkeypatch.setattr(torch.cuda, "current_device", no_device)

    def config(tables, world=1, unique=False):
        cfg = ha.EmbeddingCollectionConfig()
        for i, t in enumerate(tables):
            cfg.embedding_lookup(t, f"in{i}", f"out{i}", "sum")
        names = [t.name for t in tables]
        cfg.shard([[1] * len(tables)] * world, "mp", [("Unique", names)] if unique else None)
        return cfg
    hyb = [ha.EmbeddingTableConfig(f"h{i}", -1, 8, var_type="hybrid", max_capacity=256)
           for i in range(2)]
    dyn = ha.EmbeddingTableConfig("d0", -1, 8)
    with pytest.raises(RuntimeError, match=r"d0.*not var_type=\"hybrid\".*h0"):
        ha.EmbeddingCollection.for_rank(0, 1, config([hyb[0], dyn]), 8)
    with pytest.raises(RuntimeError, match="RMSProp.*h0.*supported: SGD, AdaGrad, Adam"):
        ha.EmbeddingCollection.for_rank(0, 1, config(hyb), 8, optimizer=_lib.OPT_RMSPROP)
    with pytest.raises(RuntimeError, match="Ftrl"):
        ha.EmbeddingCollection.for_rank(0, 1, config(hyb), 8, optimizer=_lib.OPT_FTRL)
    with pytest.raises(RuntimeError, match="Unique.*h0.*h1.*hybrid"):
        ha.EmbeddingCollection.for_rank(1, 2, config(hyb, 2, True), 8)
    with pytest.raises(RuntimeError, match=r"h0.*2\^24"):
        ha.EmbeddingCollection.for_rank(0, 1, config(hyb), 1 << 20, hotness=[17, 1])
    # a multi-hot "concat" lookup is expanded into one-key lookups later: the estimate is made on
    # the user's lookups, whose hotness list it is
    cc = ha.EmbeddingCollectionConfig()
    cc.embedding_lookup(hyb[1], "a", "oa", "sum")
    cc.embedding_lookup(hyb[0], "b", "ob", "concat")
    with pytest.raises(RuntimeError, match=r"h0.*2\^24"):
        ha.EmbeddingCollection.for_rank(0, 1, cc, 1 << 16, hotness=[1, 300], batch_major=True)
    with pytest.raises(RuntimeError, match=r"hybrid"):     # storage="hybrid" on plain tables
        ha.EmbeddingCollection.for_rank(0, 1, config([dyn]), 8, storage="hybrid")


def test_split_by_storage_kind_and_vector_size():
    """static, dynamic and hybrid tables of two vector sizes: the hybrid tables form their own
    sub-collections, one per vector size; the others are grouped as before"""
    import hugectr_amd.hugectr as hugectr
    T = hugectr.EmbeddingTableConfig
    tables = [T("s8", 100, 8), T("d8", -1, 8), T("h8", -1, 8, var_type="hybrid", max_capacity=256),
              T("h8b", -1, 8, var_type="hybrid", max_capacity=512, max_hbm_for_vectors=0.0),
              T("s16", 50, 16), T("h16", -1, 16, var_type="hybrid", max_capacity=256)]
    cfg = hugectr.EmbeddingCollectionConfig()
    for i, t in enumerate(tables + [tables[2]]):       # h8 is read by two lookups
        cfg.embedding_lookup(t, f"in{i}", f"out{i}", "sum")
    names = [t.name for t in tables]
    cfg.shard([names, names], [("mp", names[:5]), ("dp", ["h16"])])
    model = types.SimpleNamespace(world=2)
    subs = hugectr.Model._split_by_ev_size(model, cfg)
    got = {tuple(sorted({t.name for t, _, _, _ in sub.lookups})): ids for sub, ids in subs}
    assert got == {("d8", "s8"): [0, 1], ("h8", "h8b"): [2, 3, 6], ("s16",): [4], ("h16",): [5]}
    for sub, ids in subs:
        assert [cfg.lookups[l] for l in ids] == sub.lookups
        kinds = {t.hybrid for t, _, _, _ in sub.lookups}
        assert len(kinds) == 1
        # a hybrid table named under "dp" stays model parallel, as dynamic ones do
        assert sub.shard_strategy != "dp"
        assert all(sum(col) == 2 for col in zip(*sub.shard_matrix))
    # hybrid tables only, one size: nothing to split
    cfg2 = hugectr.EmbeddingCollectionConfig()
    cfg2.embedding_lookup(tables[2], "a", "oa", "sum")
    cfg2.embedding_lookup(tables[3], "b", "ob", "mean")
    (sub, ids), = hugectr.Model._split_by_ev_size(types.SimpleNamespace(world=1), cfg2)
    assert sub is cfg2 and ids == [0, 1]
    # static + dynamic of one size: one collection, as before
    cfg3 = hugectr.EmbeddingCollectionConfig()
    cfg3.embedding_lookup(tables[0], "a", "oa", "sum")
    cfg3.embedding_lookup(tables[1], "b", "ob", "sum")
    (sub, ids), = hugectr.Model._split_by_ev_size(types.SimpleNamespace(world=1), cfg3)
    assert sub is cfg3


def test_readme_example_runs_as_written():
    """the three-line example of README's table-kind paragraph, against the public surface"""
    import os
    import re
    import hugectr_amd.hugectr as hugectr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "README.md")) as f:
        blocks = re.findall(r"```python\n(.*?)```", f.read(), flags=re.S)
    snippet, = [b for b in blocks if 'var_type="hybrid"' in b and "EmbeddingTableConfig" in b]
    added = []
    env = dict(hugectr=hugectr, model=types.SimpleNamespace(add=added.append))
    exec(snippet, env)
    cfg, = added
    (t, bottom, top, comb), = cfg.lookups
    assert t.hybrid and t.max_capacity == 1 << 24 and t.init_capacity == 1 << 20
    assert t.max_hbm_for_vectors == 4 and (bottom, top, comb) == ("data0", "emb0", "sum")
    assert cfg.ownership([t], 1) == [[1]]
