"""No device: EmbeddingTableConfig(opt_params=..., init_param=...) -- the grouping of a config's
lookups by resolved optimizer, the refusals of the validation step, hugectr.InitParams and the
sinusoidal table, and the per-table optimizer heads of embedding_io.create_collection."""
import filecmp
import os
import struct
import types

import numpy as np
import pytest


def _h():
    import hugectr_amd.hugectr as hugectr
    return hugectr


def _opt(name, **kw):
    h = _h()
    return h.CreateOptimizer(optimizer_type=getattr(h.Optimizer_t, name), **kw)


def _config(tables, lookups=None, dp=()):
    h = _h()
    cfg = h.EmbeddingCollectionConfig()
    for i, t in enumerate(lookups if lookups is not None else range(len(tables))):
        cfg.embedding_lookup(tables[t], f"in{i}", f"out{i}", "sum")
    names = [t.name for t in tables]
    if dp:
        cfg.shard([names], [("mp", [n for n in names if n not in dp]), ("dp", list(dp))])
    return cfg


def _split(cfg, model_opt, world=1):
    return _h().Model._split_by_ev_size(types.SimpleNamespace(world=world, opt=model_opt), cfg)


# ---- 1. the grouping function -----------------------------------------------------------------------
def test_tables_that_resolve_alike_are_one_group_and_today_s_split():
    h = _h()
    from hugectr_amd.embedding_collection import group_lookups_by_optimizer
    ada = _opt("AdaGrad")
    plain = [h.EmbeddingTableConfig(f"t{i}", 100, 16) for i in range(3)]
    # the same optimizer spelt on the tables, and one table following the model
    same = [h.EmbeddingTableConfig("t0", 100, 16, _opt("AdaGrad")),
            h.EmbeddingTableConfig("t1", 100, 16), h.EmbeddingTableConfig("t2", 100, 16, ada)]
    for tables in (plain, same):
        cfg = _config(tables)
        groups = group_lookups_by_optimizer(cfg.lookups, ada)
        assert [ids for ids, _ in groups] == [[0, 1, 2]]
        assert groups[0][1].optimizer_type == h.Optimizer_t.AdaGrad
        (sub, ids), = _split(cfg, ada)
        assert sub is cfg and ids == [0, 1, 2]           # what the code without opt_params returns
    # ... and without a model (the existing callers of the split): no optimizer, one group
    (sub, ids), = h.Model._split_by_ev_size(types.SimpleNamespace(world=1), _config(plain))
    assert ids == [0, 1, 2]


def test_three_optimizers_give_three_groups_in_lookup_order():
    h = _h()
    from hugectr_amd.embedding_collection import group_lookups_by_optimizer
    tables = [h.EmbeddingTableConfig("t0", 100, 16, _opt("Ftrl", beta=0.1, lambda1=0.01)),
              h.EmbeddingTableConfig("t1", 100, 16, _opt("SGD")),
              h.EmbeddingTableConfig("t2", 100, 16)]
    cfg = _config(tables)
    groups = group_lookups_by_optimizer(cfg.lookups, _opt("AdaGrad"))
    assert [ids for ids, _ in groups] == [[0], [1], [2]]
    assert [o.optimizer_type.name for _, o in groups] == ["Ftrl", "SGD", "AdaGrad"]
    subs = _split(cfg, _opt("AdaGrad"))
    assert [ids for _, ids in subs] == [[0], [1], [2]]
    for sub, ids in subs:
        assert sub.lookups == [cfg.lookups[l] for l in ids]
        assert sub.shard_matrix == [[1]]
    # the lookup order decides, not the table order: t2's lookup first
    groups = group_lookups_by_optimizer(_config(tables, [2, 0, 1]).lookups, _opt("AdaGrad"))
    assert [(ids, o.optimizer_type.name) for ids, o in groups] == \
        [([0], "AdaGrad"), ([1], "Ftrl"), ([2], "SGD")]


def test_only_the_hyper_parameters_a_type_reads_split_a_group():
    h = _h()
    from hugectr_amd.embedding_collection import group_lookups_by_optimizer, optimizer_key

    def groups(a, b):
        tables = [h.EmbeddingTableConfig("t0", 100, 16, a), h.EmbeddingTableConfig("t1", 100, 16, b)]
        return [ids for ids, _ in group_lookups_by_optimizer(_config(tables).lookups, _opt("SGD"))]
    assert groups(_opt("AdaGrad", beta1=0.9), _opt("AdaGrad", beta1=0.5)) == [[0, 1]]
    assert groups(_opt("AdaGrad", epsilon=1e-7), _opt("AdaGrad", epsilon=1e-3)) == [[0], [1]]
    assert groups(_opt("AdaGrad"), _opt("AdaGrad", initial_accu_value=0.5)) == [[0], [1]]
    assert groups(_opt("SGD", epsilon=1.0, momentum_factor=0.3, atomic_update=False),
                  _opt("SGD", update_type=h.Update_t.Local)) == [[0, 1]]
    assert groups(_opt("Ftrl", lambda1=0.1), _opt("Ftrl", lambda1=0.2)) == [[0], [1]]
    assert groups(_opt("Ftrl", epsilon=1.0), _opt("Ftrl")) == [[0, 1]]
    assert groups(_opt("RMSProp", beta2=0.9), _opt("RMSProp", beta2=0.99)) == [[0], [1]]
    assert groups(_opt("RMSProp", beta1=0.1), _opt("RMSProp")) == [[0, 1]]
    assert groups(_opt("Nesterov", momentum_factor=0.9), _opt("MomentumSGD", momentum_factor=0.9)) \
        == [[0], [1]]
    # the table of the issue, field by field
    reads = {"AdaGrad": {"epsilon", "initial_accu_value"}, "Ftrl": {"beta", "lambda1", "lambda2"},
             "Adam": {"beta1", "beta2", "epsilon"}, "RMSProp": {"beta2", "epsilon"},
             "MomentumSGD": {"momentum_factor"}, "Nesterov": {"momentum_factor"}, "SGD": set()}
    for name, want in reads.items():
        base = optimizer_key(_opt(name))
        got = {f for f in ("beta", "lambda1", "lambda2", "beta1", "beta2", "epsilon",
                           "initial_accu_value", "momentum_factor")
               if optimizer_key(_opt(name, **{f: 0.123})) != base}
        assert got == want, name


def test_a_table_used_by_two_lookups_stays_in_one_group():
    h = _h()
    from hugectr_amd.embedding_collection import group_lookups_by_optimizer
    tables = [h.EmbeddingTableConfig("t0", 100, 16, _opt("SGD")),
              h.EmbeddingTableConfig("t1", 100, 16)]
    cfg = _config(tables, [0, 1, 0])
    groups = group_lookups_by_optimizer(cfg.lookups, _opt("AdaGrad"))
    assert [ids for ids, _ in groups] == [[0, 2], [1]]
    assert [ids for _, ids in _split(cfg, _opt("AdaGrad"))] == [[0, 2], [1]]


def test_the_optimizer_joins_the_other_split_keys():
    """vector size, placement and table kind still split; the optimizer splits inside them"""
    h = _h()
    sgd = _opt("SGD")
    tables = [h.EmbeddingTableConfig("s16", 100, 16, sgd), h.EmbeddingTableConfig("a16", 100, 16),
              h.EmbeddingTableConfig("s8", 100, 8, sgd), h.EmbeddingTableConfig("dp16", 50, 16, sgd),
              h.EmbeddingTableConfig("d16", -1, 16, sgd),
              h.EmbeddingTableConfig("h16", -1, 16, sgd, var_type="hybrid", max_capacity=256)]
    cfg = _config(tables, dp=("dp16",))
    got = sorted(([t.name for t, _, _, _ in sub.lookups], sub.shard_strategy == "dp")
                 for sub, _ in _split(cfg, _opt("AdaGrad")))
    assert got == [(["a16"], False), (["dp16"], True), (["h16"], False), (["s16", "d16"], False),
                   (["s8"], False)]


def test_opt_params_must_be_what_create_optimizer_returns():
    h = _h()
    with pytest.raises(RuntimeError, match=r"'tbl'.*opt_params.*CreateOptimizer"):
        h.EmbeddingTableConfig("tbl", 100, 16, opt_params="AdaGrad")
    with pytest.raises(RuntimeError, match=r"'tbl'.*init_param.*InitParams"):
        h.EmbeddingTableConfig("tbl", 100, 16, None, {"up_bound": 1.0})
    t = h.EmbeddingTableConfig("tbl", 100, 16, _opt("SGD"), h.InitParams(16))
    assert t.opt_params.optimizer_type == h.Optimizer_t.SGD
    # an opt_params that is not `initialized` follows the model, as SparseEmbedding(optimizer=)
    from hugectr_amd.embedding_collection import resolve_table_optimizer
    off = _opt("SGD")
    off.initialized = False
    model = _opt("Adam")
    assert resolve_table_optimizer(h.EmbeddingTableConfig("t", 10, 4, off), model) == (model, "model")
    assert resolve_table_optimizer(t, model) == (t.opt_params, "table")


# ---- 2. refusals of the pure validation step ------------------------------------------------------------
def test_refusals_name_table_optimizer_source_and_supported_list(monkeypatch):
    import torch
    h = _h()

    def no_device(*a, **k):
        raise AssertionError("a device call")
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    check = h.check_embedding_collection_config
    ok = h.EmbeddingTableConfig("fine", 100, 16, _opt("SGD"))
    # a static table with Adam opt_params under a model on SGD
    cfg = _config([ok, h.EmbeddingTableConfig("st", 100, 16, _opt("Adam"))])
    with pytest.raises(RuntimeError, match=r"static embedding_collection tables support SGD, AdaGrad "
                       r"and Ftrl.*static table 'st'.*Adam.*'st' opt_params.*"
                       r"supported: SGD, AdaGrad, Ftrl") as e:
        check(cfg, _opt("SGD"))
    assert "the model's" not in str(e.value) and "'fine'" not in str(e.value)
    # a hybrid table with Ftrl opt_params
    hyb = h.EmbeddingTableConfig("hy", -1, 16, _opt("Ftrl"), var_type="hybrid", max_capacity=256)
    with pytest.raises(RuntimeError, match=r"hybrid embedding_collection tables \['hy'\] do not "
                       r"support Ftrl.*'hy' opt_params.*supported: SGD, AdaGrad, Adam, MomentumSGD, "
                       r"Nesterov"):
        check(_config([ok, hyb]), _opt("SGD"))
    # a static table that resolves to the MODEL's Adam, next to one that is fine
    cfg = _config([ok, h.EmbeddingTableConfig("follows", 100, 16)])
    with pytest.raises(RuntimeError, match=r"static table 'follows'.*Adam.*the model's optimizer.*"
                       r"supported: SGD, AdaGrad, Ftrl") as e:
        check(cfg, h.CreateOptimizer())
    assert "opt_params" not in str(e.value)
    # a replicated table is a static table
    cfg = _config([ok, h.EmbeddingTableConfig("rep", 50, 16, _opt("Nesterov"))], dp=("rep",))
    with pytest.raises(RuntimeError, match=r"replicated.*'rep'.*Nesterov.*supported: SGD, AdaGrad, Ftrl"):
        check(cfg, _opt("SGD"))
    # what stays accepted: all seven on a dynamic table, the hybrid five, the static three
    for name in ("Ftrl", "Adam", "RMSProp", "AdaGrad", "Nesterov", "MomentumSGD", "SGD"):
        check(_config([h.EmbeddingTableConfig("dy", -1, 16, _opt(name)), ok]), h.CreateOptimizer())
    for name in ("SGD", "AdaGrad", "Adam", "MomentumSGD", "Nesterov"):
        check(_config([h.EmbeddingTableConfig("hy", -1, 16, _opt(name), var_type="hybrid",
                                              max_capacity=256)]), _opt("Ftrl"))
    for name in ("SGD", "AdaGrad", "Ftrl"):
        check(_config([h.EmbeddingTableConfig("st", 100, 16, _opt(name))]), h.CreateOptimizer())
    # a static table beside a dynamic one with the same optimizer is held by the dynamic table
    check(_config([h.EmbeddingTableConfig("st", 100, 16), h.EmbeddingTableConfig("dy", -1, 16)]),
          h.CreateOptimizer())


def test_a_collection_used_directly_refuses_tables_with_different_optimizers(monkeypatch):
    import torch
    import hugectr_amd as ha
    h = _h()

    def no_device(*a, **k):
        raise AssertionError("a device call")
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    tables = [h.EmbeddingTableConfig("t0", 100, 16, _opt("SGD")),
              h.EmbeddingTableConfig("t1", 100, 16, _opt("AdaGrad"))]
    for cls in (lambda c: ha.EmbeddingCollection.for_rank(0, 1, c, 8),
                lambda c: h.DataParallelCollection(c, 8, rank=0, world=1)):
        with pytest.raises(RuntimeError, match=r"t0.*t1.*does not support grouping embedding table "
                           r"with different optimizer.*hugectr.Model"):
            cls(_config(tables))
    # tables that agree replace the argument: Adam is then refused for the static table
    both = [h.EmbeddingTableConfig(f"t{i}", 100, 16, _opt("Adam")) for i in range(2)]
    with pytest.raises(RuntimeError, match="static tables support SGD, AdaGrad and Ftrl"):
        ha.EmbeddingCollection.for_rank(0, 1, _config(both), 8)


# ---- 3. InitParams -----------------------------------------------------------------------------------
def _sinusoid(rows, ev):
    r = np.arange(rows, dtype=np.float64)[:, None]
    c = np.arange(ev)[None, :]
    f = np.exp(-(c - c % 2) * np.log(10000.0) / ev)
    return np.where(c % 2 == 0, np.sin(r * f), np.cos(r * f)).astype(np.float32)


def test_init_params_checks_and_the_sinusoidal_table():
    h = _h()
    from hugectr_amd.embedding_collection import check_init_param, sinusoidal_table
    I = h.Initializer_t
    with pytest.raises(RuntimeError, match="uniform should specify up_bound"):
        h.InitParams(16, I.Uniform)
    with pytest.raises(RuntimeError, match="up_bound"):
        h.InitParams(16, I.Uniform, up_bound=0.0)
    with pytest.raises(RuntimeError, match="should specify max_sequence_len"):
        h.InitParams(16, I.Sinusoidal)
    d = h.InitParams(16)
    assert d.initializer_type == I.Default and d.up_bound == 0 and d.max_sequence_len == 0
    u = h.InitParams(16, I.Uniform, up_bound=0.25)
    assert u.up_bound == 0.25 and u.max_sequence_len == 0
    s = h.InitParams(6, I.Sinusoidal, max_sequence_len=7)
    assert (s.ev_size, s.max_sequence_len) == (6, 7)
    # size mismatch: max_sequence_len * ev_size is not the table's element count
    with pytest.raises(RuntimeError, match=r"'pos'.*7 x ev_size 6.*8 x 6"):
        check_init_param(h.EmbeddingTableConfig("pos", 8, 6, None, s))
    assert check_init_param(h.EmbeddingTableConfig("pos", 7, 6, None, s)) == "sinusoidal"
    assert check_init_param(h.EmbeddingTableConfig("pos", 21, 2, None, s)) == "sinusoidal"
    assert check_init_param(h.EmbeddingTableConfig("u", 9, 16, None, u)) == "uniform"
    assert check_init_param(h.EmbeddingTableConfig("d", 9, 16, None, d)) == "default"
    assert check_init_param(h.EmbeddingTableConfig("n", 9, 16)) == "default"
    with pytest.raises(RuntimeError, match=r"'x'.*XavierUniform.*not available"):
        check_init_param(h.EmbeddingTableConfig("x", 9, 16, None, h.InitParams(16, I.XavierUniform)))
    # bit for bit the fp64 formula rounded once
    got = sinusoidal_table(7, 6)
    want = _sinusoid(7, 6)
    assert got.dtype == np.float32 and got.shape == (7, 6)
    assert got.tobytes() == want.tobytes()
    assert (got[0] == np.array([0, 1, 0, 1, 0, 1], np.float32)).all()
    assert got[3, 0] == np.float32(np.sin(3.0)) and got[3, 1] == np.float32(np.cos(3.0))


def test_init_param_on_a_dynamic_or_hybrid_table_is_refused_by_the_validation():
    h = _h()
    u = h.InitParams(16, h.Initializer_t.Uniform, up_bound=0.5)
    check = h.check_embedding_collection_config
    with pytest.raises(RuntimeError, match=r"'dy'.*Uniform.*static tables"):
        check(_config([h.EmbeddingTableConfig("dy", -1, 16, None, u)]), _opt("SGD"))
    with pytest.raises(RuntimeError, match=r"'hy'.*Uniform.*static tables"):
        check(_config([h.EmbeddingTableConfig("hy", -1, 16, None, u, var_type="hybrid",
                                              max_capacity=256)]), _opt("SGD"))
    # a static table beside a dynamic one lives in the dynamic table: refused too, not dropped
    with pytest.raises(RuntimeError, match=r"'st'.*Uniform.*dynamic storage"):
        check(_config([h.EmbeddingTableConfig("st", 50, 16, None, u),
                       h.EmbeddingTableConfig("dy", -1, 16)]), _opt("SGD"))
    check(_config([h.EmbeddingTableConfig("st", 50, 16, None, u)]), _opt("SGD"))
    check(_config([h.EmbeddingTableConfig("dy", -1, 16, None, h.InitParams(16))]), _opt("SGD"))


# ---- 4. embedding_io.create_collection ---------------------------------------------------------------
def _head(path):
    with open(path, "rb") as f:
        return struct.unpack("<4i", f.read(16))


def test_create_collection_writes_each_table_s_optimizer_head(tmp_path):
    from hugectr_amd import embedding_io as eio
    h = _h()
    O = h.Optimizer_t
    meta = eio.MetaData([0, 1, 2], {0: 5, 1: 7, 2: 3}, {0: 16, 1: 16, 2: 16})
    per_table = {0: (2, int(O.Ftrl)), 1: (0, int(O.SGD)), 2: (1, int(O.AdaGrad))}
    d = eio.create_collection(str(tmp_path / "mixed"), 0, meta, per_table)
    for i, (ns, opt) in per_table.items():
        fn = os.path.join(d, f"opt_state{i}")
        assert _head(fn) == (eio.KIND_OPT, i, ns, opt)
        assert os.path.getsize(fn) == eio.FILE_HEAD_NBYTES + ns * meta.key_nums[i] * 16 * 4
        with eio.TableFiles(str(tmp_path / "mixed"), 0, i) as f:
            assert f.opt_state == (ns, opt)
    # a dump of some tables: ids are not file positions
    part = eio.MetaData([1, 2], {1: 7, 2: 3}, {1: 16, 2: 16})
    d = eio.create_collection(str(tmp_path / "part"), 0, part, per_table)
    assert _head(os.path.join(d, "opt_state0")) == (eio.KIND_OPT, 0, 0, int(O.SGD))
    assert _head(os.path.join(d, "opt_state1")) == (eio.KIND_OPT, 1, 1, int(O.AdaGrad))
    with pytest.raises(eio.EmbeddingIOError, match="table id 2"):
        eio.create_collection(str(tmp_path / "bad"), 0, meta, {0: (1, 3), 1: (1, 3)})


def test_one_optimizer_for_all_tables_is_byte_identical_to_the_tuple_form(tmp_path):
    from hugectr_amd import embedding_io as eio
    meta = eio.MetaData([0, 2, 5], {0: 5, 2: 0, 5: 11}, {0: 16, 2: 8, 5: 16}, np.dtype("<u4"))
    a = eio.create_collection(str(tmp_path / "tuple"), 1, meta, (2, 0))
    b = eio.create_collection(str(tmp_path / "mapping"), 1, meta, {t: (2, 0) for t in (0, 2, 5)})
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == 1 + 3 * 3
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert sorted(match) == names and not mismatch and not errors
    # and no state files at all without the argument, as before
    c = eio.create_collection(str(tmp_path / "none"), 1, meta)
    assert not [n for n in os.listdir(c) if n.startswith("opt_state")]


def test_readme_example_runs_as_written():
    """the Adam-dense plus AdaGrad-tables example of README, against the public surface"""
    import re
    h = _h()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "README.md")) as f:
        blocks = re.findall(r"```python\n(.*?)```", f.read(), flags=re.S)
    snippet, = [b for b in blocks if "opt_params=" in b]
    made = []

    def fake_model(solver, reader, opt):
        made.append(opt)
        return types.SimpleNamespace(add=made.append)
    surface = types.SimpleNamespace(**{k: v for k, v in vars(h).items() if not k.startswith("_")})
    surface.Model = fake_model
    exec(snippet, dict(hugectr=surface, solver=None, reader=None, vocab=[100 + i for i in range(26)]))
    model_opt, cfg = made
    assert model_opt.optimizer_type == h.Optimizer_t.Adam and cfg.top_name == "sparse_embedding"
    h.check_embedding_collection_config(cfg, model_opt)      # Adam on the model, static tables: fine
    (sub, ids), = _split(cfg, model_opt)
    assert sub is cfg and len(ids) == 26
    from hugectr_amd.embedding_collection import resolve_table_optimizer
    o, src = resolve_table_optimizer(cfg.lookups[3][0], model_opt)
    assert src == "table" and o.optimizer_type == h.Optimizer_t.AdaGrad and o.initial_accu_value == 0.1
