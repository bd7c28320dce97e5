"""GPU: hybrid embedding tables through the public hugectr.Model API -- EmbeddingTableConfig(...,
var_type="hybrid", max_capacity=...) in an EmbeddingCollectionConfig, Model.add / compile / train /
eval, embedding_dump / embedding_load, HIP-graph replay of the dense tower around the collection."""
import os

import numpy as np
import pytest
import torch

from test_model_gpu import SIZES, _gen

pytestmark = pytest.mark.gpu

BATCH, EV, STEPS = 64, 8, 6
SLOTS = [0, 1, 2]        # the three lookups read data0 .. data2 (C1 carries the label)
EMU = os.environ.get("HCTR_EMU") == "1"


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import hugectr_amd.hugectr as hugectr
    folder = tmp_path_factory.mktemp("hybrid_model")
    return _gen(folder, hugectr, n_train=1024, n_eval=128)


def _tables(hugectr, kinds, budget=None, max_capacity=512):
    out = []
    for i, kind in zip(SLOTS, kinds):
        if kind == "hybrid":
            kw = dict(var_type="hybrid", max_capacity=max_capacity, max_bucket_size=64)
            if budget is not None:
                kw["max_hbm_for_vectors"] = budget
            out.append(hugectr.EmbeddingTableConfig(f"t{i}", -1, EV, **kw))
        else:
            out.append(hugectr.EmbeddingTableConfig(f"t{i}", -1 if kind == "dynamic" else SIZES[i],
                                                    EV))
    return out


def _model(hugectr, p, kinds=("hybrid",) * 3, budget=None, graph=True, opt="SGD",
           max_capacity=512):
    """a small WDL-style model: three deep lookups -> MLP, plus a dense tower, one BCE loss"""
    torch.manual_seed(5)
    solver = hugectr.CreateSolver(batchsize=BATCH, batchsize_eval=BATCH, lr=0.05, vvgpu=[[0]],
                                  i64_input_key=True, max_eval_batches=1, seed=11,
                                  use_embedding_collection=True, use_cuda_graph=graph)
    reader = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet,
                                      source=[p.source], eval_source=p.eval_source,
                                      slot_size_array=SIZES, check_type=hugectr.Check_t.Non)
    optimizer = hugectr.CreateOptimizer(optimizer_type=getattr(hugectr.Optimizer_t, opt),
                                        update_type=hugectr.Update_t.Local)
    model = hugectr.Model(solver, reader, optimizer)
    model.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=13, dense_name="dense",
                            data_reader_sparse_param_array=[
                                hugectr.DataReaderSparseParam(f"data{i}", 1, True, 1)
                                for i in range(26)]))
    ebc = hugectr.EmbeddingCollectionConfig()
    tables = _tables(hugectr, kinds, budget, max_capacity)
    for i, t in zip(SLOTS, tables):
        ebc.embedding_lookup(table_config=t, bottom_name=f"data{i}", top_name=f"deep{i}",
                             combiner="sum")
    names = [t.name for t in tables]
    ebc.shard(shard_matrix=[names], shard_strategy=[("mp", names)])
    model.add(ebc)
    D, T, A = hugectr.DenseLayer, hugectr.Layer_t, hugectr.Activation_t
    model.add(D(layer_type=T.Concat, bottom_names=[f"deep{i}" for i in SLOTS], top_names=["emb"]))
    model.add(D(layer_type=T.MLP, bottom_names=["emb"], top_names=["deep"], num_outputs=[16, 1],
                activations=[A.Relu, A.Non]))
    model.add(D(layer_type=T.MLP, bottom_names=["dense"], top_names=["wide"], num_outputs=[1],
                activations=[A.Non]))
    model.add(D(layer_type=T.Add, bottom_names=["deep", "wide"], top_names=["logit"]))
    model.add(D(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["logit", "label"],
                top_names=["loss"]))
    model.compile()
    return model


def _train(model, steps=STEPS):
    losses = []
    for _ in range(steps):
        assert model.train()
        losses.append(model.get_current_loss())
    return np.array(losses, np.float64)


def _hybrid_tables(model):
    """{table name: HybridTable} of the model's hybrid collections"""
    out = {}
    for rt in model._ebc:
        e = rt["train"]
        if getattr(e, "hybrid", False):
            for t, tab in e.hyb.items():
                out[e.tables[t].name] = tab
    return out


def _contents(tab, n_state=0):
    """(keys, rows, states) sorted by key"""
    k, rows, slots, _ = tab.export(with_slots=True)
    o = torch.argsort(k)
    st = [tab.gather_slots(1 + j, slots)[o].cpu().numpy() for j in range(n_state)]
    return k[o].cpu().numpy(), rows[o].cpu().numpy(), st


@pytest.fixture(scope="module")
def base_losses(data):
    """the per-step loss of the base model (hybrid tables, untiered, graph on): the reference of
    the comparisons below, computed once"""
    import hugectr_amd.hugectr as hugectr
    m = _model(hugectr, data)
    losses = _train(m)
    assert all(rt["train"].hybrid for rt in m._ebc)
    if not EMU:  # (the host interpreter has no graphs)
        assert m._graph is not None
    assert np.isfinite(losses).all()
    stats = m._ebc[0]["train"].table_stats()
    assert set(stats) == {"t0", "t1", "t2"} and all(s["size"] > 0 for s in stats.values())
    return losses


@pytest.mark.parametrize("hbm_slots", [256, 0])
def test_tiered_model_trains_bit_equal(data, base_losses, hbm_slots):
    import hugectr_amd.hugectr as hugectr
    m = _model(hugectr, data, budget=hbm_slots * EV * 4 / 2**30)
    assert all(t.tiered and t.hbm_slots == hbm_slots for t in _hybrid_tables(m).values())
    assert np.array_equal(_train(m), base_losses)


def test_hip_graph_on_and_off(data, base_losses):
    """the collection's forward and update stay eager launches around the replayed dense tower:
    the same losses with and without the graph (fp32, SGD: to the rounding of the library's GEMM
    choice, the bound of test_hip_graph_replay_trains_like_eager_launches)"""
    import hugectr_amd.hugectr as hugectr
    from numpy.testing import assert_allclose
    m = _model(hugectr, data, graph=False)
    losses = _train(m)
    assert m._graph is None
    assert_allclose(losses, base_losses, rtol=2e-5)


def test_hybrid_and_dynamic_models_agree_from_one_checkpoint(data, tmp_path):
    """the same checkpoint (every key of the three slots, so that no lookup meets an initializer)
    loaded into a hybrid model and a dynamic model: the loss curves agree within 1e-3 relative"""
    import hugectr_amd.hugectr as hugectr
    from numpy.testing import assert_allclose
    src = _model(hugectr, data)
    for name, tab in _hybrid_tables(src).items():
        every = torch.arange(SIZES[int(name[1:])], dtype=torch.int64, device="cuda")
        tab.lookup_index(every, insert=True)
    path = str(tmp_path / "ckpt")
    src.embedding_dump(path)
    hyb, dyn = _model(hugectr, data), _model(hugectr, data, kinds=("dynamic",) * 3)
    hyb.embedding_load(path)
    dyn.embedding_load(path)
    assert not getattr(dyn._ebc[0]["train"], "hybrid", False) and dyn._ebc[0]["train"].dynamic
    for name, tab in _hybrid_tables(hyb).items():
        assert tab.size() == SIZES[int(name[1:])] and tab.rejected_count() == 0
    a, b = _train(hyb), _train(dyn)
    assert_allclose(a, b, rtol=1e-3)


def test_mixed_static_dynamic_hybrid_config_trains_and_evaluates(data):
    import hugectr_amd.hugectr as hugectr
    m = _model(hugectr, data, kinds=("static", "dynamic", "hybrid"), opt="AdaGrad")
    kinds = sorted(("hybrid" if rt["train"].hybrid else "dynamic" if rt["train"].dynamic
                    else "static", [t.name for t in rt["train"].tables]) for rt in m._ebc)
    assert kinds == [("dynamic", ["t0", "t1"]), ("hybrid", ["t2"])]   # t2 did not turn the others hybrid
    losses = _train(m)
    assert np.isfinite(losses).all()
    size = _hybrid_tables(m)["t2"].size()
    assert size > 0
    m._eval_buf = []
    assert m.eval()
    metrics = dict(m.get_eval_metrics())
    assert set(metrics) == {"AUC", "AverageLoss"}
    assert 0.0 <= metrics["AUC"] <= 1.0 and np.isfinite(metrics["AverageLoss"])
    assert _hybrid_tables(m)["t2"].size() == size          # evaluation never inserts
    rt = [rt for rt in m._ebc if rt["train"].hybrid][0]
    assert rt["eval"] is not rt["train"] and not rt["eval"].training
    assert rt["eval"].hyb is rt["train"].hyb               # the evaluation runtime shares the tables


def test_dump_with_optimizer_states_and_resume(data, tmp_path):
    """embedding_dump(optimizer_states=True) -> embedding_load into a fresh model: (key -> row,
    state) equal, and the next step's loss is bit-equal to the uninterrupted run's"""
    import hugectr_amd.hugectr as hugectr
    a = _model(hugectr, data, opt="AdaGrad", graph=False)
    _train(a, 3)
    path = str(tmp_path / "ckpt")
    a.embedding_dump(path, optimizer_states=True)
    assert os.path.exists(os.path.join(path, "embedding_collection_0", "opt_state0"))
    b = _model(hugectr, data, opt="AdaGrad", graph=False)
    _train(b, 3)            # same data position and dense weights; tables wiped below
    for tab in _hybrid_tables(b).values():
        k, _, slots, _ = tab.export(with_slots=True)
        tab.scatter_slots(0, slots, torch.zeros((k.numel(), EV), device="cuda"))
        tab.scatter_slots(1, slots, torch.zeros((k.numel(), EV), device="cuda"))
    b.embedding_load(path)
    ta, tb = _hybrid_tables(a), _hybrid_tables(b)
    for name in ta:
        ka, ra, sa = _contents(ta[name], 1)
        kb, rb, sb = _contents(tb[name], 1)
        assert np.array_equal(ka, kb) and np.array_equal(ra, rb) and np.array_equal(sa[0], sb[0])
        assert np.abs(sa[0]).sum() > 0
    assert a.train() and b.train()
    assert a.get_current_loss() == b.get_current_loss()


def _rank_shards(world, opt, budget=None, max_capacity=256):
    import hugectr_amd as ha
    tcfg = [ha.EmbeddingTableConfig(f"t{i}", -1, EV, var_type="hybrid", max_capacity=max_capacity,
                                    max_bucket_size=64,
                                    **({} if budget is None else dict(max_hbm_for_vectors=budget)))
            for i in range(2)]
    cfg = ha.EmbeddingCollectionConfig()
    for l, t in enumerate([0, 1, 0]):
        cfg.embedding_lookup(tcfg[t], f"in{l}", f"out{l}", "sum")
    # table 0 row-sharded over every rank, table 1 on the last rank
    cfg.shard([[1, 1 if g == world - 1 else 0] for g in range(world)])
    return [ha.EmbeddingCollection.for_rank(r, world, cfg, 16, lr=0.1, optimizer=opt, max_hotness=2,
                                            seed=4) for r in range(world)]


def test_two_rank_dump_loads_into_one_rank(tmp_path):
    """files written from a 2-rank sharding (for_rank + ebc_io.dump_shards; one shard tiered) load
    into a 1-rank collection, and back, with equal (key -> row, state)"""
    from hugectr_amd import _lib, ebc_io
    from test_ebc_hybrid_gpu import _step
    two = _rank_shards(2, _lib.OPT_ADAM, budget=64 * EV * 4 / 2**30)
    rng = np.random.default_rng(8)
    for it in range(2):
        lens = rng.integers(0, 3, size=3 * 16).astype(np.int64)
        br = np.zeros(3 * 16 + 1, np.int64)
        np.cumsum(lens, out=br[1:])
        keys = rng.integers(0, 60, size=int(br[-1])).astype(np.int64)
        grads = [rng.standard_normal((3, 8, EV)).astype(np.float32) for _ in range(2)]
        _step(two, keys, br, grads)

    def merged(shards):
        out = {}
        for t in range(2):
            entry = {}
            for e in shards:
                if t in e.hyb:
                    k, r, s = _contents(e.hyb[t], 2)
                    for i, key in enumerate(k.tolist()):
                        assert key not in entry
                        entry[key] = (r[i].tobytes(), s[0][i].tobytes(), s[1][i].tobytes())
            out[t] = entry
        return out
    want = merged(two)
    assert all(len(v) > 5 for v in want.values())
    p2 = str(tmp_path / "from2")
    ebc_io.dump_shards(p2, 0, two, optimizer_states=True, chunk_rows=16)
    one = _rank_shards(1, _lib.OPT_ADAM)
    ebc_io.load_shard(p2, 0, one[0], chunk_rows=16)
    assert merged(one) == want
    p1 = str(tmp_path / "from1")
    ebc_io.dump_shards(p1, 0, one, optimizer_states=True, chunk_rows=16)
    again = _rank_shards(2, _lib.OPT_ADAM)
    for e in again:
        ebc_io.load_shard(p1, 0, e, chunk_rows=16)
    assert merged(again) == want
    for e in again:   # every shard holds its own keys only
        for t, tab in e.hyb.items():
            ns, sid = len(e.owners[t]), e.owners[t].index(e.rank)
            assert (tab.export()[0] % ns == sid).all()


def test_a_load_above_max_capacity_is_refused(tmp_path):
    from hugectr_amd import _lib, ebc_io
    big = _rank_shards(1, _lib.OPT_SGD, max_capacity=256)
    big[0].hyb[0].lookup_index(torch.arange(100, dtype=torch.int64, device="cuda"), insert=True)
    big[0].hyb[1].lookup_index(torch.arange(10, dtype=torch.int64, device="cuda"), insert=True)
    path = str(tmp_path / "big")
    ebc_io.dump_shards(path, 0, big)
    small = _rank_shards(1, _lib.OPT_SGD, max_capacity=64)
    small[0].hyb[1].lookup_index(torch.arange(500, 505, dtype=torch.int64, device="cuda"),
                                 insert=True)
    before = [[x.clone() for x in small[0].hyb[t].export(with_slots=True)] for t in range(2)]
    with pytest.raises(_lib.HugeCTRAmdError, match=r"100 of 100 keys.*'t0'.*max_capacity is 64"):
        ebc_io.load_shard(path, 0, small[0])
    for t in range(2):   # table 1 would have fitted: it was not written either
        for x, y in zip(before[t], small[0].hyb[t].export(with_slots=True)):
            assert torch.equal(x, y)
    # two ranks of 64 slots each hold 50 keys each: the same files load
    pair = _rank_shards(2, _lib.OPT_SGD, max_capacity=64)
    for e in pair:
        ebc_io.load_shard(path, 0, e)
    assert [e.hyb[0].size() for e in pair] == [50, 50]


def test_a_load_that_loses_keys_inside_max_capacity_is_reported(tmp_path):
    """70 keys of ONE bucket of a 128-slot table (two buckets of 64): the shard's key count is within
    max_capacity, but six keys find no room -- the load says so instead of passing"""
    from lru_oracle import LruTable
    from hugectr_amd import _lib, ebc_io
    probe = LruTable(128, EV, "", 64)
    one_bucket = np.array([k for k in range(4000) if probe.bucket(k) == 1][:70], np.int64)
    big = _rank_shards(1, _lib.OPT_SGD, max_capacity=1024)
    big[0].hyb[0].lookup_index(torch.from_numpy(one_bucket).cuda(), insert=True)
    big[0].hyb[1].lookup_index(torch.arange(10, dtype=torch.int64, device="cuda"), insert=True)
    assert big[0].hyb[0].size() == 70
    path = str(tmp_path / "one_bucket")
    ebc_io.dump_shards(path, 0, big)
    small = _rank_shards(1, _lib.OPT_SGD, max_capacity=128)
    with pytest.raises(_lib.HugeCTRAmdError, match=r"6 of 70 keys.*did not stay.*'t0'"):
        ebc_io.load_shard(path, 0, small[0])
    assert small[0].hyb[0].size() == 64 and small[0].hyb[0].rejected_count() == 6


def test_save_params_to_files_writes_the_hybrid_tables(data, tmp_path):
    import hugectr_amd.hugectr as hugectr
    m = _model(hugectr, data, graph=False)
    _train(m, 2)
    prefix = str(tmp_path / "wdl")
    m.save_params_to_files(prefix, 2)
    d = f"{prefix}_ebc0_sparse_2.model"
    e = m._ebc[0]["train"]
    for t, tab in e.hyb.items():
        k, v = tab.export()
        assert np.array_equal(np.fromfile(os.path.join(d, f"key.table{t}.rank0"), "<i8"),
                              k.cpu().numpy())
        assert np.array_equal(np.fromfile(os.path.join(d, f"emb_vector.table{t}.rank0"), "<f4"),
                              v.cpu().numpy().reshape(-1))
        assert k.numel() > 0
