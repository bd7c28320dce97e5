"""GPU: EmbeddingTableConfig(opt_params=..., init_param=...) through hugectr.Model -- a config whose
tables carry optimizers of their own runs as one collection per optimizer and computes, bit for
bit, what the same tables compute as separate configs (same kernels, same inputs, same order);
per-table optimizer state in embedding_dump / embedding_load; Uniform and Sinusoidal first values."""
import glob
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCH, EV = 64, 16
SIZES = [120, 200, 50, 12]     # keys of data0 .. data3
HOT = [1, 3, 1, 1]             # data1 is the multi-hot input
ADA = dict(initial_accu_value=0.5, epsilon=1e-2)
FTRL = dict(beta=0.5, lambda1=0.01, lambda2=0.02)


def _gen(folder, hugectr, n_train=512, n_eval=128):
    import pyarrow as pa
    import pyarrow.parquet as pq
    p = hugectr.tools.DataGeneratorParams(
        format=hugectr.DataReaderType_t.Parquet, label_dim=1, dense_dim=4, num_slot=len(SIZES),
        i64_input_key=True, source=str(folder / "train" / "_file_list.txt"),
        eval_source=str(folder / "val" / "_file_list.txt"), slot_size_array=SIZES, nnz_array=HOT,
        dist_type=hugectr.Distribution_t.PowerLaw, power_law_type=hugectr.PowerLaw_t.Short,
        num_files=2, eval_num_files=1, num_samples_per_file=n_train // 2, num_samples=n_train,
        eval_num_samples=n_eval)
    hugectr.tools.DataGenerator(p).generate()
    for f in glob.glob(str(folder / "*" / "*.parquet")):   # a learnable label: parity of C1
        t = pq.read_table(f)
        lab = (t["C1"].to_numpy() % 2).astype(np.float32)
        t = t.set_column(t.schema.get_field_index("label"), "label", pa.array(lab, type=pa.float32()))
        pq.write_table(t, f)
    return p


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import hugectr_amd.hugectr as hugectr
    return _gen(tmp_path_factory.mktemp("table_opt"), hugectr)


def _opt(name, **kw):
    import hugectr_amd.hugectr as hugectr
    return hugectr.CreateOptimizer(optimizer_type=getattr(hugectr.Optimizer_t, name), **kw)


def _model(p, model_opt, lookups, layout="one", form="named", dp=(), frozen=False, world=1,
           compile=True):
    """lookups: [(EmbeddingTableConfig, input slot)].  layout "one": one config holds them all;
    "each": one config per table.  form "named": a top per lookup, concatenated by a Concat layer;
    "list": the list form, `top_name` given once -> [batch, lookups, ev].  Then a small WDL tower."""
    import hugectr_amd.hugectr as hugectr
    solver = hugectr.CreateSolver(batchsize=BATCH, batchsize_eval=BATCH, lr=0.05,
                                  vvgpu=[list(range(world))], i64_input_key=True,
                                  max_eval_batches=1, seed=7, use_embedding_collection=True)
    reader = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet,
                                      source=[p.source], eval_source=p.eval_source,
                                      slot_size_array=SIZES, check_type=hugectr.Check_t.Non)
    model = hugectr.Model(solver, reader, model_opt)
    model.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=4, dense_name="dense",
                            data_reader_sparse_param_array=[
                                hugectr.DataReaderSparseParam(f"data{i}", HOT[i], True, 1)
                                for i in range(len(SIZES))]))
    tables = []
    for t, _ in lookups:
        if not any(t is x for x in tables):
            tables.append(t)
    groups = [list(range(len(lookups)))] if layout == "one" else \
        [[l for l, (t, _) in enumerate(lookups) if t is x] for x in tables]
    for ids in groups:
        ebc = hugectr.EmbeddingCollectionConfig()
        if form == "list":
            ebc.embedding_lookup([lookups[l][0] for l in ids], [f"data{lookups[l][1]}" for l in ids],
                                 "emb", ["sum"] * len(ids))
        else:
            for l in ids:
                ebc.embedding_lookup(lookups[l][0], f"data{lookups[l][1]}", f"e{l}", "sum")
        names = [x.name for x in tables if any(lookups[l][0] is x for l in ids)]
        if any(n in dp for n in names):
            ebc.shard([names] * world, [("mp", [n for n in names if n not in dp]),
                                        ("dp", [n for n in names if n in dp])])
        model.add(ebc)
    D, T, A = hugectr.DenseLayer, hugectr.Layer_t, hugectr.Activation_t
    if form != "list":
        model.add(D(layer_type=T.Concat, bottom_names=[f"e{l}" for l in range(len(lookups))],
                    top_names=["emb"]))
    model.add(D(layer_type=T.MLP, bottom_names=["emb"], top_names=["deep"], num_outputs=[16, 1],
                activations=[A.Relu, A.Non]))
    model.add(D(layer_type=T.MLP, bottom_names=["dense"], top_names=["wide"], num_outputs=[1],
                activations=[A.Non]))
    model.add(D(layer_type=T.Add, bottom_names=["deep", "wide"], top_names=["logit"]))
    model.add(D(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["logit", "label"],
                top_names=["loss"]))
    if compile:
        model.compile()
        if frozen:
            model.freeze_dense()
    return model


def _train(model, steps):
    losses = []
    for _ in range(steps):
        assert model.train()
        losses.append(model.get_current_loss())
    return losses


def _rows(model):
    """{table name: (keys, rows)} of every table, keys ascending (one rank)"""
    from hugectr_amd.embedding_collection import DataParallelCollection
    out = {}
    for rt in model._ebc:
        e = rt["train"]
        for k, t in enumerate(e.tables):
            if isinstance(e, DataParallelCollection) or not (e.dynamic or e.hybrid):
                s0, n = e.row_start_of_table[k], t.max_vocabulary_size
                keys, rows = torch.arange(n), e.table[s0:s0 + n]
            elif e.hybrid:
                keys, rows = e.hyb[k].export()
            else:
                keys, rows = e.det.export(e.class_of_table[k])
            o = torch.argsort(keys.cpu())
            assert t.name not in out
            out[t.name] = (keys.cpu()[o].numpy(), rows.detach().cpu()[o].numpy().copy())
    return out


def _same_rows(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name][0], b[name][0]), name
        assert a[name][1].tobytes() == b[name][1].tobytes(), name


def _static(name, slot, opt=None, init=None):
    import hugectr_amd.hugectr as hugectr
    return hugectr.EmbeddingTableConfig(name, SIZES[slot], EV, opt, init)


# ---- 5. tables on AdaGrad under a model on Adam (compile() raised before opt_params was read) -------
def test_static_tables_on_adagrad_under_a_model_on_adam(data):
    import hugectr_amd.hugectr as hugectr

    def run(model_opt, table_opt):
        t0, t1 = _static("t0", 0, table_opt), _static("t1", 1, table_opt)
        m = _model(data, model_opt, [(t0, 0), (t1, 1)], frozen=True)
        assert len(m._ebc) == 1           # one optimizer, one runtime collection
        e = m._ebc[0]["train"]
        assert e.optimizer == int(hugectr.Optimizer_t.AdaGrad)
        losses = _train(m, 3)
        return losses, _rows(m)
    # the model on CreateOptimizer() (Adam), which no static table runs: the tables' own AdaGrad
    new = run(hugectr.CreateOptimizer(), _opt("AdaGrad", **ADA))
    old = run(_opt("AdaGrad", **ADA), None)             # the same, written the old way
    assert new[0] == old[0]
    _same_rows(new[1], old[1])
    assert np.isfinite(new[0]).all()
    # the hyper-parameters reach the kernel, not only the type
    default = run(hugectr.CreateOptimizer(), _opt("AdaGrad"))
    assert default[0][0] == new[0][0]                   # (the same first values and batch)
    assert default[0][1:] != new[0][1:]
    assert any(default[1][n][1].tobytes() != new[1][n][1].tobytes() for n in new[1])


# ---- 6. / 8. a mixed config equals separate configs; checkpoint --------------------------------------
def _mixed_lookups():
    """{t0: Ftrl, t1: SGD, t2: follows the model}; t0 is read twice, so that its group's columns
    are not adjacent in the output"""
    t0, t1, t2 = _static("t0", 0, _opt("Ftrl", **FTRL)), _static("t1", 1, _opt("SGD")), _static("t2", 2)
    return [(t0, 0), (t1, 1), (t2, 2), (t0, 3)]


def _run_mixed(data, layout, folder=None):
    """4 steps, the learning rate changed after step 2; layout "one" also writes, after step 2,
    the embedding dump with optimizer states and the dense files into `folder`"""
    m = _model(data, _opt("AdaGrad", **ADA), _mixed_lookups(), layout=layout)
    losses = _train(m, 2)
    m.set_learning_rate(0.02)
    if folder is not None:
        m.embedding_dump(os.path.join(folder, "emb"), [], optimizer_states=True)
        m.save_params_to_files(os.path.join(folder, "ck"), 2)
    losses += _train(m, 2)
    assert m.eval()
    return dict(model=m, losses=losses, rows=_rows(m), metrics=list(m.get_eval_metrics()))


@pytest.fixture(scope="module")
def mixed(data, tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("mixed_ckpt"))
    out = _run_mixed(data, "one", folder)
    out["folder"] = folder
    m = out.pop("model")
    out["collections"] = [(int(rt["train"].optimizer), rt["ids"]) for rt in m._ebc]
    return out


def test_a_mixed_config_equals_separate_configs(data, mixed):
    import hugectr_amd.hugectr as hugectr
    O = hugectr.Optimizer_t
    # three optimizers -> three runtime collections, in the order of their first lookup
    assert mixed["collections"] == [(int(O.Ftrl), [0, 3]), (int(O.SGD), [1]), (int(O.AdaGrad), [2])]
    sep = _run_mixed(data, "each")
    assert len(sep["model"]._ebc) == 3 and all(rt["whole"] for rt in sep["model"]._ebc)
    assert mixed["losses"] == sep["losses"]
    assert np.isfinite(mixed["losses"]).all() and len(set(mixed["losses"])) == 4
    _same_rows(mixed["rows"], sep["rows"])
    assert mixed["metrics"] == sep["metrics"]
    assert [n for n, _ in mixed["metrics"]] == ["AUC", "AverageLoss"]


def test_tables_without_opt_params_build_one_collection_as_before(data):
    """the unchanged default path: no opt_params anywhere -> one runtime collection per config
    (one vector size, one placement, one kind), the config object itself"""
    lookups = [(_static("t0", 0), 0), (_static("t1", 1), 1), (_static("t2", 2), 2)]
    m = _model(data, _opt("AdaGrad"), lookups)
    assert len(m._ebc) == 1 and m._ebc[0]["whole"] and m._ebc[0]["cfg"] is m.ebc_configs[0]
    assert m._ebc_stacked == {}
    # ... and opt_params that say what the model says split nothing either
    lookups = [(_static("t0", 0, _opt("AdaGrad")), 0), (_static("t1", 1), 1)]
    m = _model(data, _opt("AdaGrad"), lookups)
    assert len(m._ebc) == 1 and m._ebc[0]["whole"]


def test_the_list_form_keeps_its_columns_in_lookup_order(data):
    """top_name given once: [batch, lookups, ev] with lookup l in column l, although the lookups
    of t0 (columns 0 and 3) run in one collection and the others in two more"""
    def first_output(m, names):
        seen = []
        inner = m._forward_dense

        def spy(tensors, train, head=None):
            if not seen:
                seen.append([tensors[n].detach().clone() for n in names])
            return inner(tensors, train, head)
        m._forward_dense = spy
        assert m.train()
        return seen[0]
    one = _model(data, _opt("AdaGrad", **ADA), _mixed_lookups(), form="list")
    assert len(one._ebc) == 3 and one._shapes["emb"] == (4, EV)
    got, = first_output(one, ["emb"])
    sep = _model(data, _opt("AdaGrad", **ADA), _mixed_lookups(), layout="each")
    want = torch.stack(first_output(sep, [f"e{l}" for l in range(4)]), dim=1)
    assert got.shape == (BATCH, 4, EV) and got.dtype == want.dtype
    assert torch.equal(got, want)
    assert len({want[:, l].cpu().numpy().tobytes() for l in range(4)}) == 4
    assert one.get_current_loss() == sep.get_current_loss()


def _heads(folder, n):
    out = []
    for i in range(n):
        with open(os.path.join(folder, "emb", "embedding_collection_0", f"opt_state{i}"), "rb") as f:
            out.append(struct.unpack("<4i", f.read(16)))
    return out


def test_checkpoint_carries_each_table_s_optimizer_state(data, mixed):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    O = hugectr.Optimizer_t
    folder = mixed["folder"]
    # head: (kind 3, file index, state arrays, Optimizer_t)
    assert _heads(folder, 3) == [(3, 0, 2, int(O.Ftrl)), (3, 1, 0, int(O.SGD)),
                                 (3, 2, 1, int(O.AdaGrad))]
    d = os.path.join(folder, "emb", "embedding_collection_0")
    assert os.path.getsize(os.path.join(d, "opt_state0")) == 128 + 2 * SIZES[0] * EV * 4
    assert os.path.getsize(os.path.join(d, "opt_state1")) == 128
    # a fresh model at the data position of step 3: tables, their states and the dense part loaded
    m = _model(data, _opt("AdaGrad", **ADA), _mixed_lookups())
    for _ in range(2):
        assert m.reader.next_batch(train=True) is not None
    m.embedding_load(os.path.join(folder, "emb"))
    m.load_dense_weights(os.path.join(folder, "ck_dense_2.model"))
    m.load_dense_optimizer_states(os.path.join(folder, "ck_opt_dense_2.model"))
    m.set_learning_rate(0.02)
    assert _train(m, 2) == mixed["losses"][2:]
    _same_rows(_rows(m), mixed["rows"])
    # a model whose t0 runs another optimizer: today's rule for a state file of another optimizer
    # -- refused in the validation, nothing written, no foreign state
    t0, t1, t2 = _static("t0", 0, _opt("AdaGrad")), _static("t1", 1, _opt("SGD")), _static("t2", 2)
    other = _model(data, _opt("AdaGrad", **ADA), [(t0, 0), (t1, 1), (t2, 2), (t0, 3)])
    before = _rows(other)
    accum = [rt["train"].accum.clone() for rt in other._ebc if rt["train"].accum is not None]
    with pytest.raises(_lib.HugeCTRAmdError, match=r"'t0'.*opt_state0 holds 2 arrays of optimizer 0"):
        other.embedding_load(os.path.join(folder, "emb"))
    _same_rows(_rows(other), before)
    now = [rt["train"].accum for rt in other._ebc if rt["train"].accum is not None]
    assert len(accum) == len(now) and all(torch.equal(x, y) for x, y in zip(accum, now))


# ---- 7. dynamic, hybrid and replicated tables -----------------------------------------------------------
def test_dynamic_and_hybrid_tables_with_their_own_optimizers(data):
    import hugectr_amd.hugectr as hugectr

    def lookups():
        dyn = hugectr.EmbeddingTableConfig("dyn", -1, EV, _opt("RMSProp", beta2=0.95, epsilon=1e-4))
        hyb = hugectr.EmbeddingTableConfig("hyb", -1, EV, _opt("Nesterov", momentum_factor=0.8),
                                           var_type="hybrid", max_capacity=512, max_bucket_size=64)
        return [(dyn, 0), (hyb, 1), (_static("st", 2), 2)]
    runs = []
    for layout in ("one", "each"):
        m = _model(data, _opt("SGD"), lookups(), layout=layout)
        kinds = sorted(("hybrid" if rt["train"].hybrid else "dynamic" if rt["train"].dynamic
                        else "static", int(rt["train"].optimizer)) for rt in m._ebc)
        O = hugectr.Optimizer_t
        assert kinds == [("dynamic", int(O.RMSProp)), ("hybrid", int(O.Nesterov)),
                         ("static", int(O.SGD))]
        e = [rt["train"] for rt in m._ebc if rt["train"].hybrid][0]
        assert e.momentum_factor == 0.8 and e.table_stats()["hyb"]["optimizer"] == "Nesterov"
        runs.append((_train(m, 3), _rows(m)))
    assert runs[0][0] == runs[1][0] and np.isfinite(runs[0][0]).all()
    _same_rows(runs[0][1], runs[1][1])
    assert all(len(k) > 0 for k, _ in runs[0][1].values())


def test_a_replicated_table_with_adagrad_opt_params(data):
    from hugectr_amd.embedding_collection import DataParallelCollection

    def run(model_opt, table_opt):
        rep, mp = _static("rep", 2, table_opt), _static("mp", 0, _opt("SGD"))
        m = _model(data, model_opt, [(rep, 2), (mp, 0)], dp=("rep",), frozen=True)
        dp = [rt["train"] for rt in m._ebc if isinstance(rt["train"], DataParallelCollection)]
        assert len(m._ebc) == 2 and len(dp) == 1 and dp[0].accum is not None
        assert float(dp[0].accum[0, 0]) == 0.5 and dp[0].epsilon == 1e-2
        return _train(m, 3), _rows(m)
    new = run(_opt("SGD"), _opt("AdaGrad", **ADA))
    old = run(_opt("AdaGrad", **ADA), None)
    assert new[0] == old[0] and np.isfinite(new[0]).all()
    _same_rows(new[1], old[1])


# ---- 9. init_param -------------------------------------------------------------------------------------
def test_init_param_default_uniform_and_sinusoidal(data):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd.embedding_collection import sinusoidal_table
    I = hugectr.Initializer_t

    def build(with_init):
        init = [hugectr.InitParams(EV), hugectr.InitParams(EV, I.Uniform, up_bound=0.25),
                hugectr.InitParams(EV, I.Sinusoidal, max_sequence_len=SIZES[3])] if with_init \
            else [None] * 3
        t0, t1, t2 = _static("t0", 0, None, init[0]), _static("t1", 1, None, init[1]), \
            _static("t2", 3, None, init[2])
        # t0 is filled LAST: it keeps its bits only if t1 and t2 leave the generator where the
        # default initialiser leaves it
        return _rows(_model(data, _opt("SGD"), [(t1, 1), (t2, 3), (t0, 0)]))
    got, plain = build(True), build(False)
    assert got["t0"][1].tobytes() == plain["t0"][1].tobytes()
    assert np.abs(got["t0"][1]).max() <= (1.0 / SIZES[0]) ** 0.5
    u = got["t1"][1]
    assert u.shape == (SIZES[1], EV) and u.min() >= -0.25 and u.max() <= 0.25
    assert u.max() > 0.2 and u.min() < -0.2 and len(np.unique(u)) > u.size // 2
    assert np.abs(plain["t1"][1]).max() <= (1.0 / SIZES[1]) ** 0.5 < 0.2
    assert build(True)["t1"][1].tobytes() == u.tobytes()          # reproducible under the seed
    r = np.arange(SIZES[3], dtype=np.float64)[:, None]
    c = np.arange(EV)[None, :]
    f = np.exp(-(c - c % 2) * np.log(10000.0) / EV)
    want = np.where(c % 2 == 0, np.sin(r * f), np.cos(r * f)).astype(np.float32)
    assert got["t2"][1].tobytes() == want.tobytes() == sinusoidal_table(SIZES[3], EV).tobytes()


def test_init_param_on_a_dynamic_table_raises_at_compile(data):
    import hugectr_amd.hugectr as hugectr
    u = hugectr.InitParams(EV, hugectr.Initializer_t.Uniform, up_bound=0.25)
    dyn = hugectr.EmbeddingTableConfig("grows", -1, EV, None, u)
    m = _model(data, _opt("SGD"), [(dyn, 0), (_static("st", 2), 2)], compile=False)
    with pytest.raises(RuntimeError, match=r"'grows'.*Uniform"):
        m.compile()
    assert not m._compiled and not hasattr(m, "_ebc")


def test_summary_shows_each_table_s_optimizer(data, capsys):
    m = _model(data, _opt("AdaGrad"), _mixed_lookups())
    capsys.readouterr()
    m.summary()
    out = capsys.readouterr().out
    for name, shown in (("t0", "Ftrl (opt_params)"), ("t1", "SGD (opt_params)"),
                        ("t2", "AdaGrad (model)")):
        line, = [ln for ln in out.splitlines() if ln.strip().startswith(f"table {name}")]
        assert shown in line


# ---- 10. two ranks ----------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, source, eval_source, folder, ret):
    """(the harness of test_model_gpu's 2-rank model tests: spawned processes over gloo, both on
    this one GPU)"""
    import types
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = types.SimpleNamespace(source=source, eval_source=eval_source)
        m = _model(p, _opt("AdaGrad", **ADA), _mixed_lookups(), world=world)
        # a table's first values depend on how it is sharded: both runs continue from the
        # one-rank model's state after step 2 (tables, their optimizer states, the dense part)
        for _ in range(2):
            assert m.reader.next_batch(train=True) is not None
        m.embedding_load(os.path.join(folder, "emb"))
        m.load_dense_weights(os.path.join(folder, "ck_dense_2.model"))
        m.load_dense_optimizer_states(os.path.join(folder, "ck_opt_dense_2.model"))
        m.set_learning_rate(0.02)
        losses = _train(m, 2)
        shards = {}
        for rt in m._ebc:
            e = rt["train"]
            for k, t in enumerate(e.tables):   # every table row-sharded: key = local * world + rank
                n = -(-(t.max_vocabulary_size - rank) // world)
                s0 = e.row_start_of_table[k]
                shards[t.name] = e.table[s0:s0 + n].cpu().numpy()
        ret[rank] = ("ok", losses, shards, len(m._ebc))
    except Exception as ex:
        import traceback
        ret[rank] = ("".join(traceback.format_exception(type(ex), ex, ex.__traceback__)),)
    finally:
        dist.destroy_process_group()


def test_the_mixed_model_on_two_ranks_trains_like_one_rank(data, mixed):
    """steps 3 and 4 of the mixed model as two ranks (tables row-sharded over both; the state after
    step 2 loaded from the one-rank run's files): the mean of the ranks' losses and every table
    row agree with the one-rank run within the bounds of
    test_model_gpu.py::test_two_ranks_train_like_one_rank -- losses rtol 2e-5, rows rtol 2e-4 /
    atol 2e-6 (the gradient sums of a row are added in another order)"""
    import torch.multiprocessing as mp
    from numpy.testing import assert_allclose
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = 29500 + os.getpid() % 2000 + 41
    procs = [ctx.Process(target=_two_rank_worker,
                         args=(r, 2, port, data.source, data.eval_source, mixed["folder"], ret))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for r in range(2):
        assert ret.get(r) is not None and ret[r][0] == "ok", ret.get(r)
    assert ret[0][3] == ret[1][3] == 3
    two_loss = (np.array(ret[0][1]) + np.array(ret[1][1])) / 2
    print("losses 1 rank", mixed["losses"][2:], "2 ranks", two_loss.tolist())
    assert_allclose(two_loss, np.array(mixed["losses"][2:]), rtol=2e-5)
    for name, (_, want) in mixed["rows"].items():
        got = np.empty_like(want)
        for r in range(2):
            got[r::2] = ret[r][2][name]
        print(name, "max |difference|", float(np.abs(got - want).max()))
        assert_allclose(got, want, rtol=2e-4, atol=2e-6)
