"""GPU: Model.embedding_dump / Model.embedding_load -- the files follow the USER's
EmbeddingCollectionConfigs, whatever runtime collections Model split them into."""
import filecmp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [203, 37, 140, 70]
BATCH = 64


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    import hugectr_amd.hugectr as hugectr
    d = tmp_path_factory.mktemp("ebc_io_data")
    p = hugectr.tools.DataGeneratorParams(
        format=hugectr.DataReaderType_t.Parquet, label_dim=1, dense_dim=3, num_slot=4,
        i64_input_key=True, source=str(d / "train" / "_file_list.txt"),
        eval_source=str(d / "val" / "_file_list.txt"), slot_size_array=SIZES,
        dist_type=hugectr.Distribution_t.PowerLaw, power_law_type=hugectr.PowerLaw_t.Short,
        num_files=1, eval_num_files=1, num_samples_per_file=4 * BATCH, num_samples=4 * BATCH,
        eval_num_samples=BATCH)
    hugectr.tools.DataGenerator(p).generate()
    return p


def _model(data, seed, dynamic=False, world=1):
    """static: config 0 holds a16 (ev 16) and a8 (ev 8) -- Model runs it as two collections --
    and config 1 a model-parallel and a replicated table -- two more.  dynamic: one config, two
    hash tables."""
    import hugectr_amd.hugectr as hugectr
    solver = hugectr.CreateSolver(batchsize=BATCH, batchsize_eval=BATCH, lr=0.05,
                                  vvgpu=[list(range(world))], i64_input_key=True,
                                  max_eval_batches=1, seed=seed, use_embedding_collection=True)
    reader = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet,
                                      source=[data.source], eval_source=data.eval_source,
                                      slot_size_array=SIZES, check_type=hugectr.Check_t.Non)
    opt = hugectr.CreateOptimizer(optimizer_type=hugectr.Optimizer_t.AdaGrad,
                                  update_type=hugectr.Update_t.Global, initial_accu_value=0.0)
    model = hugectr.Model(solver, reader, opt)
    model.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=3, dense_name="dense",
                            data_reader_sparse_param_array=[
                                hugectr.DataReaderSparseParam(f"data{i}", 1, True, 1)
                                for i in range(4)]))
    T = hugectr.EmbeddingTableConfig
    if dynamic:
        spec = [[("h0", -1, 16, 0), ("h1", -1, 16, 1)]]
    else:
        spec = [[("a16", SIZES[0], 16, 0), ("a8", SIZES[1], 8, 1)],
                [("m", SIZES[2], 16, 2), ("d", SIZES[3], 16, 3)]]
    tops = []
    for c, tables in enumerate(spec):
        ebc = hugectr.EmbeddingCollectionConfig()
        for name, vocab, ev, slot in tables:
            ebc.embedding_lookup(table_config=T(name, vocab, ev), bottom_name=f"data{slot}",
                                 top_name=f"emb_{name}", combiner="sum")
            tops.append(f"emb_{name}")
        if c == 1:
            ebc.shard(shard_matrix=[["m", "d"]] * world,
                      shard_strategy=[("mp", ["m"]), ("dp", ["d"])])
        model.add(ebc)
    D, L = hugectr.DenseLayer, hugectr.Layer_t
    model.add(D(layer_type=L.Concat, bottom_names=tops + ["dense"], top_names=["concat1"]))
    model.add(D(layer_type=L.MLP, bottom_names=["concat1"], top_names=["mlp1"], num_outputs=[16, 1],
                activations=[hugectr.Activation_t.Relu, hugectr.Activation_t.Non]))
    model.add(D(layer_type=L.BinaryCrossEntropyLoss, bottom_names=["mlp1", "label"],
                top_names=["loss"]))
    model.compile()
    return model


def _tables(model):
    """{table name: (runtime collection, position)}"""
    return {tc.name: (rt["train"], k) for rt in model._ebc for k, tc in enumerate(rt["train"].tables)}


def _rows(model, name):
    e, k = _tables(model)[name]
    lay = e._io_layout(k)
    return e.table[lay["row_start"]:lay["row_start"] + lay["vocab"]].cpu().numpy().copy()


def _same_tree(a, b):
    cmp = filecmp.dircmp(a, b)
    assert not cmp.left_only and not cmp.right_only, (cmp.left_only, cmp.right_only)
    for sub in cmp.common_dirs:
        _same_tree(os.path.join(a, sub), os.path.join(b, sub))
    _, mismatch, errors = filecmp.cmpfiles(a, b, cmp.common_files, shallow=False)
    assert not mismatch and not errors, (a, mismatch, errors)


@pytest.fixture(scope="module")
def trained(data):
    m = _model(data, seed=1)
    from hugectr_amd.embedding_collection import DataParallelCollection
    kinds = sorted((type(rt["train"]) is DataParallelCollection, rt["train"].ev) for rt in m._ebc)
    assert kinds == [(False, 8), (False, 16), (False, 16), (True, 16)]   # two configs, four runtimes
    for _ in range(2):
        assert m.train()
    return m


def test_dump_load_dump_is_byte_identical(tmp_path, data, trained):
    d1, d2 = str(tmp_path / "d1"), str(tmp_path / "d2")
    trained.embedding_dump(d1, optimizer_states=True)
    assert sorted(os.listdir(d1)) == ["embedding_collection_0", "embedding_collection_1"]
    for c in range(2):   # one folder per USER config: both tables of the config, ids 0 and 1
        assert sorted(os.listdir(os.path.join(d1, f"embedding_collection_{c}"))) == sorted(
            ["meta_data"] + [f"{s}{i}" for s in ("key", "weight", "opt_state") for i in range(2)])
    from hugectr_amd import embedding_io as eio
    meta = eio.read_meta(d1, 0)
    assert meta.table_ids == [0, 1] and meta.ev_sizes == {0: 16, 1: 8}
    assert meta.key_nums == {0: SIZES[0], 1: SIZES[1]}
    with eio.TableFiles(d1, 1, 1) as f:   # table "d" of config 1: the replicated one
        assert np.array_equal(f.read_weights(), _rows(trained, "d"))
        assert np.array_equal(f.read_keys(), np.arange(SIZES[3]))
    other = _model(data, seed=2)
    assert not np.array_equal(_rows(other, "a16"), _rows(trained, "a16"))
    other.embedding_load(d1)
    for name in ("a16", "a8", "m", "d"):
        assert np.array_equal(_rows(other, name), _rows(trained, name)), name
    other.embedding_dump(d2, optimizer_states=True)
    _same_tree(d1, d2)
    assert other.train()   # (the loaded model goes on training)


def test_table_names_select_tables(tmp_path, data, trained):
    d = str(tmp_path / "one")
    trained.embedding_dump(d, table_names=["a8"])
    assert os.listdir(d) == ["embedding_collection_0"]
    assert sorted(os.listdir(os.path.join(d, "embedding_collection_0"))) == ["key0", "meta_data",
                                                                              "weight0"]
    from hugectr_amd import embedding_io as eio
    assert eio.read_meta(d, 0).table_ids == [1]   # a8 keeps its id; its files are key0 / weight0
    other = _model(data, seed=3)
    before = {n: _rows(other, n) for n in ("a16", "a8", "m", "d")}
    other.embedding_load(d, table_names=["a8"])
    assert np.array_equal(_rows(other, "a8"), _rows(trained, "a8"))
    assert not np.array_equal(before["a8"], _rows(trained, "a8"))
    for n in ("a16", "m", "d"):
        assert np.array_equal(_rows(other, n), before[n]), n
    with pytest.raises(RuntimeError, match="nosuch"):
        trained.embedding_dump(str(tmp_path / "x"), table_names=["a8", "nosuch"])
    assert not os.path.exists(str(tmp_path / "x"))
    with pytest.raises(RuntimeError, match="nosuch"):
        other.embedding_load(d, table_names=["nosuch"])
    with pytest.raises(RuntimeError, match="not in this dump"):
        other.embedding_load(d, table_names=["a16"])


def test_dynamic_model_round_trip_as_maps(tmp_path, data):
    a = _model(data, seed=1, dynamic=True)
    for _ in range(2):
        assert a.train()
    d = str(tmp_path / "dyn")
    a.embedding_dump(d)
    b = _model(data, seed=2, dynamic=True)
    b.embedding_load(d)
    for name in ("h0", "h1"):
        maps = []
        for m in (a, b):
            e, k = _tables(m)[name]
            keys, vals = e.det.export(e.class_of_table[k])
            o = np.argsort(keys.cpu().numpy())
            maps.append((keys.cpu().numpy()[o], vals.cpu().numpy()[o]))
        assert maps[0][0].size > 5
        assert np.array_equal(maps[0][0], maps[1][0]) and np.array_equal(maps[0][1], maps[1][1])
    assert b.train()
