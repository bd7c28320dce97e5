"""A model fed from Parquet files through the device path of the reader (hugectr_amd/data.py
ParquetReader, hctr_parquet_decode) trains exactly like one fed through the host path: the inputs
have the same bits and the rest of the step is the same code, so the losses are equal bit for bit.
cache_eval_data keeps the evaluation reader's first batches on the device."""
import numpy as np
import pytest
import torch

import parquet_oracle as po

pytestmark = pytest.mark.gpu

MB, STEPS = 64, 6
SIZES = [203, 500, 37]
DENSE = 4


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import pyarrow as pa
    rng = np.random.default_rng(11)

    def tab(n):
        hot = rng.integers(1, 4, size=n)
        cols = {"label": pa.array(rng.integers(0, 2, size=n).astype(np.float32), type=pa.float32())}
        for i in range(DENSE):
            cols[f"I{i + 1}"] = pa.array(rng.random(n, dtype=np.float32), type=pa.float32())
        cols["C1"] = pa.array(rng.integers(0, SIZES[0], size=n), type=pa.int64())
        cols["C2"] = pa.array([rng.integers(0, SIZES[1], size=int(k)).tolist() for k in hot],
                              type=pa.list_(pa.int64()))
        cols["C3"] = pa.array(rng.integers(0, SIZES[2], size=n).astype(np.int32), type=pa.int32())
        return pa.table(cols)

    d = tmp_path_factory.mktemp("model_pq")
    names = dict(labels=["label"], conts=[f"I{i + 1}" for i in range(DENSE)], cats=["C1", "C2", "C3"],
                 row_group_size=100)
    return (po.write_dataset(d / "train", [tab(4 * MB + 10), tab(4 * MB + 3)], **names),
            po.write_dataset(d / "val", [tab(3 * MB), tab(2 * MB)], **names))


def _build(files, decode, cache_eval_data=0):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import data
    solver = hugectr.CreateSolver(max_eval_batches=2, batchsize_eval=MB, batchsize=MB, lr=0.001,
                                  vvgpu=[[0]], repeat_dataset=True, i64_input_key=True, seed=7)
    rp = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet,
                                  source=[files[0]], eval_source=files[1],
                                  check_type=hugectr.Check_t.Non, slot_size_array=SIZES,
                                  num_workers=2, cache_eval_data=cache_eval_data)
    opt = hugectr.CreateOptimizer(optimizer_type=hugectr.Optimizer_t.SGD,
                                  update_type=hugectr.Update_t.Local, atomic_update=False)
    m = hugectr.Model(solver, rp, opt)
    D, T = hugectr.DenseLayer, hugectr.Layer_t
    m.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=DENSE, dense_name="dense",
                        data_reader_sparse_param_array=[
                            hugectr.DataReaderSparseParam("data1", [1, 3, 1], False, 3)]))
    m.add(hugectr.SparseEmbedding(
        embedding_type=hugectr.Embedding_t.DistributedSlotSparseEmbeddingHash,
        workspace_size_per_gpu_in_mb=8, embedding_vec_size=16, combiner="sum",
        sparse_embedding_name="emb", bottom_name="data1", optimizer=opt))
    m.add(D(layer_type=T.Reshape, bottom_names=["emb"], top_names=["reshape1"], leading_dim=3 * 16))
    m.add(D(layer_type=T.Concat, bottom_names=["reshape1", "dense"], top_names=["concat1"]))
    m.add(D(layer_type=T.MultiCross, bottom_names=["concat1"], top_names=["multicross1"],
            num_layers=2))
    m.add(D(layer_type=T.InnerProduct, bottom_names=["concat1"], top_names=["fc1"], num_output=64))
    m.add(D(layer_type=T.ReLU, bottom_names=["fc1"], top_names=["relu1"]))
    m.add(D(layer_type=T.Concat, bottom_names=["relu1", "multicross1"], top_names=["concat2"]))
    m.add(D(layer_type=T.InnerProduct, bottom_names=["concat2"], top_names=["fc2"], num_output=1))
    m.add(D(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["fc2", "label"], top_names=["loss"]))
    if decode == "host":
        m.reader_override = data.make_reader(rp, m.input, solver, 0, 1, torch.device("cuda"),
                                             parquet_decode="host")
    m.compile()
    return m


def _losses(m):
    out = []
    for _ in range(STEPS):
        assert m.train()
        out.append(float(m.get_current_loss()))
    m._drain_prefetch()
    torch.cuda.synchronize()
    return out


def _close(m):
    for r in (m.reader.train, m.reader.evalr):
        r.close()


def test_losses_equal_the_host_paths_bit_for_bit(files):
    m = _build(files, "auto")
    assert m.reader.train.stats()["decode"] == "device"
    got = _losses(m)
    assert m.reader.train.stats()["batches"] >= STEPS
    _close(m)
    h = _build(files, "host")
    assert h.reader.train.stats()["decode"] == "host"
    want = _losses(h)
    _close(h)
    print("device path", got, "host path", want)
    assert all(np.isfinite(got))
    assert got == want, "the same bits in, the same losses out"


def test_cached_eval_batches_give_the_same_metrics_every_round(files):
    m = _build(files, "auto", cache_eval_data=2)
    ev = m.reader.evalr
    assert ev.stats()["decode"] == "device" and m.reader.train._cache_n == 0
    for _ in range(2):
        assert m.train()
    rounds = []
    for _ in range(2):
        m._eval_buf = []
        for _ in range(2):
            assert m.eval()
        torch.cuda.synchronize()
        rounds.append(m.get_eval_metrics())
    print(rounds)
    assert rounds[0] == rounds[1]
    assert ev.stats()["batches"] == 4 and ev.stats()["files"] == 1
    _close(m)
