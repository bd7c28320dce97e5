"""GPU: solver.metrics_spec through Model.eval / get_eval_metrics / fit (hugectr_amd/metrics.py).
A wrapper in the test records the (loss, prob) pairs of the evaluation _run_batch calls and the
labels they saw; tests/metrics_oracle.py on those is the expectation.  AUC: the oracle's value to
the last bit of the fp64 division (the words are integers); HitRate: exact counters; NDCG, SMAPE and
AverageLoss: fp64 sums, within 1e-9 relative."""
import glob

import numpy as np
import pytest

import metrics_oracle as mo

pytestmark = pytest.mark.gpu
SIZES = [203, 185, 140, 70, 189, 4, 63, 12]
B = 512


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """synthetic Parquet sets as test_model_gpu.py builds them, with one and with two labels; label
    k = parity of feature C(k+1), so the model learns something"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import hugectr_amd.hugectr as hugectr
    out = {}
    for L in (1, 2):
        d = tmp_path_factory.mktemp(f"labels{L}")
        p = hugectr.tools.DataGeneratorParams(
            format=hugectr.DataReaderType_t.Parquet, label_dim=L, dense_dim=13, num_slot=len(SIZES),
            i64_input_key=True, source=str(d / "train" / "_file_list.txt"),
            eval_source=str(d / "val" / "_file_list.txt"), slot_size_array=SIZES,
            dist_type=hugectr.Distribution_t.PowerLaw, power_law_type=hugectr.PowerLaw_t.Short,
            num_files=1, eval_num_files=1, num_samples_per_file=4096, num_samples=4096,
            eval_num_samples=2048)
        hugectr.tools.DataGenerator(p).generate()
        for f in glob.glob(str(d / "*" / "*.parquet")):
            t = pq.read_table(f)
            for k in range(L):
                col = "label" if L == 1 else f"label{k}"
                lab = (t[f"C{k + 1}"].to_numpy() % 2).astype(np.float32)
                t = t.set_column(t.schema.get_field_index(col), col, pa.array(lab, type=pa.float32()))
            pq.write_table(t, f)
        out[L] = p
    return out


def _model(data, spec=None, labels=1, max_eval_batches=2, compile_it=True):
    import hugectr_amd.hugectr as hugectr
    p = data[labels]
    kw = {} if spec is None else {"metrics_spec": spec}
    solver = hugectr.CreateSolver(max_eval_batches=max_eval_batches, batchsize_eval=B, batchsize=B,
                                  lr=0.01, vvgpu=[[0]], repeat_dataset=True, i64_input_key=True, **kw)
    reader = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet,
                                      source=[p.source], eval_source=p.eval_source,
                                      slot_size_array=SIZES, check_type=hugectr.Check_t.Non)
    opt = hugectr.CreateOptimizer(optimizer_type=hugectr.Optimizer_t.Adam,
                                  update_type=hugectr.Update_t.Local)
    m = hugectr.Model(solver, reader, opt)
    L, D = hugectr.Layer_t, hugectr.DenseLayer
    sparse = [hugectr.DataReaderSparseParam("data1", 1, True, len(SIZES))]
    if labels == 1:
        m.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=13, dense_name="dense",
                            data_reader_sparse_param_array=sparse))
    else:
        m.add(hugectr.Input(label_dims=[1, 1], label_names=["la", "lb"], dense_dim=13,
                            dense_name="dense", data_reader_sparse_param_array=sparse))
    m.add(hugectr.SparseEmbedding(
        embedding_type=hugectr.Embedding_t.LocalizedSlotSparseEmbeddingHash,
        slot_size_array=SIZES, embedding_vec_size=16, combiner="sum",
        sparse_embedding_name="emb", bottom_name="data1", optimizer=opt))
    m.add(D(layer_type=L.Reshape, bottom_names=["emb"], top_names=["flat"],
            leading_dim=16 * len(SIZES)))
    m.add(D(layer_type=L.Concat, bottom_names=["flat", "dense"], top_names=["cat"]))
    for k, lab in enumerate(["label"] if labels == 1 else ["la", "lb"]):
        m.add(D(layer_type=L.MLP, bottom_names=["cat"], top_names=[f"mlp{k}"], num_outputs=[32, 1],
                activations=[hugectr.Activation_t.Relu, hugectr.Activation_t.Non]))
        m.add(D(layer_type=L.BinaryCrossEntropyLoss, bottom_names=[f"mlp{k}", lab],
                top_names=[f"loss{k}"]))
    if compile_it:
        if labels == 1:
            m.compile()
        else:
            m.compile(loss_names=["la", "lb"], loss_weights=[0.5, 0.5])
    return m, hugectr


def _record(m):
    """wraps the evaluation _run_batch calls: (loss, prob, label) of each, as the model saw them"""
    rec, run = [], m._run_batch

    def wrapped(batch, train, nxt=None):
        out = run(batch, train, nxt)
        if not train:
            rec.append((out[0].detach().clone(), out[1].detach().clone(),
                        batch["label"].detach().clone()))
        return out

    m._run_batch = wrapped
    return rec


def _host(rec):
    loss = np.array([float(l.double().cpu()) for l, _, _ in rec], np.float64)
    p = np.concatenate([q.float().cpu().numpy().reshape(q.shape[0], -1) for _, q, _ in rec])
    y = np.concatenate([t.float().cpu().numpy().reshape(t.shape[0], -1) for _, _, t in rec])
    return loss, p, y


def test_all_five_types_in_enum_order_against_the_oracle(data):
    import hugectr_amd.hugectr as hugectr
    T = hugectr.MetricsType
    spec = {T.SMAPE: 0.0, T.NDCG: 0.0, T.HitRate: 0.0, T.AverageLoss: 0.0, T.AUC: 1.0}
    m, _ = _model(data, spec)
    for _ in range(30):
        m.train()
    rec = _record(m)
    m._eval_buf = []
    for _ in range(3):
        assert m.eval()
    res = m.get_eval_metrics()
    assert [n for n, _ in res] == ["AUC", "AverageLoss", "HitRate", "NDCG", "SMAPE"]
    got = dict(res)
    loss, p, y = _host(rec)
    assert p.shape == (3 * B, 1) == y.shape
    want = {"AUC": mo.auc(p, y), "AverageLoss": float(np.mean(loss)), "HitRate": mo.hitrate(p, y),
            "NDCG": mo.ndcg(p, y), "SMAPE": mo.smape(p, y)}
    print("got", got, "\noracle", want)
    assert got["AUC"] == want["AUC"], "AUC must equal the oracle to the last bit"
    assert got["HitRate"] == want["HitRate"]
    for k in ("AverageLoss", "NDCG", "SMAPE"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), k
    assert m._metrics.per_class("AUC") == [want["AUC"]]


def test_default_spec_reset_and_repeat(data):
    m, _ = _model(data)
    assert m.get_eval_metrics() == [] and not m._eval_buf
    rec = _record(m)
    assert m.eval() and m.eval()
    assert m._eval_buf
    first = m.get_eval_metrics()
    assert [n for n, _ in first] == ["AUC", "AverageLoss"]
    assert m.get_eval_metrics() == first, "a second call repeats the first: nothing is reset"
    loss, p, y = _host(rec)
    assert dict(first)["AUC"] == mo.auc(p, y)
    m._eval_buf = []  # the reset existing callers use
    assert not m._eval_buf and m.get_eval_metrics() == []
    del rec[:]
    assert m.eval()
    loss, p, y = _host(rec)
    res = dict(m.get_eval_metrics())
    assert p.shape[0] == B and res["AUC"] == mo.auc(p, y)
    assert abs(res["AverageLoss"] - loss[0]) <= 1e-9 * abs(loss[0])


def test_fit_stops_at_the_target_auc(data, capsys):
    import hugectr_amd.hugectr as hugectr
    m, _ = _model(data, {hugectr.MetricsType.AUC: 0.0})
    m.fit(max_iter=40, display=0, eval_interval=10, snapshot=0)
    out = capsys.readouterr().out
    assert m._iter == 10, "fit must return at the first evaluation: AUC > 0.0"
    assert "Hit target accuracy AUC 0.00000 at 9 / 40 iterations with batchsize 512" in out
    assert "Finish" not in out
    m, _ = _model(data, {hugectr.MetricsType.AUC: 1.0})
    m.fit(max_iter=40, display=0, eval_interval=10, snapshot=0)
    out = capsys.readouterr().out
    assert m._iter == 40 and "Hit target" not in out and "Finish 40 iterations" in out
    assert out.count("Evaluation, AUC") == 4


def test_two_label_model_reports_the_mean_of_the_column_aucs(data, capsys):
    m, hugectr = _model(data, labels=2)
    for _ in range(30):
        m.train()
    rec = _record(m)
    m._eval_buf = []
    for _ in range(2):
        assert m.eval()
    res = m.get_eval_metrics()
    assert [n for n, _ in res] == ["AUC", "AverageLoss"]
    loss, p, y = _host(rec)
    assert p.shape == (2 * B, 2) == y.shape
    mean, per = mo.auc_mean(p, y)
    pooled = mo.auc(p.reshape(-1), y.reshape(-1))
    print("mean", mean, "per class", per, "pooled", pooled, "got", res)
    assert dict(res)["AUC"] == mean
    assert m._metrics.per_class("AUC") == per and len(per) == 2
    assert per[0] != per[1] and mean != pooled
    m.fit(max_iter=4, display=0, eval_interval=4, snapshot=0)
    assert "Evaluation, AUC: {" in capsys.readouterr().out  # the per-class line of the reference
    # anything but AUC on a model with more than one loss layer: refused at compile()
    T = hugectr.MetricsType
    m2, _ = _model(data, {T.AUC: 1.0, T.HitRate: 0.0}, labels=2, compile_it=False)
    with pytest.raises(RuntimeError, match="Metrics besides AUC are not supported for multi-task"):
        m2.compile(loss_names=["la", "lb"], loss_weights=[0.5, 0.5])


def test_store_grows_past_max_eval_batches(data):
    m, _ = _model(data, max_eval_batches=2)
    rec = _record(m)
    assert m.eval()
    cap0 = m._metrics.cap
    assert cap0 == 2 * B
    for _ in range(7):
        assert m.eval()
    assert m._metrics.cap >= 8 * B > cap0 and m._metrics.n == 8 * B
    loss, p, y = _host(rec)
    res = dict(m.get_eval_metrics())
    assert p.shape[0] == 8 * B and res["AUC"] == mo.auc(p, y)
    assert abs(res["AverageLoss"] - np.mean(loss)) <= 1e-9 * abs(np.mean(loss))


def test_auc_over_labels_that_are_not_binary_is_an_error(data):
    import torch
    m, _ = _model(data)
    assert m.eval()
    m._metrics.add_batch(torch.rand(4, 1, device="cuda"),
                         torch.tensor([[0.0], [1.0], [0.5], [1.0]], device="cuda"),
                         torch.zeros((), device="cuda"))
    with pytest.raises(RuntimeError, match="labels that are 0 or 1"):
        m.get_eval_metrics()
