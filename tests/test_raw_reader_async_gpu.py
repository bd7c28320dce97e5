"""The asynchronous Raw reader (hugectr_amd/data.py RawReader on a CUDA device): a ring of pinned
slots filled by worker threads, one copy + one decode launch per batch on a side stream.  The host
reader (CPU device) over the same file is the oracle: keys, row offsets, bucket ranges, labels and
float dense features BIT FOR BIT; integer dense features within 1 ulp (the device adds in fp32 and
takes the logarithm in fp64, the host runs np.log in fp32; tests/test_raw_decode_gpu.py holds them
to 1 ulp of the correctly rounded value)."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 64
L, DN = 1, 3
PARAMS = [("wide", [2, 1], 2), ("a", 3, 1), ("b", 1, 1)]   # legacy param + two collection lookups
SIZES = [40, 9, 100, 77]
GROUPS = [["a", "b"]]
NKEYS = 7


def _inp():
    import hugectr_amd.hugectr as hugectr
    return hugectr.Input(label_dim=L, label_name="label", dense_dim=DN, dense_name="dense",
                         data_reader_sparse_param_array=[
                             hugectr.DataReaderSparseParam(n, h, True, s) for n, h, s in PARAMS])


def _write(path, n, float_ld=True, seed=0):
    from hugectr_amd import data
    rng = np.random.default_rng(seed)
    label = rng.integers(0, 2, size=(n, L))
    dense = rng.random((n, DN)) if float_ld else rng.integers(0, 1000, size=(n, DN))
    cats = rng.integers(0, 1 << 32, size=(n, NKEYS), dtype=np.uint64)
    data.write_raw(str(path), label, dense, cats, float_label_dense=float_ld)
    return str(path)


def _readers(path, *, repeat=False, num_samples=0, ap=None, float_ld=True, i64=True, rank=0,
             world=1):
    from hugectr_amd import data
    out = []
    for dev in (torch.device("cuda"), torch.device("cpu")):
        r = data.RawReader(path, _inp(), SIZES, B, rank, world, dev, num_samples, float_ld, repeat,
                           ap, i64)
        r.ebc_groups = GROUPS
        out.append(r)
    return out


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(got, want, dense_ref=None):
    """dense_ref: for integer dense features, float32(log(float64(float32(x) + float32(1)))) of
    this rank's slice -- the device is held to 1 ulp of it, not to the host's np.log"""
    assert torch.equal(_bits(got["label"]), _bits(want["label"])), "label"
    assert got["dense"].shape == want["dense"].shape
    if dense_ref is None:
        assert torch.equal(_bits(got["dense"]), _bits(want["dense"])), "dense"
    else:
        ref = torch.from_numpy(np.ascontiguousarray(dense_ref)).view(torch.int32)
        d = (_bits(got["dense"]).long() - ref.long()).abs().max().item()
        assert d <= 1, f"integer dense: {d} ulp from the correctly rounded value"
    assert set(got["sparse"]) == set(want["sparse"])
    for name, (ro, keys) in want["sparse"].items():
        gro, gkeys = got["sparse"][name]
        assert gro.dtype == ro.dtype and gkeys.dtype == keys.dtype
        assert torch.equal(gro.cpu(), ro) and torch.equal(gkeys.cpu(), keys), name
    assert len(got["ebc"]) == len(want["ebc"])
    for (gk, gbr), (wk, wbr) in zip(got["ebc"], want["ebc"]):
        assert gk.dtype == wk.dtype and gbr.dtype == wbr.dtype
        assert torch.equal(gk.cpu(), wk) and torch.equal(gbr.cpu(), wbr)


@pytest.mark.parametrize("with_ap", [False, True])
@pytest.mark.parametrize("i64", [True, False])
def test_every_batch_survives_the_ring(tmp_path, with_ap, i64):
    """2 * ring + 3 batches, all kept alive: a ring slot or an output reused too early would change
    an earlier batch.  Each batch is also consumed on the current stream right after next_batch(),
    with no synchronisation: the hand-over itself must order the consumer behind the decode."""
    import hugectr_amd.hugectr as hugectr
    ap = hugectr.AsyncParam(num_threads=3, num_batches_per_thread=4, multi_hot_reader=False) \
        if with_ap else None
    ring = 4 if with_ap else 2
    nb = 2 * ring + 3
    path = _write(tmp_path / "train.bin", nb * B + B // 2)   # (+ a tail shorter than a batch)
    dev, host = _readers(path, ap=ap, i64=i64)
    st = dev.stats()
    assert st["decode"] == "device" and st["ring"] == ring and st["threads"] == (3 if with_ap else 2)
    kept, sums = [], []
    while True:
        b = dev.next_batch()
        if b is None:
            break
        sums.append((b["sparse"]["wide"][1].sum(), b["ebc"][0][0].sum(), b["dense"].sum()))
        kept.append(b)
    assert len(kept) == nb, "the incomplete tail is dropped"
    assert dev.next_batch() is None
    for i, b in enumerate(kept):
        want = host.next_batch()
        _assert_same(b, want)
        assert sums[i][0].item() == want["sparse"]["wide"][1].sum().item()
        assert sums[i][1].item() == want["ebc"][0][0].sum().item()
        assert sums[i][2].item() == b["dense"].sum().item()
    assert host.next_batch() is None
    st = dev.stats()
    assert st["batches"] == nb and st["wait_ms"] >= 0.0
    dev.close()


def test_repeat_wraps_and_no_repeat_ends(tmp_path):
    path = _write(tmp_path / "train.bin", 3 * B + 5)
    dev, host = _readers(path, repeat=True)
    for _ in range(3 * 3 + 1):   # three epochs and one batch
        _assert_same(dev.next_batch(), host.next_batch())
    dev.close()
    dev, host = _readers(path, repeat=False)
    for _ in range(3):
        _assert_same(dev.next_batch(), host.next_batch())
    assert dev.next_batch() is None and dev.next_batch() is None and host.next_batch() is None
    dev.close()


def test_num_samples_and_rank_slice(tmp_path):
    path = _write(tmp_path / "train.bin", 5 * B, float_ld=False)
    dev, host = _readers(path, num_samples=2 * B + 5, float_ld=False, rank=1, world=2)
    rec = np.fromfile(path, "<u4").reshape(-1, L + DN + NKEYS)
    for i in range(2):
        got, want = dev.next_batch(), host.next_batch()
        assert got["label"].shape == (B // 2, L)
        x = rec[i * B + B // 2:(i + 1) * B, L:L + DN].view(np.int32).astype(np.float32)
        ref = np.log((x + np.float32(1.0)).astype(np.float64)).astype(np.float32)
        _assert_same(got, want, dense_ref=ref)
    assert dev.next_batch() is None and host.next_batch() is None
    dev.close()


def test_async_param_conventions(tmp_path):
    """AsyncParam(multi_hot_reader): integer label word, float dense words"""
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import data
    rng = np.random.default_rng(5)
    n = 3 * B
    rec = np.concatenate([rng.integers(0, 2, size=(n, L)).astype(np.uint32),
                          rng.random((n, DN), dtype=np.float32).view(np.uint32),
                          rng.integers(0, 1 << 32, size=(n, NKEYS), dtype=np.uint64).astype(np.uint32)],
                         axis=1)
    path = str(tmp_path / "train.bin")
    rec.astype("<u4").tofile(path)
    ap = hugectr.AsyncParam(num_threads=64, num_batches_per_thread=1, multi_hot_reader=True,
                            is_dense_float=True)
    dev, host = _readers(path, ap=ap)
    assert dev.stats()["threads"] == 8 and dev.stats()["ring"] == 2   # capped / at least two slots
    for _ in range(3):
        _assert_same(dev.next_batch(), host.next_batch())
    dev.close()


def test_close_twice_and_drop_without_close(tmp_path):
    path = _write(tmp_path / "train.bin", 6 * B)
    dev, _ = _readers(path, repeat=True)
    dev.next_batch()
    threads = list(dev._threads)
    assert threads and all(t.daemon and t.is_alive() for t in threads)
    dev.close()
    dev.close()
    assert not any(t.is_alive() for t in threads)
    with pytest.raises(RuntimeError):
        dev.next_batch()
    dev, _ = _readers(path, repeat=True)
    b = dev.next_batch()
    threads = list(dev._threads)
    del dev
    gc.collect()
    assert not any(t.is_alive() for t in threads), "a dropped reader must stop its workers"
    torch.cuda.synchronize()
    assert b["label"].shape == (B, L)   # (a batch outlives its reader)


def test_make_reader_takes_the_async_path(tmp_path):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import data
    path = _write(tmp_path / "train.bin", 4 * B)
    ap = hugectr.AsyncParam(num_threads=3, num_batches_per_thread=4, multi_hot_reader=False)
    rp = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.RawAsync, source=[path],
                                  eval_source=path, check_type=hugectr.Check_t.Non,
                                  slot_size_array=SIZES, float_label_dense=True, async_param=ap)
    solver = hugectr.CreateSolver(batchsize=B, batchsize_eval=B, vvgpu=[[0]], repeat_dataset=True,
                                  i64_input_key=True)
    rd = data.make_reader(rp, _inp(), solver, 0, 1, torch.device("cuda"))
    for r in (rd.train, rd.evalr):
        st = r.stats()
        assert (st["decode"], st["threads"], st["ring"]) == ("device", 3, 4)
        r.close()


# ---- whole models fed from a Raw file ------------------------------------------------------------
MB, STEPS = 256, 8


class _HostFed:
    """Model.reader_override: the host reader's batches, copied up"""

    def __init__(self, host):
        self.train, self.evalr = host, None

    def next_batch(self, train):
        b = self.train.next_batch()
        out = {"label": b["label"].cuda(), "dense": b["dense"].cuda(),
               "sparse": {k: (ro.cuda(), keys.cuda()) for k, (ro, keys) in b["sparse"].items()}}
        if "ebc" in b:
            out["ebc"] = [(k.cuda(), r.cuda()) for k, r in b["ebc"]]
        return out

    def has_eval(self):
        return False


def _model_file(path, sizes, hot, float_ld):
    from hugectr_amd import data
    rng = np.random.default_rng(11)
    n = (STEPS + 2) * MB
    label = rng.integers(0, 2, size=(n, 1))
    dense = rng.random((n, 13)) if float_ld else rng.integers(0, 100, size=(n, 13))
    cats = np.concatenate([rng.integers(0, v, size=(n, h)) for v, h in zip(sizes, hot)], axis=1)
    data.write_raw(str(path), label, dense, cats, float_label_dense=float_ld)
    return str(path)


def _build(kind, path, float_ld, host_fed):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import data
    ebc = kind == "collection"
    sizes, hot = ([300, 50], [3, 1]) if ebc else ([203, 37, 140, 70, 11, 500], [1] * 6)
    solver = hugectr.CreateSolver(max_eval_batches=1, batchsize_eval=MB, batchsize=MB, lr=0.001,
                                  vvgpu=[[0]], repeat_dataset=True, i64_input_key=True, seed=7,
                                  use_embedding_collection=ebc)
    rp = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.RawAsync, source=[path],
                                  eval_source="", check_type=hugectr.Check_t.Non,
                                  slot_size_array=sizes, float_label_dense=float_ld)
    opt = hugectr.CreateOptimizer(optimizer_type=hugectr.Optimizer_t.SGD,
                                  update_type=hugectr.Update_t.Local, atomic_update=False)
    m = hugectr.Model(solver, rp, opt)
    D, T = hugectr.DenseLayer, hugectr.Layer_t
    if ebc:
        sp = [hugectr.DataReaderSparseParam(f"data{i}", hot[i], True, 1) for i in range(2)]
    else:
        sp = [hugectr.DataReaderSparseParam("data1", 1, True, 6)]
    m.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=13, dense_name="dense",
                        data_reader_sparse_param_array=sp))
    if ebc:
        cfg = hugectr.EmbeddingCollectionConfig()
        for i in range(2):
            cfg.embedding_lookup(table_config=hugectr.EmbeddingTableConfig(f"t{i}", sizes[i], 16),
                                 bottom_name=f"data{i}", top_name=f"emb{i}", combiner="sum")
        m.add(cfg)
        m.add(D(layer_type=T.Concat, bottom_names=["emb0", "emb1", "dense"], top_names=["concat1"]))
    else:
        m.add(hugectr.SparseEmbedding(
            embedding_type=hugectr.Embedding_t.DistributedSlotSparseEmbeddingHash,
            workspace_size_per_gpu_in_mb=8, embedding_vec_size=16, combiner="sum",
            sparse_embedding_name="emb", bottom_name="data1", optimizer=opt))
        m.add(D(layer_type=T.Reshape, bottom_names=["emb"], top_names=["reshape1"],
                leading_dim=6 * 16))
        m.add(D(layer_type=T.Concat, bottom_names=["reshape1", "dense"], top_names=["concat1"]))
    m.add(D(layer_type=T.MultiCross, bottom_names=["concat1"], top_names=["multicross1"],
            num_layers=2))
    m.add(D(layer_type=T.InnerProduct, bottom_names=["concat1"], top_names=["fc1"], num_output=64))
    m.add(D(layer_type=T.ReLU, bottom_names=["fc1"], top_names=["relu1"]))
    m.add(D(layer_type=T.Concat, bottom_names=["relu1", "multicross1"], top_names=["concat2"]))
    m.add(D(layer_type=T.InnerProduct, bottom_names=["concat2"], top_names=["fc2"], num_output=1))
    m.add(D(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["fc2", "label"], top_names=["loss"]))
    if host_fed:
        m.reader_override = _HostFed(data.RawReader(path, m.input, sizes, MB, 0, 1,
                                                    torch.device("cpu"), 0, float_ld, True, None,
                                                    True))
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


@pytest.mark.parametrize("kind", ["legacy_dcn", "collection"])
@pytest.mark.parametrize("float_ld", [True, False])
def test_model_trains_from_the_file_like_from_the_host_readers_batches(tmp_path, kind, float_ld):
    sizes, hot = ([300, 50], [3, 1]) if kind == "collection" else ([203, 37, 140, 70, 11, 500],
                                                                   [1] * 6)
    path = _model_file(tmp_path / "train.bin", sizes, hot, float_ld)
    m = _build(kind, path, float_ld, host_fed=False)
    assert m.reader.train.stats()["decode"] == "device"
    got = _losses(m)
    assert m.reader.train.stats()["batches"] >= STEPS
    m.reader.train.close()
    want = _losses(_build(kind, path, float_ld, host_fed=True))
    print("file-fed", got, "host-fed", want)
    assert all(np.isfinite(got))
    if float_ld:
        assert got == want, "float dense: the same bits in, the same losses out"
    else:
        assert np.allclose(got, want, rtol=1e-3, atol=0.0)
