"""The Raw reader on one MI355X: what a batch costs on the host path (RawReader on the CPU device +
the .to(device) copies: the work the training thread did before the reader became asynchronous)
and on the device path (ring of pinned slots, one copy + one hctr_raw_decode launch per batch), the
decode kernel alone by device events next to device-to-device copies of the same bytes, and
Model.train() fed from the file next to the same model fed one resident batch.

Writes a Raw file of the given shape under a temporary directory.  One JSON line per shape:

    python tools/raw_reader_bench.py [--batch 65536] [--batches 6] [--steps 30]
                                     [--shapes legacy_onehot,ebc_onehot,ebc_mlperf] [--no-models]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (table sizes, hotness, power-law keys, the MLP shapes)
import hugectr_amd.hugectr as hugectr  # noqa: E402
from hugectr_amd import _lib, data  # noqa: E402

SHAPES = {
    # name: (hotness per input, table sizes, one legacy param / one input per lookup)
    "legacy_onehot": ([1] * 26, bench.CRITEO_1TB, False),
    "ebc_onehot": ([1] * 26, bench.CRITEO_1TB, True),
    "ebc_mlperf": (bench.MLPERF_HOTNESS, bench.MLPERF_TABLES, True),
}


def write_file(path, B, nb, hot, sizes):
    rng = np.random.default_rng(7)
    n = B * nb
    a = np.zeros((n, 14 + sum(hot)), dtype="<u4")
    col = 14
    for v, h in zip(sizes, hot):
        a[:, col:col + h] = bench.powerlaw(rng, n * h, v, 1.1).reshape(n, h).astype("<u4")
        col += h
    a[:, 0] = (a[:, 16] % 2).astype("<i4").view("<u4")
    a[:, 1:14] = rng.random((n, 13), dtype=np.float32).view("<u4")
    a.tofile(path)


def the_input(hot, ebc):
    if ebc:
        sp = [hugectr.DataReaderSparseParam(f"data{i}", hot[i], True, 1) for i in range(26)]
    else:
        sp = [hugectr.DataReaderSparseParam("data1", 1, True, 26)]
    return hugectr.Input(label_dim=1, label_name="label", dense_dim=13, dense_name="dense",
                         data_reader_sparse_param_array=sp)


def async_param():
    return hugectr.AsyncParam(4, 4, 512000, 4, 512, True, hugectr.Alignment_t.Non,
                              multi_hot_reader=True, is_dense_float=True)


def to_device(b, dev):
    out = {"label": b["label"].to(dev), "dense": b["dense"].to(dev),
           "sparse": {k: (ro.to(dev), keys.to(dev)) for k, (ro, keys) in b["sparse"].items()}}
    if "ebc" in b:
        out["ebc"] = [(k.to(dev), r.to(dev)) for k, r in b["ebc"]]
    return out


def med(ts):
    return float(np.median(ts)) * 1e3


def event_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def reader_level(path, B, nb, hot, sizes, ebc, i64):
    dev = torch.device("cuda")
    inp = the_input(hot, ebc)
    groups = [[f"data{i}" for i in range(26)]] if ebc else []
    res = {}
    # ---- the host path: decode in numpy on the calling thread, one synchronous copy per tensor
    host = data.RawReader(path, inp, sizes, B, 0, 1, torch.device("cpu"), 0, False, True,
                          async_param(), i64)
    host.ebc_groups = groups
    t_dec, t_all = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        b = host.next_batch()
        t1 = time.perf_counter()
        to_device(b, dev)
        torch.cuda.synchronize()
        t_all.append(time.perf_counter() - t0)
        t_dec.append(t1 - t0)
    res["host_decode_ms"], res["host_decode_plus_copies_ms"] = med(t_dec), med(t_all)
    # ---- the device path
    r = data.RawReader(path, inp, sizes, B, 0, 1, dev, 0, False, True, async_param(), i64)
    r.ebc_groups = groups
    for _ in range(3):   # ring warm
        r.next_batch()
    torch.cuda.synchronize()
    w0 = r.stats()["wait_ms"]
    calls, n = [], 4 * nb
    t_begin = time.perf_counter()
    for _ in range(n):
        t0 = time.perf_counter()
        b = r.next_batch()
        calls.append(time.perf_counter() - t0)
        b["label"].sum()   # (consumed on the current stream, nothing waits on the host)
    torch.cuda.synchronize()
    res["next_batch_call_ms"] = med(calls)
    res["next_batch_call_max_ms"] = float(max(calls)) * 1e3
    res["unthrottled_ms_per_batch"] = (time.perf_counter() - t_begin) / n * 1e3
    res["wait_ms_per_batch"] = (r.stats()["wait_ms"] - w0) / n
    res["stats"] = r.stats()
    # ---- the stages alone, on the buffers of the batch the reader is at
    u, pl = r.head_unit(), r.plan
    pin, raw = u["slot"]["pin"], u["slot"]["dev"]
    arena = torch.empty(pl["arena_bytes"], dtype=torch.uint8, device=dev)
    res["bytes_in"], res["bytes_out"] = raw.numel() * 4, int(pl["arena_bytes"])
    res["segments"] = len(pl["segments"])
    torch.cuda.synchronize()
    res["decode_kernel_ms"] = event_ms(lambda: r.decode_into(arena, u, 0, _lib.stream_ptr()))
    raw2, arena2 = torch.empty_like(raw), torch.empty_like(arena)
    res["d2d_copy_bytes_in_ms"] = event_ms(lambda: raw2.copy_(raw))
    res["d2d_copy_bytes_out_ms"] = event_ms(lambda: arena2.copy_(arena))
    # a copy of n bytes moves 2 n; the decode moves bytes_in + bytes_out
    res["d2d_same_traffic_ms"] = 0.5 * (res["d2d_copy_bytes_in_ms"] + res["d2d_copy_bytes_out_ms"])
    res["h2d_pinned_copy_ms"] = event_ms(lambda: raw.copy_(pin, non_blocking=True))
    t = []
    for k in range(5):   # one worker's share of a fill is 1 / threads of this
        t0 = time.perf_counter()
        np.copyto(u["slot"]["np"], r.data[(k % nb) * B:(k % nb + 1) * B])
        t.append(time.perf_counter() - t0)
    res["memmap_to_pinned_one_thread_ms"] = med(t)
    r.close()
    return res


def build_model(path, B, nb, hot, sizes, kind, rp=None):
    """bench.py's model of the shape: DLRM (one-hot, concat lookups, Interaction) or the MLPerf
    DCNv2 (multi-hot, sum, MultiCross), embedding_collection, mixed precision, SGD.  rp: other
    DataReaderParams than the Raw file's (tools/parquet_reader_bench.py)"""
    solver = hugectr.CreateSolver(max_eval_batches=1, batchsize_eval=B, batchsize=B, lr=0.005,
                                  vvgpu=[[0]], repeat_dataset=True, i64_input_key=False,
                                  use_mixed_precision=True, scaler=1024.0,
                                  use_embedding_collection=True)
    opt = hugectr.CreateOptimizer(optimizer_type=hugectr.Optimizer_t.SGD,
                                  update_type=hugectr.Update_t.Local, atomic_update=True)
    rp = rp or hugectr.DataReaderParams(
        data_reader_type=hugectr.DataReaderType_t.RawAsync, source=[path], eval_source="",
        check_type=hugectr.Check_t.Non, num_samples=B * nb, eval_num_samples=0,
        slot_size_array=sizes, async_param=async_param())
    m = hugectr.Model(solver, rp, opt)
    m.add(the_input(hot, True))
    tables = [hugectr.EmbeddingTableConfig(name=str(i), max_vocabulary_size=v, ev_size=128)
              for i, v in enumerate(sizes)]
    mlperf = kind == "ebc_mlperf"
    ebc = hugectr.EmbeddingCollectionConfig(use_exclusive_keys=True)
    ebc.embedding_lookup(table_config=tables, bottom_name=[f"data{i}" for i in range(26)],
                         top_name="sparse_embedding",
                         combiner=["sum" if mlperf else "concat"] * 26)
    names = [str(i) for i in range(26)]
    ebc.shard(shard_matrix=[names], shard_strategy=[("mp", names)])
    m.add(ebc)
    L, T, A = hugectr.DenseLayer, hugectr.Layer_t, hugectr.Activation_t
    m.add(L(layer_type=T.MLP, bottom_names=["dense"], top_names=["mlp1"],
            num_outputs=bench.BOTTOM, act_type=A.Relu))
    if mlperf:
        m.add(L(layer_type=T.Concat, bottom_names=["sparse_embedding", "mlp1"],
                top_names=["concat1"]))
        m.add(L(layer_type=T.MultiCross, bottom_names=["concat1"], top_names=["interaction1"],
                projection_dim=512, num_layers=3))
    else:
        m.add(L(layer_type=T.Reshape, bottom_names=["sparse_embedding"],
                top_names=["sparse_embedding1"], shape=[-1, 26, 128]))
        m.add(L(layer_type=T.Interaction, bottom_names=["mlp1", "sparse_embedding1"],
                top_names=["interaction1"]))
    m.add(L(layer_type=T.MLP, bottom_names=["interaction1"], top_names=["mlp2"],
            num_outputs=bench.TOP, activations=[A.Relu] * 4 + [A.Non]))
    m.add(L(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["mlp2", "label"],
            top_names=["loss"]))
    m.compile()
    return m


def model_level(path, B, nb, hot, sizes, kind, steps):
    def run(m, n):
        for _ in range(8):
            m.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            m.train()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    m = build_model(path, B, nb, hot, sizes, kind)
    rd = m.reader.train
    res = {"ms_per_step_from_file": run(m, steps)}
    st = rd.stats()
    res["file_fed_wait_ms_per_batch"] = st["wait_ms"] / max(st["batches"], 1)
    resident = m.reader.next_batch(True)
    rd.close()
    m.reader = bench._CycleReader([resident])
    m._lookahead = None
    res["ms_per_step_resident"] = run(m, steps)
    res["final_loss"] = m.get_current_loss()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", default="legacy_onehot,ebc_onehot,ebc_mlperf")
    ap.add_argument("--no-models", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raw_reader_bench needs a GPU"
    B, nb = args.batch, args.batches
    for name in args.shapes.split(","):
        hot, sizes, ebc = SHAPES[name]
        tmp = tempfile.mkdtemp(prefix="hctr_raw_reader_bench_")
        try:
            path = os.path.join(tmp, "train_data.bin")
            write_file(path, B, nb, hot, sizes)
            out = {"shape": name, "batch": B, "words_per_sample": 14 + sum(hot),
                   "device": torch.cuda.get_device_name(0)}
            out.update(reader_level(path, B, nb, hot, sizes, ebc, i64=not ebc))
            if ebc and not args.no_models:
                out.update(model_level(path, B, nb, hot, sizes, name, args.steps))
            print(json.dumps(out), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
