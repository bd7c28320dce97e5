"""The Parquet reader on one MI355X: what a batch costs the training thread on the host path
(decode="host": read_table of a whole file when one is exhausted, numpy per batch, one pageable copy
per tensor -- what the reader did before it became asynchronous) and on the device path (worker
threads stage whole files in pinned slots, one copy per file, one hctr_parquet_decode launch per
batch), the decode kernel alone by device events next to device-to-device copies of the same bytes,
a file's pinned -> device copy, a worker's read_table + staging, and Model.train() fed from the files
next to the same model fed one resident batch.

Writes the files of the given shape under a temporary directory.  One JSON line per shape:

    python tools/parquet_reader_bench.py [--batch 65536] [--files 2] [--batches-per-file 2]
                                         [--steps 30] [--no-models]
                                         [--shapes legacy_onehot,ebc_onehot,ebc_mlperf]
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

import bench  # noqa: E402  (table sizes, hotness, power-law keys)
import hugectr_amd.hugectr as hugectr  # noqa: E402
import raw_reader_bench as rrb  # noqa: E402  (the shapes, the models, the timing helpers)
from hugectr_amd import _lib, data  # noqa: E402


def write_files(folder, B, n_files, per_file, hot, sizes):
    """reference layout; a multi-hot input is a list<int64> column of fixed length"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(7)
    n = B * per_file + B // 2   # (+ a tail shorter than a batch, dropped by the reader)
    lc, dc, cc = data.parquet_columns(1, 13, 26)
    names = []
    for f in range(n_files):
        cols = {}
        cats = [bench.powerlaw(rng, n * h, v, 1.1).astype(np.int64) for v, h in zip(sizes, hot)]
        cols[lc[0]] = pa.array((cats[2][::hot[2]] % 2).astype(np.float32))
        for c in dc:
            cols[c] = pa.array(rng.random(n, dtype=np.float32))
        for c, k, h in zip(cc, cats, hot):
            cols[c] = pa.array(k) if h == 1 else pa.ListArray.from_arrays(
                pa.array(np.arange(n + 1, dtype=np.int32) * h), pa.array(k))
        name = os.path.join(folder, f"part_{f}.parquet")
        pq.write_table(pa.table(cols), name)
        names.append(name)
    with open(os.path.join(folder, "_file_list.txt"), "w") as fl:
        fl.write(f"{len(names)}\n" + "\n".join(names) + "\n")
    meta = {"file_stats": [{"file_name": os.path.basename(x), "num_rows": n} for x in names],
            "labels": [{"col_name": lc[0], "index": 0}],
            "conts": [{"col_name": c, "index": 1 + i} for i, c in enumerate(dc)],
            "cats": [{"col_name": c, "index": 14 + i} for i, c in enumerate(cc)]}
    with open(os.path.join(folder, "_metadata.json"), "w") as fm:
        json.dump(meta, fm)
    return os.path.join(folder, "_file_list.txt"), sum(os.path.getsize(x) for x in names)


def reader_level(files, B, nb, hot, sizes, ebc, i64):
    dev = torch.device("cuda")
    inp = rrb.the_input(hot, ebc)
    groups = [[f"data{i}" for i in range(26)]] if ebc else []
    res = {}
    # ---- the host path: everything on the calling thread, the file reads included
    host = data.ParquetReader(files, inp, sizes, B, 0, 1, dev, i64, True, decode="host")
    host.ebc_groups = groups
    calls = []
    for _ in range(nb):   # one pass over the files
        t0 = time.perf_counter()
        host.next_batch()
        torch.cuda.synchronize()
        calls.append(time.perf_counter() - t0)
    res["host_ms_per_batch"] = float(np.mean(calls)) * 1e3
    res["host_ms_per_batch_without_file_reads"] = rrb.med(sorted(calls)[:max(1, nb // 2)])
    res["host_ms_call_max"] = float(max(calls)) * 1e3
    # ---- the device path
    r = data.ParquetReader(files, inp, sizes, B, 0, 1, dev, i64, True, num_workers=2, ring=2)
    r.ebc_groups = groups
    for _ in range(3):   # ring warm
        r.next_batch()
    torch.cuda.synchronize()
    w0 = r.stats()["wait_ms"]
    calls, n = [], 3 * nb
    t_begin = time.perf_counter()
    for _ in range(n):
        t0 = time.perf_counter()
        b = r.next_batch()
        calls.append(time.perf_counter() - t0)
        b["label"].sum()   # (consumed on the current stream, nothing waits on the host)
    torch.cuda.synchronize()
    res["next_batch_call_ms"] = rrb.med(calls)
    res["next_batch_call_max_ms"] = float(max(calls)) * 1e3
    res["unthrottled_ms_per_batch"] = (time.perf_counter() - t_begin) / n * 1e3
    res["wait_ms_per_batch"] = (r.stats()["wait_ms"] - w0) / n
    res["stats"] = r.stats()
    # ---- the stages alone, on the file the reader is in
    u, pl = r.head_unit(), r.plan
    st, slot = u["latch"].result, u["slot"]
    n_out, raw, pin = len(pl["outputs"]), slot["dev"], slot["pin"]
    arena = torch.empty(int(st["tab"][0, n_out]), dtype=torch.uint8, device=dev)
    used_in = sum(int(st["cnt"][0, k]) * o["esize"] for k, o in enumerate(pl["outputs"]))
    res["file_bytes_staged"], res["bytes_out"] = int(st["used"]), used_in
    res["bytes_in"] = int(st["used"]) * B // max(st["rows"], 1)
    res["segments"], res["work_items"] = len(pl["segments"]), pl["n_items"]
    res["lanes_per_sample"] = sorted({int(g) for g in pl["segments"]["group"] if g})
    torch.cuda.synchronize()
    res["decode_kernel_ms"] = rrb.event_ms(lambda: r.decode_into(arena, u, 0, _lib.stream_ptr()))
    src = torch.empty(res["bytes_in"], dtype=torch.uint8, device=dev)
    src2, arena2 = torch.empty_like(src), torch.empty_like(arena)
    res["d2d_copy_bytes_in_ms"] = rrb.event_ms(lambda: src2.copy_(src))
    res["d2d_copy_bytes_out_ms"] = rrb.event_ms(lambda: arena2.copy_(arena))
    # a copy of n bytes moves 2 n; the decode moves bytes_in + bytes_out
    res["d2d_same_traffic_ms"] = 0.5 * (res["d2d_copy_bytes_in_ms"] + res["d2d_copy_bytes_out_ms"])
    u = int(st["used"])
    res["h2d_pinned_file_copy_ms"] = rrb.event_ms(lambda: raw[:u].copy_(pin[:u], non_blocking=True))
    spare, t_read, t_stage = np.empty(pin.numel(), np.uint8), [], []
    for k in range(3):   # what one worker does per file
        import pyarrow.parquet as pq
        t0 = time.perf_counter()
        t = pq.read_table(r.files[k % len(r.files)], columns=pl["spec"]["names"], use_threads=False)
        t1 = time.perf_counter()
        data.stage_parquet_table(t, r.files[k % len(r.files)], pl["spec"], spare)
        t_read.append(t1 - t0)
        t_stage.append(time.perf_counter() - t1)
    res["worker_read_table_ms_per_file"] = rrb.med(t_read)
    res["worker_staging_ms_per_file"] = rrb.med(t_stage)
    res["batches_per_file"] = int(st["nb"])
    r.close()
    return res


def model_level(files, B, nb, hot, sizes, kind, steps):
    def run(m, n):
        for _ in range(8):
            m.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            m.train()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    rp = hugectr.DataReaderParams(
        data_reader_type=hugectr.DataReaderType_t.Parquet, source=[files], eval_source="",
        check_type=hugectr.Check_t.Non, slot_size_array=sizes, num_workers=2)
    m = rrb.build_model(files, B, nb, hot, sizes, kind, rp=rp)
    rd = m.reader.train
    res = {"ms_per_step_from_files": run(m, steps)}
    st = rd.stats()
    res["file_fed_decode"] = st["decode"]
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
    ap.add_argument("--files", type=int, default=2)
    ap.add_argument("--batches-per-file", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--shapes", default="legacy_onehot,ebc_onehot,ebc_mlperf")
    ap.add_argument("--no-models", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "parquet_reader_bench needs a GPU"
    B, nb = args.batch, args.files * args.batches_per_file
    for name in args.shapes.split(","):
        hot, sizes, ebc = rrb.SHAPES[name]
        tmp = tempfile.mkdtemp(prefix="hctr_parquet_reader_bench_")
        try:
            t0 = time.perf_counter()
            files, nbytes = write_files(tmp, B, args.files, args.batches_per_file, hot, sizes)
            out = {"shape": name, "batch": B, "keys_per_sample": sum(hot), "files": args.files,
                   "parquet_bytes": nbytes, "write_s": round(time.perf_counter() - t0, 1),
                   "device": torch.cuda.get_device_name(0)}
            out.update(reader_level(files, B, nb, hot, sizes, ebc, i64=not ebc))
            if ebc and not args.no_models:
                out.update(model_level(files, B, nb, hot, sizes, name, args.steps))
            print(json.dumps(out), flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
