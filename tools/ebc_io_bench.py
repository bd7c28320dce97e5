#!/usr/bin/env python3
"""Rates of Model.embedding_dump / embedding_load below the Model: one static table at ev_size 128
(default 2 GiB) dumped and loaded through EmbeddingCollection.export_table / import_table, and the
device leg of the load alone (hctr_ebc_io_import_static reading a filled pinned chunk over the
host link, no file in the way).  One JSON line; recorded in DESIGN.md, nothing is asserted.

  python tools/ebc_io_bench.py [--gib 2] [--ev 128] [--dir /dev/shm] [--shards 1]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--ev", type=int, default=128)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--shards", type=int, default=1, help="load as shard 0 of this many")
    ap.add_argument("--kernel-iters", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import hugectr_amd as ha
    from hugectr_amd import ebc_io
    from hugectr_amd import embedding_io as eio
    from hugectr_amd._lib import check, lib, ptr, stream_ptr

    vocab = int(a.gib * (1 << 30)) // (a.ev * 4)
    cfg = ha.EmbeddingCollectionConfig()
    cfg.embedding_lookup(ha.EmbeddingTableConfig("t", vocab, a.ev), "in", "out", "sum")
    src = ha.EmbeddingCollection.for_rank(0, 1, cfg, 64, seed=1)
    work = tempfile.mkdtemp(prefix="ebc_io_bench_", dir=a.dir)
    out = dict(vocab=vocab, ev_size=a.ev, table_gib=round(vocab * a.ev * 4 / (1 << 30), 3),
               dir=a.dir or tempfile.gettempdir(), chunk_rows=ebc_io.default_chunk_rows(a.ev))
    try:
        nbytes = vocab * (a.ev * 4 + 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ebc_io.dump_shards(work, 0, [src])
        out["dump_gbps"] = round(nbytes / (time.perf_counter() - t0) / 1e9, 2)
        dcfg = ha.EmbeddingCollectionConfig()
        dcfg.embedding_lookup(ha.EmbeddingTableConfig("t", vocab, a.ev), "in", "out", "sum")
        if a.shards > 1:
            dcfg.shard([[1]] * a.shards)
        dst = ha.EmbeddingCollection.for_rank(0, a.shards, dcfg, 64 * a.shards, seed=2)
        with eio.TableFiles(work, 0, 0) as f:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.validate_table(0, f)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            dst.import_table(0, f, validated=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        out["check_pass_keys_gbps"] = round(vocab * 8 / (t1 - t0) / 1e9, 2)
        out["load_gbps"] = round(nbytes / (t2 - t1) / 1e9, 2)
        out["load_with_check_gbps"] = round(nbytes / (t2 - t0) / 1e9, 2)
        n = -(-vocab // a.shards)
        out["load_exact"] = bool(torch.equal(dst.table[:n], src.table[0:vocab:a.shards]))
        # the device leg alone: both chunks filled once, the import kernel reads them in turn
        R = min(ebc_io.default_chunk_rows(a.ev), vocab)
        with ebc_io.IoChunks(R, a.ev, np.dtype("<i8")) as io:
            for w in range(2):
                io.keys[w][:] = np.arange(w * R, (w + 1) * R) % vocab
                io.rows[w][:] = 1.0
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for it in range(a.kernel_iters + 2):
                if it == 2:
                    ev0.record()
                check(lib.hctr_ebc_io_import_static(io._h, it & 1, R, 1, 0, vocab, 0, ptr(src.table),
                                                    None, None, stream_ptr()))
            ev1.record()
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1) / a.kernel_iters
        out["import_kernel_host_read_gbps"] = round(R * (a.ev * 4 + 8) / (ms * 1e-3) / 1e9, 2)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
