"""Step time of an embedding_collection on hybrid tables (storage="hybrid"), one GPU: forward +
backward_and_update of 4 tables, D = 128, one one-hot "sum" lookup per table, power-law keys.

  dynamic     the same collection on dynamic tables (every key kept in HBM): the yardstick
  hybrid      bounded tables, everything in HBM
  hybrid_tier the same with max_hbm_for_vectors giving H = C / 2: half the slots' rows and
              optimizer states in pinned host memory (staged per call by the table)

The tables are warmed until they hold the key set (no growth, no eviction in the timed steps), so
the three legs do the same arithmetic.  Per step and table the hybrid path makes one inserting
lookup, one find and one update call; around them, per step: route, group, row_ptrs, pool,
key_grads (one launch each), one host synchronisation (the segment offsets) and two small
asynchronous host-to-device copies from a pinned buffer (segment destinations, table descriptors).
Not part of bench.py's line.  Usage: python tools/ebc_hybrid_bench.py [--batch 65536] [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hugectr_amd as ha  # noqa: E402
from hugectr_amd import _lib  # noqa: E402

TABLES, D = 4, 128


def collection(kind, batch, capacity, optimizer):
    kw = {}
    if kind != "dynamic":
        kw = dict(var_type="hybrid", max_capacity=capacity, initializer="0.01")
        if kind == "hybrid_tier":
            kw["max_hbm_for_vectors"] = (capacity // 2) * D * 4 / 2**30
    tables = [ha.EmbeddingTableConfig(f"t{i}", -1, D, **kw) for i in range(TABLES)]
    cfg = ha.EmbeddingCollectionConfig()
    for i, t in enumerate(tables):
        cfg.embedding_lookup(t, f"in{i}", f"out{i}", "sum")
    cfg.shard([[1] * TABLES])
    return ha.EmbeddingCollection.for_rank(0, 1, cfg, batch, lr=0.01, optimizer=optimizer,
                                           max_hotness=1, batch_major=True, initializer="0.01",
                                           init_capacity=capacity)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=1 << 21, help="slots per table")
    ap.add_argument("--vocab", type=int, default=1 << 20, help="distinct keys per table")
    ap.add_argument("--alpha", type=float, default=1.05, help="power-law exponent of the keys")
    ap.add_argument("--optimizer", default="adagrad", choices=["sgd", "adagrad", "adam"])
    args = ap.parse_args()
    B, V = args.batch, args.vocab
    code = {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "adam": _lib.OPT_ADAM}[args.optimizer]
    g = torch.Generator(device="cuda").manual_seed(0)
    # power-law ranks -> keys spread over the int64 range by an odd multiplier
    def draw():
        u = torch.rand(TABLES * B, device="cuda", generator=g, dtype=torch.float64)
        r = (V ** (1.0 - u ** (1.0 / args.alpha))).to(torch.int64).clamp_(0, V - 1)
        return r * 2654435761 + 12345
    batches = [draw() for _ in range(args.iters + 3)]
    br = torch.arange(TABLES * B + 1, dtype=torch.int64, device="cuda")
    grad = torch.randn((B, TABLES, D), device="cuda") * 1e-3
    every = torch.arange(V, dtype=torch.int64, device="cuda") * 2654435761 + 12345
    res = {"batch": B, "tables": TABLES, "dim": D, "capacity": args.capacity, "vocab": V,
           "optimizer": args.optimizer, "device": torch.cuda.get_device_name(0)}
    for kind in ("dynamic", "hybrid", "hybrid_tier"):
        e = collection(kind, B, args.capacity, code)
        # warm-up: every key stored (whole batches of the key set), then three ordinary steps
        for start in range(0, V, B):
            ks = every[start:start + B]
            ks = torch.cat([ks, ks[:B - ks.numel()]]) if ks.numel() < B else ks
            e.forward(ks.repeat(TABLES), br)
        for i in range(3):
            e.forward(batches[i], br)
            e.backward_and_update(grad)
        torch.cuda.synchronize()
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        fwd = bwd = 0.0
        for i in range(args.iters):
            a.record()
            e.forward(batches[3 + i], br)
            b.record()
            e.backward_and_update(grad)
            c.record()
            c.synchronize()
            fwd += a.elapsed_time(b)
            bwd += b.elapsed_time(c)
        res[kind] = {"forward_us": round(fwd / args.iters * 1e3, 1),
                     "backward_update_us": round(bwd / args.iters * 1e3, 1)}
        if kind != "dynamic":
            res[kind]["table_stats"] = e.table_stats()["t0"]
        del e
    print(json.dumps(res))


if __name__ == "__main__":
    main()
