"""Micro-benchmark of the hybrid (LRU) table, csrc/hybrid_table.hip: capacity 2^24, 1 M keys per
call, D = 16 and 128.

  find       all keys stored (hctr_lru_find: digest line + key per key)
  insert10   inserting lookup, 10 % of the keys missing, every bucket full (90 % hits)
  insert100  inserting lookup, 100 % missing, every bucket full (every key evicts)
  insert10_filter  insert10 through the low-frequency filter at p = 0.5 (half the missing keys
             are admitted; hctr_lru_lookup_index_filtered)
  export_if  hctr_lru_export_if after one call touched about 10 % of the slots: one pass over keys
             and scores (16 B per slot) plus the matching keys, slots, scores and rows

Host-memory tier (--tier, hctr_lru_create_tiered with H = C / 2: about half of any key stream is
host-resident):
  tier_find_stage  read-only lookup of stored keys: find + staging (a host-resident key's row is
             copied into its per-call HBM row)
  tier_insert10    inserting lookup, 10 % missing, every bucket full, + staging
  tier_sgd / tier_adam  hctr_lru_apply_update on 1 M stored keys (distinct): the host slots
             staged into HBM, the sparse update, the write-back.  States per row: 0 / 2.
Host-link bytes (the bound the tier is measured against; 63 GB/s spec, the tiered table's 51 GB/s):
half the keys' rows once in for a lookup (plus the new host rows' writes for the insert), their
rows and states in and out for a step.

Algorithmic bytes per key: a hit reads the 128-B digest line, its 8-B key and its D*4-B row (the
gather that follows the lookup); an inserted key adds the row write and the evicted row read
(D*4 each; no optimizer state in this run).  Fraction = bytes / time / 8 TB/s.
Not part of bench.py's line.  Usage: python tools/hybrid_table_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hugectr_amd.hybrid_table import HybridTable  # noqa: E402

PEAK = 8e12


def timed(fn, iters):
    fn(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tot = 0.0
    for i in range(iters):
        a.record()
        fn(i + 1)
        b.record()
        b.synchronize()
        tot += a.elapsed_time(b)
    return tot / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--tier", action="store_true", help="the host-memory tier legs only")
    args = ap.parse_args()
    C, N = args.capacity, args.batch
    if args.tier:
        return tier_legs(C, N, args.iters)
    for D in (16, 128):
        t = HybridTable(C, D, "0.5", 128)
        nxt = [0]

        def fresh(n):
            k = torch.arange(nxt[0], nxt[0] + n, dtype=torch.int64, device="cuda")
            nxt[0] += n
            return k

        # fill until every bucket is full (evictions start once a bucket is)
        for _ in range(64):
            if t.size() == t.capacity:
                break
            t.lookup_index(fresh(N), insert=True)
        assert t.size() == t.capacity, "the table did not fill"
        stored, _ = t.export()
        g = torch.Generator(device="cuda").manual_seed(0)

        def hits(n):
            return stored[torch.randint(0, stored.numel(), (n,), device="cuda", generator=g)]

        hit_sets = [hits(N) for _ in range(args.iters + 1)]
        res = {}
        res["find"] = timed(lambda i: t.find(hit_sets[i]), args.iters)
        # insert10 / insert100 change the table: the hit keys are re-drawn from the live ones
        stored, _ = t.export()
        mixes = [torch.cat([hits(N - N // 10), fresh(N // 10)]) for _ in range(args.iters + 1)]
        res["insert10"] = timed(lambda i: t.lookup_index(mixes[i], insert=True), args.iters)
        news = [fresh(N) for _ in range(args.iters + 1)]
        res["insert100"] = timed(lambda i: t.lookup_index(news[i], insert=True), args.iters)
        stored, _ = t.export()
        mixes = [torch.cat([hits(N - N // 10), fresh(N // 10)]) for _ in range(args.iters + 1)]
        res["insert10_filter"] = timed(
            lambda i: t.lookup_index(mixes[i], insert=True, admit=0.5), args.iters)
        stored, _ = t.export()
        t.lookup_index(hits(t.capacity // 10), insert=True)
        t0 = len(t.call_ns)
        matched = t.export_if(t0)[0].numel()
        res["export_if"] = timed(lambda i: t.export_if(t0), args.iters)
        hit_b = 128 + 8 + 4 * D
        ins_b = hit_b + 2 * 4 * D
        adm = (N // 10) // 2
        by = {"find": N * hit_b, "insert10": (N - N // 10) * hit_b + (N // 10) * ins_b,
              "insert100": N * ins_b,
              "insert10_filter": (N - adm) * hit_b + adm * ins_b,
              "export_if": t.capacity * 16 + matched * (8 + 8 + 8 + 8 + 4 * D)}
        for name, us in res.items():
            print(json.dumps({"case": name, "D": D, "capacity": t.capacity, "batch": N,
                              "us": round(us, 1), "alg_bytes": by[name],
                              "frac_of_8TBps": round(by[name] / (us * 1e-6) / PEAK, 4),
                              **({"matched": matched} if name == "export_if" else {})}))
        t.close()


def tier_legs(C, N, iters):
    import ctypes
    from hugectr_amd import _lib
    from hugectr_amd._lib import check, lib
    for D in (16, 128):
        t = HybridTable(C, D, "0.5", 128, hbm_slots=C // 2)
        nxt = [0]

        def fresh(n):
            k = torch.arange(nxt[0], nxt[0] + n, dtype=torch.int64, device="cuda")
            nxt[0] += n
            return k

        for _ in range(64):
            if t.size() == t.capacity:
                break
            t.lookup_index(fresh(N), insert=True)
        assert t.size() == t.capacity, "the table did not fill"
        stored, _ = t.export()
        g = torch.Generator(device="cuda").manual_seed(0)

        def hits(n):
            return stored[torch.randint(0, stored.numel(), (n,), device="cuda", generator=g)]

        res, host = {}, {}
        hit_sets = [hits(N) for _ in range(iters + 1)]
        res["tier_find_stage"] = timed(lambda i: t.lookup_index(hit_sets[i], insert=False), iters)
        host["tier_find_stage"] = N // 2 * D * 4
        stored, _ = t.export()
        mixes = [torch.cat([hits(N - N // 10), fresh(N // 10)]) for _ in range(iters + 1)]
        res["tier_insert10"] = timed(lambda i: t.lookup_index(mixes[i], insert=True), iters)
        # every host-resident position staged once, the new host rows written once before that
        host["tier_insert10"] = (N // 2 + (N // 10) // 2) * D * 4
        stored, _ = t.export()
        perm = stored[torch.randperm(stored.numel(), device="cuda", generator=g)[:N]]
        slots = t.find(perm)
        grads = torch.randn((N, D), device="cuda", generator=g)
        ro = torch.arange(N + 1, dtype=torch.int64, device="cuda")
        hp = dict(lr=0.01, beta1=0.9, beta2=0.999, epsilon=1e-7, momentum=0.0, scaler=1.0)
        for name, code, ns in (("tier_sgd", _lib.OPT_SGD, 0), ("tier_adam", _lib.OPT_ADAM, 2)):
            for j in range(ns):
                t.state_ptr(j)
            u = ctypes.c_void_p()
            check(lib.hctr_updater_create(2 * N, C // 2 + 2 * N, D, ctypes.byref(u)))
            res[name] = timed(lambda i: t.apply_update(u, ro, slots, grads, code, hp, i + 1),
                              iters)
            host[name] = N // 2 * D * 4 * (1 + ns) * 2
            lib.hctr_updater_destroy(u)
        for name, us in res.items():
            print(json.dumps({"case": name, "D": D, "capacity": t.capacity,
                              "hbm_slots": t.hbm_slots, "batch": N, "us": round(us, 1),
                              "host_link_bytes": host[name],
                              "host_GBps": round(host[name] / (us * 1e-6) / 1e9, 1),
                              "bound_us_at_51GBps": round(host[name] / 51e9 * 1e6, 1)}))
        t.close()


if __name__ == "__main__":
    main()
