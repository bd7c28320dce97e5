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

Growth (--grow, hctr_lru_create_growing; D = 128, S = 128, max_load_factor 0.5):
  grow_2^k   the call that doubles a half-full table from 2^k slots, k = 20 .. 23, untiered and
             with an HBM budget of half the largest capacity (the table turns tiered at the last
             doubling), beside a call of the same 1024 new keys that does not double (grow_base:
             the probe, the read-back and the insert).  A warm-up table goes through the same
             doublings first.  copy_bytes: the old arrays copied into the new (keys, scores,
             digests, the HBM slot rows), read and written; clear_bytes: the new slots' keys,
             scores, digests and HBM rows, written; move_bytes: the moved rows, read and written
             (about half the occupied slots move).  A new host part is cleared and filled by the
             host and is not in these bytes
  grown_insert10 / made_insert10   insert10 on a table grown to 2^24 and on one created there,
             both full, alternated
  below_insert10 / at_insert10     insert10 on a half-full table of 2^24 slots that could still
             grow (it reads occ and m back every call) and on one created at 2^24 with the same
             keys, alternated: the difference is what the read-back costs

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
    ap.add_argument("--grow", action="store_true", help="the growth legs only")
    ap.add_argument("--init-capacity", type=int, default=1 << 20, help="where --grow starts")
    args = ap.parse_args()
    C, N = args.capacity, args.batch
    if args.tier:
        return tier_legs(C, N, args.iters)
    if args.grow:
        return grow_legs(C, N, args.iters, args.init_capacity)
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


def once(fn):
    """one call between device events, in us"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def grow_legs(C, N, iters, C0):
    D, S = 128, 128
    nxt = [0]

    def fresh(n):
        k = torch.arange(nxt[0], nxt[0] + n, dtype=torch.int64, device="cuda")
        nxt[0] += n
        return k

    def fill(t, upto):
        while t.size() < upto:
            t.lookup_index(fresh(min(N, upto - t.size())), insert=True)

    grown = None
    for hb in (None, C // 2):
        for measured in (False, True):
            t = HybridTable(C, D, "0.5", S, hbm_slots=hb, init_capacity=C0)
            while t.current_capacity < C:
                c = t.current_capacity
                # half full: occ + m = c / 2 does not double, one more key does
                fill(t, c // 2 - 2048)
                base = once(lambda: t.lookup_index(fresh(1024), insert=True))
                fill(t, c // 2)
                assert t.current_capacity == c
                occ, h = t.size(), t.hbm_slots
                us = once(lambda: t.lookup_index(fresh(1024), insert=True))
                assert t.current_capacity == 2 * c, "the call did not double the table"
                if measured:
                    copy_b = (c * 17 + h * D * 4) * 2
                    clear_b = c * 17 + (t.hbm_slots - h) * D * 4
                    move_b = (occ // 2) * D * 4 * 2
                    print(json.dumps({
                        "case": f"grow_2^{c.bit_length() - 1}", "D": D, "hbm_budget": hb,
                        "occupied": occ, "us": round(us, 1), "grow_base_us": round(base, 1),
                        "hbm_slots_after": t.hbm_slots, "copy_bytes": copy_b,
                        "clear_bytes": clear_b, "move_bytes": move_b,
                        "GBps": round((copy_b + clear_b + move_b) / (us * 1e-6) / 1e9, 1)}))
            if measured and hb is None:
                grown = t
            else:
                t.close()
    # a grown table beside one created at C, both full
    made = HybridTable(C, D, "0.5", S)
    pairs = [("grown_insert10", grown), ("made_insert10", made)]
    for _, t in pairs:
        for _ in range(64):
            if t.size() == t.capacity:
                break
            t.lookup_index(fresh(N), insert=True)
        assert t.size() == t.capacity, "the table did not fill"
    insert10_pair(pairs, fresh, N, iters, D)
    grown.close()
    made.close()
    # the same keys in a table that may still grow (occ + m stays below L * C) and in one that may not
    below = HybridTable(2 * C, D, "0.5", S, init_capacity=C, max_load_factor=1.0)
    at = HybridTable(C, D, "0.5", S)
    pairs = [("below_insert10", below), ("at_insert10", at)]
    first = nxt[0]
    for _, t in pairs:
        nxt[0] = first
        fill(t, C // 2)
    insert10_pair(pairs, fresh, N, iters, D)
    assert below.current_capacity == C and below.doublings == 0
    below.close()
    at.close()


def insert10_pair(pairs, fresh, N, iters, D):
    """insert10 on the tables of `pairs`, one call each in turn; every table gets the same share of
    hits (drawn from its own keys) and its own fresh keys"""
    g = torch.Generator(device="cuda").manual_seed(0)
    tot = {name: 0.0 for name, _ in pairs}
    for i in range(iters + 1):
        for name, t in pairs:
            stored, _ = t.export()
            hit = stored[torch.randint(0, stored.numel(), (N - N // 10,), device="cuda",
                                       generator=g)]
            mix = torch.cat([hit, fresh(N // 10)])
            del stored
            us = once(lambda: t.lookup_index(mix, insert=True))
            if i:
                tot[name] += us
    for name, t in pairs:
        print(json.dumps({"case": name, "D": D, "capacity": t.capacity,
                          "current_capacity": t.current_capacity, "size": t.size(), "batch": N,
                          "us": round(tot[name] / iters, 1)}))


if __name__ == "__main__":
    main()
