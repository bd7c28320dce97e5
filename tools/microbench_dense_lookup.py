"""Micro-benchmark of the SOK dense lookups (csrc/dense_lookup.hip), old code against new from the
same build.  One leg per invocation (run each under its own time limit):

  --leg group     sok.group_lookup of 26 tables (the Criteo-1TB slot sizes bench.py uses, dim 128),
                  65 536 and 1 024 int64 keys per table, power-law (alpha 1.1, bench.py's generator)
                  and uniform keys, fp32 and fp16 output, against what the library offered before:
                  26 calls of sok._gather (hctr_forward_pool with an arange row-offset array), plus
                  26 .half() casts for the fp16 result.
  --leg all2all   sok.all2all_dense_embedding at one rank, 8192 x 26 keys, dim 128, against
                  sok.lookup_sparse with every row length 1 on the same variable: forward +
                  backward + OptimizerWrapper.step.
  --leg one_call  a single group_lookup call of 26 tables and nothing else timed: the run to put
                  under `rocprofv3 --kernel-trace --stats` (one copy kernel must show).

The two sides alternate inside the process, five repeats each, device events around blocks of
--iters calls after a warm-up of both.  "At least as fast" = the new side's median is not above the
old side's median plus the old side's own spread (max - min of its five repeats); both are printed.
Share of peak: algorithmic bytes n * (8 + 4 * dim + out_bytes * dim) (key, row read, row written)
over time over the 8 TB/s HBM peak -- algorithmic, not measured traffic: repeated keys hit caches.
Not part of bench.py's line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CRITEO_1TB, gen_keys  # noqa: E402
from hugectr_amd import sok  # noqa: E402

PEAK = 8e12
REPEATS = 5


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def alternate(old, new, iters):
    for _ in range(3):
        old()
        new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(REPEATS):
        t_old.append(block_us(old, iters))
        t_new.append(block_us(new, iters))
    return t_old, t_new


def report(name, t_old, t_new, extra):
    mo, mn = statistics.median(t_old), statistics.median(t_new)
    spread = max(t_old) - min(t_old)
    rec = dict(case=name, old_us=[round(x, 2) for x in t_old], new_us=[round(x, 2) for x in t_new],
               old_median_us=round(mo, 2), new_median_us=round(mn, 2),
               old_spread_us=round(spread, 2), speedup=round(mo / mn, 3),
               new_at_least_as_fast=bool(mn <= mo + spread), **extra)
    print(json.dumps(rec), flush=True)


def tables(sizes, D, dev):
    return [torch.rand((v, D), device=dev, dtype=torch.float32) for v in sizes]


def per_table_keys(gen, n, sizes, alpha, dev):
    """[26] int64 [n] keys, each table's in [0, its rows)"""
    flat = gen_keys(gen, n, sizes, alpha, dev).view(n, len(sizes))
    offs = torch.tensor([0] + list(sizes[:-1]), device=dev).cumsum(0)
    return [(flat[:, s] - offs[s]).contiguous() for s in range(len(sizes))]


def leg_group(a, dev):
    sizes = [max(1, int(v * a.table_scale)) for v in CRITEO_1TB]
    D = a.dim
    tabs = tables(sizes, D, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    for n in a.keys:
        iters = a.iters if n > 4096 else a.iters * 10
        for alpha, dist in ((1.1, "powerlaw"), (0.0, "uniform")):
            keys = per_table_keys(gen, n, sizes, alpha, dev)
            for dt, ob in ((torch.float32, 4), (torch.float16, 2)):
                def old():
                    outs = [sok._gather(t, k, D) for t, k in zip(tabs, keys)]
                    return outs if dt == torch.float32 else [o.half() for o in outs]

                def new():
                    return sok.group_lookup(tabs, keys, dtype=dt)

                for x, y in zip(old(), new()):   # the same result, bit for bit
                    assert torch.equal(x, y)
                t_old, t_new = alternate(old, new, iters)
                nn = n * len(sizes)
                algo = nn * (8 + 4 * D + ob * D)
                mn = statistics.median(t_new)
                mo = statistics.median(t_old)
                report(f"group_lookup 26 x {n} keys {dist} {str(dt)[6:]}", t_old, t_new,
                       dict(algorithmic_bytes=algo,
                            new_share_of_8TBs_algorithmic=round(algo / (mn * 1e-6) / PEAK, 3),
                            old_share_of_8TBs_algorithmic=round(algo / (mo * 1e-6) / PEAK, 3)))


def leg_all2all(a, dev):
    sok.init()
    D, rows, n = a.dim, a.rows, a.keys[0] // 8 * 26
    w = torch.rand((rows, D), dtype=torch.float32)
    v_old, v_new = sok.Variable(w), sok.Variable(w)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    keys = torch.randint(0, rows, (n,), device=dev, generator=gen)
    ones = torch.ones_like(keys)
    opt = sok.OptimizerWrapper("sgd", lr=0.01)

    def old():
        sok.lookup_sparse(v_old, sok.Ragged(keys, ones), combiners="sum").sum().backward()
        opt.step([v_old])

    def new():
        sok.all2all_dense_embedding(v_new, keys).sum().backward()
        opt.step([v_new])

    t_old, t_new = alternate(old, new, a.iters)
    assert torch.allclose(v_old.weight, v_new.weight, rtol=1e-5, atol=1e-6)
    report(f"all2all_dense_embedding vs lookup_sparse(lengths 1), {n} keys, 1 rank, "
           "fwd + bwd + sgd step", t_old, t_new, {})


def leg_one_call(a, dev):
    sizes = [max(1, int(v * a.table_scale)) for v in CRITEO_1TB]
    tabs = tables(sizes, a.dim, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    keys = per_table_keys(gen, a.keys[0], sizes, 1.1, dev)
    torch.cuda.synchronize()
    outs = sok.group_lookup(tabs, keys)
    torch.cuda.synchronize()
    print(json.dumps(dict(case="one group_lookup call", tables=len(outs),
                          rows=int(sum(o.shape[0] for o in outs)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["group", "all2all", "one_call"], required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--table-scale", type=float, default=1.0,
                    help="scales the Criteo-1TB slot sizes (1.0: 188 M rows, 96 GB at dim 128)")
    ap.add_argument("--keys", type=lambda s: [int(x) for x in s.split(",")], default=[65536, 1024],
                    help="keys per table of the group legs (all2all: the first / 8 per table)")
    ap.add_argument("--rows", type=int, default=1 << 20, help="rows of the all2all leg's variable")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on a CPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print(json.dumps(dict(leg=a.leg, device=torch.cuda.get_device_name(0), iters=a.iters,
                          repeats=REPEATS, dim=a.dim, table_scale=a.table_scale)), flush=True)
    {"group": leg_group, "all2all": leg_all2all, "one_call": leg_one_call}[a.leg](a, dev)


if __name__ == "__main__":
    main()
