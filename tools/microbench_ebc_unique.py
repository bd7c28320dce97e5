"""embedding_collection on N GPUs, CompressionStrategy.Reduction beside CompressionStrategy.Unique:
device-side time of every stage of ONE rank and the bytes it would put on the wire, measured on one
GPU.  All N ranks are built in this process (EmbeddingCollection.for_rank; the Unique set shares the
Reduction set's tables) so that rank 0 receives what its peers would really send; the collectives
are emulated by slicing and are NOT timed -- no collective with N > 1 has run in this repository, so
whether fewer bytes buy a shorter step on xGMI stays unmeasured.

Shapes: (a) Criteo-1TB one-hot, power-law keys alpha = 1.1; (b) the same with uniform keys (little
repetition: where Unique should lose); (c) one concat sequence lookup, hotness 50, a 10^6-row table.
hipEvent timing, 3 warm-up runs, median of 21 samples, a sample = a batch of back-to-back calls.

Usage: python tools/microbench_ebc_unique.py [--world 8] [--batch 65536] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hugectr_amd as ha  # noqa: E402
import hugectr_amd.hugectr as hugectr  # noqa: E402
from hugectr_amd import _lib  # noqa: E402
from microbench_embedding import CRITEO_1TB, powerlaw  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def timed(fn, runs=21, warm=3, inner=None):
    """median over `runs` samples of the time of one call, in microseconds; a sample brackets
    `inner` back-to-back calls with two events (a single call of a few microseconds is below what
    an event pair resolves) -- inner is sized from a first look so that a sample lasts >= ~2 ms"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()

    def sample(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    if inner is None:
        inner = int(min(64, max(1, 2000.0 / max(sample(2), 1.0))))
    return float(np.median([sample(inner) for _ in range(runs)]))


def build(world, tables, lookups, combiners, B, ev, dtype, hotness, batch_major):
    sets = {}
    for strategy in ("Reduction", "Unique"):
        cfg = ha.EmbeddingCollectionConfig()
        for l, t in enumerate(lookups):
            cfg.embedding_lookup(tables[t], f"in{l}", f"out{l}", combiners[l])
        names = [t.name for t in tables]
        if len(tables) == 1:  # one table: row-sharded over every rank
            sm = [names] * world
        else:                 # table t on rank t % world
            sm = [[n for i, n in enumerate(names) if i % world == g] for g in range(world)]
        cfg.shard(sm, [("mp", names)], [(getattr(hugectr.CompressionStrategy, strategy), names)])
        kw = dict(lr=0.01, optimizer=_lib.OPT_SGD, out_dtype=dtype, batch_major=batch_major,
                  max_hotness=max(hotness), hotness=hotness)
        base = sets.get("Reduction")
        sets[strategy] = [ha.EmbeddingCollection.for_rank(
            r, world, cfg, B, tables_from=base[r] if base else None, **kw) for r in range(world)]
    return sets


def run_shape(name, world, tables, lookups, combiners, keys, br, B, ev, dtype, hotness,
              batch_major=False):
    sets = build(world, tables, lookups, combiners, B, ev, dtype, hotness, batch_major)
    red, uq = sets["Reduction"], sets["Unique"]
    gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
    bpg, esz = B // world, torch.empty(0, dtype=dtype).element_size()
    r0, u0 = red[0], uq[0]
    res = {"shape": name, "keys": int(keys.size), "distinct_keys": int(np.unique(keys).size)}
    # ---- Reduction ----
    sends = [e.route_and_pool(gk, gbr) for e in red]
    recv = torch.cat([sends[s].view(world, es.n_local, bpg, ev)[0].reshape(-1, ev)
                      for s, es in enumerate(red) if es.n_local]).contiguous()
    out = r0.network_forward(recv)
    grad = torch.randn(out.shape, device="cuda").to(dtype)
    top = torch.randn((r0.nb, ev), device="cuda").to(dtype)
    t = {"owner (route + pool)": timed(lambda: r0.route_and_pool(gk, gbr)),
         "receiver network forward": timed(lambda: r0.network_forward(recv)),
         "receiver network backward": timed(lambda: r0.network_backward(grad)),
         "owner update": timed(lambda: r0.apply_gradients(top))}
    res["reduction_us"] = t
    res["reduction_bytes_out"] = {
        "forward": (world - 1) * r0.n_local * bpg * ev * esz,
        "backward": sum(r0.n_local_of[1:]) * bpg * ev * esz}
    # ---- Unique ----
    pk = [e.route_and_compress(gk, gbr) for e in uq]
    rows, ridx, lens, u_recv = [], [], [], []
    for s, es in enumerate(uq):
        p = pk[s]
        nbp = es.n_local * bpg
        rows.append(p["rows"][:p["u_counts"][0]])
        ridx.append(p["ridx"][:p["k_counts"][0]].clone())
        lens.append(p["lens"][:nbp])
        u_recv.append(p["u_counts"][0])
    rows, ridx, lens = torch.cat(rows).contiguous(), torch.cat(ridx), torch.cat(lens)
    u0.network_forward_unique(rows, ridx, lens, u_recv)
    n_send = sum(pk[0]["u_counts"])
    sums = torch.randn((n_send, ev), device="cuda")
    t = {"owner (route + plan + counts read + gather)": timed(lambda: u0.route_and_compress(gk, gbr)),
         "receiver network forward": timed(
             lambda: u0.network_forward_unique(rows, ridx, lens, u_recv)),
         "receiver network backward (row sums)": timed(lambda: u0.network_backward_unique(grad)),
         "owner update": timed(lambda: u0.apply_row_sums(sums))}
    res["unique_us"] = t
    # the receiver kernel alone: the ABI call on buffers prepared once (the stage above also builds
    # the bucket ranges, the row offsets, the one-hot word and the output tensor)
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    from hugectr_amd.embedding_collection import _DT
    rx = u0._rx
    one_hot = (lens == 1).all().to(torch.int32).view(1)
    kout = torch.empty_like(out)
    args = (u0.bpg, u0.L, ev, u0.max_shards, ptr(u0.d_src_blocks), ptr(u0.d_combiner),
            ptr(u0.counts), 1 if batch_major else 0, ptr(rx["range"]), ptr(rx["ridx"]),
            ptr(rx["r_off"]), ptr(u0.d_blk_src), ptr(one_hot), ptr(rx["rows"]), ptr(kout),
            _DT[dtype])
    res["unique_receiver_kernel_us"] = timed(
        lambda: check(lib.hctr_ebc_uniq_network_forward(*args, stream_ptr())))
    uc, kc = pk[0]["u_counts"], pk[0]["k_counts"]
    res["unique_bytes_out"] = {
        "forward": sum(uc[1:]) * ev * esz + sum(kc[1:]) * 4 + (world - 1) * u0.n_local * bpg * 8,
        "backward": sum(u_recv[1:]) * ev * 4}
    res["unique_rows"] = {"sent_distinct": int(sum(uc)), "sent_keys": int(sum(kc)),
                          "received_distinct": int(sum(u_recv)), "received_keys": int(ridx.numel())}
    # logical traffic of the receiver kernel: one row read per key, the indices, the output
    moved = ridx.numel() * (ev * esz + 4) + u0.L * bpg * ev * esz
    res["unique_receiver_GBps"] = moved / res["unique_receiver_kernel_us"] / 1e3
    del sets, red, uq
    torch.cuda.empty_cache()
    return res


def fmt(res):
    lines = [f"== {res['shape']}: {res['keys']} keys, {res['distinct_keys']} distinct =="]
    for k in ("reduction", "unique"):
        lines.append(f"  {k} (stage = the Python stage method: kernels + its torch glue):")
        for stage, us in res[f"{k}_us"].items():
            lines.append(f"    {stage:<48s} {us:10.1f} us")
        b = res[f"{k}_bytes_out"]
        lines.append(f"    bytes out of rank 0: forward {b['forward']:>12d}   backward {b['backward']:>12d}")
    lines.append(f"  unique rows: {res['unique_rows']}")
    g = res["unique_receiver_GBps"]
    lines.append(f"  unique receiver kernel alone (hctr_ebc_uniq_network_forward, buffers prepared): "
                 f"{res['unique_receiver_kernel_us']:.1f} us")
    lines.append(f"  unique receiver kernel: {g:.0f} GB/s of row reads + indices + output "
                 f"({100 * g / HBM_PEAK_GBPS:.1f} % of the {HBM_PEAK_GBPS / 1e3:.0f} TB/s HBM peak; "
                 "repeated rows come out of L2)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--batch", type=int, default=65536, help="global batch")
    ap.add_argument("--ev", type=int, default=128)
    ap.add_argument("--max-rows", type=int, default=10_000_000,
                    help="rows per table are capped here (all N ranks' shards live on this GPU)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, B, ev, dtype = a.world, a.batch, a.ev, torch.float16
    rng = np.random.default_rng(3)
    sizes = [min(v, a.max_rows) for v in CRITEO_1TB]
    S = len(sizes)
    out = [f"# world {W}, global batch {B}, ev {ev}, fp16 vectors, tables capped at {a.max_rows} rows; "
           "rank 0's stages; the collectives are emulated by slicing and NOT timed"]
    for label, alpha in (("(a) Criteo-1TB one-hot, power-law alpha 1.1", 1.1),
                         ("(b) Criteo-1TB one-hot, uniform keys", 0.0)):
        tables = [ha.EmbeddingTableConfig(f"t{i}", v, ev) for i, v in enumerate(sizes)]
        cols = [powerlaw(rng, B, v, alpha) if alpha > 0 else rng.integers(0, v, B) for v in sizes]
        keys = np.concatenate(cols).astype(np.int64)      # feature-major: lookup * B + b
        br = np.arange(S * B + 1, dtype=np.int64)
        res = run_shape(label, W, tables, list(range(S)), ["sum"] * S, keys, br, B, ev, dtype,
                        [1] * S)
        out.append(fmt(res))
        print(out[-1], flush=True)
    Bs = max(B // 16, W)
    tables = [ha.EmbeddingTableConfig("seq", 1_000_000, ev)]
    keys = powerlaw(rng, Bs * 50, 1_000_000, 1.1).astype(np.int64)
    br = np.arange(0, Bs * 50 + 1, 50, dtype=np.int64)
    res = run_shape(f"(c) concat sequence lookup, hotness 50, 10^6 rows, batch {Bs}", W, tables, [0],
                    ["concat"], keys, br, Bs, ev, dtype, [50], batch_major=True)
    out.append(fmt(res))
    print(out[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
