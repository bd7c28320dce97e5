"""Dense Ftrl: what the flat launch costs next to a copy of its traffic, and what a Ftrl model's
step costs next to the same model on SGD (DESIGN.md §3 "Dense-tower glue").

  python tools/dense_ftrl_bench.py                   # both parts
  python tools/dense_ftrl_bench.py --part kernel     # hctr_ftrl_shadow / a copy of the same traffic
  python tools/dense_ftrl_bench.py --part model      # Model.train() on Ftrl / on SGD

kernel: one process, every launch timed with its own pair of events, `--launches` (>= 100) timed
launches after `--warm` untimed ones, the median.  The launch reads w, z, n, g and writes w, z, n
(28 B per element) and, with the 16-bit copy, 2 B more; the copy next to it is a device-to-device
copy of HALF that many bytes, which reads and writes the same traffic.  Sizes: the parameter count
of the DLRM tower bench.py trains (flattened as FusedMLP.flatten() lays it out) and 2^24.

model: the DLRM of bench.py's embedding_collection leg (static tables, use_mixed_precision, batches
resident in HBM) built once on SGD and once on Ftrl, Model.train() per step.  The tables are scaled
down (--table-scale): the sparse Ftrl keeps two state arrays per table.

Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hugectr_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402


def timed_us(fn, launches, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(t), t[0], t[-1]


def tower_elems():
    """the flat size of the DLRM tower of bench.py (every tensor padded to 4 elements)"""
    import bench
    D, S = 128, len(bench.CRITEO_1TB)
    tot = 0
    for dims in ([bench.DENSE_DIM] + bench.BOTTOM, [D + (S + 1) * S // 2 + 1] + bench.TOP):
        for i, o in zip(dims[:-1], dims[1:]):
            tot += (i * o + 3) // 4 * 4 + (o + 3) // 4 * 4
    return tot


def kernel_part(a):
    for name, n in (("dlrm_tower", tower_elems()), ("2^24", 1 << 24)):
        w = torch.rand(n, device="cuda") * 0.2 - 0.1
        z, acc = torch.zeros_like(w), torch.zeros_like(w)
        g = torch.randn(n, device="cuda") * 0.1
        w16 = torch.zeros(n, dtype=torch.float16, device="cuda")
        for shadow in (None, w16):
            def step():
                check(lib.hctr_ftrl_shadow(n, 0.05, 0.9, 0.1, 0.1, 1.0, ptr(w), ptr(z), ptr(acc),
                                           ptr(g), ptr(shadow), 1, stream_ptr()))
            per = 28 if shadow is None else 30
            src = torch.empty(n * per // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            k_us, k_lo, k_hi = timed_us(step, a.launches, a.warm)
            c_us, c_lo, c_hi = timed_us(lambda: dst.copy_(src), a.launches, a.warm)
            print(json.dumps({
                "what": "hctr_ftrl_shadow", "size": name, "elements": n,
                "w16": shadow is not None, "bytes_per_element": per,
                "launch_us_median": round(k_us, 2), "launch_us_min_max": [round(k_lo, 2), round(k_hi, 2)],
                "copy_same_traffic_us_median": round(c_us, 2),
                "copy_us_min_max": [round(c_lo, 2), round(c_hi, 2)],
                "launch_over_copy": round(k_us / c_us, 2),
                "launch_GBps": round(n * per / k_us / 1e3, 1), "launches": a.launches}), flush=True)


def build_model(a, optimizer_type, batches):
    import bench
    import hugectr_amd.hugectr as hugectr
    sizes = [max(1, int(v * a.table_scale)) for v in bench.CRITEO_1TB]
    S, B = len(sizes), a.batch
    solver = hugectr.CreateSolver(max_eval_batches=1, batchsize_eval=B, batchsize=B, lr=0.01,
                                  vvgpu=[[0]], repeat_dataset=True, i64_input_key=True,
                                  use_mixed_precision=True, scaler=1024.0)
    kw = dict(update_type=hugectr.Update_t.Global, beta=0.9, lambda1=1e-4, lambda2=0.1) \
        if optimizer_type == hugectr.Optimizer_t.Ftrl else \
        dict(update_type=hugectr.Update_t.Local, atomic_update=True)
    opt = hugectr.CreateOptimizer(optimizer_type=optimizer_type, **kw)
    reader = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet,
                                      source=["(batches resident in HBM)"], eval_source="",
                                      check_type=hugectr.Check_t.Non)
    m = hugectr.Model(solver, reader, opt)
    m.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=bench.DENSE_DIM,
                        dense_name="dense", data_reader_sparse_param_array=[
                            hugectr.DataReaderSparseParam(f"data{i}", 1, True, 1)
                            for i in range(S)]))
    names = [str(i) for i in range(S)]
    tables = [hugectr.EmbeddingTableConfig(name=names[i], max_vocabulary_size=v, ev_size=a.dim)
              for i, v in enumerate(sizes)]
    ebc = hugectr.EmbeddingCollectionConfig(use_exclusive_keys=True)
    ebc.embedding_lookup(table_config=tables, bottom_name=[f"data{i}" for i in range(S)],
                         top_name="sparse_embedding", combiner=["concat"] * S)
    ebc.shard(shard_matrix=[names], shard_strategy=[("mp", names)])
    m.add(ebc)
    L, T, A = hugectr.DenseLayer, hugectr.Layer_t, hugectr.Activation_t
    m.add(L(layer_type=T.MLP, bottom_names=["dense"], top_names=["mlp1"],
            num_outputs=bench.BOTTOM[:-1] + [a.dim], act_type=A.Relu))
    m.add(L(layer_type=T.Reshape, bottom_names=["sparse_embedding"],
            top_names=["sparse_embedding1"], shape=[-1, S, a.dim]))
    m.add(L(layer_type=T.Interaction, bottom_names=["mlp1", "sparse_embedding1"],
            top_names=["interaction1"]))
    m.add(L(layer_type=T.MLP, bottom_names=["interaction1"], top_names=["mlp2"],
            num_outputs=bench.TOP, activations=[A.Relu] * (len(bench.TOP) - 1) + [A.Non]))
    m.add(L(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["mlp2", "label"],
            top_names=["loss"]))
    m.reader_override = bench._CycleReader(batches)
    m.compile()
    return m


def model_part(a):
    import hugectr_amd.hugectr as hugectr
    import bench
    sizes = [max(1, int(v * a.table_scale)) for v in bench.CRITEO_1TB]
    S, B = len(sizes), a.batch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    ro = torch.arange(B + 1, dtype=torch.int64, device="cuda")
    batches = []
    for _ in range(a.warm_steps + a.steps):
        keys = [(torch.rand(B, device="cuda", generator=gen) * v).to(torch.int64).clamp_(0, v - 1)
                for v in sizes]
        batches.append({"dense": torch.rand((B, bench.DENSE_DIM), device="cuda", generator=gen),
                        "label": (torch.rand((B, 1), device="cuda", generator=gen) < 0.5).float(),
                        "sparse": {f"data{i}": (ro, keys[i]) for i in range(S)}})
    out = {}
    for name, t in (("SGD", hugectr.Optimizer_t.SGD), ("Ftrl", hugectr.Optimizer_t.Ftrl)):
        m = build_model(a, t, batches)
        assert m._flat_mlps, "the flat dense path is what is measured"
        for _ in range(a.warm_steps):
            m.train()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            m.train()
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) / a.steps
        del m
        torch.cuda.empty_cache()
    print(json.dumps({"what": "Model.train() per step, DLRM on static embedding_collection tables",
                      "batch": B, "dim": a.dim, "table_scale": a.table_scale, "steps": a.steps,
                      "sgd_ms": round(out["SGD"], 4), "ftrl_ms": round(out["Ftrl"], 4),
                      "ftrl_over_sgd": round(out["Ftrl"] / out["SGD"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["both", "kernel", "model"], default="both")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--table-scale", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warm-steps", type=int, default=8)
    a = ap.parse_args()
    assert a.launches >= 100
    torch.cuda.set_device(0)
    if a.part in ("both", "kernel"):
        kernel_part(a)
    if a.part in ("both", "model"):
        model_part(a)


if __name__ == "__main__":
    main()
