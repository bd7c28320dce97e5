"""Evaluation metrics on one MI355X: hctr_metric_accumulate per batch of 65 536, the AUC finalise
(hctr_metric_auc) at N = 2^20, 2^24 and 89 137 319 samples (the Criteo-1TB evaluation set), and at
the same N the parent commit's get_eval_metrics() arithmetic -- `_auc` of hugectr.py on the fp32
scores and labels its eval() kept (fp64 copies, torch.sort, unique_consecutive, cumsum).  Times are
device events around work that ends in a synchronise; peak extra device memory is torch's allocator
peak over the call (inputs excluded).  One JSON line per measurement.

    python tools/metrics_bench.py [--sizes 1048576,16777216,89137319] [--reps 5]
"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hugectr_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from hugectr_amd.hugectr import _auc  # noqa: E402
from hugectr_amd.metrics import auc_from_words  # noqa: E402


def _time(fn, reps, warm=2):
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,16777216,89137319")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=65536)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs a GPU"
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)

    # accumulate: one batch of 65 536 per call, per score dtype
    Bn, cap = args.batch, args.batch * 64
    keys = torch.empty((1, cap), dtype=torch.int32, device=dev)
    labels = torch.empty((1, cap), dtype=torch.float32, device=dev)
    counters = torch.zeros(264, dtype=torch.int64, device=dev)
    tmp = torch.empty(lib.hctr_metric_accumulate_temp_bytes(), dtype=torch.uint8, device=dev)
    y = (torch.rand(Bn, 1, device=dev, generator=g) < 0.03).float()
    for name, code, dt in (("fp32", 0, torch.float32), ("fp16", 1, torch.float16),
                           ("bf16", 2, torch.bfloat16)):
        p = torch.rand(Bn, 1, device=dev, generator=g).to(dt)

        def acc():
            for i in range(64):
                check(lib.hctr_metric_accumulate(ptr(p), code, ptr(y), Bn, 1, ptr(keys), ptr(labels),
                                                 cap, i * Bn, ptr(counters), ptr(tmp), tmp.numel(),
                                                 stream_ptr()))
        med, lo, hi = _time(acc, args.reps)
        print(json.dumps({"what": "accumulate", "scores": name, "batch": Bn,
                          "us_per_batch": round(med / 64 * 1e3, 2),
                          "us_min_max": [round(lo / 64 * 1e3, 2), round(hi / 64 * 1e3, 2)],
                          "bytes_per_sample": p.element_size() + 4 + 8}), flush=True)
    del keys, labels

    for N in [int(s) for s in args.sizes.split(",")]:
        p = torch.rand(N, device=dev, generator=g)
        y = (torch.rand(N, device=dev, generator=g) < 0.03).float()
        k = torch.empty(N, dtype=torch.int32, device=dev)
        l = torch.empty(N, dtype=torch.float32, device=dev)
        for off in range(0, N, Bn * 16):  # fill the store through the product's own entry point
            n = min(Bn * 16, N - off)
            check(lib.hctr_metric_accumulate(ptr(p[off:off + n]), 0, ptr(y[off:off + n]), n, 1, ptr(k),
                                             ptr(l), N, off, ptr(counters), ptr(tmp), tmp.numel(),
                                             stream_ptr()))
        out = torch.zeros(3, dtype=torch.int64, device=dev)

        def fin():
            tb = lib.hctr_metric_auc_temp_bytes(N)
            t = torch.empty(tb, dtype=torch.uint8, device=dev)
            check(lib.hctr_metric_auc(ptr(t), tb, ptr(k), ptr(l), N, ptr(out), stream_ptr()))
            w = out.cpu().numpy()
            return auc_from_words(int(w[0]), int(w[1]), int(w[2]))

        def srt():  # the sort alone (four digit passes over 8 B pairs)
            check(lib.hctr_radix_sort_pairs_u32(ptr(st), sb, ptr(k), ptr(ko), ptr(l), ptr(vo), N, 32,
                                                stream_ptr()))

        new_auc, new_peak = _peak(fin)
        med, lo, hi = _time(fin, args.reps)
        sb = lib.hctr_radix_sort_temp_bytes(N)
        st = torch.empty(sb, dtype=torch.uint8, device=dev)
        ko, vo = torch.empty_like(k), torch.empty(N, dtype=torch.int32, device=dev)
        smed, _, _ = _time(srt, args.reps)
        del st, ko, vo
        rec = {"what": "finalise", "N": N, "auc": new_auc, "ms": round(med, 3),
               "ms_min_max": [round(lo, 3), round(hi, 3)], "sort_only_ms": round(smed, 3),
               "peak_extra_bytes_per_sample": round(new_peak / N, 2)}
        try:
            old_auc, old_peak = _peak(lambda: _auc(p, y))
            omed, olo, ohi = _time(lambda: _auc(p, y), args.reps, warm=1)
            rec.update(parent_auc=old_auc, parent_ms=round(omed, 3),
                       parent_ms_min_max=[round(olo, 3), round(ohi, 3)],
                       parent_peak_extra_bytes_per_sample=round(old_peak / N, 2),
                       auc_difference=abs(old_auc - new_auc))
        except torch.OutOfMemoryError as e:  # reported, not hidden
            rec.update(parent_error=str(e)[:120])
        print(json.dumps(rec), flush=True)
        del p, y, k, l


if __name__ == "__main__":
    main()
