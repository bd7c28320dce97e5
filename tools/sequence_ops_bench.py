"""Times hugectr_amd.matrix_multiply, reduce_mean and fused_reshape_concat (sequence_ops.hip) next to
torch.matmul, x.mean(axis, keepdim=True) and torch.cat + slicing on the same device: forward (no
gradient wanted), forward + backward through autograd, and the forward C entry point alone on
preallocated buffers (`kernel_fwd`).  From the latter the share of a peak on what the algorithm needs:
the 8 TB/s HBM peak on the bytes of inputs + outputs for the packed matmul body, reduce_mean and the
copy; the matrix peak (2500 TFLOP/s for fp16, 157.3 for fp32 operands) on 2 batch m n k for the MFMA
body.  Device events around batches of calls, medians over rounds, the paths alternating inside a
round.  One JSON line per (case, dtype); `ratio_*` = torch / own.  Below a few tens of microseconds a
figure is the launch rate, not the kernel.

    python tools/sequence_ops_bench.py [--rounds 7] [--calls 10]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hugectr_amd as ha  # noqa: E402
from hugectr_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from hugectr_amd.layers import _DT, _matmul_shape  # noqa: E402

HBM_PEAK_GBPS = 8000.0
MFMA_PEAK_TFLOPS = {torch.float16: 2500.0, torch.float32: 157.3}
B = 65536  # DIN's batch


def matmul_case(name, sa, sb):
    def make(dt):
        a, b = (torch.randn(s, device="cuda").to(dt).requires_grad_(True) for s in (sa, sb))
        batch, m, n, k, out = _matmul_shape(a, b)
        c = torch.empty(out, dtype=dt, device="cuda")
        kernel = lambda: check(lib.hctr_matmul_fwd(batch, m, n, k, ptr(a), ptr(b), ptr(c), _DT[dt],  # noqa: E731
                                                   stream_ptr()))
        packed = m * n + n * k + m * k <= 1024
        work = {"bytes": (a.numel() + b.numel() + c.numel()) * a.element_size()} if packed else \
            {"flops": 2 * batch * m * n * k}
        # (torch.matmul has no [m, n] x [n, g, h] form; none of the shapes here uses it)
        return [a, b], lambda: ha.matrix_multiply(a, b), lambda: torch.matmul(a, b), kernel, work
    return name, make


def reduce_mean_case(name, shape, axis):
    def make(dt):
        x = torch.randn(shape, device="cuda").to(dt).requires_grad_(True)
        outer = int(torch.tensor(shape[:axis]).prod()) if axis else 1
        inner = int(torch.tensor(shape[axis + 1:]).prod()) if axis + 1 < len(shape) else 1
        y = torch.empty(outer * inner, dtype=dt, device="cuda")
        kernel = lambda: check(lib.hctr_reduce_mean_fwd(outer, shape[axis], inner, ptr(x), ptr(y),  # noqa: E731
                                                        _DT[dt], stream_ptr()))
        return ([x], lambda: ha.reduce_mean(x, axis), lambda: x.mean(axis, keepdim=True), kernel,
                {"bytes": (x.numel() + y.numel()) * x.element_size()})
    return name, make


def frc_case(name, batch, slots, widths):
    def make(dt):
        xs = [torch.randn(batch, slots, w, device="cuda").to(dt).requires_grad_(True) for w in widths]
        W = sum(widths)
        item = torch.empty(batch * (slots - 1), W, dtype=dt, device="cuda")
        ad = torch.empty(batch, W, dtype=dt, device="cuda")
        ptrs = (ctypes.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
        ws = (ctypes.c_int * len(xs))(*widths)
        kernel = lambda: check(lib.hctr_fused_reshape_concat_fwd(batch, slots, len(xs), ptrs, ws,  # noqa: E731
                                                                 ptr(item), ptr(ad), _DT[dt], stream_ptr()))

        def ref():
            X = torch.cat(xs, dim=2)
            return X[:, :-1].reshape(-1, W), X[:, -1]
        return (xs, lambda: ha.fused_reshape_concat(xs), ref, kernel,
                {"bytes": 2 * batch * slots * W * xs[0].element_size()})
    return name, make


CASES = [matmul_case("matmul DIN 65536 x (1 x 10 x 36)", (B, 1, 10), (B, 10, 36)),
         matmul_case("matmul BST 1024 x 8 x (128 x 64 x 128)", (1024, 8, 128, 64), (1024, 8, 64, 128)),
         matmul_case("matmul 4096 x 4096 x 4096", (4096, 4096), (4096, 4096)),
         reduce_mean_case("reduce_mean [65536, 10, 36] axis 1", (B, 10, 36), 1),
         frc_case("fused_reshape_concat 2 x [65536, 11, 18]", B, 11, (18, 18))]


def time_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run(args, name, make, dt):
    leaves, own, ref, kernel, work = make(dt)
    outs = lambda r: r if isinstance(r, tuple) else (r,)  # noqa: E731
    tops = [torch.randn_like(t) for t in outs(own())]

    def fwd(f):
        with torch.no_grad():
            f()

    def both(f):
        torch.autograd.backward(outs(f()), tops)
        for t in leaves:
            t.grad = None

    with torch.no_grad():
        err = max((u.float() - v.float()).abs().max().item() for u, v in zip(outs(own()), outs(ref())))
    legs = {"own_fwd": lambda: fwd(own), "torch_fwd": lambda: fwd(ref),
            "own_fwd_bwd": lambda: both(own), "torch_fwd_bwd": lambda: both(ref), "kernel_fwd": kernel}
    for f in legs.values():  # warm-up: code objects, the allocator's blocks, the library's choice
        for _ in range(3):
            f()
    times = {n: [] for n in legs}
    for _ in range(args.rounds):
        for n, f in legs.items():
            times[n].append(time_ms(f, args.calls))
    med = {n + "_ms": round(statistics.median(t), 4) for n, t in times.items()}
    sec = med["kernel_fwd_ms"] * 1e-3
    share = {"hbm_frac_fwd": round(work["bytes"] / sec / 1e9 / HBM_PEAK_GBPS, 3)} if "bytes" in work else \
        {"tflops_fwd": round(work["flops"] / sec / 1e12, 1),
         "mfma_frac_fwd": round(work["flops"] / sec / 1e12 / MFMA_PEAK_TFLOPS[dt], 3)}
    print(json.dumps({
        "case": name, "dtype": str(dt).split(".")[1], **med,
        "spread_kernel_fwd_ms": [round(min(times["kernel_fwd"]), 4), round(max(times["kernel_fwd"]), 4)],
        "ratio_fwd": round(med["torch_fwd_ms"] / med["own_fwd_ms"], 3),
        "ratio_fwd_bwd": round(med["torch_fwd_bwd_ms"] / med["own_fwd_bwd_ms"], 3), **share,
        "max_abs_diff_vs_torch": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sequence_ops_bench needs the GPU"
    for name, make in CASES:
        for dt in (torch.float16, torch.float32):
            run(args, name, make, dt)


if __name__ == "__main__":
    main()
