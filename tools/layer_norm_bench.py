"""Times hugectr_amd.layer_norm (layer_norm.hip: residual add + layer norm in one kernel each way)
next to torch.nn.functional.layer_norm(a + b, ...) on the same device, forward (no gradient wanted)
and forward + backward through autograd, and the two C entry points alone on preallocated buffers
(`kernel_*`: the forward with statistics, the backward with its finish launch).  From the latter the
share of the 8 TB/s HBM peak on the bytes the algorithm needs: forward (2 or 3) streams of rows x
hidden elements + 8 bytes of statistics a row, backward (3 or 4) streams + the statistics.  Device
events around batches of calls, medians over rounds, the paths alternating inside a round.  One JSON
line per (rows, hidden, dtype, residual); `ratio_*` = torch / own.  Below a few tens of microseconds a
figure is the launch rate, not the kernel.

    python tools/layer_norm_bench.py [--rounds 7] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hugectr_amd as ha  # noqa: E402
from hugectr_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from hugectr_amd.layers import _DT  # noqa: E402

HBM_PEAK_GBPS = 8000.0
ROWS = (65536 * 10, 1024 * 128)  # BST's batch x sequence, and a batch of 1024 x 128 positions
HIDDEN = (16, 64, 128, 1024)
EPS = 1e-5


def direct(x, res, gamma, beta, top):
    """the two entry points on preallocated buffers -> (forward, backward)"""
    rows, hidden = x.shape
    y, dz = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    scratch = torch.empty(lib.hctr_layer_norm_bwd_scratch_bytes(rows, hidden) // 4,
                          dtype=torch.float32, device=x.device)

    def fwd():
        check(lib.hctr_layer_norm_fwd(rows, hidden, ptr(x), ptr(res), ptr(gamma), ptr(beta), EPS,
                                      ptr(y), ptr(stats), _DT[x.dtype], stream_ptr()))

    def bwd():
        check(lib.hctr_layer_norm_bwd(rows, hidden, ptr(x), ptr(res), ptr(gamma), ptr(stats),
                                      ptr(top), ptr(dz), ptr(dgamma), ptr(dbeta), ptr(scratch),
                                      _DT[x.dtype], stream_ptr()))
    return fwd, bwd


def time_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "layer_norm_bench needs the GPU"
    for rows in ROWS:
        for hidden in HIDDEN:
            for dt in (torch.float16, torch.float32):
                for with_res in (False, True):
                    run(args, rows, hidden, dt, with_res)


def run(args, rows, hidden, dt, with_res):
    x, top = (torch.randn(rows, hidden, device="cuda").to(dt) for _ in range(2))
    res = torch.randn(rows, hidden, device="cuda").to(dt) if with_res else None
    gamma = (1 + 0.5 * torch.randn(hidden, device="cuda")).requires_grad_(True)
    beta = torch.randn(hidden, device="cuda").requires_grad_(True)
    leaves = [t.requires_grad_(True) for t in (x, res) if t is not None] + [gamma, beta]

    def fwd(f):
        with torch.no_grad():
            f()

    def both(f):
        f().backward(top)
        for t in leaves:
            t.grad = None

    own = lambda: ha.layer_norm(x, gamma, beta, EPS, res)  # noqa: E731
    # (torch's layer_norm wants weights of the input's dtype: the cast is part of its recipe)
    ref = lambda: torch.nn.functional.layer_norm(  # noqa: E731
        x if res is None else x + res, (hidden,), gamma.to(dt), beta.to(dt), EPS)
    err = (own().float() - ref().float()).abs().max().item()
    k_fwd, k_bwd = direct(x.detach(), None if res is None else res.detach(), gamma.detach(),
                          beta.detach(), top)
    legs = {"own_fwd": lambda: fwd(own), "torch_fwd": lambda: fwd(ref),
            "own_fwd_bwd": lambda: both(own), "torch_fwd_bwd": lambda: both(ref),
            "kernel_fwd": k_fwd, "kernel_bwd": k_bwd}
    for f in legs.values():  # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            f()
    times = {n: [] for n in legs}
    for _ in range(args.rounds):
        for n, f in legs.items():
            times[n].append(time_ms(f, args.calls))
    med = {n + "_ms": round(statistics.median(t), 4) for n, t in times.items()}
    size, streams = x.element_size(), 3 if with_res else 2
    fwd_bytes = streams * rows * hidden * size + 8 * rows
    bwd_bytes = (streams + 1) * rows * hidden * size + 8 * rows
    print(json.dumps({
        "rows": rows, "hidden": hidden, "dtype": str(dt).split(".")[1], "residual": with_res, **med,
        "spread_kernel_fwd_ms": [round(min(times["kernel_fwd"]), 4), round(max(times["kernel_fwd"]), 4)],
        "ratio_fwd": round(med["torch_fwd_ms"] / med["own_fwd_ms"], 3),
        "ratio_fwd_bwd": round(med["torch_fwd_bwd_ms"] / med["own_fwd_bwd_ms"], 3),
        "hbm_frac_fwd": round(fwd_bytes / (med["kernel_fwd_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 3),
        "hbm_frac_bwd": round(bwd_bytes / (med["kernel_bwd_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 3),
        "max_abs_diff_vs_torch": err}), flush=True)


if __name__ == "__main__":
    main()
