"""Times hugectr_amd.batch_norm and hugectr_amd.prelu_dice (batch_norm.hip: a column reduction over row
slabs + a streaming kernel, each way) next to torch on the same device: torch.nn.functional.batch_norm
in training mode, and for Dice the torch composition of the forward formula with the statistics
detached (the reference's diagonal gradient).  Forward (no gradient wanted) and forward + backward
through autograd, and the C entry points alone on preallocated buffers (`kernel_*`).  From the latter
the share of the 8 TB/s HBM peak on the COMPULSORY bytes: forward x read once and y written once,
backward x and dy read once and dx written once -- the two-pass kernels read x (and dy) twice, so
without cache residency they cannot exceed 2/3 forward and 3/5 in the BatchNorm backward.  Device
events around batches of calls, medians over rounds, the paths alternating inside a round.  One JSON
line per (op, rows, n, dtype); `ratio_*` = torch / own, below 1 where the HIP path is the slower one.

    python tools/batch_norm_bench.py [--rounds 7] [--calls 10]
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
ROWS = (65536, 65536 * 10)  # a DIN batch, and BST's batch x sequence
COLS = (64, 128, 256, 1024)
EPS, DICE_EPS, ALPHA = 1e-5, 1e-8, 0.2


def direct(op, x, gamma, beta, top):
    """the entry points on preallocated buffers -> (forward, backward)"""
    rows, n = x.shape
    y, dx = torch.empty_like(x), torch.empty_like(x)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=x.device)  # noqa: E731
    save, dgamma, dbeta, rm, rv = f32(2, n), f32(n), f32(n), f32(n).zero_(), f32(n).fill_(1)
    scratch = f32(lib.hctr_col_stats_scratch_bytes(rows, n) // 4)
    dt = _DT[x.dtype]
    if op == "batch_norm":
        return (lambda: check(lib.hctr_batch_norm_fwd(rows, n, ptr(x), ptr(gamma), ptr(beta), 1.0, EPS,
                                                      ptr(rm), ptr(rv), ptr(y), ptr(save), ptr(scratch),
                                                      1, dt, stream_ptr())),
                lambda: check(lib.hctr_batch_norm_bwd(rows, n, ptr(x), ptr(gamma), ptr(save), ptr(top),
                                                      ptr(dx), ptr(dgamma), ptr(dbeta), ptr(scratch), dt,
                                                      stream_ptr())))
    return (lambda: check(lib.hctr_prelu_dice_fwd(rows, n, ptr(x), ALPHA, DICE_EPS, ptr(y), ptr(save),
                                                  ptr(scratch), dt, stream_ptr())),
            lambda: check(lib.hctr_prelu_dice_bwd(rows, n, ptr(x), ptr(save), ALPHA, DICE_EPS, ptr(top),
                                                  ptr(dx), dt, stream_ptr())))


def torch_dice(x):
    with torch.no_grad():
        var, mean = torch.var_mean(x.float(), 0, unbiased=False)
        mean, rstd = mean.to(x.dtype), torch.rsqrt(var + DICE_EPS).to(x.dtype)
    p = torch.sigmoid((x - mean) * rstd)
    return p * x + (1 - p) * ALPHA * x


def time_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run(args, op, rows, n, dt):
    x = torch.randn(rows, n, device="cuda").to(dt).requires_grad_(True)
    top = torch.randn(rows, n, device="cuda").to(dt)
    gamma = (1 + 0.5 * torch.randn(n, device="cuda")).requires_grad_(True)
    beta = torch.randn(n, device="cuda").requires_grad_(True)
    rm, rv = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
    leaves = [x, gamma, beta]

    def fwd(f):
        with torch.no_grad():
            f()

    def both(f):
        f().backward(top)
        for t in leaves:
            t.grad = None

    if op == "batch_norm":
        own = lambda: ha.batch_norm(x, gamma, beta, rm, rv, True, 1.0, EPS)  # noqa: E731
        ref = lambda: torch.nn.functional.batch_norm(x, rm, rv, gamma, beta, True, 1.0, EPS)  # noqa: E731
    else:
        own = lambda: ha.prelu_dice(x, ALPHA, DICE_EPS)  # noqa: E731
        ref = lambda: torch_dice(x)  # noqa: E731
    err = (own().float() - ref().float()).abs().max().item()
    k_fwd, k_bwd = direct(op, x.detach(), gamma.detach(), beta.detach(), top)
    legs = {"own_fwd": lambda: fwd(own), "torch_fwd": lambda: fwd(ref),
            "own_fwd_bwd": lambda: both(own), "torch_fwd_bwd": lambda: both(ref),
            "kernel_fwd": k_fwd, "kernel_bwd": k_bwd}
    for f in legs.values():  # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            f()
    times = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, f in legs.items():
            times[name].append(time_ms(f, args.calls))
    med = {name + "_ms": round(statistics.median(t), 4) for name, t in times.items()}
    stream = rows * n * x.element_size()
    share = lambda streams, ms: round(streams * stream / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 3)  # noqa: E731
    print(json.dumps({
        "op": op, "rows": rows, "n": n, "dtype": str(dt).split(".")[1], **med,
        "spread_kernel_fwd_ms": [round(min(times["kernel_fwd"]), 4), round(max(times["kernel_fwd"]), 4)],
        "ratio_fwd": round(med["torch_fwd_ms"] / med["own_fwd_ms"], 3),
        "ratio_fwd_bwd": round(med["torch_fwd_bwd_ms"] / med["own_fwd_bwd_ms"], 3),
        "hbm_frac_fwd": share(2, med["kernel_fwd_ms"]), "hbm_frac_bwd": share(3, med["kernel_bwd_ms"]),
        "max_abs_diff_vs_torch": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--ops", default="batch_norm,prelu_dice")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "batch_norm_bench needs the GPU"
    for op in args.ops.split(","):
        for rows in ROWS:
            for n in COLS:
                for dt in (torch.float16, torch.float32):
                    run(args, op, rows, n, dt)


if __name__ == "__main__":
    main()
