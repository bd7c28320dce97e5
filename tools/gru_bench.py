"""Times hugectr_amd.gru (gru.hip) next to torch.nn.GRU on the same device: forward (no gradient
wanted), forward + backward through autograd, and the forward C entry point alone on preallocated
buffers without a reserve (`kernel_fwd`).  torch.nn.GRU gets the same weights in its own layout
(weight_ih / weight_hh in gate order r, z, n; the single bias as bias_ih, bias_hh zero -- then it
computes the same function, and `max_abs_diff_vs_torch` says so); the mapping is made for this timing
only.  From `kernel_fwd`: the share of the matrix peak (2500 TFLOP/s for fp16, 157.3 for fp32
operands) on 2 S B 3H (V + H), and the share of the 8 TB/s HBM peak on the bytes of x and y.  DIEN's
shape runs the resident instance (its HBM share is the figure to read), the others the streamed one
(the matrix share).  Device events around batches of calls,
medians over rounds, the paths alternating inside a round.  One JSON line per (case, dtype).

    python tools/gru_bench.py [--rounds 5] [--calls 3]
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
MFMA_PEAK_TFLOPS = {torch.float16: 2500.0, torch.float32: 157.3}

# (name, B, S, V, H)
CASES = [("DIEN S 10", 65536, 10, 36, 36), ("DIEN S 50", 65536, 50, 36, 36),
         ("wide", 65536, 10, 128, 128), ("largest H", 16384, 10, 256, 256)]


def time_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run(args, name, B, S, V, H, dt):
    x = (torch.rand(S, B, V, device="cuda") * 2 - 1).to(dt).requires_grad_(True)
    layer = ha.GRULayer(H, V).to(device="cuda", dtype=dt)
    ref = torch.nn.GRU(V, H).to(device="cuda", dtype=dt)
    with torch.no_grad():
        w = layer.weight
        ref.weight_ih_l0.copy_(w[:3 * H * V].view(3 * H, V))
        ref.weight_hh_l0.copy_(w[3 * H * V:3 * H * (V + H)].view(3 * H, H))
        ref.bias_ih_l0.copy_(w[-3 * H:])
        ref.bias_hh_l0.zero_()
    y = torch.empty(S, B, H, dtype=dt, device="cuda")
    top = torch.randn_like(y)
    own, theirs = lambda: layer(x), lambda: ref(x)[0]  # noqa: E731
    kernel = lambda: check(lib.hctr_gru_fwd(B, S, V, H, 0, ptr(x), ptr(layer.weight), ptr(y), None,  # noqa: E731
                                            _DT[dt], stream_ptr()))

    def fwd(f):
        with torch.no_grad():
            f()

    def both(f, params):
        f().backward(top)
        for t in (x, *params):
            t.grad = None

    with torch.no_grad():
        err = (own().float() - theirs().float()).abs().max().item()
    legs = {"own_fwd": lambda: fwd(own), "torch_fwd": lambda: fwd(theirs),
            "own_fwd_bwd": lambda: both(own, layer.parameters()),
            "torch_fwd_bwd": lambda: both(theirs, ref.parameters()), "kernel_fwd": kernel}
    for f in legs.values():  # warm-up: code objects, the allocator's blocks, the library's choice
        for _ in range(2):
            f()
    times = {n: [] for n in legs}
    for _ in range(args.rounds):
        for n, f in legs.items():
            times[n].append(time_ms(f, args.calls))
    med = {n + "_ms": round(statistics.median(t), 4) for n, t in times.items()}
    sec = med["kernel_fwd_ms"] * 1e-3
    # gru.hip's rule: the weights [3 Hc][Vc + Hc + pad] beside the tile's operands within 80 KB of LDS
    instance = "resident" if (H, V) == (36, 36) else "streamed"
    flops, nbytes = 2 * S * B * 3 * H * (V + H), S * B * (V + H) * x.element_size()
    print(json.dumps({
        "case": f"{name} (B {B}, S {S}, V {V}, H {H})", "dtype": str(dt).split(".")[1],
        "instance": instance, **med,
        "spread_kernel_fwd_ms": [round(min(times["kernel_fwd"]), 4), round(max(times["kernel_fwd"]), 4)],
        "ratio_fwd": round(med["torch_fwd_ms"] / med["own_fwd_ms"], 3),
        "ratio_fwd_bwd": round(med["torch_fwd_bwd_ms"] / med["own_fwd_bwd_ms"], 3),
        "tflops_fwd": round(flops / sec / 1e12, 2),
        "mfma_frac_fwd": round(flops / sec / 1e12 / MFMA_PEAK_TFLOPS[dt], 4),
        "hbm_frac_fwd": round(nbytes / sec / 1e9 / HBM_PEAK_GBPS, 4),
        "max_abs_diff_vs_torch": err}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gru_bench needs the GPU"
    for case in CASES:
        for dt in (torch.float16, torch.float32):
            run(args, *case, dt)


if __name__ == "__main__":
    main()
