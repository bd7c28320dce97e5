"""The data gradient of an MLP layer with the ReLU mask and the bias partials of the layer below:
the library GEMM dy = dz_next [M, K] @ W16 [K, N] + hctr_relu_bwd_bias_partials against
hctr_gemm_nt16_drelu on W16^T, per shape, on one GPU (fp16).  The table behind the `auto` rule of
HCTR_DGRAD_FUSED (hugectr_amd/dense.py, _dgrad_fused_wins; profiles/dgrad_relu_shapes.txt).

The two sides alternate in one process; a figure is microseconds per call from device events around
--calls back-to-back calls, --repeats repeats per side (min / median / max), three warm-up calls of
each side first.  The library side takes the selections of hugectr_amd/tuning/tunableop_gfx950.csv
as the model does (HCTR_TUNABLEOP=off: the library's heuristics).

  python tools/microbench_dgrad_relu.py                       # M = 65536, every tile height, rings 2 / 3
  python tools/microbench_dgrad_relu.py --m 2048,8192 --auto  # the launcher's own tile choice
  python tools/microbench_dgrad_relu.py --shapes 384x256,640x128   # other N x K"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.cuda.tunable as tunable  # noqa: E402

from hugectr_amd._lib import F16, check, lib, ptr, stream_ptr  # noqa: E402

DLRM = "512x256,1024x512,1024x1024,256x128"  # N x K: top 512, top 1024 (K 512, 1024), bottom 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="65536", help="batch sizes, comma separated")
    ap.add_argument("--shapes", default=DLRM, help="N x K of the data gradient, comma separated")
    ap.add_argument("--auto", action="store_true", help="only the launcher's own tile choice")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hugectr_amd",
                        "tuning", "tunableop_gfx950.csv")
    if os.path.exists(path) and os.environ.get("HCTR_TUNABLEOP", "file") != "off":
        import tempfile
        tunable.enable(True)
        tunable.tuning_enable(False)
        tunable.read_file(path)
        tunable.set_filename(os.path.join(tempfile.gettempdir(), f"hctr_tunableop_{os.getpid()}.csv"))
        print("library GEMM selections: tunableop_gfx950.csv", flush=True)
    else:
        print("library GEMM selections: heuristics", flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.calls

    torch.manual_seed(0)
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    for M in (int(v) for v in a.m.split(",")):
        for N, K in shapes:
            x = (torch.randn((M, K), device="cuda") / 64).half()    # dz of the layer above
            w = (torch.randn((K, N), device="cuda") * 0.05).half()  # W [out][in]
            wt = w.t().contiguous()                                 # W^T [N][K]
            y = torch.relu(torch.randn((M, N), device="cuda")).half()
            dy = torch.empty((M, N), dtype=torch.float16, device="cuda")
            dz0, dz1 = torch.empty_like(dy), torch.empty_like(dy)
            ws = torch.empty(lib.hctr_relu_bwd_bias_workspace_bytes(M, N) // 4, dtype=torch.float32,
                             device="cuda")
            part = torch.empty((M // 64 + 1) * N, dtype=torch.float32, device="cuda")  # (any tile height)
            sp = stream_ptr()

            def pair():
                torch.mm(x, w, out=dy)
                check(lib.hctr_relu_bwd_bias_partials(M, N, ptr(dy), ptr(y), ptr(dz0), ptr(ws), F16, sp))

            def fused():
                check(lib.hctr_gemm_nt16_drelu(M, N, K, ptr(x), K, ptr(wt), K, ptr(y), ptr(dz1), N,
                                               ptr(part), F16, sp))

            variants = [(None, None)] if a.auto else \
                [("64", "2"), ("128", "2"), ("128", "3")] + ([("256", "2")] if N % 256 == 0 else [])
            print(f"== M={M} N={N} K={K} fp16; us per call, {a.repeats} repeats x {a.calls} calls, "
                  "alternating", flush=True)
            for bm, st in variants:
                for name, v in (("HCTR_GEMM_BM", bm), ("HCTR_GEMM_STAGES", st)):
                    if v is None:
                        os.environ.pop(name, None)
                    else:
                        os.environ[name] = v
                for _ in range(3):
                    pair()
                    fused()
                torch.cuda.synchronize()
                tp, tf = [], []
                for _ in range(a.repeats):
                    tp.append(timed(pair))
                    tf.append(timed(fused))
                d = (dz0.float() - dz1.float()).abs().max().item()
                print(f"  BM={str(bm):>4} stages={st}: pair min {min(tp):7.1f} med {statistics.median(tp):7.1f} "
                      f"max {max(tp):7.1f} | fused min {min(tf):7.1f} med {statistics.median(tf):7.1f} "
                      f"max {max(tf):7.1f} | fused med - pair min {statistics.median(tf) - min(tp):+7.1f} | "
                      f"max |dz diff| {d:.3e}", flush=True)
            os.environ.pop("HCTR_GEMM_BM", None)
            os.environ.pop("HCTR_GEMM_STAGES", None)
            tg = [timed(lambda: torch.mm(x, w, out=dy)) for _ in range(3)]
            tr = [timed(lambda: check(lib.hctr_relu_bwd_bias_partials(M, N, ptr(dy), ptr(y), ptr(dz0), ptr(ws),
                                                                      F16, sp))) for _ in range(3)]
            print(f"  library GEMM alone med {statistics.median(tg):7.1f}; mask alone med "
                  f"{statistics.median(tr):7.1f}; auto tiles {lib.hctr_gemm_nt16_drelu_tiles(M, N)}", flush=True)


if __name__ == "__main__":
    main()
