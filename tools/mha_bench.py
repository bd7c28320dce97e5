"""Times hugectr_amd.multi_head_attention (attention.hip: two kernel families, chosen by shape) next
to the same math through torch on the device -- the reference layer's recipe: transpose to
[B, H, seq, d], bmm, scale, softmax with its 1e-6, bmm, transpose back -- forward and forward +
backward: at BST's shape and a heavy one (the kernels that hold a head in one wavefront), at a long
and a wide one (the tiled kernels).  At the heavy shape the tiled entry points are also called
directly (`tiled_*`), next to the kernels the layer picks there.  Device events around batches of
calls, medians over rounds, the paths alternating inside a round.  One JSON line per (shape,
dtype); `ratio_*` = torch / own, `ratio_tiled_*` = torch / tiled.

Three more legs per (shape, dtype), forward and forward + backward, the mask from lengths:
`mask` (sequence_mask, then attention with that mask: both launches, what a BST graph runs every
step; every length = seq), `lengths_full` (the same lengths handed to the kernels, no mask tensor)
and `lengths_ragged` (integer lengths uniform in [1, seq] from a fixed seed, len_from = len_to).
At the heavy shape the three go to the tiled entries directly.  `spread_*`: (min, max) over the
rounds; `work_frac`: the share of (32-row, 32-key) sub-tiles the ragged lengths leave the forward
and the dq sweep, `work_frac_dkv` the dkv sweep, both computed here from the lengths.

    python tools/mha_bench.py [--rounds 15] [--calls 20]
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

SHAPES = {"bst": (4096, 10, 32, 4), "heavy": (4096, 128, 256, 4),  # B, seq, hidden, heads
          "long": (1024, 512, 256, 4), "wide": (4096, 128, 512, 4)}


def tiled_direct(q, k, v, top, heads, mask_lens=None, lengths=None):
    """hctr_mha_tiled_fwd / _bwd on preallocated buffers -> (forward, forward + backward, out).
    mask_lens: each forward builds the mask from these lengths first; lengths: the *_len_* entries"""
    B, m, hidden = q.shape
    out, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    stats = torch.empty((B, heads, m, 4), dtype=torch.float32, device=q.device)
    shape = (B, heads, m, k.shape[1], hidden // heads)
    io = [ptr(q), ptr(k), ptr(v), None]
    f, b = lib.hctr_mha_tiled_fwd, lib.hctr_mha_tiled_bwd
    if lengths is not None:
        f, b = lib.hctr_mha_tiled_len_fwd, lib.hctr_mha_tiled_len_bwd
        io[3:] = [ptr(lengths[0]), ptr(lengths[1])]

    held = {}  # the mask of the last forward, for its backward

    def fwd():
        if mask_lens is not None:
            held["mask"] = ha.sequence_mask(*mask_lens, m, k.shape[1])
            io[3] = ptr(held["mask"])
        check(f(*shape, *io, ptr(out), ptr(stats), _DT[q.dtype], stream_ptr()))

    def both():
        fwd()
        check(b(*shape, *io, ptr(out), ptr(stats), ptr(top), ptr(dq), ptr(dk), ptr(dv),
                _DT[q.dtype], stream_ptr()))
    return fwd, both, out


def work_fracs(lens, seq):
    """lens: integer lengths in [1, seq], len_from = len_to -> the share of 32 x 32 sub-tiles
    attention_tiled.hip's rules keep: (forward and dq sweep, dkv sweep)"""
    sub = -(-seq // 32)
    kept_q = kept_k = 0
    for L in lens.tolist():  # nv = first_plain = L
        for w0 in range(0, seq, 32):  # a wavefront's 32 query rows: all keys if one of them is plain
            kept_q += sub if min(w0 + 32, seq) > L else -(-L // 32)
        for k0 in range(0, seq, 128):  # a block of 128 keys: past nv, from first_plain's tile on
            waves = -(-(min(k0 + 128, seq) - k0) // 32)
            kept_k += waves * (sub if k0 < L else sub - 2 * (L // 64))
    return kept_q / (len(lens) * sub * sub), kept_k / (len(lens) * sub * sub)


def torch_mha(q, k, v, heads):
    B, m, hidden = q.shape
    d = hidden // heads
    qh, kh, vh = (x.view(B, -1, heads, d).transpose(1, 2).contiguous() for x in (q, k, v))
    s = torch.matmul(qh, kh.transpose(2, 3)) / d ** 0.5
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = e / (e.sum(-1, keepdim=True) + 1e-6)
    return torch.matmul(p, vh).transpose(1, 2).contiguous().view(B, m, hidden)


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
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mha_bench needs the GPU"
    for name, (B, seq, hidden, heads) in SHAPES.items():
        for dt in (torch.float16, torch.bfloat16, torch.float32):
            q, k, v, top = (torch.randn(B, seq, hidden, device="cuda").to(dt) for _ in range(4))
            for t in (q, k, v):
                t.requires_grad_(True)

            def fwd(f):
                with torch.no_grad():
                    f()

            def both(f):
                f().backward(top)
                q.grad = k.grad = v.grad = None

            own = lambda: ha.multi_head_attention(q, k, v, None, heads)  # noqa: E731
            ref = lambda: torch_mha(q, k, v, heads)  # noqa: E731
            err = (own().float() - ref().float()).abs().max().item()
            legs = {"own_fwd": lambda: fwd(own), "torch_fwd": lambda: fwd(ref),
                    "own_fwd_bwd": lambda: both(own), "torch_fwd_bwd": lambda: both(ref)}
            if name == "heavy":
                legs["tiled_fwd"], legs["tiled_fwd_bwd"], t_out = tiled_direct(
                    q.detach(), k.detach(), v.detach(), top, heads)
            full = torch.full((B,), float(seq), device="cuda")
            ragged = torch.randint(1, seq + 1, (B,), generator=torch.Generator().manual_seed(seq))
            wf, wf_dkv = work_fracs(ragged, seq)
            ragged = ragged.float().cuda()
            full_dt = full.to(dt)  # (10, 128 and 512 are exact in bf16)
            for leg, kw in (("mask", {"mask_lens": (full_dt, full_dt)}),
                            ("lengths_full", {"lengths": (full, full)}),
                            ("lengths_ragged", {"lengths": (ragged, ragged)})):
                if name == "heavy":
                    legs[leg + "_fwd"], legs[leg + "_fwd_bwd"], _ = tiled_direct(
                        q.detach(), k.detach(), v.detach(), top, heads, **kw)
                    continue
                if leg == "mask":
                    layer = lambda ml=kw["mask_lens"]: ha.multi_head_attention(  # noqa: E731
                        q, k, v, ha.sequence_mask(*ml, seq, seq), heads)
                else:
                    layer = lambda ln=kw["lengths"]: ha.multi_head_attention(  # noqa: E731
                        q, k, v, None, heads, lengths=ln)
                legs[leg + "_fwd"] = lambda f=layer: fwd(f)
                legs[leg + "_fwd_bwd"] = lambda f=layer: both(f)
            for f in legs.values():  # warm-up: code objects, library algorithm choices
                for _ in range(3):
                    f()
            times = {n: [] for n in legs}
            for _ in range(args.rounds):
                for n, f in legs.items():
                    times[n].append(time_ms(f, args.calls))
            med = {n + "_ms": round(statistics.median(t), 4) for n, t in times.items()}
            print(json.dumps({
                "shape": name, "B": B, "seq": seq, "hidden": hidden, "heads": heads,
                "dtype": str(dt).split(".")[1], **med,
                "spread_own_fwd_ms": [round(min(times["own_fwd"]), 4), round(max(times["own_fwd"]), 4)],
                **{f"spread_{n}_ms": [round(min(t), 4), round(max(t), 4)] for n, t in times.items()
                   if n.startswith(("mask", "lengths"))},
                "work_frac": round(wf, 4), "work_frac_dkv": round(wf_dkv, 4),
                "ratio_fwd": round(med["torch_fwd_ms"] / med["own_fwd_ms"], 3),
                "ratio_fwd_bwd": round(med["torch_fwd_bwd_ms"] / med["own_fwd_bwd_ms"], 3),
                **({"ratio_tiled_fwd": round(med["torch_fwd_ms"] / med["tiled_fwd_ms"], 3),
                    "ratio_tiled_fwd_bwd": round(med["torch_fwd_bwd_ms"] / med["tiled_fwd_bwd_ms"], 3),
                    "max_abs_diff_tiled_vs_torch": (t_out.float() - ref().float()).abs().max().item()}
                   if name == "heavy" else {}),
                "max_abs_diff_vs_torch": err}), flush=True)


if __name__ == "__main__":
    main()
