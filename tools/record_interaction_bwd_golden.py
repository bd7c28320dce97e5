"""The 16-bit interaction backward's golden digests: tests/golden/interaction_bwd_layout.json.

  HCTR_LIB_VARIANT=parent python tools/record_interaction_bwd_golden.py

records sha256 digests of mlp_grad and emb_grad of every case below, computed by the library it
loads -- meant to be the PARENT's (`make -C hugectr_amd/csrc VARIANT=<parent csrc> TAG=parent`), so
that tests/test_interaction_bwd_layout_gpu.py holds a change of the kernel's LDS layout or operand
order to the parent's bits.  The inputs come from a seeded numpy generator on the host and are
rounded to the 16-bit type on the host: nothing depends on the device's RNG.  The test imports the
cases and the runner from here.

Cases: W in {32, 64, 128} x n_emb x {float16, bfloat16} x B in {1, 2049, 4099, 6149} x the four
backward entries (the gather entry also with a quarter of its row numbers missing), thinned
pairwise so that the test file runs in about ten seconds: every (W, n_emb, type) runs one entry at
one B, both stepping from one shape to the next so that the shapes that reach the MFMA kernel meet
every (B, entry) pair; W = 128, n_emb = 26 runs the whole B x entry product in float16 and one B
per entry in bfloat16.  With the grid of 2048 blocks those B make a block run 1, 2, 3 and 4
samples with a ragged last pass.
n_emb: 1, 15, 16, 26, 31 (n_ins = 16 fills one k-step of the MFMA, 17 crosses into the second, 32
leaves no padding row) -- of these only 26 has out_len % 8 == 0, which interaction_bwd16_kernel
needs: with the others hctr_interaction_bwd runs the generic kernel and the indexed and gather
entries refuse the shape, which is recorded as {"refused": true}.  5, 10 and 21 (n_ins = 6, 11, 22:
inside one k-step, and in the second) are the shapes near those edges that do reach the kernel."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "interaction_bwd_layout.json")
WS = (32, 64, 128)
N_EMB = (1, 5, 10, 15, 16, 21, 26, 31)
DTYPES = ("float16", "bfloat16")
BS = (1, 2049, 4099, 6149)
ENTRIES = ("bwd", "bwd_indexed", "bwd_indexed_scatter", "bwd_gather", "bwd_gather_missing")
NO_ROW = 0xFFFFFFFFFFFFFFFF
N_ROWS = 97      # distinct rows behind bwd_indexed
N_TABLE = 1000   # table rows behind bwd_gather
MAX_B, MAX_EMB = max(BS), max(N_EMB)


def reaches_mfma(W, n_emb):
    n_ins = n_emb + 1
    return (W + n_ins * (n_ins - 1) // 2 + 1) % 8 == 0


def cases():
    """[(W, n_emb, dtype_name, B, entry)]"""
    res, i, k = [], 0, [0, 0]  # (k: one counter for the shapes that reach the MFMA kernel, one for
    for W in WS:               # the rest; 5 entries against 4 B: the shapes meet every pair)
        for n_emb in N_EMB:
            for dt in DTYPES:
                if (W, n_emb) == (128, 26):
                    res += [(W, n_emb, dt, B, e) for j, e in enumerate(ENTRIES) for B in BS
                            if dt == DTYPES[0] or B == BS[j % 4]]
                    continue
                c = 0 if reaches_mfma(W, n_emb) else 1
                j = k[c] % 5
                res.append((W, n_emb, dt, BS[(i + j) % 4], ENTRIES[j]))
                k[c] += 1
                i += 1
    return res


def case_id(c):
    W, n_emb, dt, B, e = c
    return f"W{W}-n{n_emb}-{dt}-B{B}-{e}"


_pool = {}


def _pools(W):
    """float32 standard normals of the largest shape, drawn once per width: every case of that
    width takes its leading part"""
    if W not in _pool:
        rng = np.random.default_rng([20, W])
        n_ins = MAX_EMB + 1
        _pool.clear()
        _pool[W] = {"mlp": rng.standard_normal((MAX_B, W), dtype=np.float32),
                    "emb": rng.standard_normal((MAX_B, MAX_EMB, W), dtype=np.float32),
                    "top": rng.standard_normal((MAX_B, W + n_ins * (n_ins - 1) // 2 + 1),
                                               dtype=np.float32),
                    "rows": rng.standard_normal((N_TABLE, W), dtype=np.float32)}
    return _pool[W]


class Inputs:
    """one case's host tensors: mlp, top (rounded to the type), the entry's own row source, and
    emb [B, n_emb, W], the embedding rows the entry sees (rounded to the type)"""

    def __init__(self, c):
        import torch
        W, n_emb, dt_name, B, entry = c
        self.case = c
        dt = getattr(torch, dt_name)
        p = _pools(W)
        n_ins = n_emb + 1
        self.out_len = W + n_ins * (n_ins - 1) // 2 + 1
        self.mlp = torch.from_numpy(p["mlp"][:B]).to(dt)
        self.top = torch.from_numpy(np.ascontiguousarray(p["top"][:B, :self.out_len])).to(dt)
        rng = np.random.default_rng([W, n_emb, B, ENTRIES.index(entry)])
        self.row_of = self.rows = self.table = self.vi = None
        if entry == "bwd":
            self.emb = torch.from_numpy(np.ascontiguousarray(p["emb"][:B, :n_emb])).to(dt)
        elif entry == "bwd_indexed":
            self.rows = torch.from_numpy(p["rows"][:N_ROWS]).to(dt)
            self.row_of = torch.from_numpy(rng.integers(0, N_ROWS, (B, n_emb)).astype(np.int32))
            self.emb = self.rows[self.row_of.long()].contiguous()
        elif entry == "bwd_indexed_scatter":
            self.emb = torch.from_numpy(np.ascontiguousarray(p["emb"][:B, :n_emb])).to(dt)
            self.row_of = torch.from_numpy(
                rng.permutation(B * n_emb).astype(np.int32).reshape(B, n_emb))
            self.rows = torch.empty((B * n_emb, W), dtype=dt)
            self.rows[self.row_of.long().reshape(-1)] = self.emb.reshape(-1, W)
        else:
            self.table = torch.from_numpy(p["rows"])
            vi = rng.integers(0, N_TABLE, (B, n_emb)).astype(np.uint64)
            if entry == "bwd_gather_missing":
                vi[rng.random((B, n_emb)) < 0.25] = NO_ROW
            live = torch.from_numpy(vi != NO_ROW)
            idx = torch.from_numpy(np.where(vi != NO_ROW, vi, 0).astype(np.int64))
            self.vi = torch.from_numpy(vi.reshape(-1).view(np.int64))
            self.emb = torch.where(live[:, :, None], self.table[idx], torch.zeros(())).to(dt)


def run(inp, alloc):
    """the case's entry on the GPU.  alloc(shape, dtype) -> (tensor the kernel writes, after()),
    after() being called once the kernel has run.  Returns None where the entry refuses the shape,
    else (mlp_grad [B, W], emb_grad in the entry's own layout, emb_grad as [B, n_emb, W])."""
    import torch
    from hugectr_amd import _lib
    lib, ptr, s = _lib.lib, _lib.ptr, _lib.stream_ptr()
    W, n_emb, dt_name, B, entry = inp.case
    DT = {"float16": _lib.F16, "bfloat16": _lib.BF16}[dt_name]
    dt = getattr(torch, dt_name)
    mlp, top = inp.mlp.cuda(), inp.top.cuda()
    mg, mg_after = alloc((B, W), dt)
    if entry == "bwd":
        emb = inp.emb.cuda()
        eg, eg_after = alloc((B, n_emb, W), dt)
        rc = lib.hctr_interaction_bwd(B, n_emb, W, ptr(mlp), ptr(emb), ptr(top), ptr(mg),
                                      ptr(eg), DT, s)
    elif entry in ("bwd_indexed", "bwd_indexed_scatter"):
        rows, row_of = inp.rows.cuda(), inp.row_of.cuda()
        scatter = entry == "bwd_indexed_scatter"
        eg, eg_after = alloc((B * n_emb, W), dt)
        fn = lib.hctr_interaction_bwd_indexed_scatter if scatter else lib.hctr_interaction_bwd_indexed
        rc = fn(B, n_emb, W, ptr(mlp), ptr(rows), ptr(row_of), ptr(top), ptr(mg), ptr(eg), DT, s)
    else:
        table, vi = inp.table.cuda(), inp.vi.cuda()
        eg, eg_after = alloc((B, n_emb, W), dt)
        rc = lib.hctr_interaction_bwd_gather(B, n_emb, W, ptr(mlp), ptr(table), ptr(vi), ptr(top),
                                             ptr(mg), ptr(eg), DT, s)
    torch.cuda.synchronize()
    mg_after()
    eg_after()
    if rc != 0:
        return None
    if entry == "bwd_indexed_scatter":
        view = eg[inp.row_of.cuda().long().reshape(-1)].view(B, n_emb, W)
    else:
        view = eg.view(B, n_emb, W)
    return mg, eg, view


def digest(t):
    import torch
    return hashlib.sha256(t.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def plain_alloc(shape, dt):
    import torch
    return torch.zeros(shape, dtype=dt, device="cuda"), lambda: None


def main():
    sys.path.insert(0, ROOT)
    from hugectr_amd import _lib
    out = {}
    for c in cases():
        got = run(Inputs(c), plain_alloc)
        out[case_id(c)] = {"refused": True} if got is None else \
            {"mlp_grad": digest(got[0]), "emb_grad": digest(got[1])}
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump({"library": os.path.basename(_lib.LIB_PATH), "cases": out}, f, indent=0,
                  sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases, {sum('refused' in v for v in out.values())} refused -> {path}")


if __name__ == "__main__":
    main()
