"""Shared by the Parquet reader's tests: the small dataset (three files of 100, 64 and 37 rows written
with row_group_size=24, so every column arrives in several chunks), the numpy closed forms of
include/hugectr_amd.h for hctr_parquet_decode, and the comparison of two readers' batches."""
import json
import os

import numpy as np
import torch

ROWS = (100, 64, 37)
B = 32
SIZES = [50, 1000, 7, 90, 11, 13]          # slot_size_array: a(3 slots) b(1) c(2)
PARAMS = [("a", 3), ("b", 1), ("c", 2)]
LABELS = ["l_int", "l_f32"]
CONTS = ["d_f32", "d_f64", "d_i64"]
CATS = ["a0", "a1", "a2", "b0", "c0", "c1"]


def inp(params=PARAMS, label_dim=len(LABELS), dense_dim=len(CONTS)):
    import hugectr_amd.hugectr as hugectr
    return hugectr.Input(label_dim=label_dim, label_name="label", dense_dim=dense_dim,
                         dense_name="dense", data_reader_sparse_param_array=[
                             hugectr.DataReaderSparseParam(n, 1, True, s) for n, s in params])


def _lists(rng, n, max_len, hi, first):
    """n lists of 0..max_len keys; `first` fixes the lengths of the first rows"""
    lens = rng.integers(0, max_len + 1, size=n)
    lens[:len(first)] = first
    return [rng.integers(0, hi, size=int(k)).tolist() for k in lens]


def table(rng, n):
    import pyarrow as pa
    # a1: row 0 empty, row 1 with 70 keys, row 2 a sample in which EVERY list is empty
    a1 = _lists(rng, n, 70, 1 << 40, [0, 70, 0])
    a2 = _lists(rng, n, 2, 1 << 31, [1, 2, 0])
    cols = {
        "l_int": pa.array(rng.integers(0, 2, size=n), type=pa.int64()),
        "l_f32": pa.array(rng.random(n, dtype=np.float32), type=pa.float32()),
        "d_f32": pa.array(rng.random(n, dtype=np.float32), type=pa.float32()),
        # not representable in fp32: the cast must round to nearest even
        "d_f64": pa.array(rng.random(n) * 1e3 + 1e-9, type=pa.float64()),
        "d_i64": pa.array(rng.integers(1 << 24, 1 << 40, size=n) | 1, type=pa.int64()),
        "a0": pa.array(rng.integers(-5, 1 << 31, size=n).astype(np.int32), type=pa.int32()),
        "a1": pa.array(a1, type=pa.list_(pa.int64())),
        "a2": pa.array(a2, type=pa.large_list(pa.int32())),
        "b0": pa.array(rng.integers(0, 1 << 50, size=n), type=pa.int64()),
        "c0": pa.array(rng.integers(0, 1 << 33, size=n), type=pa.int64()),
        "c1": pa.array(rng.integers(0, 1 << 20, size=n), type=pa.int64()),
    }
    return pa.table(cols)


def write_dataset(folder, tables, labels=LABELS, conts=CONTS, cats=CATS, row_group_size=24):
    """reference layout: files, _file_list.txt, _metadata.json -> path of the file list"""
    import pyarrow.parquet as pq
    folder = str(folder)
    os.makedirs(folder, exist_ok=True)
    names, stats = [], []
    for i, t in enumerate(tables):
        name = os.path.join(folder, f"part_{i}.parquet")
        pq.write_table(t, name, row_group_size=row_group_size)
        names.append(name)
        stats.append({"file_name": os.path.basename(name), "num_rows": t.num_rows})
    with open(os.path.join(folder, "_file_list.txt"), "w") as f:
        f.write(f"{len(names)}\n" + "\n".join(names) + "\n")
    meta = {"file_stats": stats,
            "labels": [{"col_name": c, "index": i} for i, c in enumerate(labels)],
            "conts": [{"col_name": c, "index": len(labels) + i} for i, c in enumerate(conts)],
            "cats": [{"col_name": c, "index": len(labels) + len(conts) + i}
                     for i, c in enumerate(cats)]}
    with open(os.path.join(folder, "_metadata.json"), "w") as f:
        json.dump(meta, f)
    return os.path.join(folder, "_file_list.txt")


def dataset(folder, seed=7, rows=ROWS):
    rng = np.random.default_rng(seed)
    return write_dataset(folder, [table(rng, n) for n in rows])


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same(got, want):
    """every tensor of a batch equal bit for bit, dtypes and shapes included"""
    for k in ("label", "dense"):
        assert got[k].dtype == want[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        assert torch.equal(bits(got[k]), bits(want[k])), k
    assert list(got["sparse"]) == list(want["sparse"])
    for name, (ro, keys) in want["sparse"].items():
        gro, gkeys = got["sparse"][name]
        assert gro.dtype == ro.dtype and gkeys.dtype == keys.dtype, name
        assert torch.equal(gro.cpu(), ro.cpu()), name + " row offsets"
        assert torch.equal(gkeys.cpu(), keys.cpu()), name + " keys"
    assert ("ebc" in got) == ("ebc" in want)
    for (gk, gbr), (wk, wbr) in zip(got.get("ebc", []), want.get("ebc", [])):
        assert gk.dtype == wk.dtype == torch.int64 and gbr.dtype == wbr.dtype == torch.int64
        assert torch.equal(gbr.cpu(), wbr.cpu()), "bucket range"
        assert torch.equal(gk.cpu(), wk.cpu()), "collection keys"


# ---- the closed forms of include/hugectr_amd.h in numpy --------------------------------------------
def ragged_param(cols, addends, a, B):
    """cols: per slot (values, offsets or None) over a whole file -> (row_offsets, keys), int64"""
    S = len(cols)
    off = [np.arange(len(v) + 1, dtype=np.int64) if o is None else np.asarray(o, np.int64)
           for v, o in cols]
    ro = np.zeros(B * S + 1, np.int64)
    for b in range(B):
        base = sum(int(o[a + b] - o[a]) for o in off)
        for s in range(S):
            ro[b * S + s] = base + sum(int(off[t][a + b + 1] - off[t][a + b]) for t in range(s))
    ro[B * S] = sum(int(o[a + B] - o[a]) for o in off)
    keys = np.zeros(int(ro[-1]), np.int64)
    for b in range(B):
        for s in range(S):
            v, o = cols[s][0], off[s]
            n = int(o[a + b + 1] - o[a + b])
            keys[ro[b * S + s]:ro[b * S + s] + n] = \
                np.asarray(v[int(o[a + b]):int(o[a + b]) + n]).astype(np.int64) + int(addends[s])
    return ro, keys


def group(cols, a, B):
    """cols: per lookup (values, offsets or None) -> (keys, bucket_range), int64, feature-major"""
    off = [np.arange(len(v) + 1, dtype=np.int64) if o is None else np.asarray(o, np.int64)
           for v, o in cols]
    br = np.zeros(len(cols) * B + 1, np.int64)
    keys, before = [], 0
    for l, (v, _) in enumerate(cols):
        o = off[l]
        br[l * B:(l + 1) * B] = before + o[a:a + B] - o[a]
        keys.append(np.asarray(v[int(o[a]):int(o[a + B])]).astype(np.int64))
        before += int(o[a + B] - o[a])
    br[-1] = before
    return np.concatenate(keys), br
