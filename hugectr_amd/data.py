"""Dataset formats either side of the hot path: synthetic data generator and readers.

* Parquet dataset layout of the reference (`_file_list.txt`, `_metadata.json` with file_stats /
  cats / conts / labels; R/HugeCTR/src/data_readers/metadata.cpp:60-135) read with pyarrow.
  Keys get the cumulative `slot_size_array` offsets added, as the reference's Parquet reader does
  (R/HugeCTR/src/pybind/add_input.cpp:315-317), so keys are globally unique.
* Norm binary format (DataSetHeader 8 x int64, R/HugeCTR/include/common.hpp:184-191; per sample
  label[f32 x L] dense[f32 x Dn] then per slot `nnz:int32, keys[nnz]`; optional CheckSum framing
  `int32 length | payload | int8 sum`, R/HugeCTR/include/data_readers/check_sum.hpp:39-75) --
  write + read helpers (the reference's Python path marks Norm deprecated; its CPU test oracle
  still reads it, R/test/utest/embedding/sparse_embedding_hash_cpu.hpp:343-377).
* hugectr.tools.DataGenerator(DataGeneratorParams).generate()
  (R/HugeCTR/include/pybind/data_generator_wrapper.hpp:29-69; power law alpha: Long 0.9 /
  Medium 1.1 / Short 1.3, R/HugeCTR/src/data_generator.cpp:94-116).

Every rank reads the FULL batch of keys (the reference broadcasts the whole CSR to every GPU,
R/HugeCTR/src/data_readers/data_collector.cu:86-113) and its own slice of dense/label.
"""
from __future__ import annotations

import ctypes
import json
import os
import queue
import struct
import sys
import threading
import time
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np
import torch


def powerlaw_keys(rng: np.random.Generator, n: int, vocab: int, alpha: float) -> np.ndarray:
    """IntPowerLawDataSimulator (R/HugeCTR/include/data_generator.hpp:108-129), vectorised."""
    u = rng.random(n, dtype=np.float32).astype(np.float64)
    a = 1.0 - alpha
    y = ((float(vocab) ** a - 1.0) * u + 1.0) ** (1.0 / a)
    return np.clip(np.round(y) - 1, 0, vocab - 1).astype(np.int64)


@dataclass
class DataGeneratorParams:
    format: object
    label_dim: int
    dense_dim: int
    num_slot: int
    i64_input_key: bool
    source: str
    eval_source: str
    slot_size_array: Sequence[int]
    nnz_array: Sequence[int] = field(default_factory=list)
    check_type: object = None
    dist_type: object = None
    power_law_type: object = None
    alpha: float = 1.2
    num_files: int = 128
    eval_num_files: int = 32
    num_samples_per_file: int = 40960
    num_samples: int = 5242880
    eval_num_samples: int = 1310720
    float_label_dense: bool = False
    num_threads: int = 1


class DataGenerator:
    def __init__(self, data_generator_params: DataGeneratorParams):
        self.p = data_generator_params

    def _alpha(self) -> float:
        p = self.p
        dist = getattr(p.dist_type, "name", "PowerLaw")
        if dist == "Uniform":
            return 0.0
        plt = getattr(p.power_law_type, "name", "Specific")
        return {"Long": 0.9, "Medium": 1.1, "Short": 1.3}.get(plt, p.alpha)

    def _samples(self, rng, n):
        p = self.p
        alpha = self._alpha()
        nnz = list(p.nnz_array) if p.nnz_array else [1] * p.num_slot
        label = (rng.random((n, p.label_dim)) < 0.5).astype(np.float32)
        dense = rng.random((n, p.dense_dim), dtype=np.float32)
        cats = []
        for s in range(p.num_slot):
            v = int(p.slot_size_array[s])
            k = (powerlaw_keys(rng, n * nnz[s], v, alpha) if alpha > 0
                 else rng.integers(0, v, size=n * nnz[s]).astype(np.int64))
            cats.append(k.reshape(n, nnz[s]))
        return label, dense, cats

    def generate(self):
        p = self.p
        fmt = getattr(p.format, "name", str(p.format))
        rng = np.random.default_rng(20240923)
        for src, total, nfiles in ((p.source, p.num_samples, p.num_files),
                                   (p.eval_source, p.eval_num_samples, p.eval_num_files)):
            if not src:
                continue
            folder = os.path.dirname(src) or "."
            os.makedirs(folder, exist_ok=True)
            per_file = min(p.num_samples_per_file, max(1, total // max(nfiles, 1)))
            nfiles = max(1, total // per_file)
            names = []
            stats = []
            for f in range(nfiles):
                label, dense, cats = self._samples(rng, per_file)
                if fmt == "Parquet":
                    name = os.path.join(folder, f"gen_{f}.parquet")
                    write_parquet(name, label, dense, cats)
                    stats.append({"file_name": os.path.basename(name), "num_rows": per_file})
                else:
                    name = os.path.join(folder, f"gen_{f}.data")
                    write_norm(name, label, dense, cats, p.i64_input_key,
                               check_sum=getattr(p.check_type, "name", "Sum") == "Sum")
                names.append(name)
            with open(src, "w") as fl:
                fl.write(f"{len(names)}\n" + "\n".join(names) + "\n")
            if fmt == "Parquet":
                cols = parquet_columns(p.label_dim, p.dense_dim, p.num_slot)
                meta = {"file_stats": stats,
                        "labels": [{"col_name": c, "index": i} for i, c in enumerate(cols[0])],
                        "conts": [{"col_name": c, "index": p.label_dim + i}
                                  for i, c in enumerate(cols[1])],
                        "cats": [{"col_name": c, "index": p.label_dim + p.dense_dim + i}
                                 for i, c in enumerate(cols[2])]}
                with open(os.path.join(folder, "_metadata.json"), "w") as fm:
                    json.dump(meta, fm)


def parquet_columns(label_dim, dense_dim, num_slot):
    return ([f"label{i}" if label_dim > 1 else "label" for i in range(label_dim)],
            [f"I{i + 1}" for i in range(dense_dim)], [f"C{i + 1}" for i in range(num_slot)])


def write_parquet(path, label, dense, cats):
    import pyarrow as pa
    import pyarrow.parquet as pq
    lc, dc, cc = parquet_columns(label.shape[1], dense.shape[1], len(cats))
    arrays, names = [], []
    for i, c in enumerate(lc):
        arrays.append(pa.array(label[:, i], type=pa.float32()))
        names.append(c)
    for i, c in enumerate(dc):
        arrays.append(pa.array(dense[:, i], type=pa.float32()))
        names.append(c)
    for i, c in enumerate(cc):
        k = cats[i]
        if k.shape[1] == 1:
            arrays.append(pa.array(k[:, 0], type=pa.int64()))
        else:  # multi-hot: list<int64> column
            arrays.append(pa.array(k.tolist(), type=pa.list_(pa.int64())))
        names.append(c)
    pq.write_table(pa.Table.from_arrays(arrays, names=names), path)


def write_norm(path, label, dense, cats, i64_key=True, check_sum=False):
    n = label.shape[0]
    kfmt = "<i8" if i64_key else "<u4"
    with open(path, "wb") as f:
        hdr = struct.pack("<8q", 1 if check_sum else 0, n, label.shape[1], dense.shape[1], len(cats),
                          0, 0, 0)
        _w(f, hdr, check_sum)
        for i in range(n):
            rec = label[i].astype("<f4").tobytes() + dense[i].astype("<f4").tobytes()
            for k in cats:
                rec += struct.pack("<i", k.shape[1]) + k[i].astype(kfmt).tobytes()
            _w(f, rec, check_sum)


def _w(f, payload: bytes, check_sum: bool):
    if check_sum:
        s = np.frombuffer(payload, dtype=np.int8).sum(dtype=np.int64)
        f.write(struct.pack("<i", len(payload)) + payload + struct.pack("<b", int(np.int8(s))))
    else:
        f.write(payload)


def read_norm(path, i64_key=True):
    """-> (label [n,L], dense [n,Dn], row_offset [n*S+1], keys [nnz]) as the reference's
    read_a_batch builds them (sparse_embedding_hash_cpu.hpp:343-377)."""
    raw = open(path, "rb").read()
    pos = [0]
    framed = struct.unpack_from("<i", raw, 0)[0] == 64  # CheckSum framing wraps the 64-byte header

    def rd(nbytes):
        b = raw[pos[0]:pos[0] + nbytes]
        pos[0] += nbytes
        return b

    def record():
        if framed:
            ln = struct.unpack("<i", rd(4))[0]
            payload = rd(ln)
            chk = struct.unpack("<b", rd(1))[0]
            assert int(np.int8(np.frombuffer(payload, dtype=np.int8).sum(dtype=np.int64))) == chk, \
                "Norm file: checksum mismatch"
            return payload
        return None

    hdr = record() if framed else rd(64)
    err, n, L, Dn, S, _, _, _ = struct.unpack("<8q", hdr)
    ksz = 8 if i64_key else 4
    label = np.empty((n, L), np.float32)
    dense = np.empty((n, Dn), np.float32)
    ro = [0]
    keys = []
    for i in range(n):
        if framed:
            buf, o = record(), 0
        else:
            buf, o = raw, pos[0]
        label[i] = np.frombuffer(buf, "<f4", L, o)
        o += 4 * L
        dense[i] = np.frombuffer(buf, "<f4", Dn, o)
        o += 4 * Dn
        for _ in range(S):
            nnz = struct.unpack_from("<i", buf, o)[0]
            o += 4
            keys.append(np.frombuffer(buf, "<i8" if i64_key else "<u4", nnz, o).astype(np.int64))
            o += ksz * nnz
            ro.append(ro[-1] + nnz)
        if not framed:
            pos[0] = o
    return label, dense, np.asarray(ro, np.int64), (np.concatenate(keys) if keys else
                                                    np.empty(0, np.int64))


class _Latch:
    """counts the parts of one fill down; the training thread waits for zero"""

    def __init__(self, parts):
        self.left, self.lock, self.done, self.error = parts, threading.Lock(), threading.Event(), None
        self.result = None

    def part_done(self, error=None):
        with self.lock:
            self.left -= 1
            if error is not None:
                self.error = error
            if self.left == 0:
                self.done.set()


# ---- Parquet on the device: what a staged file looks like and what one decode launch writes -------
def _up64(n: int) -> int:
    return (n + 63) & ~63


def parquet_physical(arrow_type, categorical: bool):
    """(HCTR_PQ_* physical type, bytes per value, is a list) of a column the device path decodes:
    float32 / float64 / int32 / int64 for label and dense columns; int32 / int64 and list /
    large_list of them for categorical columns.  None for every other type."""
    import pyarrow as pa
    from . import _lib
    t, is_list = arrow_type, False
    if pa.types.is_list(t) or pa.types.is_large_list(t):
        if not categorical:
            return None
        t, is_list = t.value_type, True
    if pa.types.is_int32(t):
        return (_lib.PQ_I32, 4, is_list)
    if pa.types.is_int64(t):
        return (_lib.PQ_I64, 8, is_list)
    if not categorical and pa.types.is_float32(t):
        return (_lib.PQ_F32, 4, False)
    if not categorical and pa.types.is_float64(t):
        return (_lib.PQ_F64, 8, False)
    return None


def _pq_numpy(ptype):
    return (np.float32, np.float64, np.int32, np.int64)[ptype]


def parquet_decode_plan(columns, label_dim, dense_dim, params, ebc_groups, slot_offsets, batch, rank,
                        world, i64_key, mean_keys=None):
    """What one hctr_parquet_decode launch writes for one global batch (include/hugectr_amd.h),
    worked out once per reader.  columns: [(physical type, bytes, is a list)] of the label, dense
    and categorical columns in that order; params: [(top_name, slot_num)]; ebc_groups: per
    collection the top_names of its lookups' inputs; slot_offsets: one per slot; mean_keys:
    {top_name: mean keys per sample} of the ragged params, where known.
    -> {"segments" (hctr_parquet_segment records), "addend", "list", "n_items",
        "outputs": [{"esize", "const", "cols"}] -- output k holds const + sum over cols of
                   (off[a + B] - off[a]) elements of esize bytes,
        "label" / "dense": (output, shape), "sparse": {name: (row-offset output or None, key
        output, slots)}, "ebc": [(key output, bucket-range output or None, lookups)]};
    None stands for a tensor that does not depend on the data (all columns scalar)."""
    from . import _lib
    L, Dn, B = int(label_dim), int(dense_dim), int(batch)
    bpg = B // world
    NO = _lib.PQ_NO_OUTPUT
    segs, lst, add, outs, item = [], [], [], [], [0]

    def out(esize, const, cols=()):
        outs.append({"esize": esize, "const": int(const), "cols": tuple(cols)})
        return len(outs) - 1

    def push(cols, addends):
        l0 = len(lst)
        lst.extend(int(c) for c in cols)
        add.extend(int(a) for a in addends)
        return l0

    def seg(kind, out_kind, l0, n, s0, s1, o0, o1, group, lookup, n_items):
        segs.append((kind, out_kind, l0, n, s0, s1, o0, o1, group, lookup, item[0], n_items))
        item[0] += n_items

    def tiles(ns, nc):
        ts = _lib.PQ_TILE_SAMPLES * min(16, _lib.PQ_TILE_COLS // min(nc, _lib.PQ_TILE_COLS))
        return -(-ns // ts) * -(-nc // _lib.PQ_TILE_COLS)

    def to_f32(c0, n):
        # numpy stacks the columns of a group first: a group that promotes to float64 takes its
        # int64 columns through float64 on the way to float32
        o = out(4, bpg * n)
        if bpg * n > 0:
            cols = range(c0, c0 + n)
            via = np.result_type(*[_pq_numpy(columns[c][0]) for c in cols]) == np.float64
            seg(_lib.PQ_SEG_TILE, _lib.PQ_OUT_F32_VIA_F64 if via else _lib.PQ_OUT_F32,
                push(cols, [0] * n), n, rank * bpg, (rank + 1) * bpg, o, NO, 0, 0, tiles(bpg, n))
        return (o, (bpg, n))

    plan = {"sparse": {}, "ebc": []}
    plan["label"] = to_f32(0, L)
    plan["dense"] = to_f32(L, Dn)
    ksz, kkind = (8, _lib.PQ_OUT_KEY_I64) if i64_key else (4, _lib.PQ_OUT_KEY_I32)
    c, s0, col_of = L + Dn, 0, {}
    for name, S in params:
        cols = list(range(c, c + S))
        ragged = [cc for cc in cols if columns[cc][2]]
        l0 = push(cols, slot_offsets[s0:s0 + S])
        if not ragged:  # one-hot: a transpose; the row offsets are arange(B * S + 1)
            o = out(ksz, B * S)
            seg(_lib.PQ_SEG_TILE, kkind, l0, S, 0, B, o, NO, 0, 0, tiles(B, S))
            plan["sparse"][name] = (None, o, S)
        else:
            o_ro, o_k = out(ksz, B * S + 1), out(ksz, B * (S - len(ragged)), ragged)
            # lanes per sample: the power of two that covers the mean keys of a sample
            mean = (mean_keys or {}).get(name, 8.0)
            G = 1
            while G < 64 and G < mean:
                G *= 2
            seg(_lib.PQ_SEG_RAGGED, kkind, l0, S, 0, B, o_ro, o_k, G, 0,
                -(-B // (_lib.PQ_BLOCK // G)))
            plan["sparse"][name] = (o_ro, o_k, S)
        col_of[name] = (c, S)
        c += S
        s0 += S
    for names in ebc_groups:
        for nm in names:
            assert col_of[nm][1] == 1, "embedding_collection inputs carry one slot per lookup"
        cols = [col_of[nm][0] for nm in names]
        ragged = [cc for cc in cols if columns[cc][2]]
        n = len(cols)
        o_k = out(8, B * (n - len(ragged)), ragged)
        o_br = out(8, n * B + 1) if ragged else NO
        l0 = push(cols, [0] * n)
        for l in range(n):  # bucket = lookup * batch + sample: one segment per lookup
            seg(_lib.PQ_SEG_GROUP, _lib.PQ_OUT_KEY_I64, l0, n, 0, B, o_br, o_k, 0, l,
                -(-B // _lib.PQ_BLOCK))
        plan["ebc"].append((o_k, o_br if ragged else None, n))
    if not 1 <= len(segs) <= _lib.PQ_DECODE_MAX_SEGMENTS:
        raise RuntimeError(f"parquet reader: {len(segs)} output segments (1..4096 supported)")
    plan["segments"] = np.array(segs, dtype=np.dtype(_lib.PQ_SEGMENT_FIELDS))
    plan["addend"] = np.asarray(add, np.int64)
    plan["list"] = np.asarray(lst, np.uint32)
    plan["n_items"], plan["outputs"] = item[0], outs
    for g in plan["segments"]:  # every list range lies inside the lists, every column exists
        assert int(g["list0"]) + int(g["ncols"]) <= len(lst) and int(g["sample1"]) <= B
    assert all(cc < len(columns) for cc in lst)
    return plan


def parquet_slot_layout(columns, n_outputs, batch, rows, n_values):
    """byte layout of one staged file: the hctr_parquet_column table at 0, then per batch of the
    file one row of n_outputs + 1 byte offsets into its arena (the last one is the arena's size),
    then per column its values (n_values[c] of them, the chunks one behind the other) and, for a
    list column, int64 offsets[rows + 1].  -> (offset of the batch table, [(values, offsets)] per
    column, bytes used)"""
    from . import _lib
    top = _up256(len(columns) * 24)
    tab_off = top
    top = _up256(top + (rows // batch) * (n_outputs + 1) * 8)
    lay = []
    for (_, esz, is_list), nv in zip(columns, n_values):
        v = top
        top = _up64(top + int(nv) * esz)
        o = _lib.PQ_NO_OFFSETS
        if is_list:
            o = top
            top = _up64(top + (rows + 1) * 8)
        lay.append((v, o))
    return tab_off, lay, max(top, 256)


def stage_parquet_table(table, path, spec, buf):
    """lays a file's columns into buf (uint8, a pinned file slot) as parquet_slot_layout says.
    spec: {"names", "columns", "batch", "outputs"}.  Value buffers are copied at their physical
    width, chunk by chunk (no combine_chunks, no widening); a list column's offsets are rebased
    over the whole file, one vectorised pass per chunk.
    -> {"rows", "nb", "tab" (int64 [nb, outputs + 1] byte offsets), "cnt" (elements per output),
        "tab_off", "used"}"""
    from . import _lib
    columns, B, outs = spec["columns"], spec["batch"], spec["outputs"]
    rows = table.num_rows
    parts_of, n_values = [], []
    for name, phys in zip(spec["names"], columns):
        col = table.column(name)
        if parquet_physical(col.type, phys[2] or name in spec.get("cats", ())) != tuple(phys):
            raise RuntimeError(f"{path}: column {name} is {col.type}, not the type the reader "
                               "was built for")
        if col.null_count > 0:
            raise RuntimeError(f"{path}: column {name} holds nulls")
        parts = []
        for ch in col.chunks:
            if len(ch) == 0:
                continue
            if phys[2]:
                if ch.values.null_count > 0:
                    raise RuntimeError(f"{path}: column {name} holds nulls")
                o = ch.offsets.to_numpy()
                parts.append((o, ch.values.to_numpy(zero_copy_only=True)[o[0]:o[-1]]))
            else:
                parts.append((None, ch.to_numpy(zero_copy_only=True)))
        parts_of.append(parts)
        n_values.append(sum(len(v) for _, v in parts))
    tab_off, lay, used = parquet_slot_layout(columns, len(outs), B, rows, n_values)
    if used > buf.size:
        raise RuntimeError(f"{path}: {used} bytes to stage, the file slot holds {buf.size}")
    desc = np.zeros(len(columns), dtype=np.dtype(_lib.PQ_COLUMN_FIELDS))
    offs = [None] * len(columns)
    for i, ((pt, esz, is_list), parts, (v_off, o_off)) in enumerate(zip(columns, parts_of, lay)):
        desc[i] = (v_off, o_off, pt, esz)
        dst = buf[v_off:v_off + n_values[i] * esz].view(_pq_numpy(pt))
        if is_list:
            od = buf[o_off:o_off + (rows + 1) * 8].view(np.int64)
            od[0] = 0
            offs[i] = od
        pos = r = 0
        for o, v in parts:
            assert v.dtype == dst.dtype
            dst[pos:pos + len(v)] = v
            if is_list:  # rebased: this chunk's first value sits at pos
                n = len(o) - 1
                np.add(o[1:], pos - int(o[0]), out=od[r + 1:r + 1 + n], dtype=np.int64)
                r += n
            pos += len(v)
    # sizes of every batch's outputs from the offsets just written: no device round trip
    nb = rows // B
    cnt = np.empty((nb, len(outs)), np.int64)
    for k, o in enumerate(outs):
        n = np.full(nb, o["const"], np.int64)
        for cc in o["cols"]:
            n += offs[cc][B:nb * B + 1:B] - offs[cc][0:nb * B:B]
        cnt[:, k] = n
    size = (cnt * np.asarray([o["esize"] for o in outs], np.int64) + 255) & ~255
    tab = np.zeros((nb, len(outs) + 1), np.int64)
    np.cumsum(size, axis=1, out=tab[:, 1:])
    buf[tab_off:tab_off + tab.nbytes].view(np.int64)[:] = tab.reshape(-1)
    buf[:desc.nbytes] = desc.view(np.uint8)
    return {"rows": rows, "nb": nb, "tab": tab, "cnt": cnt, "tab_off": tab_off, "used": used}


def _parquet_file_info(path):
    """footer only: (Arrow schema, rows, {top-level column: values over all row groups}).  The
    value count of a list column includes one entry per empty list, so it bounds the staged size."""
    import pyarrow.parquet as pq
    md = pq.read_metadata(path)
    nv = {}
    for r in range(md.num_row_groups):
        rg = md.row_group(r)
        for j in range(rg.num_columns):
            cm = rg.column(j)
            top = cm.path_in_schema.split(".")[0]
            nv[top] = nv.get(top, 0) + cm.num_values
    return md.schema.to_arrow_schema(), md.num_rows, nv


def _stage_worker(tasks):
    """worker thread of the asynchronous Parquet reader: (event after the slot's last copy up, the
    pinned slot, file, spec, latch).  Holds no reference to the reader."""
    import pyarrow.parquet as pq
    while True:
        t = tasks.get()
        if t is None:
            return
        ev, buf, path, spec, latch = t
        try:
            t0 = time.perf_counter()
            # (Arrow's own pool is sized by the machine's CPU count: one thread, this one)
            table = pq.read_table(path, columns=spec["names"], use_threads=False)
            if ev is not None:
                ev.synchronize()  # the pinned slot is free once its last file has been copied up
            latch.result = stage_parquet_table(table, path, spec, buf)
            latch.result["stage_s"] = time.perf_counter() - t0
            latch.part_done()
        except BaseException as e:  # handed to next_batch()
            latch.part_done(e)
        t = ev = buf = latch = table = None  # (nothing of the file is held while waiting)


class ParquetReader:
    """Streams batches from a reference-layout Parquet dataset.

    On a CUDA device the reader is asynchronous (DESIGN.md "Parquet reader"): worker threads read
    the coming files and stage their column buffers in pinned file slots, a side stream copies a
    staged file up once and turns its columns into a batch with ONE launch (hctr_parquet_decode),
    and next_batch() only makes the consumer's stream wait for that launch.  On a CPU device, with
    decode="host", or when a column has a type the kernel does not take, every batch is decoded on
    the host, as it always was.  cache_batches = N > 0: the first N batches are kept and handed out
    round-robin for ever (DataReaderParams.cache_eval_data)."""

    def __init__(self, file_list: str, inp, slot_size_array, batch, rank, world, device, i64_key,
                 repeat: bool, *, num_workers: int = 2, ring: int = 2, cache_batches: int = 0,
                 decode: str = "auto"):
        import pyarrow.parquet as pq
        self.pq = pq
        lines = [l.strip() for l in open(file_list) if l.strip()]
        self.files = lines[1:1 + int(lines[0])]
        folder = os.path.dirname(file_list) or "."
        self.files = [f if os.path.isabs(f) or os.path.exists(f) else os.path.join(folder, os.path.basename(f))
                      for f in self.files]
        meta_path = os.path.join(folder, "_metadata.json")
        if not os.path.exists(meta_path):
            raise RuntimeError(f"{meta_path} not found (Parquet datasets need _metadata.json)")
        meta = json.load(open(meta_path))
        self.label_cols = [c["col_name"] for c in meta["labels"]]
        self.cont_cols = [c["col_name"] for c in meta["conts"]]
        self.cat_cols = [c["col_name"] for c in meta["cats"]]
        self.inp, self.batch, self.rank, self.world = inp, batch, rank, world
        self.device, self.repeat = device, repeat
        self.key_dtype = torch.int64 if i64_key else torch.int32
        ssa = list(slot_size_array)
        self.slot_offsets = np.concatenate([[0], np.cumsum(ssa)[:-1]]).astype(np.int64) if ssa \
            else np.zeros(len(self.cat_cols), np.int64)
        self._file_idx, self._buf, self._pos = 0, None, 0
        self._epoch_done = False
        # embedding_collection models (see RawReader.ebc_groups): slot of every one-slot input
        self._ebc_groups = []
        self._slot_of = {}
        s0 = 0
        for p in inp.sparse_params:
            self._slot_of[p.top_name] = (s0, p.slot_num)
            s0 += p.slot_num
        if decode not in ("auto", "host", "device"):
            raise ValueError(f"ParquetReader: decode={decode!r} (auto, host or device)")
        self._cache_n, self._cache, self._served = max(0, int(cache_batches or 0)), [], 0
        self._batches, self._files_staged, self._wait_s = 0, 0, 0.0
        self._threads, self._closed, self._tasks = [], False, None
        self._ring = min(4, max(2, int(ring)))
        self._workers = max(1, min(self._ring, int(num_workers), 8))
        self._async = False
        dev_type = device.type if isinstance(device, torch.device) else str(device).split(":")[0]
        if decode != "host" and dev_type == "cuda":
            self._async = self._check_schemas()
        if decode == "device" and not self._async:
            raise RuntimeError("ParquetReader: decode='device' needs a CUDA device and label / "
                               "dense / categorical columns of the accepted types")
        if self._async:
            self._start_device()

    @property
    def ebc_groups(self):
        return self._ebc_groups

    @ebc_groups.setter
    def ebc_groups(self, groups):
        self._ebc_groups = groups
        if self._async and self._plan is not None:
            self._rewind()  # (batches in flight were decoded by the old plan)
            self._plan = None
        if self._cache:  # (kept batches carry the old collections' CSRs)
            self._cache, self._served = [], 0
        if self._async:
            self._issued_total = 0

    def stats(self):
        """decode: where a batch is decoded; ring / threads: file slots and staging workers of the
        asynchronous path (0 on the host path); batches: handed out so far; files: files staged
        (host path: read); wait_ms: total time next_batch() waited for a staging worker"""
        return {"decode": "device" if self._async else "host",
                "ring": self._ring if self._async else 0,
                "threads": self._workers if self._async else 0,
                "batches": self._batches, "files": self._files_staged,
                "wait_ms": self._wait_s * 1e3}

    def close(self):
        """stops the staging workers (idempotent; also run when the reader is dropped)"""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        self._stop_workers()

    def _stop_workers(self):
        for _ in self._threads:
            self._tasks.put(None)
        if not sys.is_finalizing():  # (at interpreter exit daemon threads no longer run)
            for t in self._threads:
                t.join()
        self._threads = []
        if self._async:
            self._fjobs, self._issued = [], []
            self._slots = [{"pin": None, "np": None, "dev": None, "event": None}
                           for _ in range(self._ring)]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def next_batch(self):
        if self._closed:
            raise RuntimeError("ParquetReader: next_batch() after close()")
        if self._cache_n and len(self._cache) >= self._cache_n:
            b = self._cache[self._served % self._cache_n]
            self._served += 1
            self._batches += 1
            return b
        b = self._next_device() if self._async else self._next_host()
        if b is None:
            return None
        self._batches += 1
        if self._cache_n:
            self._cache.append(b)
            self._served += 1
            if len(self._cache) >= self._cache_n:
                self._stop_workers()  # nothing further is read
        return b

    # ---- the asynchronous path ---------------------------------------------------------------------
    def _check_schemas(self) -> bool:
        """footers of all files (no data is read): True when every label / dense / categorical
        column of every file has one of the accepted physical types, the same in all files"""
        names = self.label_cols + self.cont_cols + self.cat_cols
        ncat0 = len(self.label_cols) + len(self.cont_cols)
        self._columns, self._file_rows, self._file_values = None, [], []
        for f in self.files:
            schema, rows, nv = _parquet_file_info(f)
            cols = []
            for i, n in enumerate(names):
                phys = parquet_physical(schema.field(n).type, i >= ncat0) \
                    if n in schema.names and n in nv else None
                if phys is None:
                    return False
                cols.append(phys)
            if self._columns is None:
                self._columns = cols
            elif cols != self._columns:
                return False
            self._file_rows.append(rows)
            self._file_values.append([nv[n] for n in names])
        return self._columns is not None

    def _start_device(self):
        self._stream = torch.cuda.Stream(device=self.device)
        self._slots = [{"pin": None, "np": None, "dev": None, "event": None}
                       for _ in range(self._ring)]
        self._plan = None        # built by the first next_batch(): ebc_groups is set after
        self._fjobs = []         # files staged or being staged, oldest first
        self._issued = []        # batches on the side stream, oldest first
        self._stage_idx, self._stage_row = 0, 0   # next file to stage / its first row
        self._fseq, self._issued_total = 0, 0
        self._mean_keys = None

    def _ensure_workers(self):
        if self._threads:
            return
        self._tasks = queue.Queue()
        self._threads = [threading.Thread(target=_stage_worker, args=(self._tasks,), daemon=True,
                                          name=f"hctr-parquet-stage-{i}")
                         for i in range(self._workers)]
        for t in self._threads:
            t.start()

    def decode_plan(self, mean_keys=None):
        """parquet_decode_plan of this reader's configuration (host arrays only)"""
        return parquet_decode_plan(self._columns, len(self.label_cols), len(self.cont_cols),
                                   [(p.top_name, p.slot_num) for p in self.inp.sparse_params],
                                   self._ebc_groups, self.slot_offsets, self.batch, self.rank,
                                   self.world, self.key_dtype == torch.int64, mean_keys)

    def _build_plan(self):
        from . import _lib
        if self._mean_keys is None:
            # mean keys per sample of every param, from the footers: the value count of a list
            # column (an empty list counts once), 1 per row of a scalar column
            self._mean_keys, rows = {}, max(1, sum(self._file_rows))
            c = len(self.label_cols) + len(self.cont_cols)
            for p in self.inp.sparse_params:
                tot = sum(sum(nv[c:c + p.slot_num]) for nv in self._file_values)
                self._mean_keys[p.top_name] = tot / rows
                c += p.slot_num
        pl = self.decode_plan(self._mean_keys)
        blob = np.concatenate([pl["segments"].view(np.uint8).reshape(-1),
                               pl["addend"].view(np.uint8), pl["list"].view(np.uint8)])
        with torch.cuda.stream(self._stream):  # (read by the decode launches of that stream)
            pl["device"] = torch.from_numpy(blob).to(self.device)
        # tensors that do not depend on the data: built once with the host path's arithmetic and
        # handed out with every batch (nothing downstream writes them, DESIGN.md "Raw reader")
        B = self.batch
        pl["ro"] = {name: torch.from_numpy(np.arange(B * S + 1, dtype=np.int64))
                    .to(self.device, self.key_dtype)
                    for name, (o_ro, _, S) in pl["sparse"].items() if o_ro is None}
        pl["gbr"] = [torch.from_numpy(np.arange(n * B + 1, dtype=np.int64)).to(self.device)
                     if o_br is None else None for _, o_br, n in pl["ebc"]]
        pl["spec"] = {"names": self.label_cols + self.cont_cols + self.cat_cols,
                      "cats": tuple(self.cat_cols), "columns": [tuple(c) for c in self._columns],
                      "batch": B, "outputs": pl["outputs"]}
        self._plan = pl

    def _submit_stage(self) -> bool:
        """hands the next file to the workers, into the slot whose file was dropped longest ago"""
        if self._cache_n and self._issued_total >= self._cache_n:
            return False
        idx = self._stage_idx
        if idx >= len(self.files):
            if not self.repeat:
                return False
            idx = 0
        self._stage_idx = idx + 1
        assert len(self._fjobs) < self._ring
        slot = self._slots[self._fseq % self._ring]
        self._fseq += 1
        pl = self._plan
        need = parquet_slot_layout(pl["spec"]["columns"], len(pl["outputs"]), self.batch,
                                   self._file_rows[idx], self._file_values[idx])[2]
        if slot["pin"] is None or slot["pin"].numel() < need:  # grow-only
            slot["pin"] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
            slot["np"] = slot["pin"].numpy()
        latch = _Latch(1)
        self._ensure_workers()
        self._tasks.put((slot["event"], slot["np"], self.files[idx], pl["spec"], latch))
        self._fjobs.append({"idx": idx, "slot": slot, "latch": latch, "row": self._stage_row,
                            "up": False})
        self._stage_row = 0
        return True

    def _fill_ring(self):
        while len(self._fjobs) < self._ring and self._submit_stage():
            pass

    def _copy_up(self, fj):
        """side stream: the staged file pinned -> device, once"""
        t0 = time.perf_counter()
        fj["latch"].done.wait()
        self._wait_s += time.perf_counter() - t0
        if fj["latch"].error is not None:
            self._fjobs.pop(0)
            raise fj["latch"].error
        res, slot = fj["latch"].result, fj["slot"]
        fj["res"], fj["up"] = res, True
        self._files_staged += 1
        if res["rows"] < self.batch:
            self._fjobs.pop(0)
            raise RuntimeError("parquet file holds fewer rows than one batch")
        with torch.cuda.stream(self._stream):
            # device buffers are used on the side stream only, so they come from its pool:
            # dropped with a decode in flight, their memory goes back to the stream that uses it
            if slot["dev"] is None or slot["dev"].numel() < res["used"]:
                slot["dev"] = torch.empty(slot["pin"].numel(), dtype=torch.uint8,
                                          device=self.device)
            slot["dev"][:res["used"]].copy_(slot["pin"][:res["used"]], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        slot["event"] = ev

    def _issue_one(self) -> bool:
        """side stream: one decode launch of the next batch into a fresh arena, an event"""
        from . import _lib
        if self._cache_n and self._issued_total >= self._cache_n:
            return False
        B = self.batch
        while True:
            self._fill_ring()
            if not self._fjobs:
                return False
            fj = self._fjobs[0]
            if not fj["up"]:
                self._copy_up(fj)
            if fj["row"] + B <= fj["res"]["rows"]:
                break
            self._fjobs.pop(0)  # the incomplete tail is dropped; the slot takes the next file
        res, dev, pl = fj["res"], fj["slot"]["dev"], self._plan
        a, k = fj["row"], fj["row"] // B
        fj["row"] += B
        n_out = len(pl["outputs"])
        nseg = len(pl["segments"])
        with torch.cuda.stream(self._stream):
            arena = torch.empty(max(int(res["tab"][k, n_out]), 256), dtype=torch.uint8,
                                device=self.device)
            tab = dev[res["tab_off"] + k * (n_out + 1) * 8:]
            _lib.check(_lib.lib.hctr_parquet_decode(
                _lib.ptr(dev), _lib.ptr(dev), len(self._columns), _lib.ptr(pl["device"]), nseg,
                len(pl["list"]), pl["n_items"], res["rows"], a, B, _lib.ptr(arena), _lib.ptr(tab),
                n_out, ctypes.c_void_p(self._stream.cuda_stream)))
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._issued.append({"arena": arena, "event": ev, "tab": res["tab"][k], "cnt": res["cnt"][k],
                             "pos": (fj["idx"], a)})
        self._issued_total += 1
        return True

    def _rewind(self):
        """forgets the files and batches in flight: the next batch handed out is read again"""
        for fj in self._fjobs:
            fj["latch"].done.wait()
        if self._issued:
            self._stage_idx, self._stage_row = self._issued[0]["pos"]
        elif self._fjobs:
            self._stage_idx, self._stage_row = self._fjobs[0]["idx"], self._fjobs[0]["row"]
        self._issued_total -= len(self._issued)
        self._fjobs, self._issued = [], []

    def _next_device(self):
        if self._plan is None:
            self._build_plan()
        # this batch and the next one are on the side stream before this one is handed over
        while len(self._issued) < 2 and self._issue_one():
            pass
        if not self._issued:
            return None
        job = self._issued.pop(0)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(job["event"])
        arena, pl, tab, cnt = job["arena"], self._plan, job["tab"], job["cnt"]
        arena.record_stream(cur)  # allocated on the side stream, consumed on this one

        def cut(o, dtype):
            n = int(cnt[o]) * pl["outputs"][o]["esize"]
            return arena[int(tab[o]):int(tab[o]) + n].view(dtype)

        (lo, lshape), (do, dshape) = pl["label"], pl["dense"]
        out = {"label": cut(lo, torch.float32).view(*lshape),
               "dense": cut(do, torch.float32).view(*dshape), "sparse": {}}
        for name, (o_ro, o_k, _) in pl["sparse"].items():
            ro = pl["ro"][name] if o_ro is None else cut(o_ro, self.key_dtype)
            out["sparse"][name] = (ro, cut(o_k, self.key_dtype))
        if self._ebc_groups:
            out["ebc"] = [(cut(o_k, torch.int64),
                           pl["gbr"][g] if o_br is None else cut(o_br, torch.int64))
                          for g, (o_k, o_br, _) in enumerate(pl["ebc"])]
        return out

    # ---- the host path -----------------------------------------------------------------------------
    def _load_next_file(self) -> bool:
        if self._file_idx >= len(self.files):
            if not self.repeat:
                return False
            self._file_idx = 0
        t = self.pq.read_table(self.files[self._file_idx])
        self._file_idx += 1
        self._files_staged += 1
        label = np.stack([t[c].to_numpy() for c in self.label_cols], 1).astype(np.float32)
        dense = (np.stack([t[c].to_numpy() for c in self.cont_cols], 1).astype(np.float32)
                 if self.cont_cols else np.zeros((t.num_rows, 0), np.float32))
        cats = []
        for s, c in enumerate(self.cat_cols):
            col = t[c]
            if str(col.type).startswith(("list", "large_list")):
                # multi-hot column: (row offsets, flat keys) straight from the Arrow buffers
                arr = col.combine_chunks()
                off = arr.offsets.to_numpy().astype(np.int64)
                vals = arr.values.to_numpy().astype(np.int64)[off[0]:off[-1]] + self.slot_offsets[s]
                cats.append((off - off[0], vals))
            else:
                cats.append(col.to_numpy().astype(np.int64) + self.slot_offsets[s])
        self._buf, self._pos = (label, dense, cats), 0
        return True

    def _next_host(self):
        B = self.batch
        if self._buf is None or self._pos + B > self._buf[0].shape[0]:
            # the reference drops the incomplete tail of a file (drop_incomplete_batch=True)
            if not self._load_next_file():
                return None
            if self._buf[0].shape[0] < B:
                raise RuntimeError("parquet file holds fewer rows than one batch")
        label, dense, cats = self._buf
        a, b = self._pos, self._pos + B
        self._pos = b
        bpg = B // self.world
        sl = slice(a + self.rank * bpg, a + (self.rank + 1) * bpg)
        out = {"label": torch.from_numpy(label[sl]).to(self.device),
               "dense": torch.from_numpy(dense[sl]).to(self.device), "sparse": {}}
        # one DataReaderSparseParam may cover a contiguous group of slots
        s0 = 0
        for p in self.inp.sparse_params:
            group = cats[s0:s0 + p.slot_num]
            s0 += p.slot_num
            if all(isinstance(g, np.ndarray) for g in group):  # one-hot fast path
                keys = np.stack([g[a:b] for g in group], 1).reshape(-1)
                ro = np.arange(B * p.slot_num + 1, dtype=np.int64)
            else:
                # ragged group: bucket (sample, slot) order, vectorised per slot
                lens = np.empty((B, p.slot_num), np.int64)
                for s, g in enumerate(group):
                    lens[:, s] = (g[0][a + 1:b + 1] - g[0][a:b]) if isinstance(g, tuple) else 1
                ro = np.concatenate([[0], np.cumsum(lens.reshape(-1))]).astype(np.int64)
                keys = np.empty(int(ro[-1]), np.int64)
                starts = ro[:-1].reshape(B, p.slot_num)
                for s, g in enumerate(group):
                    if isinstance(g, tuple):
                        off, vals = g
                        seg = vals[off[a]:off[b]]
                        # destination of every key: its bucket's start + position inside the bucket
                        inner = np.arange(seg.size) - np.repeat(off[a:b] - off[a], lens[:, s])
                        keys[np.repeat(starts[:, s], lens[:, s]) + inner] = seg
                    else:
                        keys[starts[:, s]] = g[a:b]
            kt = torch.from_numpy(keys)
            rt = torch.from_numpy(ro)
            if self.key_dtype != torch.int64:
                kt, rt = kt.to(torch.int32), rt.to(torch.int32)
            out["sparse"][p.top_name] = (rt.to(self.device), kt.to(self.device))
        if self.ebc_groups:  # the collections' global feature-major CSRs, raw keys
            out["ebc"] = []
            for names in self.ebc_groups:
                ks, lens = [], []
                for n in names:
                    s, slots = self._slot_of[n]
                    assert slots == 1, "embedding_collection inputs carry one slot per lookup"
                    g = cats[s]
                    if isinstance(g, tuple):
                        off, vals = g
                        ks.append(vals[off[a]:off[b]] - self.slot_offsets[s])
                        lens.append(off[a + 1:b + 1] - off[a:b])
                    else:
                        ks.append(g[a:b] - self.slot_offsets[s])
                        lens.append(np.ones(B, np.int64))
                gbr = np.zeros(len(names) * B + 1, np.int64)
                np.cumsum(np.concatenate(lens), out=gbr[1:])
                out["ebc"].append((torch.from_numpy(np.concatenate(ks).astype(np.int64)).to(self.device),
                                   torch.from_numpy(gbr).to(self.device)))
        return out


# ---- Raw format (docs/source/api/python_interface.md "Raw"; R/HugeCTR/src/data_readers/multi_hot/) ---
# one binary file, fixed-size samples: label[label_dim] dense[dense_dim] keys[sum of hotness], every
# field 4 bytes: label/dense float32 (float_label_dense / is_dense_float) or int32/uint32 (dense is
# then fed through log(x + 1)), keys uint32 with STATIC hotness per slot taken from the Input layer.
def write_raw(path, label, dense, cats, float_label_dense=True):
    """cats: [num_samples, sum_hotness] keys in slot-major order"""
    n = label.shape[0]
    ld = (np.asarray(label, np.float32) if float_label_dense else np.asarray(label, np.int32))
    dd = (np.asarray(dense, np.float32) if float_label_dense else np.asarray(dense, np.uint32))
    rec = np.concatenate([ld.view(np.uint32).reshape(n, -1), dd.view(np.uint32).reshape(n, -1),
                          np.asarray(cats, np.uint32).reshape(n, -1)], axis=1)
    rec.astype("<u4").tofile(path)


def _up256(n: int) -> int:
    return (n + 255) & ~255


def raw_decode_plan(label_dim, dense_dim, params, ebc_groups, slot_offsets, batch, rank, world,
                    float_label, float_dense, i64_key):
    """What one hctr_raw_decode launch writes for one global batch (include/hugectr_amd.h), worked
    out once per reader.  params: [(top_name, [hotness per slot])] in record order; ebc_groups:
    per collection the top_names of its lookups' inputs; slot_offsets: one per slot.
    -> {"width", "segments" (hctr_raw_segment records), "addend" (int64 per column),
        "arena_bytes", "label" / "dense": (byte offset, shape), "sparse": {name: (offset, n)},
        "ebc": [(offset, n)]}; every output starts on a 256-byte boundary of the arena."""
    from . import _lib
    L, Dn, B = int(label_dim), int(dense_dim), int(batch)
    bpg = B // world
    width = L + Dn + sum(sum(h) for _, h in params)
    segs, addend, top = [], np.zeros(width, np.int64), [0]

    def take(nbytes):
        off = top[0]
        top[0] = _up256(off + nbytes)
        return off

    def seg(col0, ncols, kind, s0, s1, off):
        if ncols > 0 and s1 > s0:
            segs.append((col0, ncols, kind, 0, s0, s1, off))

    plan = {"width": width, "sparse": {}, "ebc": []}
    plan["label"] = (take(bpg * L * 4), (bpg, L))
    seg(0, L, _lib.RAW_BITS if float_label else _lib.RAW_I2F, rank * bpg, (rank + 1) * bpg,
        plan["label"][0])
    plan["dense"] = (take(bpg * Dn * 4), (bpg, Dn))
    seg(L, Dn, _lib.RAW_BITS if float_dense else _lib.RAW_LOG1P, rank * bpg, (rank + 1) * bpg,
        plan["dense"][0])
    ksz, kind = (8, _lib.RAW_KEY_I64) if i64_key else (4, _lib.RAW_KEY_I32)
    col, s0, col_of = L + Dn, 0, {}
    for name, hot in params:
        w = sum(hot)
        addend[col:col + w] = np.repeat(np.asarray(slot_offsets[s0:s0 + len(hot)], np.int64), hot)
        off = take(B * w * ksz)
        seg(col, w, kind, 0, B, off)
        plan["sparse"][name] = (off, B * w)
        col_of[name] = (col, w)
        col += w
        s0 += len(hot)
    for names in ebc_groups:
        n = sum(col_of[nm][1] for nm in names) * B
        off = take(n * 8)
        plan["ebc"].append((off, n))
        for nm in names:  # bucket = lookup * batch + sample: one segment per lookup, back to back
            c0, w = col_of[nm]
            seg(c0, w, _lib.RAW_RAWKEY_I64, 0, B, off)
            off += B * w * 8
    plan["arena_bytes"] = max(top[0], 256)
    plan["segments"] = np.array(segs, dtype=np.dtype(_lib.RAW_SEGMENT_FIELDS))
    plan["addend"] = addend
    if not 1 <= len(segs) <= _lib.RAW_DECODE_MAX_SEGMENTS:
        raise RuntimeError(f"raw reader: {len(segs)} output segments (1..4096 supported)")
    esz = {_lib.RAW_KEY_I64: 8, _lib.RAW_RAWKEY_I64: 8}
    for g in plan["segments"]:  # every destination range lies inside the arena
        end = int(g["dst_offset"]) + int(g["sample1"] - g["sample0"]) * int(g["ncols"]) * \
            esz.get(int(g["kind"]), 4)
        assert end <= plan["arena_bytes"] and int(g["col0"]) + int(g["ncols"]) <= width
    return plan


def _fill_worker(tasks):
    """worker thread of the asynchronous reader: (event of the slot's last decode, destination rows
    of the pinned slot, source rows of the memmap, latch).  Holds no reference to the reader."""
    while True:
        t = tasks.get()
        if t is None:
            return
        ev, dst, src, latch = t
        try:
            if ev is not None:
                ev.synchronize()  # the slot is free once its last batch has been decoded
            np.copyto(dst, src)   # (releases the GIL)
            latch.part_done()
        except BaseException as e:  # handed to next_batch()
            latch.part_done(e)
        del t, ev, dst, src, latch


class RawReader:
    """DataReaderType_t.RawAsync: streams batches of a Raw file (np.memmap; the reference uses
    Linux AIO worker threads -- I/O engines are outside the scope contract, the FORMAT is not).

    On a CUDA device the reader is asynchronous (DESIGN.md "Raw reader"): worker threads copy the
    records of the coming batches into a ring of pinned slots, a side stream copies a slot up and
    splits it with ONE launch (hctr_raw_decode), and next_batch() only makes the consumer's stream
    wait for that launch.  On a CPU device the batch is decoded on the host, as it always was."""

    def __init__(self, path: str, inp, slot_size_array, batch, rank, world, device, num_samples,
                 float_label_dense: bool, repeat: bool, async_param=None, i64_key: bool = True):
        self.inp, self.batch, self.rank, self.world, self.device = inp, batch, rank, world, device
        self.repeat = repeat
        # keys AND row offsets carry the model's key type (solver.i64_input_key), as the
        # reference's SparseTensor<TypeKey> does
        self.key_dtype = torch.int64 if i64_key else torch.int32
        # two conventions exist in the reference:
        # * the multi-hot async reader (AsyncParam, split_batch.cu:28-66): the label word is ALWAYS
        #   an int32 (cast to float), dense words are floats when is_dense_float else ints fed
        #   through log(x + 1) -- the MLPerf raw files (samples/dlrm/preprocessing/convert_to_raw.py);
        # * files of the data generator (data_generator.hpp:977-1040): float_label_dense decides
        #   for label AND dense together.
        if async_param is not None and getattr(async_param, "multi_hot_reader", True):
            self.float_label, self.float_dense = False, bool(async_param.is_dense_float)
        else:
            self.float_label = self.float_dense = bool(float_label_dense)
        self.hot = []  # static hotness per slot, over all sparse params
        for p in inp.sparse_params:
            h = p.nnz_per_slot
            self.hot += list(h) if isinstance(h, (list, tuple)) else [int(h)] * p.slot_num
        self.width = inp.label_dim + inp.dense_dim + sum(self.hot)
        words = os.path.getsize(path) // 4
        n = words // self.width
        if num_samples:
            n = min(n, int(num_samples))
        if n < batch:
            raise RuntimeError("raw file holds fewer samples than one batch")
        self.data = np.memmap(path, dtype="<u4", mode="r", shape=(n, self.width))
        self.n, self._pos = n, 0
        ssa = list(slot_size_array)
        self.slot_offsets = (np.concatenate([[0], np.cumsum(ssa)[:-1]]).astype(np.int64) if ssa
                             else np.zeros(len(self.hot), np.int64))
        # embedding_collection models: Model.compile names, per collection, the inputs of its
        # lookups in lookup order; the reader then hands over the collection's global
        # feature-major CSR (raw keys, bucket = lookup * batch + sample) ready-made -- cutting it
        # out of 26 per-input tensors on the GPU costs ~100 tiny launches per step
        self._ebc_groups = []
        self._col_of = {}
        col, s0 = inp.label_dim + inp.dense_dim, 0
        for p in inp.sparse_params:
            hot = self.hot[s0:s0 + p.slot_num]
            self._col_of[p.top_name] = (col, sum(hot), p.slot_num)
            col += sum(hot)
            s0 += p.slot_num
        self._batches, self._wait_s = 0, 0.0
        self._async = torch.device(device).type == "cuda"
        self._threads, self._closed = [], False
        if self._async:
            self._start_async(async_param)

    def _start_async(self, async_param):
        """ring, side stream and fill workers.  AsyncParam: num_batches_per_thread = slots of the
        ring (at least 2), num_threads = fill workers (at most 8; never sized by the machine)"""
        self._ring = max(2, int(getattr(async_param, "num_batches_per_thread", 0) or 0))
        nthreads = max(1, min(8, int(getattr(async_param, "num_threads", 0) or 2)))
        self._stream = torch.cuda.Stream(device=self.device)
        self._slots = []
        for _ in range(self._ring):
            pin = torch.empty((self.batch, self.width), dtype=torch.int32, pin_memory=True)
            # the device raw buffers (and the plan, _build_plan) are used on the side stream only,
            # so they come from its pool: dropped with a decode in flight, their memory goes
            # back to the stream that still uses it
            with torch.cuda.stream(self._stream):
                dev = torch.empty((self.batch, self.width), dtype=torch.int32, device=self.device)
            self._slots.append((pin, pin.numpy().view(np.uint32), dev))
        self._tasks = queue.Queue()
        self._threads = [threading.Thread(target=_fill_worker, args=(self._tasks,), daemon=True,
                                          name=f"hctr-raw-fill-{i}") for i in range(nthreads)]
        for t in self._threads:
            t.start()
        self._plan = None       # built by the first next_batch(): ebc_groups is set after
        self._pending = []      # batches in flight, oldest first
        self._slot_event = [None] * self._ring
        self._seq = 0           # batches planned so far (slot = seq % ring)

    @property
    def ebc_groups(self):
        return self._ebc_groups

    @ebc_groups.setter
    def ebc_groups(self, groups):
        self._ebc_groups = groups
        if self._async and self._plan is not None:
            self._rewind()  # (batches in flight were split by the old plan)
            self._plan = None

    def stats(self):
        """decode: where a batch is split; ring / threads: slots and fill workers of the
        asynchronous path (0 on the host path); batches: handed out so far; wait_ms: total time
        next_batch() waited for a fill worker"""
        return {"decode": "device" if self._async else "host",
                "ring": self._ring if self._async else 0, "threads": len(self._threads),
                "batches": self._batches, "wait_ms": self._wait_s * 1e3}

    def close(self):
        """stops the fill workers (idempotent; also run when the reader is dropped)"""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        for _ in self._threads:
            self._tasks.put(None)
        if not sys.is_finalizing():  # (at interpreter exit daemon threads no longer run)
            for t in self._threads:
                t.join()
        self._threads = []
        if self._async:
            self._pending = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the asynchronous path ---------------------------------------------------------------------
    def _params(self):
        """[(top_name, [hotness per slot])] in record order"""
        params, s0 = [], 0
        for p in self.inp.sparse_params:
            params.append((p.top_name, [int(h) for h in self.hot[s0:s0 + p.slot_num]]))
            s0 += p.slot_num
        return params

    def decode_plan(self):
        """raw_decode_plan of this reader's configuration (host arrays only)"""
        for names in self._ebc_groups:
            for n in names:
                assert self._col_of[n][2] == 1, "embedding_collection inputs carry one slot per lookup"
        return raw_decode_plan(self.inp.label_dim, self.inp.dense_dim, self._params(),
                               self._ebc_groups, self.slot_offsets, self.batch, self.rank,
                               self.world, self.float_label, self.float_dense,
                               self.key_dtype == torch.int64)

    def _build_plan(self):
        params, pl = self._params(), self.decode_plan()
        blob = np.concatenate([pl["segments"].view(np.uint8).reshape(-1),
                               pl["addend"].view(np.uint8)])
        with torch.cuda.stream(self._stream):  # (read by the decode launches of that stream)
            pl["device"] = torch.from_numpy(blob).to(self.device)
        # row offsets / bucket ranges follow from the static hotness alone: built once with the
        # host path's arithmetic and handed out with every batch (nothing downstream writes them)
        B = self.batch
        pl["ro"] = {}
        for name, hot in params:
            ro = np.concatenate([[0], np.cumsum(np.tile(hot, B))]).astype(np.int64)
            pl["ro"][name] = torch.from_numpy(ro).to(self.device, self.key_dtype)
        pl["gbr"] = []
        for names in self._ebc_groups:
            lens = [np.full(B, self._col_of[n][1], np.int64) for n in names]
            gbr = np.zeros(len(names) * B + 1, np.int64)
            np.cumsum(np.concatenate(lens), out=gbr[1:])
            pl["gbr"].append(torch.from_numpy(gbr).to(self.device))
        self._plan = pl

    def _plan_next(self):
        """file position of the next batch, as the host path walks the file; None at its end"""
        B = self.batch
        if self._pos + B > self.n:  # incomplete tail dropped, as the reference does
            if not self.repeat:
                return None
            self._pos = 0
        pos = self._pos
        self._pos += B
        return pos

    def _submit_fill(self):
        """plans the next batch and hands its records to the workers, each a contiguous range of
        samples; the slot's last decode must be through before a worker writes into it"""
        pos = self._plan_next()
        if pos is None:
            return
        slot = self._seq % self._ring
        assert all(j["slot"] != slot or j["event"] is not None for j in self._pending)
        self._seq += 1
        B, T = self.batch, len(self._threads)
        cuts = [B * i // T for i in range(T + 1)]
        parts = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        latch = _Latch(len(parts))
        dst = self._slots[slot][1]
        for a, b in parts:
            self._tasks.put((self._slot_event[slot], dst[a:b], self.data[pos + a:pos + b], latch))
        self._pending.append({"pos": pos, "slot": slot, "latch": latch, "event": None})

    def _issue(self, job):
        """side stream: pinned slot -> device, one decode launch into a fresh arena, an event"""
        from . import _lib
        t0 = time.perf_counter()
        job["latch"].done.wait()
        self._wait_s += time.perf_counter() - t0
        if job["latch"].error is not None:
            raise job["latch"].error
        pin, _, dev = self._slots[job["slot"]]
        pl = self._plan
        with torch.cuda.stream(self._stream):
            dev.copy_(pin, non_blocking=True)
            arena = torch.empty(pl["arena_bytes"], dtype=torch.uint8, device=self.device)
            _lib.check(_lib.lib.hctr_raw_decode(
                _lib.ptr(dev), self.batch, self.width, _lib.ptr(pl["device"]), len(pl["segments"]),
                _lib.ptr(arena), ctypes.c_void_p(self._stream.cuda_stream)))
            ev = torch.cuda.Event()
            ev.record(self._stream)
        job["arena"], job["event"] = arena, ev
        self._slot_event[job["slot"]] = ev

    def _rewind(self):
        """forgets the batches in flight: the next one handed out is read again"""
        for job in self._pending:
            job["latch"].done.wait()
        if self._pending:
            self._pos = self._pending[0]["pos"]
        self._pending = []

    def _next_async(self):
        if self._closed:
            raise RuntimeError("RawReader: next_batch() after close()")
        if self._plan is None:
            self._build_plan()
        while len(self._pending) < self._ring:  # (first call, or after a rewind)
            n = len(self._pending)
            self._submit_fill()
            if len(self._pending) == n:
                break
        if not self._pending:
            return None
        # this batch and the next one are on the side stream before this one is handed over
        for job in self._pending[:2]:
            if job["event"] is None:
                self._issue(job)
                self._submit_fill()  # the slot's next batch: its workers wait for this decode
        job = self._pending.pop(0)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(job["event"])
        arena, pl = job["arena"], self._plan
        arena.record_stream(cur)  # allocated on the side stream, consumed on this one

        def cut(off, n, dtype, esz):
            return arena[off:off + n * esz].view(dtype)

        (lo, lshape), (do, dshape) = pl["label"], pl["dense"]
        out = {"label": cut(lo, lshape[0] * lshape[1], torch.float32, 4).view(*lshape),
               "dense": cut(do, dshape[0] * dshape[1], torch.float32, 4).view(*dshape),
               "sparse": {}}
        ksz = 8 if self.key_dtype == torch.int64 else 4
        for name, (off, n) in pl["sparse"].items():
            out["sparse"][name] = (pl["ro"][name], cut(off, n, self.key_dtype, ksz))
        if self._ebc_groups:
            out["ebc"] = [(cut(off, n, torch.int64, 8), pl["gbr"][g])
                          for g, (off, n) in enumerate(pl["ebc"])]
        self._batches += 1
        return out

    def next_batch(self):
        if self._async:
            return self._next_async()
        B = self.batch
        if self._pos + B > self.n:  # incomplete tail dropped, as the reference does
            if not self.repeat:
                return None
            self._pos = 0
        blk = np.asarray(self.data[self._pos:self._pos + B])
        self._pos += B
        L, Dn = self.inp.label_dim, self.inp.dense_dim
        bpg = B // self.world
        sl = slice(self.rank * bpg, (self.rank + 1) * bpg)
        label = (blk[:, :L].view(np.float32) if self.float_label
                 else blk[:, :L].view(np.int32).astype(np.float32))
        dense = (blk[:, L:L + Dn].view(np.float32) if self.float_dense
                 else np.log(blk[:, L:L + Dn].view(np.int32).astype(np.float32) + np.float32(1.0)))
        out = {"label": torch.from_numpy(np.ascontiguousarray(label[sl])).to(self.device),
               "dense": torch.from_numpy(np.ascontiguousarray(dense[sl])).to(self.device),
               "sparse": {}}
        col, s0 = L + Dn, 0
        for p in self.inp.sparse_params:
            hot = self.hot[s0:s0 + p.slot_num]
            w = sum(hot)
            keys = blk[:, col:col + w].astype(np.int64)
            offs = np.repeat(self.slot_offsets[s0:s0 + p.slot_num], hot)
            keys = (keys + offs[None, :]).reshape(-1)
            ro = np.concatenate([[0], np.cumsum(np.tile(hot, B))]).astype(np.int64)
            col += w
            s0 += p.slot_num
            out["sparse"][p.top_name] = (torch.from_numpy(ro).to(self.device, self.key_dtype),
                                         torch.from_numpy(keys).to(self.device, self.key_dtype))
        if self.ebc_groups:
            out["ebc"] = []
            for names in self.ebc_groups:
                ks, lens = [], []
                for n in names:
                    c0, w, slots = self._col_of[n]
                    assert slots == 1, "embedding_collection inputs carry one slot per lookup"
                    ks.append(blk[:, c0:c0 + w].astype(np.int64).reshape(-1))
                    lens.append(np.full(B, w, np.int64))
                gbr = np.zeros(len(names) * B + 1, np.int64)
                np.cumsum(np.concatenate(lens), out=gbr[1:])
                out["ebc"].append((torch.from_numpy(np.concatenate(ks)).to(self.device),
                                   torch.from_numpy(gbr).to(self.device)))
        self._batches += 1
        return out


class _Readers:
    def __init__(self, train, evalr):
        self.train, self.evalr = train, evalr

    def next_batch(self, train: bool):
        r = self.train if train else self.evalr
        return None if r is None else r.next_batch()

    def has_eval(self) -> bool:
        return self.evalr is not None


def _resolve(path: str) -> str:
    """a dataset path of a script as is, or -- when it does not exist and HCTR_DATA_ROOT is set --
    under that root (scripts of the reference name absolute container paths like
    /data/train_data.bin, R/test/embedding_collection_test/dgx_a100_one_hot.py:236-237)"""
    root = os.environ.get("HCTR_DATA_ROOT")
    if path and root and not os.path.exists(path):
        cand = os.path.join(root, path.lstrip("/"))
        if os.path.exists(cand):
            return cand
    return path


def make_reader(rp, inp, solver, rank, world, device, parquet_decode="auto"):
    """parquet_decode: ParquetReader's decode ("host" keeps a CUDA device's readers on the host path)"""
    fmt = getattr(rp.data_reader_type, "name", str(rp.data_reader_type))
    import copy
    rp = copy.copy(rp)
    rp.source = [_resolve(p) for p in rp.source]
    rp.eval_source = _resolve(rp.eval_source)
    if fmt == "RawAsync":
        train = RawReader(rp.source[0], inp, rp.slot_size_array, solver.batchsize, rank, world,
                          device, rp.num_samples, rp.float_label_dense, solver.repeat_dataset,
                          rp.async_param, solver.i64_input_key)
        evalr = None
        if rp.eval_source and os.path.exists(rp.eval_source) and solver.batchsize_eval > 0:
            evalr = RawReader(rp.eval_source, inp, rp.slot_size_array, solver.batchsize_eval, rank,
                              world, device, rp.eval_num_samples, rp.float_label_dense, True,
                              rp.async_param, solver.i64_input_key)
        return _Readers(train, evalr)
    if fmt != "Parquet":
        # the reference's Python path rejects Norm/Raw as deprecated (add_input.cpp:318-325)
        raise RuntimeError(f"DataReaderType_t.{fmt} is deprecated in the reference and not supported; "
                           "use Parquet")
    train = ParquetReader(rp.source[0], inp, rp.slot_size_array, solver.batchsize, rank, world,
                          device, solver.i64_input_key, solver.repeat_dataset,
                          num_workers=rp.num_workers, decode=parquet_decode)
    evalr = None
    if rp.eval_source and os.path.exists(rp.eval_source) and solver.batchsize_eval > 0:
        evalr = ParquetReader(rp.eval_source, inp, rp.slot_size_array, solver.batchsize_eval, rank,
                              world, device, solver.i64_input_key, True,
                              num_workers=rp.num_workers, cache_batches=rp.cache_eval_data,
                              decode=parquet_decode)
    return _Readers(train, evalr)
