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


class ParquetReader:
    """Streams batches from a reference-layout Parquet dataset."""

    def __init__(self, file_list: str, inp, slot_size_array, batch, rank, world, device, i64_key,
                 repeat: bool):
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
        self.ebc_groups = []
        self._slot_of = {}
        s0 = 0
        for p in inp.sparse_params:
            self._slot_of[p.top_name] = (s0, p.slot_num)
            s0 += p.slot_num

    def _load_next_file(self) -> bool:
        if self._file_idx >= len(self.files):
            if not self.repeat:
                return False
            self._file_idx = 0
        t = self.pq.read_table(self.files[self._file_idx])
        self._file_idx += 1
        label = np.stack([t[c].to_numpy() for c in self.label_cols], 1).astype(np.float32)
        dense = (np.stack([t[c].to_numpy() for c in self.cont_cols], 1).astype(np.float32)
                 if self.cont_cols else np.zeros((t.num_rows, 0), np.float32))
        cats = []
        for s, c in enumerate(self.cat_cols):
            col = t[c]
            if str(col.type).startswith("list"):
                # multi-hot column: (row offsets, flat keys) straight from the Arrow buffers
                arr = col.combine_chunks()
                off = arr.offsets.to_numpy().astype(np.int64)
                vals = arr.values.to_numpy().astype(np.int64)[off[0]:off[-1]] + self.slot_offsets[s]
                cats.append((off - off[0], vals))
            else:
                cats.append(col.to_numpy().astype(np.int64) + self.slot_offsets[s])
        self._buf, self._pos = (label, dense, cats), 0
        return True

    def next_batch(self):
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


class _Latch:
    """counts the parts of one fill down; the training thread waits for zero"""

    def __init__(self, parts):
        self.left, self.lock, self.done, self.error = parts, threading.Lock(), threading.Event(), None

    def part_done(self, error=None):
        with self.lock:
            self.left -= 1
            if error is not None:
                self.error = error
            if self.left == 0:
                self.done.set()


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


def make_reader(rp, inp, solver, rank, world, device):
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
                          device, solver.i64_input_key, solver.repeat_dataset)
    evalr = None
    if rp.eval_source and os.path.exists(rp.eval_source) and solver.batchsize_eval > 0:
        evalr = ParquetReader(rp.eval_source, inp, rp.slot_size_array, solver.batchsize_eval, rank,
                              world, device, solver.i64_input_key, True)
    return _Readers(train, evalr)
