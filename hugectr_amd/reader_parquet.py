"""Reader of the reference's Parquet dataset layout (`_file_list.txt`, `_metadata.json`; data.py):
what a staged file looks like, the plan one hctr_parquet_decode launch gets, and ParquetReader, whose
device path runs on the shared prefetch pipeline (reader_prefetch.py) with one file per staged
unit."""
from __future__ import annotations

import functools
import json
import os
import time

import numpy as np
import torch

from .reader_prefetch import PrefetchReader, _Latch, _round_up, feature_major_csr


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
    top = _round_up(len(columns) * 24, 256)
    tab_off = top
    top = _round_up(top + (rows // batch) * (n_outputs + 1) * 8, 256)
    lay = []
    for (_, esz, is_list), nv in zip(columns, n_values):
        v = top
        top = _round_up(top + int(nv) * esz, 64)
        o = _lib.PQ_NO_OFFSETS
        if is_list:
            o = top
            top = _round_up(top + (rows + 1) * 8, 64)
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


def _stage_file(buf, path, spec, ev):
    """a worker's task: reads a file and stages it in buf, the pinned slot, once ev (after the
    slot's last copy up, or None) is through -> stage_parquet_table's dict + "stage_s\""""
    import pyarrow.parquet as pq
    t0 = time.perf_counter()
    # (Arrow's own pool is sized by the machine's CPU count: one thread, this one)
    table = pq.read_table(path, columns=spec["names"], use_threads=False)
    if table.num_rows < spec["batch"]:
        raise RuntimeError("parquet file holds fewer rows than one batch")
    if ev is not None:
        ev.synchronize()  # the pinned slot is free once its last file has been copied up
    res = stage_parquet_table(table, path, spec, buf)
    res["stage_s"] = time.perf_counter() - t0
    return res


class ParquetReader(PrefetchReader):
    """Streams batches from a reference-layout Parquet dataset.

    On a CUDA device the reader is asynchronous (DESIGN.md "Parquet reader"): worker threads read
    the coming files and stage their column buffers in pinned file slots, a side stream copies a
    staged file up once and turns its columns into a batch with ONE launch (hctr_parquet_decode),
    and next_batch() only makes the consumer's stream wait for that launch.  On a CPU device, with
    decode="host", or when a column has a type the kernel does not take, every batch is decoded on
    the host, as it always was.  cache_batches = N > 0: the first N batches are kept and handed out
    round-robin for ever (DataReaderParams.cache_eval_data).  ring: file slots (2 to 4);
    num_workers: staging workers (at most one per slot, at most 8)."""

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
        ring = min(4, max(2, int(ring)))
        super().__init__(inp, slot_size_array, len(self.cat_cols), batch, rank, world, device,
                         repeat, i64_key, ring=ring, workers=max(1, min(ring, int(num_workers), 8)),
                         thread_name="hctr-parquet-stage", cache_batches=cache_batches)
        self._file_idx, self._buf, self._pos = 0, None, 0   # the host path's place
        self._stage_idx, self._stage_row = 0, 0   # the device path's: next file to stage / its first row
        self._files_staged, self._mean_keys = 0, None
        if decode not in ("auto", "host", "device"):
            raise ValueError(f"ParquetReader: decode={decode!r} (auto, host or device)")
        on_device = decode != "host" and self._on_cuda and self._check_schemas()
        if decode == "device" and not on_device:
            raise RuntimeError("ParquetReader: decode='device' needs a CUDA device and label / "
                               "dense / categorical columns of the accepted types")
        if on_device:  # grow-only slots, sized by the files they meet
            self._start_device([{"pin": None, "np": None, "dev": None, "event": None}
                                for _ in range(self._ring)])

    def stats(self):
        """PrefetchReader.stats() and files: files staged (host path: read)"""
        return dict(super().stats(), files=self._files_staged)

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

    def decode_plan(self, mean_keys=None):
        """parquet_decode_plan of this reader's configuration (host arrays only)"""
        return parquet_decode_plan(self._columns, len(self.label_cols), len(self.cont_cols),
                                   [(p.top_name, p.slot_num) for p in self.inp.sparse_params],
                                   self._ebc_groups, self.slot_offsets, self.batch, self.rank,
                                   self.world, self.key_dtype == torch.int64, mean_keys)

    def decode_into(self, arena, unit, k, stream):
        """the one hctr_parquet_decode launch: batch k of the unit's file, staged in its device
        buffer -> arena (uint8, unit["latch"].result["tab"][k, -1] bytes) on stream (a pointer)"""
        from . import _lib
        pl, res, dev = self._plan, unit["latch"].result, unit["slot"]["dev"]
        n_out = len(pl["outputs"])
        tab = dev[res["tab_off"] + k * (n_out + 1) * 8:]
        _lib.check(_lib.lib.hctr_parquet_decode(
            _lib.ptr(dev), _lib.ptr(dev), len(self._columns), _lib.ptr(pl["device"]),
            len(pl["segments"]), len(pl["list"]), pl["n_items"], res["rows"], k * self.batch,
            self.batch, _lib.ptr(arena), _lib.ptr(tab), n_out, stream))

    # ---- what the prefetch pipeline asks for -------------------------------------------------------
    def _make_plan(self):
        if self._mean_keys is None:
            # mean keys per sample of every param, from the footers: the value count of a list
            # column (an empty list counts once), 1 per row of a scalar column
            self._mean_keys, rows = {}, max(1, sum(self._file_rows))
            c = len(self.label_cols) + len(self.cont_cols)
            for p in self.inp.sparse_params:
                tot = sum(sum(nv[c:c + p.slot_num]) for nv in self._file_values)
                self._mean_keys[p.top_name] = tot / rows
                c += p.slot_num
        pl, B = self.decode_plan(self._mean_keys), self.batch
        pl["upload"] = [pl["segments"], pl["addend"], pl["list"]]
        pl["ro"] = {name: np.arange(B * S + 1, dtype=np.int64)
                    for name, (o_ro, _, S) in pl["sparse"].items() if o_ro is None}
        pl["gbr"] = [np.arange(n * B + 1, dtype=np.int64) if o_br is None else None
                     for _, o_br, n in pl["ebc"]]
        pl["layout"] = (pl["label"], pl["dense"], {name: t[:2] for name, t in pl["sparse"].items()},
                        [t[:2] for t in pl["ebc"]])
        pl["spec"] = {"names": self.label_cols + self.cont_cols + self.cat_cols,
                      "cats": tuple(self.cat_cols), "columns": [tuple(c) for c in self._columns],
                      "batch": B, "outputs": pl["outputs"]}
        return pl

    def _seek(self, pos):
        self._stage_idx, self._stage_row = pos

    def _stage(self, slot):
        """hands the next file to the workers"""
        idx = self._stage_idx
        if idx >= len(self.files):
            if not self.repeat:
                return None
            idx = 0
        self._stage_idx = idx + 1
        pl = self._plan
        need = parquet_slot_layout(pl["spec"]["columns"], len(pl["outputs"]), self.batch,
                                   self._file_rows[idx], self._file_values[idx])[2]
        if slot["pin"] is None or slot["pin"].numel() < need:  # grow-only
            slot["pin"] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
            slot["np"] = slot["pin"].numpy()
        latch = _Latch(1)
        self._submit(functools.partial(_stage_file, slot["np"], self.files[idx], pl["spec"]),
                     slot["event"], latch)
        u = {"latch": latch, "pos": (idx, self._stage_row)}
        self._stage_row = 0
        return u

    def _copy_up(self, u):
        """the staged file pinned -> device, once"""
        res, slot = u["latch"].result, u["slot"]
        self._files_staged += 1
        # device buffers are used on the side stream only, so they come from its pool:
        # dropped with a decode in flight, their memory goes back to the stream that uses it
        if slot["dev"] is None or slot["dev"].numel() < res["used"]:
            slot["dev"] = torch.empty(slot["pin"].numel(), dtype=torch.uint8, device=self.device)
        slot["dev"][:res["used"]].copy_(slot["pin"][:res["used"]], non_blocking=True)

    def _batch(self, u):
        """the unit's next batch; the incomplete tail of a file is dropped"""
        res, B, (idx, row) = u["latch"].result, self.batch, u["pos"]
        k = row // B
        u["pos"] = (idx, row + B)
        return (k, max(int(res["tab"][k, -1]), 256),
                list(zip(res["tab"][k].tolist(), res["cnt"][k].tolist())),
                row + 2 * B > res["rows"])

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
        if self._ebc_groups:  # the collections' global feature-major CSRs, raw keys
            out["ebc"] = []
            for names in self._ebc_groups:
                ks, lens = [], []
                for n in names:
                    s = self._slot_of[n][0]
                    g = cats[s]
                    if isinstance(g, tuple):
                        off, vals = g
                        ks.append(vals[off[a]:off[b]] - self.slot_offsets[s])
                        lens.append(off[a + 1:b + 1] - off[a:b])
                    else:
                        ks.append(g[a:b] - self.slot_offsets[s])
                        lens.append(np.ones(B, np.int64))
                out["ebc"].append(feature_major_csr(ks, lens, self.device))
        return out
