"""Reader of the Raw format (data.write_raw; docs/source/api/python_interface.md "Raw";
R/HugeCTR/src/data_readers/multi_hot/): the plan one hctr_raw_decode launch gets and RawReader, whose
device path runs on the shared prefetch pipeline (reader_prefetch.py) with one batch per staged
unit."""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

from .reader_prefetch import (PrefetchReader, _Latch, _round_up, bucket_ranges,
                              feature_major_csr)


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
        top[0] = _round_up(off + nbytes, 256)
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


def _fill(dst, src, ev):
    """a worker's task: a contiguous range of a batch's records, memmap -> pinned slot"""
    if ev is not None:
        ev.synchronize()  # the slot is free once its last batch has been copied up
    np.copyto(dst, src)   # (releases the GIL)


def _row_offsets(hot, B):
    """row offsets of a param follow from its static hotness alone"""
    return np.concatenate([[0], np.cumsum(np.tile(hot, B))]).astype(np.int64)


class RawReader(PrefetchReader):
    """DataReaderType_t.RawAsync: streams batches of a Raw file (np.memmap; the reference uses
    Linux AIO worker threads -- I/O engines are outside the scope contract, the FORMAT is not).

    On a CUDA device the reader is asynchronous (DESIGN.md "Raw reader"): worker threads copy the
    records of the coming batches into a ring of pinned slots, a side stream copies a slot up and
    splits it with ONE launch (hctr_raw_decode), and next_batch() only makes the consumer's stream
    wait for that launch.  On a CPU device the batch is decoded on the host, as it always was.
    AsyncParam: num_batches_per_thread = slots of the ring (at least 2), num_threads = fill workers
    (at most 8; never sized by the machine)."""

    def __init__(self, path: str, inp, slot_size_array, batch, rank, world, device, num_samples,
                 float_label_dense: bool, repeat: bool, async_param=None, i64_key: bool = True):
        self.hot = []  # static hotness per slot, over all sparse params
        for p in inp.sparse_params:
            h = p.nnz_per_slot
            self.hot += list(h) if isinstance(h, (list, tuple)) else [int(h)] * p.slot_num
        super().__init__(inp, slot_size_array, len(self.hot), batch, rank, world, device, repeat,
                         i64_key, thread_name="hctr-raw-fill",
                         ring=max(2, int(getattr(async_param, "num_batches_per_thread", 0) or 0)),
                         workers=max(1, min(8, int(getattr(async_param, "num_threads", 0) or 2))))
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
        self.width = inp.label_dim + inp.dense_dim + sum(self.hot)
        words = os.path.getsize(path) // 4
        n = words // self.width
        if num_samples:
            n = min(n, int(num_samples))
        if n < batch:
            raise RuntimeError("raw file holds fewer samples than one batch")
        self.data = np.memmap(path, dtype="<u4", mode="r", shape=(n, self.width))
        self.n, self._pos = n, 0
        # top_name -> (first column of the record, columns, slots)
        self._col_of, col = {}, inp.label_dim + inp.dense_dim
        for name, hot in self._params():
            self._col_of[name] = (col, sum(hot), len(hot))
            col += sum(hot)
        if self._on_cuda:
            slots = []
            for _ in range(self._ring):  # fixed slots of one batch each
                pin = torch.empty((batch, self.width), dtype=torch.int32, pin_memory=True)
                slots.append({"pin": pin, "np": pin.numpy().view(np.uint32), "dev": None,
                                     "event": None})
            self._start_device(slots)
            # the device raw buffers (and the plan) are used on the side stream only, so they
            # come from its pool: dropped with a decode in flight, their memory goes back to the
            # stream that still uses it
            with torch.cuda.stream(self._stream):
                for s in self._slots:
                    s["dev"] = torch.empty((batch, self.width), dtype=torch.int32, device=device)

    def _params(self):
        """[(top_name, [hotness per slot])] in record order"""
        return [(name, [int(h) for h in self.hot[s0:s0 + n]])
                for name, (s0, n) in self._slot_of.items()]

    def decode_plan(self):
        """raw_decode_plan of this reader's configuration (host arrays only)"""
        return raw_decode_plan(self.inp.label_dim, self.inp.dense_dim, self._params(),
                               self._ebc_groups, self.slot_offsets, self.batch, self.rank,
                               self.world, self.float_label, self.float_dense,
                               self.key_dtype == torch.int64)

    def decode_into(self, arena, unit, k, stream):
        """the one hctr_raw_decode launch: the batch in the unit's device buffer -> arena
        (uint8, decode_plan()["arena_bytes"]) on stream (a pointer).  k: a unit holds one batch"""
        from . import _lib
        pl = self._plan
        _lib.check(_lib.lib.hctr_raw_decode(
            _lib.ptr(unit["slot"]["dev"]), self.batch, self.width, _lib.ptr(pl["device"]),
            len(pl["segments"]), _lib.ptr(arena), stream))

    # ---- what the prefetch pipeline asks for -------------------------------------------------------
    def _make_plan(self):
        pl, B = self.decode_plan(), self.batch
        pl["upload"] = [pl["segments"], pl["addend"]]
        pl["ro"] = {name: _row_offsets(hot, B) for name, hot in self._params()}
        pl["gbr"] = [bucket_ranges([np.full(B, self._col_of[n][1], np.int64) for n in names])
                     for names in self._ebc_groups]
        # a batch's outputs are a constant of the plan: label, dense, the params, the collections
        (lo, lshape), (do, dshape) = pl["label"], pl["dense"]
        pl["cuts"] = [(lo, lshape[0] * lshape[1]), (do, dshape[0] * dshape[1]),
                      *pl["sparse"].values(), *pl["ebc"]]
        ns = len(pl["sparse"])
        pl["layout"] = ((0, lshape), (1, dshape),
                        {name: (None, 2 + i) for i, name in enumerate(pl["sparse"])},
                        [(2 + ns + g, None) for g in range(len(pl["ebc"]))])
        return pl

    def _plan_next(self):
        """file position of the next batch; None at the file's end"""
        B = self.batch
        if self._pos + B > self.n:  # incomplete tail dropped, as the reference does
            if not self.repeat:
                return None
            self._pos = 0
        pos = self._pos
        self._pos += B
        return pos

    def _seek(self, pos):
        self._pos = pos

    def _stage(self, slot):
        """plans the next batch and hands its records to the workers, each a contiguous range of
        samples"""
        pos = self._plan_next()
        if pos is None:
            return None
        B, T = self.batch, self._workers
        ends = [B * i // T for i in range(T + 1)]
        parts = [(a, b) for a, b in zip(ends[:-1], ends[1:]) if b > a]
        latch = _Latch(len(parts))
        for a, b in parts:
            self._submit(functools.partial(_fill, slot["np"][a:b], self.data[pos + a:pos + b]),
                         slot["event"], latch)
        return {"latch": latch, "pos": pos}

    def _copy_up(self, u):
        u["slot"]["dev"].copy_(u["slot"]["pin"], non_blocking=True)

    def _batch(self, u):
        return 0, self._plan["arena_bytes"], self._plan["cuts"], True

    # ---- the host path -----------------------------------------------------------------------------
    def _next_host(self):
        pos = self._plan_next()
        if pos is None:
            return None
        B = self.batch
        blk = np.asarray(self.data[pos:pos + B])
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
        for name, hot in self._params():
            col, w, _ = self._col_of[name]
            s0 = self._slot_of[name][0]
            offs = np.repeat(self.slot_offsets[s0:s0 + len(hot)], hot)
            keys = (blk[:, col:col + w].astype(np.int64) + offs[None, :]).reshape(-1)
            out["sparse"][name] = (torch.from_numpy(_row_offsets(hot, B)).to(self.device, self.key_dtype),
                                   torch.from_numpy(keys).to(self.device, self.key_dtype))
        if self._ebc_groups:
            out["ebc"] = []
            for names in self._ebc_groups:
                cols = [self._col_of[n][:2] for n in names]
                out["ebc"].append(feature_major_csr(
                    [blk[:, c0:c0 + w].astype(np.int64).reshape(-1) for c0, w in cols],
                    [np.full(B, w, np.int64) for _, w in cols], self.device))
        return out
