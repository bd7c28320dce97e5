"""export_table / import_table of the embedding_collection runtimes: tables and optimizer state
between device memory and the files of embedding_io.py, in chunks through the two pinned host
buffers of hctr_ebc_io_* (csrc/ebc_io.hip).  The counterpart of dump_by_id / load_by_id of the
reference's grouped tables (R/HugeCTR/embedding_storage/ragged_static_embedding.cu,
dynamic_embedding.cu:432-472) with the key filter `key % num_shards == shard_id` of
add_embedding_collection's loader (R/HugeCTR/src/pybind/model.cpp:521-665) moved onto the device.

Thin ctypes calls and file reads; no arithmetic here."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, embedding_io
from ._lib import check, lib, ptr, stream_ptr


def default_chunk_rows(ev_size: int) -> int:
    """about 64 MiB per pinned buffer: key + row + two state rows per entry"""
    return max(1, (64 << 20) // (8 + 3 * 4 * int(ev_size)))


class IoChunks:
    """hctr_ebc_io: two pinned chunks seen as numpy arrays (keys / rows / state[0..1] of chunk w)"""

    def __init__(self, chunk_rows: int, ev_size: int, key_dtype):
        self.R, self.ev = int(chunk_rows), int(ev_size)
        self.key_dtype = np.dtype(key_dtype)
        self._h = ctypes.c_void_p()
        kt = _lib.KEY_I64 if self.key_dtype.itemsize == 8 else _lib.KEY_U32
        check(lib.hctr_ebc_io_create(self.R, self.ev, kt, ctypes.byref(self._h)))
        self.keys, self.rows, self.state = [], [], []
        for w in range(2):
            p = [ctypes.c_void_p() for _ in range(4)]
            check(lib.hctr_ebc_io_chunk(self._h, w, *[ctypes.byref(x) for x in p]))
            self.keys.append(self._view(p[0].value, self.R * self.key_dtype.itemsize, self.key_dtype))
            f = [self._view(x.value, self.R * self.ev * 4, np.dtype("<f4")).reshape(self.R, self.ev)
                 for x in p[1:]]
            self.rows.append(f[0])
            self.state.append(f[1:])

    @staticmethod
    def _view(addr, nbytes, dtype):
        return np.frombuffer((ctypes.c_char * nbytes).from_address(addr), dtype=dtype)

    def wait(self, w: int):
        check(lib.hctr_ebc_io_wait(self._h, w))

    def close(self):
        if getattr(self, "_h", None):
            self.keys = self.rows = self.state = None  # (views of memory that goes away)
            lib.hctr_ebc_io_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False


def _addr(t: torch.Tensor, row: int = 0):
    return ctypes.c_void_p(t.data_ptr() + row * t.shape[1] * 4)


class TableIO:
    """Mixin of EmbeddingCollection and DataParallelCollection.  The host class provides
    `_io_layout(t)` (dict: dynamic, num_shards, shard_id, vocab, row_start | cls | hybrid (the
    shard's HybridTable), writes; None for a table this rank does not hold), `_io_state_arrays()` (the static optimizer state tensors)
    and `tables`, `ev`, `optimizer`, `dev`."""

    # -- what there is to write ---------------------------------------------------------------------
    def io_state_count(self) -> int:
        """optimizer state arrays per row that export_table(optimizer_states=True) writes"""
        if getattr(self, "dynamic", False) or getattr(self, "hybrid", False):
            return {_lib.OPT_ADAM: 2, _lib.OPT_SGD: 0}.get(self.optimizer, 1)
        return {_lib.OPT_ADAGRAD: 1, _lib.OPT_FTRL: 2}.get(self.optimizer, 0)

    def io_check_optimizer_states(self):
        """raises where the state cannot be exported: a dynamic table whose step runs on the
        unique-key flow keeps its state in a second key -> state table, not at the row numbers of
        the flat row store.  A hybrid table keeps its state at the slot numbers, either tier, for
        every optimizer it has: always exportable."""
        from .embedding_collection import _FLAT_STEP
        if getattr(self, "hybrid", False):
            return
        if getattr(self, "dynamic", False) and not (self._dyn_flat and self.optimizer in _FLAT_STEP):
            raise _lib.HugeCTRAmdError(
                "optimizer_states=True: dynamic tables keep exportable optimizer state only for "
                "the steps that run on the flat row store (SGD, AdaGrad, Adam, MomentumSGD with "
                "HCTR_DYNAMIC_FLAT unset); Nesterov, RMSProp, Ftrl and HCTR_DYNAMIC_FLAT=0 use "
                "the unique-key flow")

    def table_key_count(self, t: int) -> int:
        """keys of table t that this rank writes in export_table"""
        lay = self._io_layout(t)
        if lay is None or not lay["writes"]:
            return 0
        if lay.get("hybrid") is not None:
            return lay["hybrid"].size()
        if lay["dynamic"]:
            return int(self.det.size_per_class()[lay["cls"]])
        return embedding_io.static_shard_key_count(lay["vocab"], lay["num_shards"], lay["shard_id"])

    def _io_static_arrays(self, want_states: bool):
        arrays = [self.table]
        if want_states:
            arrays += self._io_state_arrays()
        return arrays

    # -- device -> files ----------------------------------------------------------------------------
    def export_table(self, t: int, files: embedding_io.TableFiles, keys_before: int = 0,
                     optimizer_states: bool = False, chunk_rows: int = None) -> int:
        """Writes this rank's keys and rows of table t (its position in `self.tables`) at key
        number `keys_before` of `files` (opened "r+"); with optimizer_states also the state rows
        into opt_state<i>.  Returns the number of keys written.  A static shard goes through the
        pinned chunks by asynchronous copies, chunk k + 1 on its way while chunk k is written to
        the files.  A dynamic table exports one class with hctr_det_export: that needs a SECOND
        DEVICE COPY of the class (keys and rows, and of its state rows) while it is written."""
        lay = self._io_layout(t)
        n = self.table_key_count(t)
        if n == 0:
            return 0
        self._io_match(files, t)
        ns = self.io_state_count() if optimizer_states else 0
        if optimizer_states:
            self.io_check_optimizer_states()
            if files.opt_state != (ns, int(self.optimizer)):
                raise _lib.HugeCTRAmdError(f"{files.label}: opt_state file {files.opt_state} does "
                                           f"not match ({ns}, {int(self.optimizer)})")
        R = int(chunk_rows or default_chunk_rows(self.ev))
        if lay.get("hybrid") is not None:
            return self._export_hybrid(lay["hybrid"], files, keys_before, ns, R)
        if lay["dynamic"]:
            return self._export_dynamic(lay, files, keys_before, ns, R)
        arrays = self._io_static_arrays(ns > 0)
        S, sid, r0 = lay["num_shards"], lay["shard_id"], lay["row_start"]

        def flush(io, w, start, m):
            io.wait(w)
            files.write("key", keys_before + start, io.keys[w][:m])
            files.write("weight", keys_before + start, io.rows[w][:m])
            for a in range(ns):
                files.write("opt_state", keys_before + start, io.state[w][a][:m], a)

        with IoChunks(min(R, n), self.ev, files.key_dtype) as io:
            pending, w = None, 0
            for start in range(0, n, io.R):
                m = min(io.R, n - start)
                st = [_addr(a, r0 + start) for a in arrays[1:]] + [None, None]
                check(lib.hctr_ebc_io_export_static(io._h, w, m, sid + start * S, S,
                                                    _addr(arrays[0], r0 + start), st[0], st[1],
                                                    stream_ptr()))
                if pending:
                    flush(io, *pending)
                pending, w = (w, start, m), w ^ 1
            flush(io, *pending)
        return n

    def _export_dynamic(self, lay, files, keys_before, ns, R):
        cls = lay["cls"]
        keys, vals = self.det.export(cls)
        n = int(keys.numel())
        states = []
        if ns and n:
            _, rows, _ = self.det.lookup_rows(keys, [cls], [0, n], insert=False, want_ptrs=False)
            stores = self.det.state_store(ns)
            _, total = self.det.row_store()
            for a in range(ns):
                out = torch.empty((n, self.ev), dtype=torch.float32, device=self.dev)
                check(lib.hctr_ebc_uniq_gather_rows(n, self.ev, ptr(rows), stores[a], total, ptr(out),
                                                    _lib.F32, stream_ptr()))
                states.append(out)
        for start in range(0, n, R):
            sl = slice(start, min(start + R, n))
            files.write("key", keys_before + start,
                        keys[sl].cpu().numpy().astype(files.key_dtype))
            files.write("weight", keys_before + start, vals[sl].cpu().numpy())
            for a, s in enumerate(states):
                files.write("opt_state", keys_before + start, s[sl].cpu().numpy(), a)
        return n

    def _export_hybrid(self, tab, files, keys_before, ns, R):
        """the occupied slots in slot order (hctr_lru_export); state rows through the slot-addressed
        gather, which reaches host-resident slots as well (hctr_lru_gather_slots)"""
        keys, vals, slots, _ = tab.export(with_slots=True)
        n = int(keys.numel())
        states = []
        for a in range(ns if n else 0):
            tab.state_ptr(a)  # (allocated, zeroed, if the optimizer has not stepped yet)
            states.append(tab.gather_slots(1 + a, slots))
        for start in range(0, n, R):
            sl = slice(start, min(start + R, n))
            files.write("key", keys_before + start,
                        keys[sl].cpu().numpy().astype(files.key_dtype))
            files.write("weight", keys_before + start, vals[sl].cpu().numpy())
            for a, s in enumerate(states):
                files.write("opt_state", keys_before + start, s[sl].cpu().numpy(), a)
        return n

    # -- files -> device ----------------------------------------------------------------------------
    def _io_match(self, files, t):
        if files.ev_size != self.ev:
            raise _lib.HugeCTRAmdError(
                f"{files.label}: the files hold ev_size {files.ev_size}, table "
                f"{self.tables[t].name!r} has ev_size {self.ev}")

    def _io_load_states(self, files, optimizer_states):
        """number of state arrays to load: the file's when it names this optimizer and this number
        of arrays, 0 when there is no file (the arrays are left alone)"""
        if optimizer_states is False or files.opt_state is None:
            return 0
        ns = self.io_state_count()
        if files.opt_state != (ns, int(self.optimizer)):
            raise _lib.HugeCTRAmdError(
                f"{files.label}: opt_state{files.index} holds {files.opt_state[0]} arrays of "
                f"optimizer {files.opt_state[1]}, this table runs optimizer {int(self.optimizer)} "
                f"with {ns}")
        if ns:
            self.io_check_optimizer_states()
        return ns

    def validate_table(self, t: int, files: embedding_io.TableFiles, chunk_rows: int = None,
                       optimizer_states=None):
        """Everything import_table checks, without writing a row: ev_size, the optimizer of the
        state file, and (the check pass, keys only) every key inside [0, vocab) of a static table /
        non-negative for a dynamic one.  Returns {owned, foreign} key counts."""
        lay = self._io_layout(t)
        if lay is None:
            return dict(owned=0, foreign=0)
        self._io_match(files, t)
        self._io_load_states(files, optimizer_states)
        n = files.key_num
        counts = torch.zeros(3, dtype=torch.int64, device=self.dev)
        if n:
            R = min(int(chunk_rows or default_chunk_rows(self.ev)), n)
            with IoChunks(R, self.ev, files.key_dtype) as io:
                w = 0
                for start in range(0, n, R):
                    m = min(R, n - start)
                    io.wait(w)
                    files.read_into("key", start, io.keys[w][:m])
                    check(lib.hctr_ebc_io_check(io._h, w, m, lay["num_shards"], lay["shard_id"],
                                                lay["vocab"], ptr(counts), stream_ptr()))
                    w ^= 1
                io.wait(0)
                io.wait(1)
        own, foreign, bad = [int(x) for x in counts.cpu().tolist()]
        if bad:
            what = ("negative" if lay["dynamic"] else
                    f"outside [0, max_vocabulary_size = {lay['vocab']})")
            raise _lib.HugeCTRAmdError(f"{files.label}: {bad} of {n} keys are {what}; nothing "
                                       f"was loaded into table {self.tables[t].name!r}")
        tab = lay.get("hybrid")
        if tab is not None and own > tab.capacity:
            raise _lib.HugeCTRAmdError(
                f"{files.label}: {own} of {n} keys belong to shard {lay['shard_id']} of "
                f"{lay['num_shards']} of hybrid table {self.tables[t].name!r}, whose max_capacity "
                f"is {tab.capacity} slots; nothing was loaded")
        return dict(owned=own, foreign=foreign)

    def import_table(self, t: int, files: embedding_io.TableFiles, chunk_rows: int = None,
                     optimizer_states=None, validated: bool = False):
        """Loads the keys of `files` that this rank owns into table t, in place (addresses stay:
        a captured graph stays valid; a hybrid table that is still growing may move, and the
        collection reads its address every step).  Validation first (validate_table; validated=True: the
        caller did it), then the rows: a static table scatters every owned key's row to its place
        (rows whose key is not in the file keep their value -- the reference only inserts), a
        dynamic table inserts the owned keys (hctr_det_lookup_rows with insert) and stores their
        rows (hctr_det_scatter_update), a hybrid table does the same through hctr_lru_lookup_index
        and hctr_lru_scatter_slots -- refused by validate_table, before anything is written, when
        the shard would receive more keys than its max_capacity.  Optimizer state is loaded when the dump has a state file
        for this optimizer (optimizer_states=False: never); without one the state is left alone."""
        lay = self._io_layout(t)
        if lay is None:
            return
        if not validated:
            self.validate_table(t, files, chunk_rows, optimizer_states)
        ns = self._io_load_states(files, optimizer_states)
        n = files.key_num
        if n == 0:
            return
        R = min(int(chunk_rows or default_chunk_rows(self.ev)), n)
        S, sid = lay["num_shards"], lay["shard_id"]
        tab = lay.get("hybrid")
        owned = []  # (hybrid) the keys this shard took from the files, chunk by chunk
        if lay["dynamic"]:
            cls = lay.get("cls")
            okeys = torch.empty(R, dtype=torch.int64, device=self.dev)
            obuf = [torch.empty((R, self.ev), dtype=torch.float32, device=self.dev)
                    for _ in range(1 + ns)]
        else:
            arrays = self._io_static_arrays(ns > 0)
            dst = [ptr(a) for a in arrays[1:1 + ns]] + [None, None]
        with IoChunks(R, self.ev, files.key_dtype) as io:
            w = 0
            for start in range(0, n, R):
                m = min(R, n - start)
                io.wait(w)
                files.read_into("key", start, io.keys[w][:m])
                files.read_into("weight", start, io.rows[w][:m])
                for a in range(ns):
                    files.read_into("opt_state", start, io.state[w][a][:m], a)
                if not lay["dynamic"]:
                    check(lib.hctr_ebc_io_import_static(io._h, w, m, S, sid, lay["vocab"],
                                                        lay["row_start"], ptr(arrays[0]), dst[0],
                                                        dst[1], stream_ptr()))
                    w ^= 1
                    continue
                got = ctypes.c_size_t()
                so = [ptr(b) for b in obuf[1:]] + [None, None]
                check(lib.hctr_ebc_io_select(io._h, w, m, S, sid, lay["vocab"], ptr(okeys),
                                             ptr(obuf[0]), so[0], so[1], ctypes.byref(got),
                                             stream_ptr()))
                w ^= 1
                k = int(got.value)
                if k == 0:
                    continue
                if tab is not None:
                    # an inserting lookup stores the owned keys (one call, one tick of LRU time,
                    # per chunk), then rows and states go to their slots, either tier.  A key its
                    # bucket has no room for is not stored: counted by the table (`rejected`).
                    tab.lookup_index(okeys[:k], insert=True)
                    owned.append(okeys[:k].clone())
                    slots = tab.find(okeys[:k])
                    tab.scatter_slots(0, slots, obuf[0][:k])
                    for a in range(ns):
                        tab.state_ptr(a)
                        tab.scatter_slots(1 + a, slots, obuf[1 + a][:k])
                    torch.cuda.synchronize()  # (okeys / obuf are refilled by the next chunk)
                    continue
                _, rows, _ = self.det.lookup_rows(okeys[:k], [cls], [0, k], insert=True,
                                                  want_ptrs=False)
                self.det.scatter_update(okeys[:k], obuf[0][:k], [cls], [0, k])
                if ns:
                    stores = self.det.state_store(ns)
                    _, total = self.det.row_store()
                    for a in range(ns):
                        check(lib.hctr_ebc_io_scatter_rows(k, self.ev, ptr(rows), ptr(obuf[1 + a]),
                                                           stores[a], total, stream_ptr()))
                torch.cuda.synchronize()  # (okeys / obuf are refilled by the next chunk)
            io.wait(0)
            io.wait(1)
        if owned:
            # within max_capacity a key can still be lost: its bucket had no room (rejected), or a
            # later chunk -- a later tick of LRU time -- evicted it.  Found again, all of them, or
            # the load is reported as incomplete.
            missing = sum(int((tab.find(k) < 0).sum()) for k in owned)
            if missing:
                raise _lib.HugeCTRAmdError(
                    f"{files.label}: {missing} of {sum(int(k.numel()) for k in owned)} keys of "
                    f"shard {sid} of {S} did not stay in hybrid table {self.tables[t].name!r} "
                    f"(bucket overflow or eviction by a later chunk; size {tab.size()}, rejected "
                    f"{tab.rejected_count()}, max_capacity {tab.capacity}): the table holds an "
                    "incomplete load")


# ---- whole collections: one process, any number of rank shards (tests, tools, Model) -------------

def _table_ids(coll, table_ids):
    return list(range(len(coll.tables))) if table_ids is None else [int(t) for t in table_ids]


def dump_shards(path: str, c: int, shards, table_ids=None, optimizer_states: bool = False,
                chunk_rows: int = None, id_of_table=None):
    """Writes <path>/embedding_collection_<c> from the rank shards of ONE collection held by this
    process (`shards`: the objects of EmbeddingCollection.for_rank(r, world, ...) for every r, or
    the one collection of a single-GPU run), ascending rank -- no collective.  table_ids: positions
    in `shards[0].tables` (default: all); id_of_table maps them to the ids written to the files
    (default: the position)."""
    first = shards[0]
    tids = _table_ids(first, table_ids)
    id_of = id_of_table or {t: t for t in tids}
    if optimizer_states:
        for s in shards:
            s.io_check_optimizer_states()
    counts = {t: [s.table_key_count(t) for s in shards] for t in tids}
    kd = np.dtype("<i8") if getattr(first, "key_dtype", torch.int64) == torch.int64 else np.dtype("<u4")
    meta = embedding_io.MetaData([id_of[t] for t in tids], {id_of[t]: sum(counts[t]) for t in tids},
                                 {id_of[t]: first.ev for t in tids}, kd)
    opt = (first.io_state_count(), int(first.optimizer)) if optimizer_states else None
    embedding_io.create_collection(path, c, meta, opt)
    meta = embedding_io.read_meta(path, c)
    for t in tids:
        with embedding_io.TableFiles(path, c, id_of[t], "r+", meta, first.tables[t].name) as f:
            before = 0
            for s, n in zip(shards, counts[t]):
                s.export_table(t, f, before, optimizer_states, chunk_rows)
                before += n
    torch.cuda.synchronize()


def load_shard(path: str, c: int, coll, table_ids=None, chunk_rows: int = None,
               optimizer_states=None, id_of_table=None):
    """Loads <path>/embedding_collection_<c> into one collection (or one rank's shard of it):
    every table is validated before the first row is written."""
    tids = _table_ids(coll, table_ids)
    id_of = id_of_table or {t: t for t in tids}
    meta = embedding_io.read_meta(path, c)
    opened = []
    try:
        for t in tids:
            opened.append((t, embedding_io.TableFiles(path, c, id_of[t], "r", meta,
                                                      coll.tables[t].name)))
        for t, f in opened:
            coll.validate_table(t, f, chunk_rows, optimizer_states)
        for t, f in opened:
            coll.import_table(t, f, chunk_rows, optimizer_states, validated=True)
    finally:
        for _, f in opened:
            f.close()
    torch.cuda.synchronize()
