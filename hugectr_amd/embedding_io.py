"""The bytes of Model.embedding_dump / embedding_load: one folder per embedding collection, one key
and one weight file per table, independent of how the tables were sharded.  Pure numpy; imports
without a GPU.  Restated from EmbeddingParameterIO
(R/HugeCTR/embedding_storage/weight_io/parameter_IO.cpp), the deviations are listed in
INTEGRATION.md "embedding_dump / embedding_load".

  <path>/embedding_collection_<c>/meta_data          (dump_metadata :179-260, load_metadata :37-82)
      int32[5]   {number of tables, key type (0 = uint32, 1 = int64), value type (0 = fp32), 0,
                  max ev_size}   -- the reference leaves [4] zero on dump and reads it on load;
                  written here, ignored when reading
      int32[n]   table ids, ascending
      uint64[n]  key_num per table (NOT 8-byte aligned: it starts at byte 20 + 4 n)
      int32[n]   ev_size per table
  <path>/embedding_collection_<c>/key<i>, weight<i>  (dump_embedding_weight :262-446)
      128-byte head (FileHeadNbytes; write_file_head :551-578): int32 {1 = key | 2 = weight, i},
      zeros; then key_num keys in the collection's key type / [key_num][ev_size] fp32 rows in the
      same order.  i = position in the SORTED list of dumped table ids (:292-296).
  <path>/embedding_collection_<c>/opt_state<i>       (not in the reference, which throws at :448-452)
      head int32 {3, i, number of state arrays, Optimizer_t value}; the arrays one after another,
      each [key_num][ev_size] fp32 in the key file's order.

c is the index of the user's EmbeddingCollectionConfig in the order it was added to the model; a
table's id its position in that config, in order of first appearance in its lookups
(emb_table_config_list_, R/HugeCTR/include/embeddings/embedding_collection.hpp:205-214).  With
several writers the owners' portions follow one another in ascending rank order; a rank whose keys
start `keys_before` keys into the file writes its rows at weight_offset(keys_before, ev_size).
"""
from __future__ import annotations

import os
import shutil
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

FILE_HEAD_NBYTES = 128       # FileHeadNbytes (data_info.hpp)
META_HEAD_NBYTES = 20        # MetaDataHeadLength: int32[5]
META_VALID_NBYTES = 36       # MetaDataValidLength (data_info.hpp:22-25): the head and one table
KIND_KEY, KIND_WEIGHT, KIND_OPT = 1, 2, 3  # EmbeddingFileType
_KEY_DTYPES = {0: np.dtype("<u4"), 1: np.dtype("<i8")}


class EmbeddingIOError(RuntimeError):
    pass


def key_type_code(key_dtype) -> int:
    dt = np.dtype(key_dtype)
    if dt.itemsize == 8:
        return 1
    if dt.itemsize == 4:
        return 0
    raise EmbeddingIOError(f"embedding files hold uint32 or int64 keys, not {dt}")


def collection_dir(path: str, c: int) -> str:
    return os.path.join(path, f"embedding_collection_{int(c)}")


def file_head(kind: int, index: int, a: int = 0, b: int = 0) -> bytes:
    """the 128-byte head of a key / weight / opt_state file"""
    return struct.pack("<4i", kind, index, a, b) + bytes(FILE_HEAD_NBYTES - 16)


def weight_offset(keys_before: int, ev_size: int) -> int:
    """byte offset of the rows of a writer whose first key is key number `keys_before` of the
    file (the reference's MPI branch multiplies a BYTE offset by the row size, :395-396)"""
    return FILE_HEAD_NBYTES + keys_before * ev_size * 4


def key_offset(keys_before: int, key_dtype) -> int:
    return FILE_HEAD_NBYTES + keys_before * np.dtype(key_dtype).itemsize


def state_offset(array: int, key_num: int, keys_before: int, ev_size: int) -> int:
    return FILE_HEAD_NBYTES + (array * key_num + keys_before) * ev_size * 4


@dataclass
class MetaData:
    table_ids: List[int]
    key_nums: Dict[int, int]
    ev_sizes: Dict[int, int]
    key_dtype: np.dtype = field(default_factory=lambda: np.dtype("<i8"))

    def file_index(self, table_id: int) -> int:
        """i of key<i> / weight<i>: found through the id list (the reference opens key<table_id>,
        right only when every table was dumped)"""
        try:
            return self.table_ids.index(int(table_id))
        except ValueError:
            raise EmbeddingIOError(f"table id {table_id} is not in this dump (it holds "
                                   f"{self.table_ids})") from None

    def to_bytes(self) -> bytes:
        ids = sorted(self.table_ids)
        n = len(ids)
        head = struct.pack("<5i", n, key_type_code(self.key_dtype), 0, 0,
                           max([self.ev_sizes[t] for t in ids] or [0]))
        return (head + struct.pack(f"<{n}i", *ids) +
                struct.pack(f"<{n}Q", *[self.key_nums[t] for t in ids]) +
                struct.pack(f"<{n}i", *[self.ev_sizes[t] for t in ids]))


def parse_meta(buf: bytes) -> MetaData:
    if len(buf) < META_VALID_NBYTES:
        raise EmbeddingIOError(f"meta_data of {len(buf)} bytes is too small, could not be valid "
                               f"(at least {META_VALID_NBYTES})")
    n, kt, vt, _, _ = struct.unpack_from("<5i", buf, 0)
    if n < 1 or len(buf) != META_HEAD_NBYTES + 16 * n:
        raise EmbeddingIOError(f"meta_data names {n} tables and is {len(buf)} bytes long, not "
                               f"{META_HEAD_NBYTES + 16 * max(n, 0)}")
    if kt not in _KEY_DTYPES:
        raise EmbeddingIOError(f"meta_data: unknown key type {kt}")
    if vt != 0:
        raise EmbeddingIOError(f"meta_data: value type {vt}; only fp32 (0) rows are supported")
    ids = list(struct.unpack_from(f"<{n}i", buf, META_HEAD_NBYTES))
    kn = struct.unpack_from(f"<{n}Q", buf, META_HEAD_NBYTES + 4 * n)
    ev = struct.unpack_from(f"<{n}i", buf, META_HEAD_NBYTES + 12 * n)
    return MetaData(ids, dict(zip(ids, kn)), dict(zip(ids, ev)), _KEY_DTYPES[kt])


def read_meta(path: str, c: int) -> MetaData:
    fn = os.path.join(collection_dir(path, c), "meta_data")
    if not os.path.exists(fn):
        raise EmbeddingIOError(f"{fn} not found")
    with open(fn, "rb") as f:
        return parse_meta(f.read())


def create_collection(path: str, c: int, meta: MetaData, opt_state=None) -> str:
    """Removes and rewrites <path>/embedding_collection_<c> ONLY (the reference deletes the whole
    <path> per collection, :185, and so loses the collections written before): meta_data and, per
    table, key<i> / weight<i> (/ opt_state<i> when opt_state = (number of arrays, Optimizer_t
    value), or {table id: (number of arrays, Optimizer_t value)} where the tables of the collection
    run different optimizers) with their heads, at full size -- every owner then writes its portion
    at its offset."""
    d = collection_dir(path, c)
    os.makedirs(path, exist_ok=True)
    if os.path.isdir(d):
        shutil.rmtree(d)
    os.makedirs(d)
    meta = MetaData(sorted(meta.table_ids), meta.key_nums, meta.ev_sizes, np.dtype(meta.key_dtype))
    with open(os.path.join(d, "meta_data"), "wb") as f:
        f.write(meta.to_bytes())
    for i, t in enumerate(meta.table_ids):
        kn, ev = meta.key_nums[t], meta.ev_sizes[t]
        files = [(f"key{i}", file_head(KIND_KEY, i), kn * meta.key_dtype.itemsize),
                 (f"weight{i}", file_head(KIND_WEIGHT, i), kn * ev * 4)]
        if opt_state is not None:
            if isinstance(opt_state, dict) and t not in opt_state:
                raise EmbeddingIOError(f"create_collection: no optimizer state entry for table id "
                                       f"{t} (given for {sorted(opt_state)})")
            ns, opt = opt_state[t] if isinstance(opt_state, dict) else opt_state
            files.append((f"opt_state{i}", file_head(KIND_OPT, i, int(ns), int(opt)),
                          int(ns) * kn * ev * 4))
        for name, head, body in files:
            with open(os.path.join(d, name), "wb") as f:
                f.write(head)
                f.truncate(FILE_HEAD_NBYTES + body)
    return d


class TableFiles:
    """The files of one table of a dump, opened for reading (validated: head, and the key count and
    ev_size of key file, weight file and meta_data agree) or for writing a portion of them."""

    def __init__(self, path: str, c: int, table_id: int, mode: str = "r", meta: Optional[MetaData] = None,
                 name: Optional[str] = None):
        assert mode in ("r", "r+")
        self.dir = collection_dir(path, c)
        self.meta = meta or read_meta(path, c)
        self.table_id = int(table_id)
        self.label = f"table {name!r} (id {table_id})" if name else f"table id {table_id}"
        self.index = self.meta.file_index(table_id)
        self.key_num = int(self.meta.key_nums[self.table_id])
        self.ev_size = int(self.meta.ev_sizes[self.table_id])
        self.key_dtype = np.dtype(self.meta.key_dtype)
        self._f = {}
        for kind, stem in ((KIND_KEY, "key"), (KIND_WEIGHT, "weight")):
            fn = os.path.join(self.dir, f"{stem}{self.index}")
            if not os.path.exists(fn):
                raise EmbeddingIOError(f"{self.label}: {fn} not found")
            self._f[stem] = open(fn, mode + "b", buffering=0)
            self._check_head(stem, kind)
        ksz = os.path.getsize(self._f["key"].name) - FILE_HEAD_NBYTES
        wsz = os.path.getsize(self._f["weight"].name) - FILE_HEAD_NBYTES
        if ksz != self.key_num * self.key_dtype.itemsize:
            self.close()
            raise EmbeddingIOError(
                f"{self.label}: the key file holds {ksz / self.key_dtype.itemsize:g} keys, "
                f"meta_data says {self.key_num}")
        if wsz != self.key_num * self.ev_size * 4:
            self.close()
            raise EmbeddingIOError(
                f"{self.label}: the weight file holds {wsz} bytes of rows, not {self.key_num} keys "
                f"x ev_size {self.ev_size} x 4 (another ev_size or key count)")
        # optimizer state: (number of arrays, Optimizer_t value) or None when there is no file
        self.opt_state = None
        fn = os.path.join(self.dir, f"opt_state{self.index}")
        if os.path.exists(fn):
            self._f["opt_state"] = open(fn, mode + "b", buffering=0)
            _, _, ns, opt = self._check_head("opt_state", KIND_OPT)
            if os.path.getsize(fn) != FILE_HEAD_NBYTES + ns * self.key_num * self.ev_size * 4:
                self.close()
                raise EmbeddingIOError(f"{self.label}: opt_state{self.index} does not hold {ns} "
                                       f"arrays of {self.key_num} x {self.ev_size} fp32")
            self.opt_state = (ns, opt)

    def _check_head(self, stem, kind):
        f = self._f[stem]
        f.seek(0)
        head = f.read(FILE_HEAD_NBYTES)
        if len(head) < FILE_HEAD_NBYTES:
            self.close()
            raise EmbeddingIOError(f"{self.label}: {f.name} is shorter than its {FILE_HEAD_NBYTES}"
                                   "-byte head")
        vals = struct.unpack_from("<4i", head, 0)
        if vals[0] != kind or vals[1] != self.index:
            self.close()
            raise EmbeddingIOError(f"{self.label}: {f.name} has head {vals[:2]}, expected "
                                   f"({kind}, {self.index})")
        return vals

    def close(self):
        for f in self._f.values():
            f.close()
        self._f = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    # -- portions: `first` = key number inside the file, out / data = C-contiguous numpy arrays ------
    def _where(self, stem, first, array=0):
        if stem == "key":
            return key_offset(first, self.key_dtype)
        if stem == "weight":
            return weight_offset(first, self.ev_size)
        return state_offset(array, self.key_num, first, self.ev_size)

    def read_into(self, stem: str, first: int, out: np.ndarray, array: int = 0):
        f = self._f[stem]
        f.seek(self._where(stem, first, array))
        view = memoryview(out).cast("B")
        got = 0
        while got < len(view):
            n = f.readinto(view[got:])
            if not n:
                raise EmbeddingIOError(f"{self.label}: {f.name} ended early")
            got += n

    def write(self, stem: str, first: int, data: np.ndarray, array: int = 0):
        f = self._f[stem]
        f.seek(self._where(stem, first, array))
        f.write(memoryview(np.ascontiguousarray(data)).cast("B"))

    # -- whole-table convenience (small tables, tests, tools) ---------------------------------------
    def read_keys(self) -> np.ndarray:
        out = np.empty(self.key_num, dtype=self.key_dtype)
        if self.key_num:
            self.read_into("key", 0, out)
        return out

    def read_weights(self) -> np.ndarray:
        out = np.empty((self.key_num, self.ev_size), dtype="<f4")
        if self.key_num:
            self.read_into("weight", 0, out)
        return out

    def read_states(self) -> List[np.ndarray]:
        out = []
        for a in range(self.opt_state[0] if self.opt_state else 0):
            s = np.empty((self.key_num, self.ev_size), dtype="<f4")
            if self.key_num:
                self.read_into("opt_state", 0, s, a)
            out.append(s)
        return out


def write_collection(path: str, c: int, tables: Dict[int, tuple], key_dtype="<i8", optimizer=None):
    """whole tables from host arrays: tables = {table id: (keys [n], weights [n, ev][, states])};
    optimizer = Optimizer_t value when states are given (tools, tests, converters)"""
    ids = sorted(tables)
    meta = MetaData(ids, {t: int(np.asarray(tables[t][0]).shape[0]) for t in ids},
                    {t: int(np.asarray(tables[t][1]).shape[1]) for t in ids}, np.dtype(key_dtype))
    nstate = {len(tables[t][2]) if len(tables[t]) > 2 else 0 for t in ids}
    if optimizer is not None and len(nstate) != 1:
        raise EmbeddingIOError("every table of a collection carries the same number of state arrays")
    create_collection(path, c, meta, (nstate.pop(), optimizer) if optimizer is not None else None)
    for t in ids:
        with TableFiles(path, c, t, "r+", meta) as tf:
            tf.write("key", 0, np.asarray(tables[t][0]).astype(meta.key_dtype))
            tf.write("weight", 0, np.asarray(tables[t][1], dtype="<f4"))
            if optimizer is not None:
                for a, s in enumerate(tables[t][2]):
                    tf.write("opt_state", 0, np.asarray(s, dtype="<f4"), a)
    return meta


def static_shard_key_count(vocab: int, num_shards: int, shard_id: int) -> int:
    """keys of a static table's shard: shard_id + j * num_shards < vocab"""
    return max(0, -(-(int(vocab) - shard_id) // num_shards))
