"""What the Raw and the Parquet reader share (DESIGN.md "The readers' prefetch pipeline"): the
construction state, next_batch() with its batch cache, the worker pool, the ring of staged units, the
side-stream issue, the hand-over to the consumer's stream, the rewind and the plan upload.

A *staged unit* occupies one ring slot and yields one or more batches: a Raw unit is one batch, a
Parquet unit is one file.  A subclass says what a unit is (_stage, _copy_up, _batch), performs the
one decode launch (decode_into), builds its plan (_make_plan), seeks (_seek) and decodes on the
host (_next_host)."""
from __future__ import annotations

import ctypes
import queue
import sys
import threading
import time

import numpy as np
import torch


def _round_up(n: int, a: int) -> int:
    """n rounded up to a multiple of a (a power of two)"""
    return (n + a - 1) & ~(a - 1)


def slot_offsets(slot_size_array, n_slots):
    """what is added to the keys of every slot: the sizes of the slots before it"""
    ssa = list(slot_size_array)
    return (np.concatenate([[0], np.cumsum(ssa)[:-1]]).astype(np.int64) if ssa
            else np.zeros(n_slots, np.int64))


def bucket_ranges(lens):
    """lens: per lookup the key counts of its samples -> bucket range, bucket = lookup * batch + sample"""
    gbr = np.zeros(sum(len(l) for l in lens) + 1, np.int64)
    np.cumsum(np.concatenate(lens), out=gbr[1:])
    return gbr


def feature_major_csr(ks, lens, device):
    """a collection's global feature-major CSR on the host path: (raw keys, bucket range) from the
    keys and the key counts of its lookups, in lookup order"""
    return (torch.from_numpy(np.concatenate(ks).astype(np.int64, copy=False)).to(device),
            torch.from_numpy(bucket_ranges(lens)).to(device))


class _Latch:
    """counts the parts of one staged unit down; the training thread waits for zero"""

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


def _worker(tasks):
    """worker thread of an asynchronous reader.  A task is (callable, event after which the pinned
    slot is free or None, latch): the callable gets the event, waits for it before it writes into
    the slot (whatever does not touch the slot comes first) and returns the latch's result.  An
    error goes to the latch and the worker lives on; None ends it.  Holds no reference to the
    reader."""
    while True:
        t = tasks.get()
        if t is None:
            return
        fn, ev, latch = t
        try:
            latch.result = fn(ev)
            latch.part_done()
        except BaseException as e:  # handed to next_batch()
            latch.part_done(e)
        t = fn = ev = latch = None  # (nothing of the unit is held while waiting)


class PrefetchReader:
    """Base of RawReader and ParquetReader.  On a CUDA device (after _start_device) worker threads
    stage the coming units in a ring of pinned slots, a side stream copies a staged unit up and
    turns it into batches with one launch each, and next_batch() only makes the consumer's stream
    wait for that launch; otherwise every batch comes from the subclass's host path.
    cache_batches = N > 0: the first N batches are kept and handed out round-robin for ever."""

    def __init__(self, inp, slot_size_array, n_slots, batch, rank, world, device, repeat, i64_key,
                 *, ring, workers, thread_name, cache_batches=0):
        self.inp, self.batch, self.rank, self.world = inp, batch, rank, world
        self.device, self.repeat = device, repeat
        self._on_cuda = (device.type if isinstance(device, torch.device)
                         else str(device).split(":")[0]) == "cuda"
        # keys AND row offsets carry the model's key type (solver.i64_input_key), as the
        # reference's SparseTensor<TypeKey> does
        self.key_dtype = torch.int64 if i64_key else torch.int32
        self.slot_offsets = slot_offsets(slot_size_array, n_slots)
        # embedding_collection models: Model.compile names, per collection, the inputs of its
        # lookups in lookup order; the reader then hands over the collection's global
        # feature-major CSR (raw keys, bucket = lookup * batch + sample) ready-made -- cutting it
        # out of 26 per-input tensors on the GPU costs ~100 tiny launches per step
        self._ebc_groups = []
        self._slot_of, s0 = {}, 0   # top_name -> (first slot, slots)
        for p in inp.sparse_params:
            self._slot_of[p.top_name] = (s0, p.slot_num)
            s0 += p.slot_num
        self._cache_n, self._cache, self._served = max(0, int(cache_batches or 0)), [], 0
        self._batches, self._wait_s = 0, 0.0
        self._ring, self._workers, self._thread_name = ring, workers, thread_name
        self._async, self._threads, self._tasks, self._closed = False, [], None, False

    def _start_device(self, slots):
        """takes the device path.  slots: one dict per ring slot with "pin" (pinned tensor), "np"
        (its numpy view), "dev" (device tensor), "event" (after which "pin" may be overwritten)"""
        self._async, self._slots = True, slots
        self._stream = torch.cuda.Stream(device=self.device)
        self._stream_ptr = ctypes.c_void_p(self._stream.cuda_stream)
        self._plan = None     # built by the first next_batch(): ebc_groups is set after
        self._units = []      # staged or being staged, not yet exhausted, oldest first
        self._issued = []     # batches on the side stream, oldest first
        self._useq = 0        # units staged so far (slot = useq % ring)

    @property
    def ebc_groups(self):
        return self._ebc_groups

    @ebc_groups.setter
    def ebc_groups(self, groups):
        for names in groups:
            for n in names:
                assert self._slot_of[n][1] == 1, "embedding_collection inputs carry one slot per lookup"
        self._ebc_groups = groups
        if self._async and self._plan is not None:
            self._rewind()  # (batches in flight were decoded by the old plan)
            self._plan = None
        self._cache, self._served = [], 0  # (kept batches carry the old collections' CSRs)

    def stats(self):
        """decode: where a batch is decoded; ring / threads: slots and workers of the asynchronous
        path (0 on the host path); batches: handed out so far; wait_ms: total time next_batch()
        waited for a worker"""
        a = self._async
        return {"decode": "device" if a else "host", "ring": self._ring if a else 0,
                "threads": self._workers if a else 0, "batches": self._batches,
                "wait_ms": self._wait_s * 1e3}

    def close(self):
        """stops the workers (idempotent; also run when the reader is dropped)"""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        self._stop_workers()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def next_batch(self):
        if self._closed:
            raise RuntimeError(f"{type(self).__name__}: next_batch() after close()")
        n = self._cache_n
        if n and len(self._cache) >= n:
            b = self._cache[self._served % n]
        else:
            b = self._next_device() if self._async else self._next_host()
            if b is None:
                return None
            if n:
                self._cache.append(b)
                if len(self._cache) >= n and self._async:  # nothing further is read
                    self._rewind()  # (a regroup reads on from the first batch not handed out)
                    self._stop_workers()
        self._served += 1
        self._batches += 1
        return b

    # ---- worker pool -------------------------------------------------------------------------------
    def _submit(self, fn, ev, latch):
        """hands a task to the workers, which start with the first one"""
        if not self._threads:
            self._tasks = queue.Queue()
            self._threads = [threading.Thread(target=_worker, args=(self._tasks,), daemon=True,
                                              name=f"{self._thread_name}-{i}")
                             for i in range(self._workers)]
            for t in self._threads:
                t.start()
        self._tasks.put((fn, ev, latch))

    def _stop_workers(self):
        for _ in self._threads:
            self._tasks.put(None)
        if not sys.is_finalizing():  # (at interpreter exit daemon threads no longer run)
            for t in self._threads:
                t.join()
        self._threads = []
        if self._async:
            self._units, self._issued = [], []
            for s in self._slots:
                s.update(pin=None, np=None, dev=None, event=None)

    # ---- the pipeline ------------------------------------------------------------------------------
    def _enough(self):
        """a full cache needs nothing beyond its batches"""
        return self._cache_n and len(self._cache) + len(self._issued) >= self._cache_n

    def _fill_ring(self):
        """stages the coming units, each into the slot whose unit was exhausted longest ago"""
        while len(self._units) < self._ring and not self._enough():
            slot = self._slots[self._useq % self._ring]
            u = self._stage(slot)
            if u is None:
                return
            u["slot"], u["up"] = slot, False
            self._useq += 1
            self._units.append(u)

    def _await(self, u) -> bool:
        """waits for the unit's workers.  A worker's error is raised when the batches issued
        before it have been handed out (False until then)"""
        t0 = time.perf_counter()
        u["latch"].done.wait()
        self._wait_s += time.perf_counter() - t0
        if u["latch"].error is None:
            return True
        if self._issued:
            return False
        self._units.pop(0)
        raise u["latch"].error

    def _mark(self):
        ev = torch.cuda.Event()
        ev.record(self._stream)
        return ev

    def _issue_one(self) -> bool:
        """side stream: the head unit copied up if it has not been, one decode launch of its next
        batch into a fresh arena, an event"""
        if not self._units or self._enough():
            return False
        u = self._units[0]
        if not u["up"] and not self._await(u):
            return False
        job = {"pos": u["pos"]}
        k, nbytes, job["cuts"], last = self._batch(u)
        with torch.cuda.stream(self._stream):
            fresh = not u["up"]
            if fresh:
                self._copy_up(u)
            # allocated on the side stream, so from its pool
            job["arena"] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.decode_into(job["arena"], u, k, self._stream_ptr)
            job["event"] = self._mark()
        if fresh:  # recorded behind the copy up, the one operation that reads the pinned slot
            u["slot"]["event"], u["up"] = job["event"], True
        self._issued.append(job)
        if last:
            self._units.pop(0)
            self._fill_ring()  # the slot's next unit: its worker waits for the event above
        return True

    def head_unit(self):
        """the staged unit the next batch is cut from, copied up: {"slot": {"pin", "np", "dev"},
        "latch", "pos", ...}; None at the end of the data.  For tools that time a stage alone
        (decode_into on its buffers)."""
        self._fill_ring()
        if not self._units:
            return None
        u = self._units[0]
        if not u["up"]:
            if not self._await(u):
                return None
            with torch.cuda.stream(self._stream):
                self._copy_up(u)
                u["slot"]["event"], u["up"] = self._mark(), True
        return u

    @property
    def plan(self):
        """the plan in use on the device path: decode_plan() and what _upload_plan() adds"""
        return self._plan

    def _rewind(self):
        """forgets the units and batches in flight: the next batch handed out is read again"""
        for u in self._units:
            u["latch"].done.wait()
        if self._issued or self._units:
            self._seek((self._issued or self._units)[0]["pos"])
        self._units, self._issued = [], []

    def _next_device(self):
        if self._plan is None:
            self._upload_plan()
        self._fill_ring()
        # this batch and the next one are on the side stream before this one is handed over
        while len(self._issued) < 2 and self._issue_one():
            pass
        if not self._issued:
            return None
        job = self._issued.pop(0)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(job["event"])
        arena, cuts, pl = job["arena"], job["cuts"], self._plan
        arena.record_stream(cur)  # allocated on the side stream, consumed on this one

        def cut(o, dtype):
            off, n = cuts[o]
            return arena[off:off + n * dtype.itemsize].view(dtype)

        (lo, lshape), (do, dshape), sparse, ebc = pl["layout"]
        kd = self.key_dtype
        out = {"label": cut(lo, torch.float32).view(*lshape),
               "dense": cut(do, torch.float32).view(*dshape), "sparse": {}}
        for name, (o_ro, o_k) in sparse.items():
            out["sparse"][name] = (pl["ro"][name] if o_ro is None else cut(o_ro, kd), cut(o_k, kd))
        if self._ebc_groups:
            out["ebc"] = [(cut(o_k, torch.int64),
                           pl["gbr"][g] if o_br is None else cut(o_br, torch.int64))
                          for g, (o_k, o_br) in enumerate(ebc)]
        return out

    def _upload_plan(self):
        """the subclass's plan with its arrays on the device and its static tensors built.
        _make_plan() adds to decode_plan(): "upload" (the arrays the kernel reads, concatenated
        into pl["device"]), "ro" {name: row offsets} and "gbr" [bucket range or None] of the
        outputs that do not depend on the data (built once with the host path's arithmetic and
        handed out with every batch: nothing downstream writes them), and "layout": (label,
        dense: (output, shape), {name: (row-offset output or None, key output)}, [(key output,
        bucket-range output or None)]), the outputs being indices into a batch's cuts."""
        pl = self._make_plan()
        blob = np.concatenate([a.view(np.uint8).reshape(-1) for a in pl.pop("upload")])
        with torch.cuda.stream(self._stream):  # (read by the decode launches of that stream)
            pl["device"] = torch.from_numpy(blob).to(self.device)
        pl["ro"] = {name: torch.from_numpy(a).to(self.device, self.key_dtype)
                    for name, a in pl["ro"].items()}
        pl["gbr"] = [None if a is None else torch.from_numpy(a).to(self.device) for a in pl["gbr"]]
        self._plan = pl
