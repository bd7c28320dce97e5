"""Bounded key -> vector table with LRU eviction: thin ctypes calls into hctr_lru_* (the backend of
sok.DynamicVariable(var_type="hybrid"); semantics in include/hugectr_amd.h and DESIGN.md "Hybrid
table").  No compute here."""
from __future__ import annotations

import ctypes
import math
import sys
import time
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

FILTERED = -2  # HCTR_LRU_FILTERED as int64: a key the low-frequency filter did not admit


def admit_below(p: float) -> int:
    """the filter's integer threshold ceil(p * 2^32): a key is admitted iff its 32-bit draw is below it
    (p = 1 admits every key, p = 0 none)"""
    return int(math.ceil(float(p) * 4294967296.0))


def first_call_since(call_ns: Sequence[int], threshold_ns: int) -> Optional[int]:
    """t0: the number (1, 2, ...) of the first inserting call issued at or after threshold_ns, None
    when there is none"""
    for t, ns in enumerate(call_ns, 1):
        if ns >= threshold_ns:
            return t
    return None


def check_hbm_budget(max_hbm_for_vectors) -> float:
    """max_hbm_for_vectors (GiB of value rows in HBM) as a float: a non-negative int or float;
    bool, NaN, negative or non-numeric values raise ValueError"""
    g = max_hbm_for_vectors
    if isinstance(g, bool) or not isinstance(g, (int, float)) or math.isnan(g) or g < 0:
        raise ValueError(f"max_hbm_for_vectors must be a non-negative number of GiB, not {g!r}")
    return float(g)


def check_load_factor(load) -> float:
    """max_load_factor as a float: a number in (0, 1]; anything else raises ValueError"""
    if isinstance(load, bool) or not isinstance(load, (int, float)) or not 0.0 < float(load) <= 1.0:
        raise ValueError(f"max_load_factor must be a number in (0, 1], not {load!r}")
    return float(load)


def check_capacities(max_capacity, init_capacity=None, bucket_size: int = 128):
    """the geometry hctr_lru_create_growing accepts, checked without a device: max_capacity (and
    init_capacity, when given) positive ints, init_capacity <= max_capacity, bucket_size 64, 128,
    192 or 256, and max_capacity = init_capacity * 2^j in whole buckets; ValueError otherwise"""
    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if max_capacity is None:
        raise ValueError('var_type="hybrid" needs max_capacity')
    if not is_int(max_capacity) or max_capacity < 1:
        raise ValueError(f"max_capacity must be a positive int, not {max_capacity!r}")
    S = bucket_size
    if not is_int(S) or S not in (64, 128, 192, 256):
        raise ValueError(f"max_bucket_size must be 64, 128, 192 or 256, not {S!r}")
    if init_capacity is None:
        return
    if not is_int(init_capacity) or init_capacity < 1:
        raise ValueError(f"init_capacity must be a positive int, not {init_capacity!r}")
    if init_capacity > max_capacity:
        raise ValueError(f"init_capacity {init_capacity} is above max_capacity {max_capacity}")
    b0, b1 = -(-init_capacity // S), -(-max_capacity // S)
    if b1 % b0 or (b1 // b0) & (b1 // b0 - 1):
        raise ValueError(f"max_capacity {max_capacity} must be init_capacity {init_capacity} "
                         f"times a power of two, in whole buckets of {S}")


def hbm_slots_for(max_hbm_for_vectors, dim: int, capacity: int, bucket_size: int) -> int:
    """H = min(C, floor(G * 2^30 / (dim * 4) / S) * S): the slots whose rows fit in G GiB of HBM,
    in whole buckets (C = capacity rounded up to whole buckets of S = bucket_size)"""
    g = check_hbm_budget(max_hbm_for_vectors)
    S = int(bucket_size)
    C = -(-int(capacity) // S) * S
    if math.isinf(g):
        return C
    return min(C, math.floor(g * 2**30 / (int(dim) * 4) / S) * S)


class HybridTable:
    """capacity slots (rounded up to whole buckets of bucket_size), dim fp32 per row.  close()
    frees the device memory; __del__ only does so as a fallback outside interpreter shutdown.
    call_ns[t - 1] is clock() (time.time_ns unless replaced) when inserting call t was issued.
    hbm_slots=H < capacity (a multiple of bucket_size): slots >= H keep their rows and optimizer
    states in host memory (hctr_lru_create_tiered); None or H >= capacity: all in HBM.
    init_capacity=C0 < capacity (capacity = C0 * 2^j in whole buckets): the table starts with C0
    slots and an inserting call doubles it, up to capacity, while the occupied slots plus the
    call's new keys exceed max_load_factor times the slots (hctr_lru_create_growing).  capacity
    stays the bound size can reach; current_capacity and doublings follow the table, and so do
    hbm_slots and placement(): at current_capacity C the HBM slots are min(C, H)."""

    def __init__(self, capacity: int, dim: int, initializer: str = "", bucket_size: int = 128,
                 key_dtype=torch.int64, seed: int = 0, clock: Optional[Callable[[], int]] = None,
                 hbm_slots: Optional[int] = None, *, init_capacity: Optional[int] = None,
                 max_load_factor: float = 0.5):
        self.dim = int(dim)
        self.clock = clock or time.time_ns
        self.call_ns: List[int] = []
        self.key_dtype = key_dtype
        self._h = ctypes.c_void_p()
        kt = _lib.KEY_I64 if key_dtype == torch.int64 else _lib.KEY_U32
        # (no budget: SIZE_MAX, never tiered)
        budget = ctypes.c_size_t(-1).value if hbm_slots is None else int(hbm_slots)
        check(lib.hctr_lru_create_growing(
            int(capacity if init_capacity is None else init_capacity), int(capacity),
            float(max_load_factor), int(bucket_size), self.dim, kt, str(initializer).encode(),
            int(seed), budget, ctypes.byref(self._h)))
        c, s = ctypes.c_size_t(), ctypes.c_size_t()
        check(lib.hctr_lru_capacity(self._h, ctypes.byref(c), ctypes.byref(s)))
        self.capacity, self.bucket_size = int(c.value), int(s.value)
        self._hbm_budget = min(budget, self.capacity)

    def _growth(self) -> Tuple[int, int, int]:
        a, b, d = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
        check(lib.hctr_lru_growth(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(d)))
        return int(a.value), int(b.value), int(d.value)

    @property
    def current_capacity(self) -> int:
        """the slots the table has now (capacity once it has grown all the way)"""
        return self._growth()[0]

    @property
    def doublings(self) -> int:
        return self._growth()[2]

    @property
    def hbm_slots(self) -> int:
        """the slots whose rows are in HBM at the capacity the table has now"""
        return self.placement()[0]

    @property
    def tiered(self) -> bool:
        """part of the table's slots are, or will be once it has grown, in host memory"""
        return self._hbm_budget < self.capacity

    def update_rows(self, staged: int) -> int:
        """the row bound of an hctr_updater that serves apply_update calls of up to `staged` keys:
        the slots in HBM and, on a tiered table, the host slots staged after them.  It grows with
        the table until the table has reached its capacity or its HBM budget."""
        return self.hbm_slots + (int(staged) if self.tiered else 0)

    def placement(self) -> Tuple[int, int, int]:
        """(hbm_slots, rows of the HBM row store (slots + per-call rows), host rows)"""
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        check(lib.hctr_lru_placement(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def close(self):
        if getattr(self, "_h", None):
            lib.hctr_lru_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _keys(self, keys: torch.Tensor) -> torch.Tensor:
        return keys.to(self.key_dtype).contiguous()

    def lookup_index(self, keys: torch.Tensor, insert: bool, evict: bool = False,
                     admit: Optional[float] = None, out: Optional[torch.Tensor] = None):
        """row numbers int64[n] (rows >= hbm_slots: per-call rows holding the initializer's value
        or, on a tiered table, a host-resident key's row);
        with evict=True also (evicted keys, evicted rows [m, dim]) -- one host synchronisation.
        admit=p (insert only): the low-frequency filter; keys it does not admit get FILTERED.
        out: a contiguous int64[n] tensor that receives the row numbers instead of a new one."""
        keys = self._keys(keys)
        n = keys.numel()
        idx = torch.empty(n, dtype=torch.int64, device=keys.device) if out is None else out
        assert idx.numel() == n and idx.dtype == torch.int64 and idx.is_contiguous()
        if insert:
            self.call_ns.append(int(self.clock()))
        ek = ev = m = None
        if evict:
            ek = torch.empty(n, dtype=self.key_dtype, device=keys.device)
            ev = torch.empty((n, self.dim), dtype=torch.float32, device=keys.device)
            m = ctypes.c_size_t()
        out = (ptr(idx), ptr(ek), ptr(ev), ctypes.byref(m) if evict else None, stream_ptr())
        if admit is not None and insert:
            check(lib.hctr_lru_lookup_index_filtered(self._h, ptr(keys), n, admit_below(admit),
                                                     *out))
        else:
            check(lib.hctr_lru_lookup_index(self._h, ptr(keys), n, 1 if insert else 0, *out))
        return (idx, ek[:m.value], ev[:m.value]) if evict else idx

    def compact(self, offsets: torch.Tensor, rows: torch.Tensor, keys: torch.Tensor,
                weights: Optional[torch.Tensor] = None):
        """(offsets, rows, keys, weights) of a ragged batch without its FILTERED positions, order
        kept inside every sample -- one host synchronisation"""
        keys = self._keys(keys)
        n, B = rows.numel(), offsets.numel() - 1
        dev = rows.device
        o_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        o_rows = torch.empty(n, dtype=torch.int64, device=dev)
        o_keys = torch.empty(n, dtype=self.key_dtype, device=dev)
        o_w = torch.empty(n, dtype=torch.float32, device=dev) if weights is not None else None
        w = weights.float().contiguous() if weights is not None else None
        kept = ctypes.c_size_t()
        check(lib.hctr_lru_compact(self._h, B, n, ptr(offsets.contiguous()), ptr(rows), ptr(keys),
                                   ptr(w), ptr(o_off), ptr(o_rows), ptr(o_keys), ptr(o_w),
                                   ctypes.byref(kept), stream_ptr()))
        m = kept.value
        return o_off, o_rows[:m], o_keys[:m], (o_w[:m] if o_w is not None else None)

    def find(self, keys: torch.Tensor) -> torch.Tensor:
        """slot of every stored key, INVALID for the others; no side effects"""
        keys = self._keys(keys)
        idx = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
        check(lib.hctr_lru_find(self._h, ptr(keys), keys.numel(), ptr(idx), stream_ptr()))
        return idx

    def rows_ptr(self) -> Tuple[int, int]:
        p, cap = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib.hctr_lru_rows(self._h, ctypes.byref(p), ctypes.byref(cap)))
        return p.value, int(cap.value)

    def state_ptr(self, i: int) -> int:
        p = ctypes.c_void_p()
        check(lib.hctr_lru_state(self._h, int(i), ctypes.byref(p), stream_ptr()))
        return p.value

    def host_part_ptr(self, array: int = 0) -> int:
        """device address of the host part of rows (0) or state array - 1; 0 when there is none"""
        p = ctypes.c_void_p()
        check(lib.hctr_lru_host_part(self._h, int(array), ctypes.byref(p)))
        return p.value or 0

    def gather_slots(self, array: int, slots: torch.Tensor) -> torch.Tensor:
        """[n, dim] rows (array 0) or state array - 1 of the slots, either tier; a row whose slot
        is not valid (>= capacity) is zero"""
        slots = slots.to(torch.int64).contiguous()
        out = torch.zeros((slots.numel(), self.dim), dtype=torch.float32, device=slots.device)
        check(lib.hctr_lru_gather_slots(self._h, int(array), ptr(slots), slots.numel(), ptr(out),
                                        stream_ptr()))
        return out

    def scatter_slots(self, array: int, slots: torch.Tensor, values: torch.Tensor,
                      add: bool = False):
        """array[slot] = values (or += with add); distinct slots, invalid ones skipped"""
        slots = slots.to(torch.int64).contiguous()
        v = values.reshape(-1, self.dim).float().contiguous()
        check(lib.hctr_lru_scatter_slots(self._h, int(array), ptr(slots), slots.numel(), ptr(v),
                                         1 if add else 0, stream_ptr()))

    def apply_update(self, updater, ro: torch.Tensor, slots: torch.Tensor, grads: torch.Tensor,
                     optimizer: int, hp: dict, times: int):
        """one sparse optimizer step on the slots' rows and states (hctr_lru_apply_update; the
        states the optimizer needs must have been allocated through state_ptr)"""
        check(lib.hctr_lru_apply_update(
            self._h, updater, ro.numel() - 1, slots.numel(), ptr(ro), ptr(slots),
            ptr(grads.contiguous()), _lib.F32, optimizer, hp["lr"], hp["beta1"], hp["beta2"],
            hp["epsilon"], hp["momentum"], hp["scaler"], int(times), stream_ptr()))

    def _export(self, min_score: int, n: int):
        """(keys, rows [g, dim], slots, scores) of the first n exported slots (hctr_lru_export_if)"""
        keys = torch.empty(n, dtype=self.key_dtype, device="cuda")
        slots = torch.empty(n, dtype=torch.int64, device="cuda")
        scores = torch.empty(n, dtype=torch.int64, device="cuda")
        rows = torch.empty((n, self.dim), dtype=torch.float32, device="cuda")
        got = ctypes.c_size_t()
        if n:
            check(lib.hctr_lru_export_if(self._h, min_score, ptr(keys), ptr(slots), ptr(scores),
                                         ptr(rows), n, ctypes.byref(got), None, stream_ptr()))
        g = got.value
        return keys[:g], rows[:g], slots[:g], scores[:g]

    def export(self, with_slots: bool = False):
        """(keys, rows [n, dim]) of the occupied slots in slot order; with_slots=True adds their
        slots and scores (int64)"""
        out = self._export(0, self.size())
        return out if with_slots else out[:2]

    def export_if(self, min_score: int):
        """(keys, rows [n, dim], slots, scores) of the occupied slots with score >= min_score, in
        slot order (min_score <= 1: every occupied slot)"""
        got, matched = ctypes.c_size_t(), ctypes.c_size_t()
        ms = max(int(min_score), 0)
        check(lib.hctr_lru_export_if(self._h, ms, None, None, None, None, 0, ctypes.byref(got),
                                     ctypes.byref(matched), stream_ptr()))
        return self._export(ms, matched.value)

    def filtered_count(self) -> int:
        out = ctypes.c_uint64()
        check(lib.hctr_lru_filtered_count(self._h, ctypes.byref(out), stream_ptr()))
        return int(out.value)

    def size(self) -> int:
        out = ctypes.c_size_t()
        check(lib.hctr_lru_size(self._h, ctypes.byref(out), stream_ptr()))
        return int(out.value)

    def rejected_count(self) -> int:
        out = ctypes.c_uint64()
        check(lib.hctr_lru_rejected_count(self._h, ctypes.byref(out), stream_ptr()))
        return int(out.value)

