"""Sequential restatement of the hybrid table's low-frequency filter and export_if (include/
hugectr_amd.h hctr_lru_lookup_index_filtered / hctr_lru_export_if, DESIGN.md "Hybrid table"), on
top of tests/lru_oracle.py.  Test infrastructure only: the product never imports it.

In an inserting call t with admission probability p, a key the table does not hold is admitted iff
    u(seed, key, t) = splitmix64(seed ^ splitmix64(key ^ splitmix64(t))) >> 32  <  ceil(p * 2^32);
stored keys are hits as always.  A refused key is left out of the call entirely: it is not
inserted, touches no score, is not rejected, and each of its positions counts as filtered.
"""
import math

import numpy as np

from lru_oracle import EMPTY, LruTable

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def admit_draw(seed: int, keys, t: int) -> np.ndarray:
    """u(seed, key, t) for every key (numpy uint64 arithmetic), as uint64 values below 2^32"""
    k = np.asarray(keys).astype(np.int64).view(np.uint64) if np.asarray(keys).dtype != np.uint64 \
        else np.asarray(keys)
    tt = _splitmix_np(np.array([t], dtype=np.uint64))
    return _splitmix_np(np.uint64(seed) ^ _splitmix_np(k ^ tt)) >> np.uint64(32)


def admit_below(p: float) -> int:
    return int(math.ceil(float(p) * 4294967296.0))


class FilterLruTable(LruTable):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.filtered = 0

    def lookup(self, keys, insert: bool, admit=None):
        """admit=None: LruTable.lookup.  admit=p (insert only): (vectors [n, D] (zero where
        filtered), slots [n] (-1: not stored), evicted keys, evicted rows, filtered mask [n])"""
        if admit is None or not insert:
            return super().lookup(keys, insert)
        ukeys = np.array([self._u(k) for k in keys], dtype=np.uint64)
        stored = np.array([int(k) in self.where for k in ukeys], dtype=bool)
        draw = admit_draw(self.seed, ukeys, self.t + 1)
        filt = ~stored & (draw >= np.uint64(admit_below(admit)))
        self.filtered += int(filt.sum())
        kept = ukeys[~filt]
        vec_k, slots_k, ev_k, ev_r = super().lookup([int(k) for k in kept], True)
        n = ukeys.size
        vec = np.zeros((n, self.D), dtype=np.float32)
        slots = np.full(n, -1, dtype=np.int64)
        vec[~filt] = vec_k
        slots[~filt] = slots_k
        return vec, slots, ev_k, ev_r, filt

    def export_if(self, min_score: int):
        """(keys uint64, slots, scores, rows) of the occupied slots with score >= min_score, in slot
        order"""
        sel = (self.keys != np.uint64(EMPTY)) & (self.scores >= np.uint64(max(min_score, 0)))
        s = np.nonzero(sel)[0]
        return self.keys[s].copy(), s, self.scores[s].copy(), self.rows[s].copy()
