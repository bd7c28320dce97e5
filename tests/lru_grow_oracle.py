"""Sequential restatement of the hybrid table's growth (include/hugectr_amd.h
hctr_lru_create_growing, DESIGN.md "Hybrid table"), on top of tests/lru_oracle.py and
tests/lru_filter_oracle.py.  Test infrastructure only: the product never imports it.

The table starts with C0 slots.  An inserting call takes occ = the occupied slots and m = its
distinct keys that are not stored (the reserved key aside; in a filtered call only admitted keys get
this far) once, doubles C while C < Cmax and occ + m > L * C, and then runs as LruTable's call on
the capacity reached.  Read-only calls and the empty call never grow the table.

One doubling, nb buckets -> 2 nb: a key of bucket b now hashes to b or to b + nb.  The keys of b
that move take, in ascending old-slot order, slots (b + nb) * S + 0, 1, ... with their score, row
and states, and leave empty slots; the others keep everything.
"""
import numpy as np

from lru_filter_oracle import FilterLruTable
from lru_oracle import EMPTY, LruTable, murmur3


class GrowLruTable(LruTable):
    def __init__(self, init_capacity: int, max_capacity: int, dim: int, initializer: str = "",
                 bucket_size: int = 128, seed: int = 0, key_bytes: int = 8, num_state: int = 0,
                 max_load_factor: float = 0.5):
        super().__init__(init_capacity, dim, initializer, bucket_size, seed, key_bytes, num_state)
        S = bucket_size
        self.Cmax = -(-max_capacity // S) * S
        c = self.C
        while c < self.Cmax:
            c *= 2
        if c != self.Cmax:
            raise ValueError(f"max_capacity {max_capacity} is not init_capacity {init_capacity} "
                             "times a power of two")
        self.L = float(np.float32(max_load_factor))     # a float32 widened to double
        if not 0.0 < self.L <= 1.0:
            raise ValueError("max_load_factor must be in (0, 1]")
        self.doublings = 0
        self.last_moves = []      # (old slot, new slot) of the latest doubling, in bucket order

    def double(self):
        S, nb, C = self.S, self.nb, self.C

        def wider(a, fill):
            out = np.full((2 * C,) + a.shape[1:], fill, dtype=a.dtype)
            out[:C] = a
            return out

        self.keys = wider(self.keys, np.uint64(EMPTY))
        self.scores = wider(self.scores, 0)
        self.rows = wider(self.rows, 0)
        self.states = [wider(st, 0) for st in self.states]
        self.last_moves = []
        for b in range(nb):
            rank = 0
            for s in range(b * S, (b + 1) * S):
                k = int(self.keys[s])
                if k == EMPTY or murmur3(k, self.key_bytes) % (2 * nb) == b:
                    continue
                d = (b + nb) * S + rank
                rank += 1
                self.keys[d], self.scores[d], self.rows[d] = self.keys[s], self.scores[s], \
                    self.rows[s]
                for st in self.states:
                    st[d] = st[s]
                self.keys[s], self.scores[s] = np.uint64(EMPTY), 0
                self.where[k] = d
                self.last_moves.append((s, d))
        self.C, self.nb = 2 * C, 2 * nb
        self.doublings += 1

    def lookup(self, keys, insert: bool):
        if insert and len(keys) and self.C < self.Cmax:
            occ = len(self.where)
            m = len({self._u(k) for k in keys} - set(self.where) - {EMPTY})
            while self.C < self.Cmax and occ + m > self.L * self.C:
                self.double()
        return super().lookup(keys, insert)


class GrowFilterLruTable(FilterLruTable, GrowLruTable):
    """the filter's super().lookup(kept, True) lands in GrowLruTable.lookup: m counts admitted keys"""


def checked_calls(calls: int = 24):
    """[(keys int64, train)]: the input on which a table grown from 128 to 1024 slots (S = 64) was
    checked against one created at 1024: 3 doublings, 675 keys, nothing evicted or rejected in
    either, fullest bucket 57 of 64.  Every fourth call is read-only."""
    rng = np.random.default_rng(7)
    out = []
    for call in range(calls):
        n = int(rng.integers(20, 120))
        keys = (rng.zipf(1.3, size=n) * 7919 + 13 * call) % 100000
        out.append((keys.astype(np.int64), call % 4 != 3))
    return out
