"""Sequential numpy restatement of the hybrid table's semantics (include/hugectr_amd.h hctr_lru_*,
DESIGN.md "Hybrid table").  Test infrastructure only: the product never imports it.

One inserting call t:
  1. keys already stored get score t;
  2. the call's distinct missing keys, bucket by bucket, ascending key (as unsigned integers) inside
     a bucket: the lowest empty slot, else the victim = smallest (score, slot) among scores < t
     (its (key, row) is evicted), else the key is rejected;
  3. a new row gets the initializer's value, its optimizer state rows are zeroed.
A read-only call changes nothing; a key that is not stored reads the initializer's value.
"""
import numpy as np

EMPTY = (1 << 64) - 1
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _block(h, k):
    k = (k * 0xCC9E2D51) & M32
    k = _rotl(k, 15)
    k = (k * 0x1B873593) & M32
    h ^= k
    h = _rotl(h, 13)
    return (h * 5 + 0xE6546B64) & M32


def _fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def murmur3(key: int, key_bytes: int = 8) -> int:
    """MurmurHash3_x86_32 of the key's bytes, seed 0 (hctr_hash_keys)"""
    u = key & M64
    if key_bytes == 4:
        return _fmix(_block(0, u & M32) ^ 4)
    return _fmix(_block(_block(0, u & M32), u >> 32) ^ 8)


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def parse_initializer(ini: str):
    """(constant or None): "ones" | "zeros" | a float literal, else uniform (0, 1]"""
    if ini == "ones":
        return 1.0
    if ini == "zeros":
        return 0.0
    try:
        return float(np.float32(float(ini))) if ini else None
    except ValueError:
        return None


def init_vector(const, seed: int, key: int, D: int) -> np.ndarray:
    if const is not None:
        return np.full(D, const, dtype=np.float32)
    u = key & M64
    out = np.empty(D, dtype=np.float32)
    for e in range(D):
        h = _splitmix(seed ^ _splitmix((u * 0x100000001B3 + e) & M64))
        out[e] = (np.float32(h >> 40) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)
    return out


class LruTable:
    def __init__(self, capacity: int, dim: int, initializer: str = "", bucket_size: int = 128,
                 seed: int = 0, key_bytes: int = 8, num_state: int = 0):
        S = bucket_size
        self.S, self.D, self.seed, self.key_bytes = S, dim, seed, key_bytes
        self.C = -(-capacity // S) * S
        self.nb = self.C // S
        self.const = parse_initializer(initializer)
        self.keys = np.full(self.C, EMPTY, dtype=np.uint64)
        self.scores = np.zeros(self.C, dtype=np.uint64)
        self.rows = np.zeros((self.C, dim), dtype=np.float32)
        self.states = [np.zeros((self.C, dim), dtype=np.float32) for _ in range(num_state)]
        self.t = 0
        self.rejected = 0
        self.where = {}  # key (unsigned) -> slot

    def bucket(self, key: int) -> int:
        return murmur3(key, self.key_bytes) % self.nb

    def init(self, key: int) -> np.ndarray:
        return init_vector(self.const, self.seed, key, self.D)

    def _u(self, key) -> int:
        return int(key) & (M64 if self.key_bytes == 8 else M32)

    def find(self, keys):
        """slot per key, -1 when not stored"""
        return np.array([self.where.get(self._u(k), -1) for k in keys], dtype=np.int64)

    def lookup(self, keys, insert: bool):
        """(vectors [n, D], slots [n] (-1: not stored), evicted keys, evicted rows [m, D])"""
        keys = [self._u(k) for k in keys]
        ev_k, ev_r = [], []
        if insert:
            self.t += 1
            t = self.t
            for k in keys:
                if k in self.where:
                    self.scores[self.where[k]] = t
            missing = sorted({k for k in keys if k not in self.where and k != EMPTY},
                             key=lambda k: (self.bucket(k), k))
            rejected_keys = [k for k in set(keys) if k == EMPTY and k not in self.where]
            self.rejected += len(rejected_keys)
            for k in missing:
                b = self.bucket(k)
                base = b * self.S
                sl = None
                for s in range(base, base + self.S):
                    if self.keys[s] == np.uint64(EMPTY):
                        sl = s
                        break
                if sl is None:
                    best = None
                    for s in range(base, base + self.S):
                        if int(self.scores[s]) < t and (best is None or
                                                        (int(self.scores[s]), s) < best):
                            best = (int(self.scores[s]), s)
                    if best is None:
                        self.rejected += 1
                        continue
                    sl = best[1]
                    old = int(self.keys[sl])
                    ev_k.append(old)
                    ev_r.append(self.rows[sl].copy())
                    del self.where[old]
                self.keys[sl] = np.uint64(k)
                self.scores[sl] = t
                self.rows[sl] = self.init(k)
                for st in self.states:
                    st[sl] = 0.0
                self.where[k] = sl
        slots = np.array([self.where.get(k, -1) for k in keys], dtype=np.int64)
        vec = np.stack([self.rows[s] if s >= 0 else self.init(k) for k, s in zip(keys, slots)]) \
            if keys else np.zeros((0, self.D), dtype=np.float32)
        ev_rows = np.stack(ev_r) if ev_r else np.zeros((0, self.D), dtype=np.float32)
        return vec, slots, np.array(ev_k, dtype=np.uint64), ev_rows

    def size(self) -> int:
        return len(self.where)

    def export(self):
        """(keys uint64, rows) of the occupied slots in slot order"""
        occ = self.keys != np.uint64(EMPTY)
        return self.keys[occ].copy(), self.rows[occ].copy()
