"""Shared synthetic-input builders for the parity tests (seeded, numpy)."""
import numpy as np


def make_csr(rng, batch, slot_num, max_hot, vocab_per_slot, empty_frac=0.2, one_hot=False,
             key_offset=True):
    """Full-batch CSR as the reference's reader hands it to every GPU: row_offset[batch*slot+1],
    keys with cumulative slot offsets added (R/HugeCTR/src/pybind/add_input.cpp:315-317)."""
    buckets = batch * slot_num
    if one_hot:
        lens = np.ones(buckets, dtype=np.int64)
    else:
        lens = rng.integers(0, max_hot + 1, size=buckets).astype(np.int64)
        lens[rng.random(buckets) < empty_frac] = 0
    ro = np.zeros(buckets + 1, dtype=np.int64)
    np.cumsum(lens, out=ro[1:])
    nnz = int(ro[-1])
    slot_of_bucket = np.tile(np.arange(slot_num), batch)
    slot_of_key = np.repeat(slot_of_bucket, lens)
    keys = rng.integers(0, vocab_per_slot, size=nnz).astype(np.int64)
    if key_offset:
        keys = keys + slot_of_key * vocab_per_slot
    return ro, keys


def assert_close(a, b, rtol, atol, what=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    bad = err > tol
    assert not bad.any(), (f"{what}: {bad.sum()} / {bad.size} mismatches, max abs err "
                           f"{err.max():.3e}, max rel {np.max(err / (np.abs(b) + 1e-30)):.3e}")


# ---- device buffers of the matrix files (test_pool_matrix_gpu.py, test_ebc_matrix_gpu.py) ---------
GUARD = 64


def torch_dtype(dt):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]


def lib_code(dt):
    from hugectr_amd import _lib
    return {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}[dt]


class DevIn:
    """a device copy of a host array (kept next to it: the call must leave it unchanged);
    mis: the device data starts that many elements into its allocation"""

    def __init__(self, a, mis=0):
        import torch
        self.host = np.array(a)
        raw = self.host
        if raw.dtype == np.uint64:
            raw = raw.view(np.int64)
        elif raw.dtype == np.uint32:
            raw = raw.view(np.int32)
        flat = torch.from_numpy(raw.reshape(-1))
        base = torch.zeros(flat.numel() + mis, dtype=flat.dtype)
        base[mis:] = flat
        self.base = base.to("cuda")
        self.t = self.base[mis:]
        self.raw = raw.reshape(-1)

    @property
    def p(self):
        from hugectr_amd import _lib
        return _lib.ptr(self.t)

    def assert_unchanged(self, what):
        got = self.t.cpu().numpy()
        assert got.tobytes() == self.raw.tobytes(), f"the call changed its input {what}"


class DevOut:
    """rows x D output behind a poison fill, GUARD rows of poison after it; mis as for DevIn.
    dt: "f32" / "f16" / "bf16" (poison = NaN; int_bits: the raw 32 / 16-bit patterns, poison = all
    ones, a NaN in every type) or "i32" / "i64" (integers, always raw, poison = all ones = -1)"""

    def __init__(self, rows, D, dt, mis=0, int_bits=False):
        import torch
        int_bits = int_bits or dt in ("i32", "i64")
        self.rows, self.D, self.mis, self.int_bits = rows, D, mis, int_bits
        n = (rows + GUARD) * D
        if int_bits:
            tdt = {"f32": torch.int32, "i32": torch.int32, "i64": torch.int64}.get(dt, torch.int16)
            self.base = torch.full((n + mis + 8,), -1, dtype=tdt, device="cuda")
        else:
            self.base = torch.full((n + mis + 8,), float("nan"), dtype=torch_dtype(dt),
                                   device="cuda")
        self.t = self.base[mis:mis + n]

    @property
    def p(self):
        from hugectr_amd import _lib
        return _lib.ptr(self.t)

    def fill(self, a):
        """an in/out buffer (an accumulator, a master weight): the rows start as the host array a,
        whose element type is the buffer's"""
        import torch
        raw = np.ascontiguousarray(a).reshape(-1)
        assert raw.size == self.rows * self.D
        self.t[:raw.size].copy_(torch.from_numpy(raw))
        return self

    def result(self):
        """the rows as fp32 (or raw integers); asserts that everything around them is untouched"""
        b = self.base if self.int_bits else self.base.float()
        b = b.cpu().numpy()
        lo, hi = self.mis, self.mis + self.rows * self.D
        around = np.concatenate([b[:lo], b[hi:]])
        assert around.size >= GUARD * self.D
        if self.int_bits:
            assert (around == -1).all(), "write outside the output rows"
        else:
            assert np.isnan(around).all(), "write outside the output rows"
        return b[lo:hi].reshape(self.rows, self.D)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape
    if not (g == w).all():
        bad = np.argwhere(g != w)
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at row {r} "
                             f"col {c}: got {got[r, c]!r} want {want[r, c]!r}")
