"""Every dispatch branch of the gather / pool family (hugectr_amd/csrc/embedding_kernels.hip) through
the C ABI, against the CPU oracle (bit for bit) or numpy fp64 (bounds derived from the arithmetic):
hctr_forward_pool / _multihot / _mapped, hctr_forward_pool_ptrs / _ptrs_mapped,
hctr_forward_pool_weighted, hctr_expand_key_grads, hctr_forward_reorder / hctr_backward_reorder, and
wgrad_kernel (sparse_update.hip) through SparseEmbeddingHash.

Every call writes into a NaN-poisoned (integers: all-ones) buffer with GUARD rows behind the last
real row that must still hold the poison afterwards, and its inputs must come back unchanged.

Grid-stride loops.  All launches use kBlock = 256 threads; pooling is capped at 2048 blocks, the
weighted / expand kernels at 8192, reorder and wgrad at 2048.  One pass of the grid covers
cap x groups_per_block x buckets_per_group work items; the cases marked "grid" below use
2 x that + 37 buckets (reorder / wgrad: more than 2 x that many units), i.e. two full passes and
a partial third:

  kernel                                   one pass covers        case that exceeds it
  pool_vec4_kernel<64, BU=4>   D = 256     2048 *  4 * 4 = 32768  test_pool_grid / test_one_hot_grid, 65573
  pool_vec4_kernel<32, BU=4>   D = 128     2048 *  8 * 4 = 65536  test_pool_grid / test_one_hot_grid, 131109
  pool_flat_kernel<64, NB=8>   D = 256     2048 *  4 * 8 = 65536  test_pool_grid[flat], 131109
  pool_generic_kernel          any D       2048 *  4 * 1 =  8192  test_pool_grid[D = 11, 70], 16421
  pool_ptrs_vec4_kernel<64, 4> D = 256     2048 *  4 * 4 = 32768  test_ptrs_grid, 65573
  pool_ptrs_generic_kernel     any D       2048 *  4 * 1 =  8192  test_ptrs_grid[D = 11], 16421
  pool_weighted_vec4_kernel<64> D = 256    8192 *  4     = 32768  test_weighted_grid, 65573
  pool_weighted_kernel         any D       8192 *  4     = 32768  test_weighted_grid[D = 6], 65573
  expand_key_grads_vec4_kernel<64>         8192 *  4     = 32768  test_expand_grid, 65573
  expand_key_grads_kernel      any D       8192 *  4     = 32768  test_expand_grid[D = 6], 65573
  reorder_kernel<float4 | float | u16>     2048 * 256   = 524288  test_reorder_grid, > 1.1 M units
  wgrad_kernel                             2048 * 256   = 524288  test_wgrad_grid, 1126400 elements

Smaller vec4 sizes are left out of the grid cases: a pass covers 2048 * (256 / LPR) * 4 buckets, so
D = 64 would already need 262 181 buckets and D = 4 over four million to loop three times; the loop
body is the same template.  Under HCTR_EMU=1 (the host interpreter) the grid cases are dropped."""
import functools
import os

import numpy as np
import pytest

# the device-buffer plumbing is shared with the other matrix files
from util import DevIn as _In, DevOut as _Out, assert_bits as _assert_bits
from util import lib_code as _code, torch_dtype as _torch_dtype

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
U = 2.0 ** -24  # unit roundoff of fp32
LPR_D = [4, 8, 16, 32, 64, 128, 256]     # the seven vec4 cases of every switch
MOD4_GENERIC_D = [12, 20, 512]           # D % 4 == 0 outside the switch -> generic
GENERIC_D = [1, 3, 6, 11, 70]            # odd, even (align2 mean rule), more than 64 lanes
DTYPES = ["f32", "f16", "bf16"]


def _grid(cases):
    return [] if EMU else cases


# ---- inputs (built once per shape, never written again) ------------------------------------------
@functools.lru_cache(maxsize=None)
def _ragged(nb, V, seed=0, mean_len=3.0, invalid=True):
    """row_offset / value_index of nb ragged buckets: ~30 % empty, three leading empties, one bucket
    of 300 keys, a long last bucket, lengths 0..9 otherwise (1, 3, 4, 5, 9 forced), ~5 % INVALID"""
    from oracle import pyoracle
    rng = np.random.default_rng(1000 + seed)
    hi = int(2 * mean_len / 0.7) + 1
    lens = rng.integers(0, hi, size=nb)
    lens[rng.random(nb) < 0.3] = 0
    if nb >= 16:
        lens[:3] = 0
        lens[3:9] = [1, 3, 4, 5, 9, 300]
        lens[nb // 2] = 77
        lens[-1] = 19
    ro = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(lens, out=ro[1:])
    vi = rng.integers(0, V, size=int(ro[-1])).astype(np.uint64)
    if invalid:
        vi[rng.random(vi.size) < 0.05] = pyoracle.INVALID
    ro.setflags(write=False)
    vi.setflags(write=False)
    return ro, vi


@functools.lru_cache(maxsize=None)
def _one_hot(nb, V, seed=0):
    """one key per bucket, ~5 % INVALID, INVALID forced at the first and the last position"""
    from oracle import pyoracle
    rng = np.random.default_rng(2000 + seed)
    vi = rng.integers(0, V, size=nb).astype(np.uint64)
    vi[rng.random(nb) < 0.05] = pyoracle.INVALID
    vi[0] = vi[nb - 1] = pyoracle.INVALID
    if nb > 2:
        vi[1] = 1  # (and a live key next to each of them)
        vi[nb - 2] = 2
    ro = np.arange(nb + 1, dtype=np.int64)
    ro.setflags(write=False)
    vi.setflags(write=False)
    return ro, vi


@functools.lru_cache(maxsize=None)
def _table(V, D):
    t = np.random.default_rng(3000 + D).standard_normal((V, D)).astype(np.float32)
    t.setflags(write=False)
    return t


def _want(oracle_mod, kind, nb, V, D, comb, dt):
    """the oracle's pooled vectors; the small shapes are computed once and shared"""
    return (_want_cached if nb <= 2048 else _want_new)(oracle_mod, kind, nb, V, D, comb, dt)


def _want_new(oracle_mod, kind, nb, V, D, comb, dt):
    ro, vi = (_one_hot if kind == "onehot" else _ragged)(nb, V)
    tab = _table(V, D)
    if dt == "f32":
        w = oracle_mod.forward(ro, vi, tab, D, comb)
    else:
        w = oracle_mod.forward_mixed(ro, vi, tab, D, comb, dt)
    w.setflags(write=False)
    return w


_want_cached = functools.lru_cache(maxsize=None)(_want_new)


def _transposed(want, samples, lookups):
    """[lookup][sample] bucket order -> [sample][lookup] rows: row u at (u % samples) * lookups +
    u / samples"""
    D = want.shape[1]
    return np.ascontiguousarray(want.reshape(lookups, samples, D).transpose(1, 0, 2)).reshape(-1, D)


def _run_pool(entry, nb, D, comb, ro, ktype, vi, tab, out, dt, samples=0, lookups=0, word=None):
    """entry: 'bucket' = hctr_forward_pool, 'flat' = hctr_forward_pool_multihot,
    'mapped-bucket' / 'mapped-flat' = hctr_forward_pool_mapped with multi_hot 0 / 1"""
    from hugectr_amd import _lib
    L = _lib.lib
    if entry == "bucket":
        rc = L.hctr_forward_pool(nb, D, comb, ro.p, ktype, vi.p, tab.p, out.p, _code(dt),
                                 _lib.stream_ptr())
    elif entry == "flat":
        rc = L.hctr_forward_pool_multihot(nb, D, comb, ro.p, ktype, vi.p, tab.p, out.p, _code(dt),
                                          _lib.stream_ptr())
    else:
        rc = L.hctr_forward_pool_mapped(nb, D, comb, ro.p, ktype, vi.p, tab.p, out.p, _code(dt),
                                        1 if entry == "mapped-flat" else 0, samples, lookups,
                                        word.p if word is not None else None, _lib.stream_ptr())
    _lib.check(rc)


def _pool_case(oracle, entry, nb, V, D, comb, dt, u32=False, out_mis=0, tab_mis=0, onehot=False,
               samples=0, lookups=0, word=None):
    """one launch -> the output rows; checks oracle parity, the guard rows and the inputs"""
    from hugectr_amd import _lib
    ro_h, vi_h = (_one_hot if onehot else _ragged)(nb, V)
    ro = _In(ro_h.astype(np.uint32) if u32 else ro_h)
    vi, tab = _In(vi_h), _In(_table(V, D), mis=tab_mis)
    w = _In(np.array([word], dtype=np.uint32)) if word is not None else None
    out = _Out(nb, D, dt, mis=out_mis)
    _run_pool(entry, nb, D, comb, ro, _lib.KEY_U32 if u32 else _lib.KEY_I64, vi, tab, out, dt,
              samples, lookups, w)
    got = out.result()
    want = _want(oracle, "onehot" if onehot else "ragged", nb, V, D, comb, dt)
    if samples:
        want = _transposed(want, samples, lookups)
    _assert_bits(got, want, f"{entry} D={D} comb={comb} {dt} nb={nb}")
    for x, name in ((ro, "row_offset"), (vi, "value_index"), (tab, "table")):
        x.assert_unchanged(name)
    if w is not None:
        w.assert_unchanged("one_hot")
    return got


# ---- 1. index-form pooling -----------------------------------------------------------------------
NB, V = 1003, 500


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("comb", [0, 1])
@pytest.mark.parametrize("D", LPR_D + MOD4_GENERIC_D + GENERIC_D)
def test_pool_matrix(oracle, D, comb, dt):
    """1a: every LPR, the generic sizes, every output type, both combiners, both kernels: the
    oracle's bits, and the bucket and the flat kernel agree with each other"""
    a = _pool_case(oracle, "bucket", NB, V, D, comb, dt)
    b = _pool_case(oracle, "flat", NB, V, D, comb, dt)
    _assert_bits(a, b, "bucket vs flat kernel")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("comb", [0, 1])
@pytest.mark.parametrize("D", [16, 128, 11])
@pytest.mark.parametrize("entry", ["bucket", "flat"])
def test_pool_u32_offsets(oracle, entry, D, comb, dt):
    """1a: row_offset as uint32 (KEY_U32)"""
    _pool_case(oracle, entry, NB, V, D, comb, dt, u32=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ["out", "table"])
@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("entry", ["bucket", "flat"])
def test_pool_misaligned(oracle, entry, D, which, dt):
    """1b: `out` one element (4 / 2 bytes) or `table` 4 bytes into its allocation -> the generic
    kernel at a vec4 size: same bits as the aligned call (and the oracle)"""
    for comb in (0, 1):
        a = _pool_case(oracle, entry, NB, V, D, comb, dt)
        b = _pool_case(oracle, entry, NB, V, D, comb, dt, out_mis=int(which == "out"),
                       tab_mis=int(which == "table"))
        _assert_bits(a, b, "aligned vs misaligned")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [4, 16, 128, 256])
@pytest.mark.parametrize("nb", [1, 3, 4, 5, 1003])
def test_one_hot_word(oracle, nb, D, dt):
    """1c: the one-hot loop (word = 1) against the general loop (word = 0) on the same one-key
    buckets; bucket counts around the BU = 4 unroll, INVALID at position 0 and at the clamped tail"""
    for comb in (0, 1):
        a = _pool_case(oracle, "mapped-bucket", nb, V, D, comb, dt, onehot=True, word=1)
        b = _pool_case(oracle, "mapped-bucket", nb, V, D, comb, dt, onehot=True, word=0)
        _assert_bits(a, b, "word = 1 vs word = 0")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("samples,lookups", [(37, 5), (8, 26)])
@pytest.mark.parametrize("path,D", [("bucket", 16), ("bucket", 128), ("flat", 16), ("flat", 128),
                                    ("onehot", 16), ("onehot", 128), ("bucket", 11), ("flat", 11)])
def test_output_map(oracle, path, D, samples, lookups, dt):
    """1d: OutMap: bucket u = [lookup][sample] is stored at row [sample][lookup]"""
    nb = samples * lookups
    for comb in (0, 1):
        if path == "onehot":
            _pool_case(oracle, "mapped-bucket", nb, V, D, comb, dt, onehot=True, word=1,
                       samples=samples, lookups=lookups)
        else:
            _pool_case(oracle, "mapped-" + path, nb, V, D, comb, dt, samples=samples,
                       lookups=lookups)


def _factor(n):
    f = next(k for k in range(3, 1000) if n % k == 0)
    return n // f, f


@pytest.mark.parametrize("entry,D,dt", _grid([
    ("bucket", 256, "f32"), ("bucket", 128, "f32"), ("flat", 256, "f32"), ("flat", 256, "f16"),
    ("bucket", 11, "f32"), ("bucket", 70, "f32")]))
def test_pool_grid(oracle, entry, D, dt):
    """1e: 2 x (buckets of one grid pass) + 37 ragged buckets (table in the module docstring)"""
    cover = 8192 if D % 4 else 2048 * (256 // (D // 4)) * (8 if entry == "flat" else 4)
    _pool_case(oracle, entry, 2 * cover + 37, V, D, 1, dt)


@pytest.mark.parametrize("D,dt,word,mapped", _grid([
    (256, "f32", 1, False), (256, "f32", 0, False), (128, "f32", 1, False), (128, "f32", 0, False),
    (128, "bf16", 1, False), (256, "f32", 1, True)]))
def test_one_hot_grid(oracle, D, dt, word, mapped):
    """1e: the one-hot loop from its second pass on (the prefetched indices of pass i + 1 are used),
    with the word set and clear, and once through the output map"""
    nb = 2 * 2048 * (256 // (D // 4)) * 4 + 37
    samples, lookups = _factor(nb) if mapped else (0, 0)
    _pool_case(oracle, "mapped-bucket", nb, V, D, 0, dt, onehot=True, word=word, samples=samples,
               lookups=lookups)


# ---- 2. pointer-form pooling ---------------------------------------------------------------------
def _ptrs_case(oracle, nb, D, comb, dt, out_mis=0, samples=0, lookups=0, split=False):
    from hugectr_amd import _lib
    from oracle import pyoracle
    ro_h, vi_h = _ragged(nb, V)
    tab_h = _table(V, D)
    ro = _In(ro_h)
    live = vi_h != pyoracle.INVALID
    idx = np.where(live, vi_h, 0).astype(np.int64)
    if split:  # rows [0, V/2) and [V/2, V) in two allocations (a dynamic table's per-class stores)
        tabs = [_In(tab_h[:V // 2]), _In(np.zeros(12345, np.float32)), _In(tab_h[V // 2:])]
        base = np.where(idx < V // 2, tabs[0].t.data_ptr(),
                        tabs[2].t.data_ptr() - (V // 2) * D * 4).astype(np.int64)
    else:
        tabs = [_In(tab_h)]
        base = np.full(idx.size, tabs[0].t.data_ptr(), dtype=np.int64)
    rows = _In(np.where(live, base + idx * (D * 4), 0).astype(np.int64))
    out = _Out(nb, D, dt, mis=out_mis)
    if samples:
        rc = _lib.lib.hctr_forward_pool_ptrs_mapped(nb, D, comb, ro.p, rows.p, out.p, _code(dt),
                                                    samples, lookups, _lib.stream_ptr())
    else:
        rc = _lib.lib.hctr_forward_pool_ptrs(nb, D, comb, ro.p, rows.p, out.p, _code(dt),
                                             _lib.stream_ptr())
    _lib.check(rc)
    got = out.result()
    want = _want(oracle, "ragged", nb, V, D, comb, dt)
    if samples:
        want = _transposed(want, samples, lookups)
    _assert_bits(got, want, f"ptrs D={D} comb={comb} {dt} nb={nb}")
    for x, name in [(ro, "row_offset"), (rows, "rows")] + [(t, "table") for t in tabs]:
        x.assert_unchanged(name)
    return got


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("comb", [0, 1])
@pytest.mark.parametrize("D", LPR_D + [12, 6, 11, 70])
def test_ptrs_matrix(oracle, D, comb, dt):
    _ptrs_case(oracle, NB, D, comb, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_ptrs_misaligned_out(oracle, dt):
    for comb in (0, 1):
        a = _ptrs_case(oracle, NB, 16, comb, dt)
        b = _ptrs_case(oracle, NB, 16, comb, dt, out_mis=1)
        _assert_bits(a, b, "aligned vs misaligned")


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("D", [32, 11])
def test_ptrs_output_map(oracle, D, dt):
    for samples, lookups in ((37, 5), (8, 26)):
        _ptrs_case(oracle, samples * lookups, D, 1, dt, samples=samples, lookups=lookups)


@pytest.mark.parametrize("D", [64, 11])
def test_ptrs_two_allocations(oracle, D):
    _ptrs_case(oracle, NB, D, 1, "f32", split=True)


@pytest.mark.parametrize("D", _grid([256, 11]))
def test_ptrs_grid(oracle, D):
    _ptrs_case(oracle, 2 * (8192 if D % 4 else 32768) + 37, D, 1, "f32")


# ---- 3. weighted pooling and its gradient --------------------------------------------------------
# u = 2^-24.  A length-n fp32 dot product summed in key order is off by at most ~n u sum|w_j row_j|
# (n roundings on the longest chain: one product, n - 1 adds); the mean adds the rounding of the
# weight sum, of the division and of the result's own representation: (n + 3) u / |denom|.
def _weighted_bound(n, abs_terms, denom):
    return (n[:, None] + 3) * U * abs_terms / np.abs(denom)[:, None]


# g = top * (w / denom): one rounding each for the quotient and the product, two for the fp32
# weight sum of the short buckets these cases use -> 4 u |ref|.
def _grad_bound(ref):
    return 4 * U * np.abs(ref)


@functools.lru_cache(maxsize=None)
def _weights(nnz):
    w = (np.random.default_rng(4000).random(nnz) + 0.1).astype(np.float32)
    w.setflags(write=False)
    return w


def _weighted_ref(ro, vi, w, tab, comb):
    """fp64: sum_j w_j row_j (/ sum_j w_j for mean; INVALID rows add 0 but their weight counts)
    -> (reference, sum_j |w_j row_j|, denominator, bucket lengths)"""
    from oracle import pyoracle
    nb, nnz = ro.size - 1, vi.size
    live = vi != pyoracle.INVALID
    rows = tab.astype(np.float64)[np.where(live, vi, 0).astype(np.int64)] * live[:, None]
    w64 = np.ones(nnz) if w is None else w.astype(np.float64)
    terms = rows * w64[:, None]
    n = np.diff(ro)
    b = np.repeat(np.arange(nb), n)
    s = np.zeros((nb, tab.shape[1]))
    sa = np.zeros_like(s)
    np.add.at(s, b, terms)
    np.add.at(sa, b, np.abs(terms))
    den = np.ones(nb)
    if comb == 1:
        den = np.zeros(nb)
        np.add.at(den, b, w64)
        den[n == 0] = 1.0
    return s / den[:, None], sa, den, n


def _weighted_case(oracle, nb, D, comb, weighted, out_mis=0, mean_len=3.0):
    from hugectr_amd import _lib
    ro_h, vi_h = _ragged(nb, V, mean_len=mean_len)
    tab_h = _table(V, D)
    w_h = _weights(vi_h.size) if weighted else None
    ro, vi, tab = _In(ro_h), _In(vi_h), _In(tab_h)
    w = _In(w_h) if weighted else None
    out = _Out(nb, D, "f32", mis=out_mis)
    _lib.check(_lib.lib.hctr_forward_pool_weighted(nb, D, comb, ro.p, vi.p, w.p if w else None,
                                                   tab.p, out.p, _lib.stream_ptr()))
    got = out.result()
    ref, sa, den, n = _weighted_ref(ro_h, vi_h, w_h, tab_h, comb)
    err, bound = np.abs(got.astype(np.float64) - ref), _weighted_bound(n, sa, den)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"weighted D={D} comb={comb} w={weighted}: max err / bound = "
              f"{np.nanmax(np.where(bound > 0, err / bound, 0.0)):.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), \
        f"weighted pooling D={D} comb={comb}: {(err > bound).sum()} elements outside the bound"
    if not weighted and comb == 0:  # multiplying by 1.0 is exact
        _assert_bits(got, oracle.forward(ro_h, vi_h, tab_h, D, 0), "weights = None, sum")
    for x, name in ((ro, "row_offset"), (vi, "value_index"), (tab, "table")):
        x.assert_unchanged(name)
    if w:
        w.assert_unchanged("weights")
    return got


def _expand_case(nb, D, comb, weighted, out_mis=0, mean_len=3.0):
    from hugectr_amd import _lib
    # the 300-key bucket only without weights (its denominator is then an exact count): the bound
    # below allows the weight sum two roundings
    ro_h, vi_h = _ragged(nb, V, mean_len=mean_len)
    if weighted:
        lens = np.diff(ro_h)
        lens = np.where(lens > 9, 9, lens)
        ro_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(ro_h[-1])
    w_h = _weights(nnz) if weighted else None
    top_h = np.random.default_rng(5000 + D).standard_normal((nb, D)).astype(np.float32)
    ro, top = _In(ro_h), _In(top_h)
    w = _In(w_h) if weighted else None
    out = _Out(nnz, D, "f32", mis=out_mis)
    _lib.check(_lib.lib.hctr_expand_key_grads(nb, D, comb, ro.p, w.p if w else None, top.p, out.p,
                                              _lib.stream_ptr()))
    got = out.result()  # NaN left in a row = a key without its gradient; writes for empty buckets
    n = np.diff(ro_h)   # would land on a neighbour's rows or on the guard rows
    b = np.repeat(np.arange(nb), n)
    w64 = np.ones(nnz) if w_h is None else w_h.astype(np.float64)
    den = np.ones(nb)
    if comb == 1:
        den = np.zeros(nb)
        np.add.at(den, b, w64)
    ref = top_h.astype(np.float64)[b] * (w64 / den[b])[:, None]
    err, bound = np.abs(got.astype(np.float64) - ref), _grad_bound(ref)
    print(f"expand D={D} comb={comb} w={weighted}: max err / (u |ref|) = "
          f"{np.max(err / (U * np.abs(ref))):.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), \
        f"key gradients D={D} comb={comb}: {(err > bound).sum()} elements outside the bound"
    if not weighted and comb == 0:  # a bit copy of the bucket's top row
        _assert_bits(got, top_h[b], "weights = None, sum")
    ro.assert_unchanged("row_offset")
    top.assert_unchanged("top_grad")
    if w:
        w.assert_unchanged("weights")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("comb", [0, 1])
@pytest.mark.parametrize("D", LPR_D + [6, 12, 70])
def test_weighted_matrix(oracle, D, comb, weighted):
    _weighted_case(oracle, 203, D, comb, weighted)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("comb", [0, 1])
@pytest.mark.parametrize("D", LPR_D + [6, 12, 70])
def test_expand_matrix(D, comb, weighted):
    _expand_case(203, D, comb, weighted)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("comb", [0, 1])
def test_weighted_expand_misaligned(oracle, comb, weighted):
    """`out` / `key_grads` 4 bytes into the allocation: the generic kernels at D = 16"""
    _weighted_case(oracle, 203, 16, comb, weighted, out_mis=1)
    _expand_case(203, 16, comb, weighted, out_mis=1)


@pytest.mark.parametrize("D", _grid([256, 6]))
def test_weighted_grid(oracle, D):
    _weighted_case(oracle, 2 * 32768 + 37, D, 1, True, mean_len=1.5)
    _weighted_case(oracle, 2 * 32768 + 37, D, 0, False, mean_len=1.5)


@pytest.mark.parametrize("D", _grid([256, 6]))
def test_expand_grid(D):
    _expand_case(2 * 32768 + 37, D, 1, True, mean_len=1.5)
    _expand_case(2 * 32768 + 37, D, 0, False, mean_len=1.5)


# ---- 3b. the sign of zero ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("comb", [0, 1])
@pytest.mark.parametrize("D", [8, 6])
def test_negative_zero_rows(oracle, D, comb, dt):
    """a table of -0.0 only, 16 buckets of 0, 1 and 3 keys, vec4 (D = 8) and generic (D = 6) path:
    the sum starts at +0.0f, so (+0.0) + (-0.0) = +0.0 is what every kernel stores (an accumulator
    that started from the first row instead would store -0.0); the oracle's bits, sign included"""
    from hugectr_amd import _lib
    nb, rows = 16, 8
    lens = np.array([0, 1, 3] * 6)[:nb]
    ro_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vi_h = (np.arange(ro_h[-1]) % rows).astype(np.uint64)
    tab_h = np.full((rows, D), -0.0, dtype=np.float32)
    assert np.signbit(tab_h).all()
    if dt == "f32":
        want = oracle.forward(ro_h, vi_h, tab_h, D, comb)
    else:
        want = oracle.forward_mixed(ro_h, vi_h, tab_h, D, comb, dt)
    ro, vi, tab = _In(ro_h), _In(vi_h), _In(tab_h)
    ptrs = _In((tab.t.data_ptr() + vi_h.astype(np.int64) * (D * 4)).astype(np.int64))
    L, s = _lib.lib, _lib.stream_ptr()
    calls = {
        "pool": lambda o: L.hctr_forward_pool(nb, D, comb, ro.p, _lib.KEY_I64, vi.p, tab.p, o.p,
                                              _code(dt), s),
        "multihot": lambda o: L.hctr_forward_pool_multihot(nb, D, comb, ro.p, _lib.KEY_I64, vi.p,
                                                           tab.p, o.p, _code(dt), s),
        "ptrs": lambda o: L.hctr_forward_pool_ptrs(nb, D, comb, ro.p, ptrs.p, o.p, _code(dt), s),
    }
    if dt == "f32":  # the weighted entry's only output type
        calls["weighted"] = lambda o: L.hctr_forward_pool_weighted(nb, D, comb, ro.p, vi.p, None,
                                                                   tab.p, o.p, s)
    for name, call in calls.items():
        out = _Out(nb, D, dt)
        _lib.check(call(out))
        _assert_bits(out.result(), want, f"-0.0 rows, {name} D={D} comb={comb} {dt}")
    for x, name in ((ro, "row_offset"), (vi, "value_index"), (tab, "table"), (ptrs, "rows")):
        x.assert_unchanged(name)


# ---- 4. reorder ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _perm(bpg, S, D, N):
    """forward: out.flat[i] = in.flat[perm[i]] -- the oracle run on an fp32 array of element
    indices (exact below 2^24)"""
    from oracle import pyoracle
    total = bpg * S * D
    assert total < 2 ** 24
    p = pyoracle.forward_reorder(np.arange(total, dtype=np.float32), bpg, S, D, N)
    p = p.reshape(-1).astype(np.int64)
    assert (np.sort(p) == np.arange(total)).all()
    p.setflags(write=False)
    return p


def _reorder(fwd, bpg, S, D, N, x, dt, mis):
    from hugectr_amd import _lib
    src = _In(x, mis=mis)
    out = _Out(bpg * S, D, dt, mis=mis, int_bits=True)
    fn = _lib.lib.hctr_forward_reorder if fwd else _lib.lib.hctr_backward_reorder
    _lib.check(fn(bpg, S, D, N, src.p, out.p, _code(dt), _lib.stream_ptr()))
    got = out.result().reshape(-1)
    src.assert_unchanged("in")
    return got


def _reorder_case(bpg, S, D, N, dt, mis=0):
    perm = _perm(bpg, S, D, N)
    idt = np.int32 if dt == "f32" else np.int16
    info = np.iinfo(idt)
    x = np.random.default_rng(bpg + S + D + N).integers(info.min, info.max, size=perm.size,
                                                        endpoint=True).astype(idt)
    y = _reorder(True, bpg, S, D, N, x, dt, mis)
    assert (y == x[perm]).all(), "forward_reorder is not the oracle's permutation"
    inv = np.empty_like(x)
    inv[perm] = x
    z = _reorder(False, bpg, S, D, N, x, dt, mis)
    assert (z == inv).all(), "backward_reorder is not the inverse permutation"
    assert (_reorder(False, bpg, S, D, N, y, dt, mis) == x).all(), "backward(forward(x)) != x"


# form: (D, dtype, elements the pointers are offset by)
REORDER_FORMS = [(128, "f32", 0), (64, "f16", 0),    # 16-byte units
                 (11, "f32", 0), (16, "f32", 1),     # fp32 scalars (odd row / 4 bytes off)
                 (6, "bf16", 0), (8, "f16", 1)]      # 16-bit scalars (12-byte row / 2 bytes off)


@pytest.mark.parametrize("D,dt,mis", REORDER_FORMS)
@pytest.mark.parametrize("S,N", [(26, 1), (26, 2), (26, 8), (7, 3), (2, 4), (5, 5)])
def test_reorder(S, N, D, dt, mis):
    _reorder_case(7, S, D, N, dt, mis)


@pytest.mark.parametrize("bpg,S,D,N,dt", _grid([(1400, 26, 128, 8, "f32"), (4000, 26, 11, 3, "f32"),
                                                (4000, 26, 11, 8, "bf16")]))
def test_reorder_grid(bpg, S, D, N, dt):
    """more than 2 x 524288 units (float4 / float / 16-bit) -> three passes of the grid"""
    units = bpg * S * (D * (4 if dt == "f32" else 2) // 16 if D % 8 == 0 else D)
    assert units > 2 * 2048 * 256
    _reorder_case(bpg, S, D, N, dt)


# ---- 5. wgrad_kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_wgrad_grid(oracle, dt):
    """B * S * D = 1 126 400 elements (one pass of wgrad_kernel covers 524 288), mean, ragged.
    fp16 found wgrad_kernel returning +0.0 for a gradient of -0.0 in a bucket of n > 1 keys (one
    element of this input underflows to -0.0 in fp16; more are planted)"""
    import torch
    import hugectr_amd as ha
    from hugectr_amd import _lib
    from util import make_csr
    B, S, D, hot, vps = (11 if EMU else 1100), 8, 128, 4, 50
    rng = np.random.default_rng(6000)
    opt = ha.OptParams(optimizer=_lib.OPT_SGD, lr=0.1, atomic_update=False)
    emb = ha.SparseEmbeddingHash(_lib.EMB_LOCALIZED, B, 0, S * vps, D, S * hot, S, 1, opt,
                                 out_dtype=_torch_dtype(dt))
    emb.init_params()
    ro, keys = make_csr(rng, B, S, hot, vps, empty_frac=0.3)
    emb.forward(True, torch.from_numpy(ro).to("cuda"), torch.from_numpy(keys).to("cuda"))
    g = (rng.standard_normal((B * S, D)) * 3).astype(np.float32)
    g[::7, 3] = -0.0  # -0.0 * (1 / n) is -0.0: a multiply fused into fma(g, sc, +0) returns +0.0
    top = torch.from_numpy(g).to("cuda").to(_torch_dtype(dt)).view(B, S, D).contiguous()
    keep = top.clone()
    emb.backward(top)
    got = emb.get_wgrad().float().cpu().numpy().reshape(-1, D)
    want = oracle.backward(ro, g, D, 1) if dt == "f32" else oracle.backward_mixed(ro, g, D, 1, dt)
    _assert_bits(got, want, f"wgrad {dt}")
    assert torch.equal(top, keep), "backward changed the top gradient"
