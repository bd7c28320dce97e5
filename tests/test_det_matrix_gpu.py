"""GPU parity matrix of the dynamic embedding table (csrc/det.hip) against oracle/det_oracle.py:
every kernel's dispatch branch, the second trip of every grid-stride loop, every verb, the remove
sequences (keys equal to the former erasure marks among them) and both launch forms of the
optimizer step.  Public ABI only.

Lookups, scatters and removes are compared bit-exact.  The optimizer steps are compared with an
fp64 evaluation of the oracle's formulas: with E = max |oracle32 - oracle64| over the tensor, the
kernel must satisfy |gpu - oracle64| <= 4 E + ulp32(|oracle64|) elementwise (4: FMA contraction and
the fused `w += delta`, which the fp32 oracle does not have; one ulp: where the fp32 oracle happens
to be exact).  Every optimizer case prints E and the measured error."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KB = [8, 4]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kd(torch, kb):
    return torch.int64 if kb == 8 else torch.uint32


def _keys(torch, k, kb):
    k = np.asarray(k)
    if kb == 8:
        return _dev(torch, k.astype(np.int64))
    return _dev(torch, k.astype(np.uint32).view(np.int32))


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64).tolist()


def _index(t, c, keys_t, insert=0):
    """hctr_det_lookup_index: rows inside class c (-1: no row)"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    out = torch.empty(keys_t.numel(), dtype=torch.int64, device="cuda")
    check(lib.hctr_det_lookup_index(t._h, c, ptr(keys_t), keys_t.numel(), insert, ptr(out),
                                    stream_ptr()))
    return out.cpu().numpy()


def _rows_addr(t, c):
    from hugectr_amd._lib import check, lib
    p, cap = ctypes.c_void_p(), ctypes.c_size_t()
    check(lib.hctr_det_rows(t._h, c, ctypes.byref(p), ctypes.byref(cap)))
    return int(p.value)


def _export(t, c, kb):
    """(keys ascending as int64, vectors in that order) of class c"""
    k, v = t.export(c)
    k = k.cpu().numpy()
    k = k.astype(np.int64) if kb == 8 else k.view(np.uint32).astype(np.int64)
    v = v.cpu().numpy()
    order = np.argsort(k, kind="stable")
    return k[order], v[order]


def _oracle_export(o, c):
    ks = np.array(sorted(o.maps[c]), dtype=np.int64)
    vs = (np.stack([o.maps[c][int(k)] for k in ks]) if ks.size
          else np.zeros((0, o.dims[c]), dtype=o.dt))
    return ks, vs


def _same_as_oracle(t, o, kb, what):
    """sizes and, per class, export == the oracle's map (bit-exact, every key once)"""
    sizes = o.size_per_class()
    assert t.size_per_class() == sizes, what
    for c, n in enumerate(sizes):
        if n == 0:
            continue
        k, v = _export(t, c, kb)
        ok, ov = _oracle_export(o, c)
        assert np.array_equal(k, ok), f"{what}: exported keys of class {c}"
        assert np.array_equal(v.view(np.uint32), ov.view(np.uint32)), f"{what}: class {c} vectors"


# ================================ gather / lookup dispatch ========================================
@pytest.mark.parametrize("kb", KB)
def test_packed_lookup_takes_float4_scalar_by_dim_and_scalar_by_alignment(kb):
    """classes [8, 6, 8, 127] in one packed lookup; the dim-6 class has an odd key count, so the
    second dim-8 class writes to an `out` that is 8 but not 16 bytes aligned"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    from oracle.det_oracle import DetOracle
    rng = np.random.default_rng(11 + kb)
    dims, counts = [8, 6, 8, 127], [5, 3, 7, 4]
    sp, so = [0, 1, 2, 3], _offsets(counts)
    assert (counts[0] * dims[0] + counts[1] * dims[1]) * 4 % 16 == 8
    t = DynamicEmbeddingTable(dims, "0.25", initial_capacity=16, key_dtype=_kd(torch, kb))
    o = DetOracle(dims, 0.25)
    keys = rng.choice(2**31 - 1, size=sum(counts), replace=False).astype(np.int64)
    kt = _keys(torch, keys, kb)
    first = t.lookup(kt, sp, so)
    assert first.data_ptr() % 16 == 0
    assert np.array_equal(first.cpu().numpy(), o.lookup(keys, sp, so))
    # distinct values per key and element: a wrong row or column shows
    upd = (np.arange(first.numel(), dtype=np.float32) + 0.5)
    t.scatter_update(kt, _dev(torch, upd), sp, so)
    o.scatter(keys, upd, sp, so, add=False)
    # the same keys in another order per class, with one key twice
    perm = np.concatenate([so[i] + rng.permutation(counts[i]) for i in range(4)])
    k2 = keys[perm]
    k2[so[2] + 1] = k2[so[2]]
    got = t.lookup(_keys(torch, k2, kb), sp, so)
    assert got.data_ptr() % 16 == 0
    assert np.array_equal(got.cpu().numpy(), o.lookup(k2, sp, so))
    assert t.size_per_class() == o.size_per_class() == counts
    # find-only: keys that miss give row -1 and a null address, hits the address of their row
    k3 = k2.copy()
    missing = [so[0] + 2, so[1], so[2] + 6, so[3] + 3]
    k3[missing] = np.arange(1, 5) + 2**31 - 10
    ptrs, rows, base = t.lookup_rows(_keys(torch, k3, kb), sp, so, insert=False)
    ptrs, rows = ptrs.cpu().numpy(), rows.cpu().numpy()
    hit = np.ones(k3.size, dtype=bool)
    hit[missing] = False
    assert (rows[~hit] == -1).all() and (ptrs[~hit] == 0).all()
    assert t.size_per_class() == counts
    for c in range(4):
        sl = slice(so[c], so[c + 1])
        inside = _index(t, c, _keys(torch, k3[sl], kb))
        assert np.array_equal(inside >= 0, hit[sl])
        want_rows = np.where(hit[sl], base[c] + inside, -1)
        want_ptrs = np.where(hit[sl], _rows_addr(t, c) + 4 * dims[c] * inside, 0)
        assert np.array_equal(rows[sl], want_rows) and np.array_equal(ptrs[sl], want_ptrs)


@pytest.mark.parametrize("kb", KB)
@pytest.mark.parametrize("dim,n", [(128, 70000), (127, 17000)])
def test_lookup_and_scatter_update_beyond_the_grid_caps(dim, n, kb):
    """dim 128 x 70 000: the float4 gather's loop takes a second trip (8192 blocks of 256); dim 127
    x 17 000: so do the scalar gather (8192), scatter_update (4096) and the row initialiser (2048)"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    assert n * (dim // 4 if dim % 4 == 0 else dim) > 8192 * 256
    t = DynamicEmbeddingTable([dim], "0.25", initial_capacity=1024, key_dtype=_kd(torch, kb))
    keys = np.arange(n, dtype=np.int64) * 5 + 3
    kt = _keys(torch, keys, kb)
    first = t.lookup(kt)
    assert bool((first == 0.25).all()), "a new row was not initialised"
    assert np.array_equal(_index(t, 0, kt), np.arange(n)), "rows are the first positions"
    vals = np.arange(n * dim, dtype=np.float32).reshape(n, dim)  # (< 2^24: exact and distinct)
    t.scatter_update(kt, _dev(torch, vals.reshape(-1)))
    perm = np.random.default_rng(dim).permutation(n)
    got = t.lookup(_keys(torch, keys[perm], kb)).cpu().numpy().reshape(n, dim)
    assert np.array_equal(got, vals[perm])
    assert t.size_per_class() == [n]


@pytest.mark.parametrize("kb", KB)
def test_multi_class_find_and_row_pass_beyond_the_grid_cap(kb):
    """THE SLOW CASE of this file: 2 200 000 distinct keys (> 8192 x 256) of dim 4 over three
    classes through det_find_multi_kernel / det_rows_multi_kernel, inserting once, then find-only"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    counts = [700000, 800001, 699999]
    n = sum(counts)
    assert n > 8192 * 256
    sp, so = [0, 1, 2], _offsets(counts)
    t = DynamicEmbeddingTable([4, 4, 4], "0.5", initial_capacity=1 << 20, key_dtype=_kd(torch, kb))
    keys = np.arange(n, dtype=np.int64) * 7 + 3
    kt = _keys(torch, keys, kb)
    pos = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
    store, _ = t.row_store()
    ptrs, rows, base = t.lookup_rows(kt, sp, so, insert=True)
    want = np.repeat(np.asarray(base[:3], dtype=np.int64), counts) + pos
    assert np.array_equal(rows.cpu().numpy(), want), "insert: base[class] + position in class"
    assert np.array_equal(ptrs.cpu().numpy(), store + 16 * want)
    assert t.size_per_class() == counts
    ptrs, rows, base2 = t.lookup_rows(kt, sp, so, insert=False)  # (the address / row pass)
    assert base2 == base and np.array_equal(rows.cpu().numpy(), want)
    assert np.array_equal(ptrs.cpu().numpy(), store + 16 * want)
    _, rows, _ = t.lookup_rows(kt, sp, so, insert=False, want_ptrs=False)  # (the probe's own rows)
    assert np.array_equal(rows.cpu().numpy(), want)
    assert t.row_store()[0] == store


@pytest.mark.parametrize("kb", KB)
@pytest.mark.parametrize("verb", ["lookup", "lookup_rows"])
def test_a_class_that_owns_two_ranges_of_one_call(verb, kb):
    """id_spaces [0, 1, 0]: a key unseen in both ranges of class 0 gets ONE row, returned at both"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    from oracle.det_oracle import DetOracle
    dims = [8, 8]
    sp, so = [0, 1, 0], [0, 6, 11, 18]
    keys = np.array([10, 11, 12, 13, 14, 15,   20, 21, 10, 11, 22,   16, 13, 17, 18, 16, 10, 19],
                    dtype=np.int64) * 1000003
    t = DynamicEmbeddingTable(dims, "0.25", initial_capacity=16, key_dtype=_kd(torch, kb))
    o = DetOracle(dims, 0.25)
    kt = _keys(torch, keys, kb)
    if verb == "lookup":
        assert np.array_equal(t.lookup(kt, sp, so).cpu().numpy(), o.lookup(keys, sp, so))
    else:
        o.lookup(keys, sp, so)
        t.lookup_rows(kt, sp, so, insert=True)
    assert t.size_per_class() == o.size_per_class() == [10, 5]
    # rows = first occurrences in the order of the call, class by class
    order = [{}, {}]
    for i, c in enumerate(sp):
        for k in keys[so[i]:so[i + 1]]:
            order[c].setdefault(int(k), len(order[c]))
    ptrs, rows, base = t.lookup_rows(kt, sp, so, insert=False)
    want = np.concatenate([[base[c] + order[c][int(k)] for k in keys[so[i]:so[i + 1]]]
                           for i, c in enumerate(sp)])
    assert np.array_equal(rows.cpu().numpy(), want)
    assert np.array_equal(ptrs.cpu().numpy(), t.row_store()[0] + 32 * want)
    # distinct values, read back through both ranges
    upd = np.arange(keys.size * 8, dtype=np.float32)
    t.scatter_update(kt, _dev(torch, upd), sp, so)
    o.scatter(keys, upd, sp, so, add=False)
    assert np.array_equal(t.lookup(kt, sp, so).cpu().numpy(), o.lookup(keys, sp, so))
    _same_as_oracle(t, o, kb, "two ranges of one class")


@pytest.mark.parametrize("kb", KB)
def test_lookup_unsafe_addresses_stay_valid_when_another_class_grows(kb):
    import torch
    from hugectr_amd import _lib
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    rng = np.random.default_rng(kb)
    dims, counts = [8, 6], [13, 9]
    sp, so = [0, 1], _offsets(counts)
    t = DynamicEmbeddingTable(dims, "0.25", initial_capacity=16, key_dtype=_kd(torch, kb))
    keys = rng.choice(2**31 - 1, size=sum(counts), replace=False).astype(np.int64)
    keys[3] = keys[0]  # (a key twice: one row, one address)
    kt = _keys(torch, keys, kb)
    ptrs = t.lookup_unsafe(kt, sp, so).cpu().numpy()

    def expected():
        return np.concatenate([_rows_addr(t, c) + 4 * dims[c] *
                               _index(t, c, _keys(torch, keys[so[c]:so[c + 1]], kb))
                               for c in range(2)])
    assert np.array_equal(ptrs, expected())
    assert t.size_per_class() == [12, 9]
    upd = np.arange(counts[0] * 8 + counts[1] * 6, dtype=np.float32) + 1
    upd[3 * 8:4 * 8] = upd[:8]
    t.scatter_update(kt, _dev(torch, upd), sp, so)
    addr0 = _rows_addr(t, 0)
    # class 1 grows 16 -> 1024
    more = rng.choice(2**31 - 1, size=600, replace=False).astype(np.int64) + 2**31
    if kb == 4:
        more = more - 2**30
    t.lookup(_keys(torch, more, kb), [1], [0, more.size])
    assert t.capacity_per_class()[0] == 16 and t.capacity_per_class()[1] > 16
    assert _rows_addr(t, 0) == addr0
    assert np.array_equal(t.lookup_unsafe(kt, sp, so).cpu().numpy(), ptrs)
    assert np.array_equal(ptrs, expected())
    assert np.array_equal(t.lookup(kt, sp, so).cpu().numpy(), upd)
    # what lies at the addresses of class 0 (the library's own gather on the class's rows)
    r0 = _dev(torch, (ptrs[:counts[0]] - addr0) // 32)
    out = torch.empty((counts[0], 8), dtype=torch.float32, device="cuda")
    seg = torch.arange(counts[0] + 1, dtype=torch.int64, device="cuda")
    check(lib.hctr_forward_pool(counts[0], 8, 0, ptr(seg), _lib.KEY_I64, ptr(r0), addr0, ptr(out),
                                _lib.F32, stream_ptr()))
    assert np.array_equal(out.cpu().numpy().reshape(-1), upd[:counts[0] * 8])


def test_random_initializer_does_not_depend_on_how_the_keys_are_batched():
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 2**40, size=1200, dtype=np.int64)[rng.integers(0, 1200, size=3000)]
    a = DynamicEmbeddingTable([12], "", initial_capacity=64, seed=9)
    b = DynamicEmbeddingTable([12], "", initial_capacity=64, seed=9)
    one = a.lookup(_dev(torch, keys)).cpu().numpy()
    three = np.concatenate([b.lookup(_dev(torch, keys[i:i + 1000])).cpu().numpy()
                            for i in (0, 1000, 2000)])
    assert np.array_equal(one, three)
    assert a.size_per_class() == b.size_per_class() == [np.unique(keys).size]
    assert one.min() > 0.0 and one.max() <= 1.0


# ====================================== scatter_add ================================================
@pytest.mark.parametrize("kb", KB)
def test_scatter_add_with_heavy_duplication_is_exact(kb):
    """40 distinct keys in 12 000 positions (two classes); integer-valued updates in [-4, 4] keep
    every partial sum exact in fp32, so any order of the atomic adds gives the oracle's bits.  A
    third of the keys is unknown to the table and some were removed: both are skipped."""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    from oracle.det_oracle import DetOracle
    rng = np.random.default_rng(40 + kb)
    dims = [6, 8]
    t = DynamicEmbeddingTable(dims, "0.5", initial_capacity=16, key_dtype=_kd(torch, kb))
    o = DetOracle(dims, 0.5)
    sp = [0, 1]
    distinct = rng.choice(2**31 - 1, size=40, replace=False).astype(np.int64)
    d0, d1 = distinct[:20], distinct[20:]
    known = np.concatenate([d0[:13], d1[:13]])  # 14 of the 40 stay unknown
    t.lookup(_keys(torch, known, kb), sp, [0, 13, 26])
    o.lookup(known, sp, [0, 13, 26])
    gone = np.concatenate([d0[:3], d1[:2]])
    t.remove(_keys(torch, gone, kb), sp, [0, 3, 5])
    o.remove(gone, sp, [0, 3, 5])
    keys = np.concatenate([d0[rng.integers(0, 20, size=6000)], d1[rng.integers(0, 20, size=6000)]])
    so = [0, 6000, 12000]
    upd = rng.integers(-4, 5, size=6000 * 6 + 6000 * 8).astype(np.float32)
    t.scatter_add(_keys(torch, keys, kb), _dev(torch, upd), sp, so)
    o.scatter(keys, upd, sp, so, add=True)
    assert o.size_per_class() == [10, 11]
    _same_as_oracle(t, o, kb, "scatter_add with duplicates")
    got = t.lookup(_keys(torch, known, kb), sp, [0, 13, 26]).cpu().numpy()
    assert np.array_equal(got, o.lookup(known, sp, [0, 13, 26]))


# ========================================= remove ==================================================
@pytest.mark.parametrize("kb", KB)
def test_remove_lookup_cycles_with_growth_while_keys_are_erased(kb):
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    from oracle.det_oracle import DetOracle
    rng = np.random.default_rng(70 + kb)
    t = DynamicEmbeddingTable([8], "0.25", initial_capacity=16, key_dtype=_kd(torch, kb))
    o = DetOracle([8], 0.25)
    pool = rng.choice(2**31 - 1, size=400, replace=False).astype(np.int64)
    serial = [0]

    def lookup(k):
        got = t.lookup(_keys(torch, k, kb)).cpu().numpy()
        assert np.array_equal(got, o.lookup(k, [0], [0, k.size]))

    def mark(k):  # distinct values: a vector that moved or was re-initialised shows
        upd = (np.arange(k.size * 8, dtype=np.float32) + serial[0]) * 0.5
        serial[0] += k.size * 8
        t.scatter_update(_keys(torch, k, kb), _dev(torch, upd))
        o.scatter(k, upd, [0], [0, k.size], add=False)

    def remove(k):
        t.remove(_keys(torch, k, kb))
        o.remove(k, [0], [0, k.size])

    live, fresh = pool[:12], 12
    lookup(live)
    mark(live)
    victims = np.concatenate([live[:8], live[:3], pool[-5:]])  # duplicates and unknown keys
    for rnd in range(3):
        remove(victims)
        _same_as_oracle(t, o, kb, f"round {rnd}: removed")
        cap = t.capacity_per_class()[0]
        grow = pool[fresh:fresh + 20 * 2**rnd]  # the class grows while the erased entries are there
        fresh += grow.size
        lookup(grow)
        assert t.capacity_per_class()[0] > cap
        _same_as_oracle(t, o, kb, f"round {rnd}: grown")
        lookup(live)  # the erased keys come back with the initial value, the others keep theirs
        _same_as_oracle(t, o, kb, f"round {rnd}: looked up again")
        mark(live[:8])
        remove(live[:8])
        lookup(live[:8])
        mark(live[2:10])
        _same_as_oracle(t, o, kb, f"round {rnd}: removed and looked up twice")


@pytest.mark.parametrize("kb", KB)
def test_remove_batch_beyond_the_grid_cap_with_racing_duplicates(kb):
    """600 000 positions (> 2048 x 256) in which 5 000 live and 1 000 unknown keys repeat"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    rng = np.random.default_rng(600 + kb)
    n_live, n_rm = 8000, 5000
    t = DynamicEmbeddingTable([4], "0.25", initial_capacity=1024, key_dtype=_kd(torch, kb))
    live = np.arange(n_live, dtype=np.int64) * 11 + 5
    vals = np.arange(n_live * 4, dtype=np.float32).reshape(n_live, 4)
    t.lookup(_keys(torch, live, kb))
    t.scatter_update(_keys(torch, live, kb), _dev(torch, vals.reshape(-1)))
    gone = rng.permutation(n_live)[:n_rm]
    cand = np.concatenate([live[gone], np.arange(1000, dtype=np.int64) * 11 + 6])
    batch = np.concatenate([cand, cand[rng.integers(0, cand.size, size=600000 - cand.size)]])
    batch = batch[rng.permutation(batch.size)]
    assert batch.size == 600000 > 2048 * 256
    t.remove(_keys(torch, batch, kb))
    assert t.size_per_class() == [n_live - n_rm]
    keep = np.setdiff1d(np.arange(n_live), gone)
    k, v = _export(t, 0, kb)
    assert np.array_equal(k, live[keep]) and np.array_equal(v, vals[keep])
    assert (_index(t, 0, _keys(torch, live[gone], kb)) == -1).all()
    # removed again: nothing left to erase
    t.remove(_keys(torch, batch[:300000], kb))
    assert t.size_per_class() == [n_live - n_rm]


@pytest.mark.parametrize("kb", KB)
def test_a_key_equal_to_the_former_erasure_mark_is_an_ordinary_key(kb, oracle):
    """0xFFFFFFFE (32-bit) / INT64_MAX - 1 (64-bit) were what remove() once wrote over an erased
    slot's key: a lookup of that key then matched the first erased slot on its probe chain and the
    key was re-initialised.  Neighbours that sit earlier on its chain are removed; its vector, the
    sizes and the export must not change."""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable
    from oracle.det_oracle import DetOracle
    T = 0xFFFFFFFE if kb == 4 else 2**63 - 2
    cap = 64
    size = int(np.float32(cap) / np.float32(0.75))  # slots of the class's index
    home = int(oracle.hash_keys([T], kb)[0]) % size
    cand = np.arange(1, 4000, dtype=np.int64) * 7919
    slot = oracle.hash_keys(cand, kb).astype(np.int64) % size
    back = (home - slot) % size  # how far in front of T's home slot a key's home slot lies
    chain = np.concatenate([cand[back == b][:2] for b in (0, 1, 2)])  # fills home .. and pushes T on
    assert chain.size == 6
    rest = cand[back > 12][:33]
    t = DynamicEmbeddingTable([8], "0.25", initial_capacity=cap, key_dtype=_kd(torch, kb))
    o = DetOracle([8], 0.25)

    def both(fn_t, fn_o):
        fn_t()
        fn_o()
        _same_as_oracle(t, o, kb, "former erasure mark as a key")

    first = np.concatenate([chain, rest])
    both(lambda: t.lookup(_keys(torch, first, kb)), lambda: o.lookup(first, [0], [0, first.size]))
    kT = np.array([T], dtype=np.int64)
    both(lambda: t.lookup(_keys(torch, kT, kb)), lambda: o.lookup(kT, [0], [0, 1]))
    assert t.capacity_per_class() == [cap] and t.size_per_class() == [40]
    marker = np.arange(8, dtype=np.float32) + 1000
    both(lambda: t.scatter_update(_keys(torch, kT, kb), _dev(torch, marker)),
         lambda: o.scatter(kT, marker, [0], [0, 1], add=False))
    both(lambda: t.remove(_keys(torch, chain, kb)), lambda: o.remove(chain, [0], [0, chain.size]))
    assert t.size_per_class() == [34]
    assert _index(t, 0, _keys(torch, kT, kb))[0] >= 0, "the key lost its row to an erased neighbour"
    got = t.lookup(_keys(torch, kT, kb)).cpu().numpy()
    assert np.array_equal(got, marker), "the marker vector did not come back"
    _same_as_oracle(t, o, kb, "after the lookup")
    # the key itself can be removed and come back, its neighbours too
    both(lambda: t.remove(_keys(torch, kT, kb)), lambda: o.remove(kT, [0], [0, 1]))
    again = np.concatenate([chain[:3], kT])
    both(lambda: t.lookup(_keys(torch, again, kb)), lambda: o.lookup(again, [0], [0, again.size]))
    assert t.size_per_class() == [37]


# ==================================== optimizer step ===============================================
HYP = dict(lr=0.05, scaler=2.0, beta1=0.9, beta2=0.999, epsilon=1e-6, momentum_factor=0.8,
           rmsprop_beta=0.95, ftrl_lambda1=0.01, ftrl_lambda2=0.02, ftrl_beta=0.5)
OPTS = ["sgd", "momentum", "nesterov", "adagrad", "rmsprop", "adam", "ftrl"]
FORMS = {"tiled012": ([8, 8, 8], [0, 1, 2]), "tiled020": ([8, 8, 8], [0, 2, 0]),
         "loop": ([16, 6], [0, 1])}


def _codes(name):
    from hugectr_amd import _lib
    from oracle import det_oracle as D
    return {"sgd": (_lib.OPT_SGD, D.SGD), "momentum": (_lib.OPT_MOMENTUM_SGD, D.MOMENTUM),
            "nesterov": (_lib.OPT_NESTEROV, D.NESTEROV), "adagrad": (_lib.OPT_ADAGRAD, D.ADAGRAD),
            "rmsprop": (_lib.OPT_RMSPROP, D.RMSPROP), "adam": (_lib.OPT_ADAM, D.ADAM),
            "ftrl": (_lib.OPT_FTRL, D.FTRL)}[name]


def _num_state(name):
    return {"sgd": 0, "adam": 2, "ftrl": 2}.get(name, 1)


def _oracle_update(ow, os_, code, keys, sp, so, ev, wg, times):
    from oracle import det_oracle as D
    D.update(ow, os_, code, keys, sp, so, ev, wg, lr=HYP["lr"], scaler=HYP["scaler"],
             beta1=HYP["beta1"], beta2=HYP["beta2"], eps=HYP["epsilon"],
             momentum=HYP["momentum_factor"], rms_beta=HYP["rmsprop_beta"],
             lambda1=HYP["ftrl_lambda1"], lambda2=HYP["ftrl_lambda2"], ftrl_beta=HYP["ftrl_beta"],
             times=times)


def _gapped_permuted_starts(rng, lens, gap=3):
    """ev_start_indices with `gap` unused elements after every key's gradient, the keys' gradients
    laid out in a random order (not ascending); the unused elements are NaN"""
    order = rng.permutation(lens.size)
    start = np.zeros(lens.size, dtype=np.int64)
    start[order] = np.concatenate([[0], np.cumsum(lens[order] + gap)[:-1]])
    total = int((lens + gap).sum())
    wg = np.full(total, np.nan, dtype=np.float32)
    for s, n in zip(start, lens):
        wg[s:s + n] = rng.standard_normal(n).astype(np.float32)
    return start.astype(np.int32), wg


def _within_oracle_error(what, got, o32, o64):
    """|gpu - oracle64| <= 4 E + ulp32(|oracle64|), E = max |oracle32 - oracle64| (module docstring)"""
    assert got.shape == o32.shape == o64.shape and o64.dtype == np.float64
    E = float(np.max(np.abs(o32.astype(np.float64) - o64))) if o64.size else 0.0
    err = np.abs(got.astype(np.float64) - o64)
    tol = 4.0 * E + np.spacing(np.abs(o64).astype(np.float32)).astype(np.float64)
    worst = float(err.max()) if err.size else 0.0
    print(f"[det-matrix] {what}: E = {E:.3e}  gpu error = {worst:.3e}")
    bad = ~(err <= tol)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements outside 4 E + ulp, "
                           f"E = {E:.3e}, worst error {worst:.3e}")
    return E, worst


def _compare_tables(what, t, o32, o64, kb):
    """sizes and keys exactly, vectors within the oracle's own error; all classes as one tensor"""
    assert t.size_per_class() == o32.size_per_class() == o64.size_per_class(), what
    g, a, b = [], [], []
    for c, n in enumerate(o32.size_per_class()):
        if n == 0:
            continue
        k, v = _export(t, c, kb)
        k32, v32 = _oracle_export(o32, c)
        k64, v64 = _oracle_export(o64, c)
        assert np.array_equal(k, k32) and np.array_equal(k, k64), f"{what}: keys of class {c}"
        g.append(v.reshape(-1)), a.append(v32.reshape(-1)), b.append(v64.reshape(-1))
    return _within_oracle_error(what, np.concatenate(g), np.concatenate(a), np.concatenate(b))


@pytest.mark.parametrize("kb", KB)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", OPTS)
def test_update_matches_the_oracle_in_both_launch_forms(name, form, kb):
    """three steps; weights and state start at 16 rows per class and grow between and inside the
    steps; ev_start_indices has gaps and is not ascending; the last two keys of every range are
    unknown to the weights at their step (skipped with their state created; inserted by Ftrl)"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable, DynamicTableOptimizer
    from oracle.det_oracle import DetOracle
    code = _codes(name)
    ns = _num_state(name)
    dims, sp = FORMS[form]
    rng = np.random.default_rng(OPTS.index(name) * 16 + list(FORMS).index(form) * 2 + kb // 8)
    t = DynamicEmbeddingTable(dims, "0.5", initial_capacity=16, key_dtype=_kd(torch, kb))
    opt = DynamicTableOptimizer(t, code[0], initial_capacity=16, **HYP)
    sdims = [d * max(ns, 1) for d in dims]
    ow = [DetOracle(dims, 0.5), DetOracle(dims, 0.5, dtype=np.float64)]
    os_ = [DetOracle(sdims, 0.0), DetOracle(sdims, 0.0, dtype=np.float64)]
    hi = 2**40 if kb == 8 else 2**32 - 1
    pools = [rng.choice(hi, size=90, replace=False).astype(np.int64) for _ in dims]
    for step in range(3):
        per = 10 + 4 * step
        drawn = {c: rng.permutation(pools[c])[:per * sp.count(c)] for c in set(sp)}
        taken = {c: 0 for c in set(sp)}
        parts = []
        for c in sp:
            parts.append(drawn[c][taken[c]:taken[c] + per])
            taken[c] += per
        keys = np.concatenate(parts)
        so = _offsets([per] * len(sp))
        seen = np.concatenate([p[:-2] for p in parts])
        so_seen = _offsets([per - 2] * len(sp))
        t.lookup(_keys(torch, seen, kb), sp, so_seen)  # (forward of the step)
        for o in ow:
            o.lookup(seen, sp, so_seen)
        lens = np.repeat([dims[c] for c in sp], per)
        ev, wg = _gapped_permuted_starts(rng, lens)
        assert (np.diff(ev) < 0).any()
        opt.update(_keys(torch, keys, kb), _dev(torch, ev), _dev(torch, wg), sp, so)
        for w, s in zip(ow, os_):
            _oracle_update(w, s, code[1], keys, sp, so, ev, wg, step + 1)
        tag = f"{name} {form} u{kb * 8} step {step}"
        _compare_tables(tag + " weights", t, ow[0], ow[1], kb)
        if ns:
            _compare_tables(tag + " state", opt.states, os_[0], os_[1], kb)
    assert max(t.capacity_per_class()) > 16
    if ns:
        assert max(opt.states.capacity_per_class()) > 16


_BIG = {}


def _big_adagrad_reference():
    """one AdaGrad step on 17 000 keys of dim 127 (both launch forms share it): fp32 and fp64"""
    if not _BIG:
        from oracle.det_oracle import DetOracle
        n, dim = 17000, 127
        rng = np.random.default_rng(127)
        keys = np.arange(n, dtype=np.int64) * 3 + 1
        ev, wg = _gapped_permuted_starts(rng, np.full(n, dim, dtype=np.int64), gap=1)
        res = []
        for dt in (np.float32, np.float64):
            w, s = DetOracle([dim], 0.5, dtype=dt), DetOracle([dim], 0.0, dtype=dt)
            w.lookup(keys[:-5], [0], [0, n - 5])
            _oracle_update(w, s, _codes("adagrad")[1], keys, [0], [0, n], ev, wg, 1)
            res.append((_oracle_export(w, 0), _oracle_export(s, 0)))
        _BIG.update(keys=keys, ev=ev, wg=wg, w32=res[0][0], s32=res[0][1], w64=res[1][0],
                    s64=res[1][1])
    return _BIG


@pytest.mark.parametrize("form", ["tiled", "loop"])
def test_adagrad_step_beyond_the_grid_caps(form):
    """17 000 keys x dim 127 > 8192 x 256 elements: second trip of det_update_ptr_kernel (two
    classes of one dimension in one call) and of det_update_kernel (one class, cap 4096)"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable, DynamicTableOptimizer
    ref = _big_adagrad_reference()
    keys, n, dim = ref["keys"], ref["keys"].size, 127
    assert n * dim > 8192 * 256
    dims, sp, so = ([dim, dim], [0, 1], [0, n // 2, n]) if form == "tiled" else ([dim], [0], [0, n])
    t = DynamicEmbeddingTable(dims, "0.5", initial_capacity=1024)
    opt = DynamicTableOptimizer(t, _codes("adagrad")[0], initial_capacity=1024, **HYP)
    so_seen = so[:-1] + [n - 5]  # the last five keys are unknown to the weights
    t.lookup(_dev(torch, keys[:-5]), sp, so_seen)
    opt.update(_dev(torch, keys), _dev(torch, ref["ev"]), _dev(torch, ref["wg"]), sp, so)

    def whole(tab):  # the classes hold disjoint keys: one key-ordered tensor
        ks, vs = zip(*[_export(tab, c, 8) for c in range(len(dims))])
        ks, vs = np.concatenate(ks), np.concatenate(vs)
        order = np.argsort(ks, kind="stable")
        return ks[order], vs[order]
    for what, tab, r32, r64 in (("weights", t, ref["w32"], ref["w64"]),
                                ("state", opt.states, ref["s32"], ref["s64"])):
        k, v = whole(tab)
        assert np.array_equal(k, r32[0]) and np.array_equal(k, r64[0])
        _within_oracle_error(f"adagrad 17000x127 {form} {what}", v, r32[1], r64[1])
    assert t.size() == n - 5 and opt.states.size() == n


@pytest.mark.parametrize("kb", KB)
@pytest.mark.parametrize("name", OPTS)
def test_tiled_and_per_class_launches_give_the_same_bits(name, kb):
    """the same keys and gradients through dims [8, 8, 8] as three id spaces of one call (one
    launch over row addresses) and class by class (one launch per class over row numbers).  Class
    by class = three one-space calls; for Adam, whose step counter advances per call, one call
    whose ranges leave key 0 unowned, which the tiled form does not take either."""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable, DynamicTableOptimizer
    code = _codes(name)
    ns = _num_state(name)
    dims, sp = [8, 8, 8], [0, 1, 2]
    rng = np.random.default_rng(900 + OPTS.index(name) * 2 + kb // 8)
    tabs = [DynamicEmbeddingTable(dims, "0.5", initial_capacity=16, key_dtype=_kd(torch, kb))
            for _ in range(2)]
    opts = [DynamicTableOptimizer(t, code[0], initial_capacity=16, **HYP) for t in tabs]
    pools = [rng.choice(2**31 - 1, size=80, replace=False).astype(np.int64) for _ in dims]
    for step in range(3):
        counts = [int(rng.integers(9, 30)) for _ in dims]
        parts = [rng.permutation(pools[c])[:counts[c]] for c in sp]
        keys, so = np.concatenate(parts), _offsets(counts)
        seen, so_seen = np.concatenate([p[:-2] for p in parts]), _offsets([c - 2 for c in counts])
        ev, wg = _gapped_permuted_starts(rng, np.full(keys.size, 8, dtype=np.int64))
        for t in tabs:
            t.lookup(_keys(torch, seen, kb), sp, so_seen)
        opts[0].update(_keys(torch, keys, kb), _dev(torch, ev), _dev(torch, wg), sp, so)
        if name == "adam":
            k1 = np.concatenate([[12345], keys])
            e1 = np.concatenate([[0], ev]).astype(np.int32)
            opts[1].update(_keys(torch, k1, kb), _dev(torch, e1), _dev(torch, wg), sp,
                           [x + 1 for x in so])
        else:
            for c in sp:
                sl = slice(so[c], so[c + 1])
                opts[1].update(_keys(torch, keys[sl], kb), _dev(torch, ev[sl]), _dev(torch, wg),
                               [c], [0, counts[c]])
        for pair in ([tabs] + ([[o.states for o in opts]] if ns else [])):
            assert pair[0].size_per_class() == pair[1].size_per_class()
            for c in sp:
                ka, va = _export(pair[0], c, kb)
                kb_, vb = _export(pair[1], c, kb)
                assert np.array_equal(ka, kb_)
                assert np.array_equal(va.view(np.uint32), vb.view(np.uint32)), (name, step, c)


@pytest.mark.parametrize("kb", KB)
@pytest.mark.parametrize("form", ["tiled", "loop"])
@pytest.mark.parametrize("name", ["sgd", "adagrad"])
def test_update_and_scatter_on_removed_keys_leave_the_table_unchanged(name, form, kb):
    """removed keys are skipped by update / scatter_add / scatter_update like keys the table never
    saw; the state table still gains their zero-initialised entry, as in the oracle"""
    import torch
    from hugectr_amd.dynamic_table import DynamicEmbeddingTable, DynamicTableOptimizer
    from oracle.det_oracle import DetOracle
    code = _codes(name)
    ns = _num_state(name)
    dims = [8, 8] if form == "tiled" else [16, 6]
    sp, counts = [0, 1], [14, 11]
    so = _offsets(counts)
    rng = np.random.default_rng(300 + kb + len(name))
    t = DynamicEmbeddingTable(dims, "0.5", initial_capacity=16, key_dtype=_kd(torch, kb))
    opt = DynamicTableOptimizer(t, code[0], initial_capacity=16, **HYP)
    ow = [DetOracle(dims, 0.5), DetOracle(dims, 0.5, dtype=np.float64)]
    os_ = [DetOracle(dims, 0.0), DetOracle(dims, 0.0, dtype=np.float64)]
    keys = rng.choice(2**31 - 1, size=sum(counts), replace=False).astype(np.int64)
    kt = _keys(torch, keys, kb)
    n_el = counts[0] * dims[0] + counts[1] * dims[1]
    vals = rng.standard_normal(n_el).astype(np.float32)
    t.lookup(kt, sp, so)
    t.scatter_update(kt, _dev(torch, vals), sp, so)
    gone = np.concatenate([keys[2:7], keys[so[1] + 1:so[1] + 5]])
    t.remove(_keys(torch, gone, kb), sp, [0, 5, 9])
    for o in ow:
        o.lookup(keys, sp, so)
        o.scatter(keys, vals, sp, so, add=False)
        o.remove(gone, sp, [0, 5, 9])
    _same_as_oracle(t, ow[0], kb, "before the step")
    lens = np.repeat(dims, counts)
    ev, wg = _gapped_permuted_starts(rng, lens)
    opt.update(kt, _dev(torch, ev), _dev(torch, wg), sp, so)
    for w, s in zip(ow, os_):
        _oracle_update(w, s, code[1], keys, sp, so, ev, wg, 1)
    tag = f"{name} {form} u{kb * 8} removed keys"
    _compare_tables(tag + " weights", t, ow[0], ow[1], kb)
    assert t.size_per_class() == [9, 7]
    if ns:
        _compare_tables(tag + " state", opt.states, os_[0], os_[1], kb)
        assert opt.states.size_per_class() == counts
    # scatter_add / scatter_update of removed keys only: nothing changes
    before = [_export(t, c, kb) for c in range(2)]
    upd = rng.integers(1, 5, size=5 * dims[0] + 4 * dims[1]).astype(np.float32)
    t.scatter_add(_keys(torch, gone, kb), _dev(torch, upd), sp, [0, 5, 9])
    t.scatter_update(_keys(torch, gone, kb), _dev(torch, upd), sp, [0, 5, 9])
    assert t.size_per_class() == [9, 7]
    for c in range(2):
        k, v = _export(t, c, kb)
        assert np.array_equal(k, before[c][0])
        assert np.array_equal(v.view(np.uint32), before[c][1].view(np.uint32))
