"""GPU: hybrid DynamicVariables that grow from init_capacity to max_capacity (hctr_lru_create_growing,
csrc/hybrid_table.hip: lru_split_kernel + lru_move_kernel) against the sequential restatement in
tests/lru_grow_oracle.py -- slot by slot through every doubling -- and beside a table created at
max_capacity, an untiered twin, and the CPU optimizer oracle.  S = 64, 128 -> 1024 slots."""
import datetime as dt
import functools

import numpy as np
import pytest

from lru_grow_oracle import GrowFilterLruTable, GrowLruTable, checked_calls
from lru_oracle import EMPTY, LruTable

pytestmark = pytest.mark.gpu

S, C0, CMAX = 64, 128, 1024
UTC = dt.timezone.utc


def _u64(t):
    return t.cpu().numpy().astype(np.int64).view(np.uint64)


def _cuda(keys):
    import torch
    return torch.from_numpy(np.asarray(keys).astype(np.int64)).cuda()


def _var(D=8, init="", seed=5, grow=True, **kw):
    from hugectr_amd import sok
    sok.init()
    if grow:
        kw["init_capacity"] = C0
    return sok.DynamicVariable(D, init, var_type="hybrid", max_bucket_size=S, max_capacity=CMAX,
                               seed=seed, **kw)


def _check_table(var, orc: LruTable):
    """every occupied slot (key, score, row), the counters and the capacity: bit for bit"""
    k, w, sl, sc = var._lru.export(with_slots=True)
    occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
    assert np.array_equal(sl.cpu().numpy(), occ)
    assert np.array_equal(_u64(k), orc.keys[occ])
    assert np.array_equal(sc.cpu().numpy().astype(np.uint64), orc.scores[occ])
    assert np.array_equal(w.cpu().numpy(), orc.rows[occ])
    assert var.size == orc.size() and var._lru.rejected_count() == orc.rejected
    assert var._lru.capacity == CMAX
    assert var._lru.current_capacity == orc.C
    assert var._lru.doublings == getattr(orc, "doublings", 0)


@functools.lru_cache(maxsize=None)
def _mixed_calls():
    """[(keys, train)] x 24: power-law keys with repeats, every third call read-only.  Call 6 brings
    about 600 fresh keys while the table has 256 slots (two doublings in one call); call 19 brings
    1500 to the table at its largest capacity, which evicts and rejects."""
    rng = np.random.default_rng(11)
    out = []
    for call in range(24):
        n = int(rng.integers(30, 80)) if call < 6 else int(rng.integers(50, 400))
        keys = (rng.zipf(1.2, size=n) + (call // 4) * 300) % 6000
        if call == 6:
            keys = np.concatenate([keys, 10000 + rng.choice(5000, size=600, replace=False)])
        if call == 19:
            keys = np.concatenate([keys, 20000 + rng.choice(9000, size=1500, replace=False)])
        out.append((keys.astype(np.int64), call % 3 != 2))
    return tuple(out)


def _run_mixed(var, orc):
    from hugectr_amd import sok
    caps, evicted = [], 0
    for call, (keys, train) in enumerate(_mixed_calls()):
        kt = _cuda(keys)
        caps.append(orc.C)
        if train:
            vals, ek, ev = sok.sparse_read_and_evict(var, kt)
        else:
            vals = var.sparse_read(kt)
        wv, _, ok, orow = orc.lookup(keys, insert=train)
        assert np.array_equal(vals.detach().cpu().numpy(), wv), call
        if train:
            assert np.array_equal(_u64(ek), ok), call
            assert np.array_equal(ev.cpu().numpy(), orow), call
            evicted += ok.size
        _check_table(var, orc)
    var._pending.clear()
    return caps, evicted


@pytest.mark.parametrize("initializer", ["", "11"])
def test_bit_exact_through_growth(initializer):
    var = _var(8, initializer)
    orc = GrowLruTable(C0, CMAX, 8, initializer, S, seed=5)
    assert var._lru.current_capacity == C0 and var._lru.doublings == 0
    caps, evicted = _run_mixed(var, orc)
    assert caps[6] == 256 and caps[7] == CMAX        # the 600-key call doubled twice
    assert orc.doublings == 3 and 128 in caps and caps[19] == CMAX
    assert evicted > 0 and orc.rejected > 0          # the table at its largest capacity evicts


@pytest.mark.parametrize("same", [False, True])
def test_no_growth_unless_asked(same):
    """no init_capacity, or init_capacity == max_capacity: the table created at max_capacity"""
    var = _var(8, "", init_capacity=CMAX, grow=False) if same else _var(8, "", grow=False)
    assert var._lru.current_capacity == var._lru.capacity == CMAX and var._lru.doublings == 0
    assert var.config_dict["init_capacity"] == (CMAX if same else 1 << 20)
    _run_mixed(var, LruTable(CMAX, 8, "", S, seed=5))
    assert var._lru.current_capacity == CMAX and var._lru.doublings == 0


def test_grown_equals_created_at_max_capacity():
    """without evictions or rejections, where a key's slot is does not show: values every call, and
    key -> (score, row) at the end"""
    import torch
    from hugectr_amd import sok
    grown, full = _var(4, "", seed=1), _var(4, "", seed=1, grow=False)
    og, of = GrowLruTable(C0, CMAX, 4, "", S, seed=1), LruTable(CMAX, 4, "", S, seed=1)
    evicted = 0
    for keys, train in checked_calls():
        kt = _cuda(keys)
        if train:
            a, b = (sok.sparse_read_and_evict(v, kt) for v in (grown, full))
            assert a[1].numel() == 0 and b[1].numel() == 0
            a, b = a[0].detach(), b[0].detach()
        else:
            a, b = grown.sparse_read(kt), full.sparse_read(kt)
        assert torch.equal(a, b)
        evicted += og.lookup(keys, train)[2].size + of.lookup(keys, train)[2].size
    assert evicted == 0 and og.rejected == 0 and of.rejected == 0      # the precondition
    assert grown._lru.doublings == og.doublings == 3
    maps = []
    for v in (grown, full):
        k, w, _, sc = v._lru.export(with_slots=True)
        maps.append({int(a): (int(b), c.tobytes())
                     for a, b, c in zip(k.cpu().numpy(), sc.cpu().numpy(), w.cpu().numpy())})
        v._pending.clear()
    assert maps[0] == maps[1] and len(maps[0]) == og.size() == 675


def _opt_params(name, wrapper):
    from oracle import pyoracle as orc
    o = orc.OptParamsC()
    hp = wrapper.hp
    o.optimizer, o.update_type, o.lr = {"adagrad": orc.OPT_ADAGRAD, "adam": orc.OPT_ADAM}[name], 0, \
        hp["lr"]
    o.beta1, o.beta2, o.epsilon = hp["beta1"], hp["beta2"], hp["epsilon"]
    o.momentum_factor, o.scaler, o.times, o.state_half = hp["momentum"], hp["scaler"], \
        wrapper.times, 0
    return o


def _oracle_step(orc_t: LruTable, keys, kg, name, wrapper):
    """OptimizerWrapper.step on the oracle: keys found again, the gone ones dropped"""
    from oracle import pyoracle as orc
    slots = orc_t.find(keys)
    live = slots >= 0
    if not live.any():
        return
    st = orc_t.states + [None, None]
    orc.update_params(np.arange(int(live.sum()) + 1), slots[live].astype(np.uint64),
                      np.ascontiguousarray(kg[live]), _opt_params(name, wrapper), orc_t.rows,
                      st[0], st[1])


def _train_calls():
    """the checked input's keys, every call a training call"""
    return [keys for keys, _ in checked_calls(16)]


@pytest.mark.parametrize("opt_name", ["adagrad", "adam"])
def test_states_move_with_their_keys(opt_name):
    """an optimizer step after every call, across all three doublings: rows and states of every
    occupied slot follow the oracle stepped by the CPU optimizer (to the tolerance of
    test_sok_hybrid_gpu.py::test_training_through_lookup_sparse, whose step this is)"""
    import torch
    from hugectr_amd import sok
    D, ns = 8, {"adagrad": 1, "adam": 2}[opt_name]
    var = _var(D, "", seed=3)
    wrapper = sok.OptimizerWrapper(opt_name, lr=0.05)
    orc = GrowLruTable(C0, CMAX, D, "", S, seed=3, num_state=ns)
    rng = np.random.default_rng(2)
    caps = set()
    for it, keys in enumerate(_train_calls()):
        G = rng.standard_normal((keys.size, D)).astype(np.float32)
        vals, _, _ = sok.sparse_read_and_evict(var, _cuda(keys))
        vec, _, _, _ = orc.lookup(keys, insert=True)
        assert np.array_equal(vals.detach().cpu().numpy(), vec), it
        (vals * torch.from_numpy(G).cuda()).sum().backward()
        wrapper.step([var])
        _oracle_step(orc, keys, G, opt_name, wrapper)
        k, rows, sl, _ = var._lru.export(with_slots=True)
        occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
        assert np.array_equal(sl.cpu().numpy(), occ) and np.array_equal(_u64(k), orc.keys[occ])
        assert np.allclose(rows.cpu().numpy(), orc.rows[occ], rtol=1e-6, atol=1e-6), it
        for j in range(ns):
            st = var._lru.gather_slots(1 + j, sl).cpu().numpy()
            assert np.allclose(st, orc.states[j][occ], rtol=1e-6, atol=1e-6), (it, j)
            assert np.abs(st).sum() > 0
        assert var._lru.current_capacity == orc.C
        caps.add(orc.C)
    assert caps == {128, 256, 512, 1024}


def _budget(hbm_slots, D):
    """the max_hbm_for_vectors (GiB) that gives exactly hbm_slots HBM slots"""
    return hbm_slots * D * 4 / 2**30


def _same_tables(var, twin, states):
    """what test_sok_hybrid_tier_gpu.py's _same_tables compares -- export (keys, slots, scores,
    rows), size, rejected count, every state -- bit-equal"""
    import torch
    a = var._lru.export(with_slots=True)
    b = twin._lru.export(with_slots=True)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)
    assert var.size == twin.size
    assert var._lru.rejected_count() == twin._lru.rejected_count()
    for j in range(states):
        assert torch.equal(var._lru.gather_slots(1 + j, a[2]), twin._lru.gather_slots(1 + j, b[2]))


@pytest.mark.parametrize("hb", [256, 0])
def test_tiered_growth_equals_the_untiered_twin(hb):
    """an HBM budget of 256 slots (the table becomes tiered when it grows past them) and of none,
    with Adam steps: everything observable equals the untiered growing twin's after every call,
    and at every capacity C the placement is H = min(C, budget), C - H host rows"""
    import torch
    from hugectr_amd import sok
    D = 8
    var = _var(D, "", seed=7, max_hbm_for_vectors=_budget(hb, D))
    twin = _var(D, "", seed=7)
    assert var.tiered and not twin.tiered
    opts = [sok.OptimizerWrapper("adam", lr=0.05) for _ in range(2)]
    rng = np.random.default_rng(6)
    calls = _train_calls() + [20000 + rng.choice(9000, size=1500, replace=False)]
    caps = set()
    for it, keys in enumerate(calls):
        G = torch.from_numpy(rng.standard_normal((keys.size, D)).astype(np.float32)).cuda()
        outs = []
        for v, o in zip((var, twin), opts):
            vals, ek, ev = sok.sparse_read_and_evict(v, _cuda(keys))
            (vals * G).sum().backward()
            o.step([v])
            outs.append((vals.detach(), ek, ev))
        for x, y in zip(*outs):
            assert x.shape == y.shape and torch.equal(x, y), it
        _same_tables(var, twin, 2)
        C = twin._lru.current_capacity
        caps.add(C)
        assert var._lru.current_capacity == C and var._lru.doublings == twin._lru.doublings
        H = min(C, hb)
        p = var._lru.placement()
        assert (p[0], p[2]) == (H, C - H) and var._lru.hbm_slots == H
        assert var._lru.rows_ptr()[1] == H
        assert twin._lru.placement()[0] == C and twin._lru.placement()[2] == 0
        if H < C:
            assert bool((var._lru.find(_cuda(keys)) >= H).any())     # keys do live in host memory
    assert caps == {128, 256, 512, 1024}
    assert outs[0][1].numel() > 0 and var._lru.rejected_count() > 0   # the last call evicted


def _ragged(keys, lens):
    import torch
    from hugectr_amd import sok
    return sok.Ragged(_cuda(keys), torch.from_numpy(lens).cuda())


def _pool_kept(vec, lens, filt, D):
    """the path's own pooling kernel over the oracle's kept keys (vectors as a table, in order)"""
    import torch
    from hugectr_amd import sok
    bag = np.repeat(np.arange(lens.size), lens)
    kept_lens = np.bincount(bag[~filt], minlength=lens.size).astype(np.int64)
    table = torch.from_numpy(np.ascontiguousarray(vec[~filt])).cuda()
    if table.shape[0] == 0:
        return np.zeros((lens.size, D), dtype=np.float32)
    ro = sok._offsets(torch.from_numpy(kept_lens).cuda())
    rows = torch.arange(table.shape[0], dtype=torch.int64, device="cuda")
    return sok._pool(table, ro, rows, None, 0, D).cpu().numpy()


def test_filtered_growth():
    """filter_ratio 0.5 through lookup_sparse(use_low_frequency_filter=True): only admitted keys
    count toward the load, and the table, its capacity and the filtered count follow the oracle"""
    from hugectr_amd import sok
    D = 8
    var = _var(D, "", seed=5, filter_ratio=0.5)
    orc = GrowFilterLruTable(C0, CMAX, D, "", S, seed=5)
    rng = np.random.default_rng(12)
    caps = set()
    for call in range(10):
        B = 700 if call == 8 else int(rng.integers(30, 90))
        lens = rng.integers(0, 4, size=B)
        keys = rng.integers(0, 3000, size=int(lens.sum())) + 200 * call
        out = sok.lookup_sparse(var, _ragged(keys, lens), combiners="sum",
                                use_low_frequency_filter=True)
        vec, _, _, _, filt = orc.lookup(keys, insert=True, admit=0.5)
        assert filt.any() and not filt.all()
        assert np.array_equal(out.detach().cpu().numpy(), _pool_kept(vec, lens, filt, D)), call
        _check_table(var, orc)
        assert var._lru.filtered_count() == orc.filtered
        caps.add(orc.C)
    assert caps == {128, 256, 512, 1024} and orc.filtered > 0
    var._pending.clear()


class _Clock:
    """injected clock: whole seconds, in nanoseconds"""

    def __init__(self):
        self.s = 0

    def __call__(self):
        return self.s * 1_000_000_000


def test_incremental_dump_after_growth():
    """a threshold between two doublings: the slots touched since, wherever growth has put them"""
    from hugectr_amd import sok
    var = _var(8, "", seed=6)
    orc = GrowFilterLruTable(C0, CMAX, 8, "", S, seed=6)
    clock = _Clock()
    var._lru.clock = clock
    at = {}
    for call, keys in enumerate(_train_calls()):
        clock.s = 10 * (call + 1)
        sok.sparse_read_and_evict(var, _cuda(keys))
        orc.lookup(keys, insert=True)
        at.setdefault(orc.doublings, call + 1)        # the call that made doubling d
    var._pending.clear()
    assert orc.doublings == 3
    t0 = at[2] + 1                                    # after the second doubling, before the third
    assert at[2] < t0 <= at[3]
    _check_table(var, orc)
    keys, values = sok.incremental_model_dump(var, dt.datetime.fromtimestamp(10 * t0, tz=UTC))
    ok, _, _, orow = orc.export_if(t0)
    assert 0 < ok.size < orc.size()
    assert np.array_equal(keys[0].view(np.uint64), ok) and np.array_equal(values[0], orow)


def test_dump_and_load_after_growth(tmp_path):
    """sok.dump of a grown variable, sok.load into a fresh growing one: the same key -> (row, state)
    map, and the capacity the rule gives for one call that brings every key"""
    import torch
    from hugectr_amd import sok
    D = 8
    var = _var(D, "0.25", seed=1, name="grown")
    opt = sok.OptimizerWrapper("adagrad", lr=0.1)
    for keys in _train_calls()[:5]:
        vals, _, _ = sok.sparse_read_and_evict(var, _cuda(keys))
        (vals * vals).sum().backward()
        opt.step([var])
    n, C = var.size, var._lru.current_capacity
    assert var._lru.doublings == 2 and C == 512
    sok.dump(str(tmp_path), [var], opt)
    var2 = _var(D, "zeros", seed=1, name="grown")
    opt2 = sok.OptimizerWrapper("adagrad", lr=0.1)
    sok.load(str(tmp_path), [var2], opt2)
    want = C0
    while want < CMAX and n > 0.5 * want:             # occ = 0, m = n
        want *= 2
    assert var2._lru.current_capacity == want and var2.size == n
    k1, w1, s1 = sok._var_arrays(var, opt)
    k2, w2, s2 = sok._var_arrays(var2, opt2)
    assert torch.equal(k1, k2) and torch.equal(w1, w2) and torch.equal(s1[0], s2[0])
    assert float(s1[0].abs().sum()) > 0
