"""GPU: the hybrid DynamicVariable's low-frequency admission filter (lookup_sparse(...,
use_low_frequency_filter=True)) and sok.incremental_model_dump, against the sequential restatement
in tests/lru_filter_oracle.py (table slot by slot, counters, pooled outputs, optimizer state)."""
import datetime as dt
import os

import numpy as np
import pytest

from lru_filter_oracle import FilterLruTable
from lru_oracle import EMPTY

pytestmark = pytest.mark.gpu

UTC = dt.timezone.utc


def _u64(t):
    return t.cpu().numpy().astype(np.int64).view(np.uint64)


class _Clock:
    """injected clock: whole seconds, in nanoseconds"""

    def __init__(self):
        self.s = 0

    def __call__(self):
        return self.s * 1_000_000_000


def _at(s):
    return dt.datetime.fromtimestamp(s, tz=UTC)


def _ragged(keys, lens, w=None):
    import torch
    from hugectr_amd import sok
    ids = sok.Ragged(torch.from_numpy(keys.astype(np.int64)).cuda(), torch.from_numpy(lens).cuda())
    sw = sok.Ragged(torch.from_numpy(w).cuda(), torch.from_numpy(lens).cuda()) \
        if w is not None else None
    return ids, sw


def _pool_kept(vec, lens, w, filt, comb):
    """the path's own pooling kernel over the oracle's kept keys (vectors as a table, in order)"""
    import torch
    from hugectr_amd import sok
    bag = np.repeat(np.arange(lens.size), lens)
    kept_lens = np.bincount(bag[~filt], minlength=lens.size).astype(np.int64)
    table = torch.from_numpy(np.ascontiguousarray(vec[~filt])).cuda()
    if table.shape[0] == 0:
        return np.zeros((lens.size, vec.shape[1]), dtype=np.float32)
    ro = sok._offsets(torch.from_numpy(kept_lens).cuda())
    rows = torch.arange(table.shape[0], dtype=torch.int64, device="cuda")
    wk = torch.from_numpy(np.ascontiguousarray(w[~filt])).cuda() if w is not None else None
    return sok._pool(table, ro, rows, wk, 1 if comb == "mean" else 0, vec.shape[1]).cpu().numpy()


def _check_table(var, orc):
    k, w, sl, sc = var._lru.export(with_slots=True)
    occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
    assert np.array_equal(sl.cpu().numpy(), occ)
    assert np.array_equal(_u64(k), orc.keys[occ])
    assert np.array_equal(sc.cpu().numpy().astype(np.uint64), orc.scores[occ])
    assert np.array_equal(w.cpu().numpy(), orc.rows[occ])
    assert var._lru.rejected_count() == orc.rejected
    assert var._lru.filtered_count() == orc.filtered


def test_reference_incremental_dump_scenario():
    """lookup_sparse_hkv_incremental_dump_test.py, shrunk: after every iteration the dump since the
    previous iteration's end holds exactly the keys of this iteration"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(1)
    dims, hot, combs = [128, 4], [10, 3], ["mean", "sum"]
    clock = _Clock()
    vs = [sok.DynamicVariable(d, str(3 + i), var_type="hybrid", max_capacity=16384)
          for i, d in enumerate(dims)]
    for v in vs:
        v._lru.clock = clock
    opt = sok.OptimizerWrapper("sgd", lr=1.0)
    B, rows = 64, 2000
    records, times = [], []
    for it in range(5):
        ids, uniq = [], []
        for h in hot:
            lens = rng.integers(1, h + 1, size=B)
            keys = rng.integers(0, rows, size=int(lens.sum()))
            ids.append(_ragged(keys, lens)[0])
            uniq.append(np.unique(keys))
        records.append(uniq)
        clock.s = 10 * it + 5
        outs = sok.lookup_sparse(vs, ids, combiners=combs)
        sum(o.sum() for o in outs).backward()
        opt.step(vs)
        times.append(_at(10 * it + 8))
        if it > 0:
            keys, values = sok.incremental_model_dump(vs, times[it - 1])
            assert len(keys) == len(values) == 2
            for j in range(2):
                assert np.array_equal(np.sort(keys[j]), records[it][j]), (it, j)
                assert values[j].shape == (keys[j].size, dims[j])
                # every dumped row is the variable's current row
                got = vs[j].sparse_read(torch.from_numpy(keys[j]).cuda()).cpu().numpy()
                assert np.array_equal(values[j], got)
    # per-variable thresholds; a threshold after the last call gives nothing
    keys, values = sok.incremental_model_dump(vs, [_at(0), _at(100)])
    assert np.array_equal(np.sort(keys[0]), np.unique(np.concatenate([r[0] for r in records])))
    assert keys[1].size == 0 and values[1].shape == (0, 4)
    for v in vs:
        v._pending.clear()


def test_export_if_against_the_oracle():
    """keys, slots, scores and rows of export_if after calls with evictions and rejections: threshold
    0 (everything), mid-sequence, and past the last call (nothing)"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(4)
    D = 8
    var = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=256, seed=6)
    orc = FilterLruTable(256, D, "", 128, seed=6)
    clock = _Clock()
    var._lru.clock = clock
    for call in range(8):
        n = 600 if call == 5 else int(rng.integers(40, 200))
        keys = rng.integers(0, 1500, size=n) + 100 * call
        clock.s = 10 * (call + 1)
        sok.sparse_read_and_evict(var, torch.from_numpy(keys).cuda())
        orc.lookup(keys, insert=True)
    var._pending.clear()
    assert orc.rejected > 0
    _check_table(var, orc)
    for t0 in (0, 4, 8, 9):
        k, w, sl, sc = var._lru.export_if(t0)
        ok, osl, osc, orow = orc.export_if(t0)
        assert np.array_equal(_u64(k), ok), t0
        assert np.array_equal(sl.cpu().numpy(), osl), t0
        assert np.array_equal(sc.cpu().numpy().astype(np.uint64), osc), t0
        assert np.array_equal(w.cpu().numpy(), orow), t0
    assert var._lru.export_if(9)[0].numel() == 0
    # through the public call: threshold = call 4's time -> t0 = 4
    keys, values = sok.incremental_model_dump(var, _at(40))
    ok, _, _, orow = orc.export_if(4)
    assert np.array_equal(keys[0].view(np.uint64), ok) and np.array_equal(values[0], orow)
    keys, _ = sok.incremental_model_dump([var], [_at(81)])
    assert keys[0].size == 0


def test_reference_low_frequency_scenario():
    """lookup_sparse_hkv_low_frequency_test.py, with filter_ratio 0: after one pre-training batch a
    filtered lookup pools the stored keys alone; samples of new keys only come out zero; nothing is
    inserted, and the step leaves the new keys absent"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(2)
    dims, init, combs = [128, 4], [13, 17], ["sum", "mean"]
    vs = [sok.DynamicVariable(d, str(init[i]), var_type="hybrid", max_capacity=8192,
                              filter_ratio=0.0) for i, d in enumerate(dims)]
    opt = sok.OptimizerWrapper("momentum", lr=1.0, momentum=0.9)
    B, R = 256, 1000
    pre = []
    ids = []
    for _ in dims:
        keys = rng.integers(0, R, size=B)
        pre.append(np.unique(keys))
        ids.append(_ragged(keys, np.ones(B, dtype=np.int64))[0])
    outs = sok.lookup_sparse(vs, ids, combiners=combs)
    sum(o.sum() for o in outs).backward()
    opt.step(vs)
    sizes = [v.size for v in vs]
    ids, raw = [], []
    for _ in dims:
        lens = rng.integers(1, 4, size=B)
        keys = rng.integers(0, 2 * R, size=int(lens.sum()))
        raw.append((keys, lens))
        ids.append(_ragged(keys, lens)[0])
    outs = sok.lookup_sparse(vs, ids, combiners=combs, use_low_frequency_filter=True)
    for j, (v, o) in enumerate(zip(vs, outs)):
        keys, lens = raw[j]
        stored = np.isin(keys, pre[j])
        vec = v.sparse_read(torch.from_numpy(keys).cuda()).cpu().numpy()
        want = _pool_kept(vec, lens, None, ~stored, combs[j])
        got = o.detach().cpu().numpy()
        assert np.array_equal(got, want), j
        bag = np.repeat(np.arange(B), lens)
        only_new = np.bincount(bag[stored], minlength=B) == 0
        assert only_new.any() and (got[only_new] == 0).all()
        assert (np.abs(got[~only_new]).sum(1) > 0).all()
        assert v.size == sizes[j] and v._lru.filtered_count() == int((~stored).sum())
        assert v._lru.rejected_count() == 0
    sum(o.sum() for o in outs).backward()
    opt.step(vs)
    for j, v in enumerate(vs):
        keys, _ = raw[j]
        new = np.unique(keys[~np.isin(keys, pre[j])])
        assert (v._lru.find(torch.from_numpy(new).cuda()) == -1).all()
        assert v.size == sizes[j]


@pytest.mark.parametrize("initializer", ["", "11"])
def test_bit_exact_against_the_oracle_p03(initializer):
    """filter_ratio 0.3 over calls with evictions and rejections: the table slot by slot, the filtered
    / rejected counters, and sum / mean / weighted outputs equal to the path's pooling of the
    oracle's kept keys"""
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(12)
    D = 8
    var = sok.DynamicVariable(D, initializer, var_type="hybrid", max_capacity=256, seed=5,
                              filter_ratio=0.3)
    orc = FilterLruTable(256, D, initializer, 128, seed=5)
    for call in range(9):
        comb = ["sum", "mean"][call % 2]
        weighted = call % 3 == 2
        B = 1200 if call == 4 else int(rng.integers(20, 120))   # call 4 overflows the buckets
        lens = rng.integers(0, 4, size=B)
        keys = rng.integers(0, 3000, size=int(lens.sum())) + 200 * call
        w = (rng.random(keys.size) + 0.5).astype(np.float32) if weighted else None
        ids, sw = _ragged(keys, lens, w)
        out = sok.lookup_sparse(var, ids, sw, combiners=comb, use_low_frequency_filter=True)
        vec, slots, _, _, filt = orc.lookup(keys, insert=True, admit=0.3)
        assert filt.any() and not filt.all()
        assert np.array_equal(out.detach().cpu().numpy(), _pool_kept(vec, lens, w, filt, comb)), call
        _check_table(var, orc)
    assert orc.rejected > 0 and orc.filtered > 0
    var._pending.clear()


def _keygrads(lens, w, G, comb):
    bag = np.repeat(np.arange(lens.size), lens)
    wt = np.ones(bag.size, dtype=np.float32) if w is None else w
    kg = G[bag] * wt[:, None]
    if comb == "mean":
        den = np.zeros(lens.size, dtype=np.float32)
        np.add.at(den, bag, wt)
        kg = kg / den[bag][:, None]
    return kg.astype(np.float32)


def _oracle_step(orc_t, keys, kg, name, wrapper):
    from oracle import pyoracle as orc
    slots = orc_t.find(keys)
    live = slots >= 0
    if not live.any():
        return
    codes = {"sgd": orc.OPT_SGD, "adam": orc.OPT_ADAM}
    o = orc.OptParamsC()
    hp = wrapper.hp
    o.optimizer, o.update_type, o.lr = codes[name], 0, hp["lr"]
    o.beta1, o.beta2, o.epsilon = hp["beta1"], hp["beta2"], hp["epsilon"]
    o.momentum_factor, o.scaler, o.times, o.state_half = hp["momentum"], hp["scaler"], wrapper.times, 0
    st = orc_t.states + [None, None]
    orc.update_params(np.arange(int(live.sum()) + 1), slots[live].astype(np.uint64),
                      np.ascontiguousarray(kg[live]), o, orc_t.rows, st[0], st[1])


@pytest.mark.parametrize("opt_name", ["sgd", "adam"])
@pytest.mark.parametrize("comb", ["sum", "mean"])
def test_training_with_the_filter(opt_name, comb):
    """lookup_sparse(use_low_frequency_filter=True) + OptimizerWrapper.step: admitted keys follow the
    CPU optimizer on the kept keys; filtered keys have no row and no state"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(8)
    D = 16
    var = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=512, seed=3,
                              filter_ratio=0.5)
    wrapper = sok.OptimizerWrapper(opt_name, lr=0.05)
    ns = {"sgd": 0, "adam": 2}[opt_name]
    orc = FilterLruTable(512, D, "", 128, seed=3, num_state=ns)
    for it in range(5):
        B = 64
        lens = rng.integers(1, 5, size=B)
        keys = rng.integers(0, 900, size=int(lens.sum())).astype(np.int64)
        G = rng.standard_normal((B, D)).astype(np.float32)
        out = sok.lookup_sparse(var, _ragged(keys, lens)[0], combiners=comb,
                                use_low_frequency_filter=True)
        vec, _, _, _, filt = orc.lookup(keys, insert=True, admit=0.5)
        assert np.allclose(out.detach().cpu().numpy(), _pool_kept(vec, lens, None, filt, comb),
                           rtol=1e-5, atol=1e-5), it
        (out * torch.from_numpy(G).cuda()).sum().backward()
        wrapper.step([var])
        bag = np.repeat(np.arange(B), lens)
        kept_lens = np.bincount(bag[~filt], minlength=B)
        _oracle_step(orc, keys[~filt], _keygrads(kept_lens, None, G, comb), opt_name, wrapper)
        k, rows, sl, _ = var._lru.export(with_slots=True)
        occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
        assert np.array_equal(sl.cpu().numpy(), occ) and np.array_equal(_u64(k), orc.keys[occ])
        assert np.allclose(rows.cpu().numpy(), orc.rows[occ], rtol=1e-6, atol=1e-6), it
        cap = var._lru.capacity
        for j in range(ns):
            st = sok._view_f32(var._lru.state_ptr(j), (cap, D)).cpu().numpy()[occ]
            assert np.allclose(st, orc.states[j][occ], rtol=1e-6, atol=1e-6), (it, j)
        gone = np.unique(keys[filt])
        gone = gone[~np.isin(gone.view(np.uint64), orc.keys)]
        assert (var._lru.find(torch.from_numpy(gone).cuda()) == -1).all()
    assert orc.filtered > 0


def test_filter_off_and_p1_give_todays_bits():
    """use_low_frequency_filter=False, and filter_ratio 1 with the flag on, equal the plain path bit
    for bit: outputs, table, optimizer result"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(9)
    D = 8
    mk = lambda **kw: sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=256, seed=2, **kw)
    base, off, p1 = mk(), mk(filter_ratio=0.5), mk(filter_ratio=1.0)
    opt = sok.OptimizerWrapper("adagrad", lr=0.1)
    for it in range(4):
        lens = rng.integers(0, 4, size=400 if it == 0 else 96)   # call 1 fills whole buckets
        keys = rng.integers(0, 1000, size=int(lens.sum()))
        w = (rng.random(keys.size) + 0.5).astype(np.float32)
        ids, sw = _ragged(keys, lens, w)
        a = sok.lookup_sparse(base, ids, sw, combiners="mean")
        b = sok.lookup_sparse(off, ids, sw, combiners="mean", use_low_frequency_filter=False)
        c = sok.lookup_sparse(p1, ids, sw, "mean", True, True)
        assert torch.equal(a, b) and torch.equal(a, c), it
        for o in (a, b, c):
            (o * o).sum().backward()
        opt.step([base, off, p1])
    ka, va, sa, ca = base._lru.export(with_slots=True)
    for v in (off, p1):
        kb, vb, sb, cb = v._lru.export(with_slots=True)
        assert torch.equal(ka, kb) and torch.equal(va, vb) and torch.equal(sa, sb)
        assert torch.equal(ca, cb)
        assert v._lru.rejected_count() == base._lru.rejected_count()
    assert p1._lru.filtered_count() == 0 and base._lru.rejected_count() > 0


def _two_rank_run(rank, world, clock_s):
    """3 filtered mean lookups (weighted in the middle one) + SGD; returns per-call outputs of this
    rank's samples and the dump since the second call"""
    import torch
    from hugectr_amd import sok
    rng = np.random.default_rng(31)               # the same stream on every rank
    D, B = 8, 40
    var = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=4096 // world, seed=7,
                              filter_ratio=0.5)
    clock = _Clock()
    var._lru.clock = clock
    opt = sok.OptimizerWrapper("sgd", lr=0.1)
    outs = []
    for call in range(3):
        lens = rng.integers(0, 5, size=2 * B)   # the global batch
        keys = rng.integers(0, 3000, size=int(lens.sum()))
        w = (rng.random(keys.size) + 0.5).astype(np.float32) if call == 1 else None
        G = rng.standard_normal((lens.size, D)).astype(np.float32)
        per = lens.size // world
        off = np.concatenate([[0], np.cumsum(lens)])
        sl = slice(off[rank * per], off[(rank + 1) * per])
        ids, sw = _ragged(keys[sl], lens[rank * per:(rank + 1) * per],
                          w[sl] if w is not None else None)
        clock.s = clock_s[call]
        out = sok.lookup_sparse(var, ids, sw, combiners="mean", use_low_frequency_filter=True)
        (out * torch.from_numpy(G[rank * per:(rank + 1) * per]).cuda()).sum().backward()
        opt.step([var])
        outs.append(out.detach().cpu().numpy())
    keys, values = sok.incremental_model_dump(var, _at(clock_s[1]))
    return outs, keys[0], values[0]


def _worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from hugectr_amd import sok
        sok.init()
        outs, k, v = _two_rank_run(rank, world, [10, 20, 30])
        ret[rank] = ("ok", [o.tolist() for o in outs], k.tolist(), v.tolist())
    except Exception as e:  # pragma: no cover - reported by the parent
        import traceback
        ret[rank] = (f"{e!r}\n{traceback.format_exc()}",)
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_gloo():
    """p = 0.5, mean: the two-rank outputs equal the one-rank run, and the gathered incremental dump
    equals the one-rank dump as a sorted set"""
    import torch.multiprocessing as mp
    from hugectr_amd import sok
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = 29500 + (os.getpid() + 1311) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    for r in range(2):
        if ret.get(r, ("missing",))[0] != "ok":
            print(f"--- rank {r} ---\n{ret.get(r)}")
    assert ret.get(0, ("",))[0] == "ok" and ret.get(1, ("",))[0] == "ok"
    sok.init()
    outs1, k1, v1 = _two_rank_run(0, 1, [10, 20, 30])
    for call in range(3):
        two = np.concatenate([np.array(ret[r][1][call], dtype=np.float32) for r in range(2)])
        assert two.shape == outs1[call].shape
        assert np.allclose(two, outs1[call], rtol=1e-5, atol=1e-6), call
    # every rank returns the gathered dump: each copy is the one-rank dump
    o1 = np.argsort(k1)
    assert k1.size > 0
    for r in range(2):
        k = np.array(ret[r][2], dtype=np.int64)
        v = np.array(ret[r][3], dtype=np.float32).reshape(-1, 8)
        o = np.argsort(k)
        assert np.array_equal(k[o], k1[o1]), r
        assert np.allclose(v[o], v1[o1], rtol=1e-5, atol=1e-6), r
