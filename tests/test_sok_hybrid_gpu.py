"""GPU: sok.DynamicVariable(var_type="hybrid") -- the bounded LRU table of csrc/hybrid_table.hip --
against the sequential restatement of its semantics in tests/lru_oracle.py (slot by slot: key,
score, row; returned vectors; evicted pairs in order; rejected count) and the CPU optimizer oracle."""
import os

import numpy as np
import pytest

from lru_oracle import EMPTY, LruTable

pytestmark = pytest.mark.gpu


def _u64(t):
    return t.cpu().numpy().astype(np.int64).view(np.uint64)


def _check_table(var, orc: LruTable):
    """every occupied slot: key, score, row -- bit for bit"""
    k, w, sl, sc = var._lru.export(with_slots=True)
    occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
    assert np.array_equal(sl.cpu().numpy(), occ)
    assert np.array_equal(_u64(k), orc.keys[occ])
    assert np.array_equal(sc.cpu().numpy().astype(np.uint64), orc.scores[occ])
    assert np.array_equal(w.cpu().numpy(), orc.rows[occ])
    assert var.size == orc.size()
    assert var._lru.rejected_count() == orc.rejected


def _opt_params(name, wrapper):
    from oracle import pyoracle as orc
    codes = {"sgd": orc.OPT_SGD, "adagrad": orc.OPT_ADAGRAD, "adam": orc.OPT_ADAM}
    o = orc.OptParamsC()
    hp = wrapper.hp
    o.optimizer, o.update_type, o.lr = codes[name], 0, hp["lr"]
    o.beta1, o.beta2, o.epsilon = hp["beta1"], hp["beta2"], hp["epsilon"]
    o.momentum_factor, o.scaler, o.times, o.state_half = hp["momentum"], hp["scaler"], wrapper.times, 0
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


def test_reference_scenario_read_and_evict():
    """sparse_read_evict.py: 5 x 8192 fresh keys through a 16384-slot table, loss = sum, SGD lr 1:
    every evicted value is 11 - 1 = 10, no key is evicted twice, the counts add up"""
    import torch
    from hugectr_amd import sok
    sok.init()
    var = sok.DynamicVariable(16, "11", var_type="hybrid", init_capacity=8192, max_capacity=16384)
    assert var.backend_type == "hybrid" and var.config_dict["max_capacity"] == 16384
    opt = sok.OptimizerWrapper("sgd", lr=1.0)
    cap = var._lru.capacity
    seen_evicted = set()
    inserted = 0
    for it in range(5):
        keys = torch.arange(it * 8192, (it + 1) * 8192, dtype=torch.int64, device="cuda")
        vals, ek, ev = sok.sparse_read_and_evict(var, keys)
        assert torch.all(vals == 11.0)
        vals.sum().backward()
        opt.step([var])
        if ev.numel():
            assert torch.all(ev == 10.0), it
        ek_set = set(ek.cpu().tolist())
        assert len(ek_set) == ek.numel() and not (ek_set & seen_evicted)
        seen_evicted |= ek_set
        inserted += 8192
        size = var.size
        assert size <= cap
        assert size + len(seen_evicted) + var._lru.rejected_count() == inserted
    k, w = sok.export(var)
    assert torch.all(w == 10.0) and k.numel() == var.size
    assert len(seen_evicted) > 0


@pytest.mark.parametrize("initializer", ["", "11"])
def test_bit_exact_against_the_oracle(initializer):
    """8 buckets x 128 slots, power-law keys with repeats, training and evaluation lookups mixed"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(11)
    D = 8
    var = sok.DynamicVariable(D, initializer, var_type="hybrid", max_capacity=1024, seed=5)
    orc = LruTable(1024, D, initializer, 128, seed=5)
    for call in range(20):
        n = int(rng.integers(50, 900)) if call != 13 else 3000   # call 13 overflows buckets
        keys = (rng.zipf(1.2, size=n) + (call // 4) * 500) % 6000
        kt = torch.from_numpy(keys.astype(np.int64)).cuda()
        train = call % 3 != 2
        if train:
            vals, ek, ev = sok.sparse_read_and_evict(var, kt)
        else:
            vals = var.sparse_read(kt)
        wv, _, ok, orow = orc.lookup(keys, insert=train)
        assert np.array_equal(vals.detach().cpu().numpy(), wv), call
        if train:
            assert np.array_equal(_u64(ek), ok), call
            assert np.array_equal(ev.cpu().numpy(), orow), call
        _check_table(var, orc)
    assert orc.rejected > 0          # the 3000-key call filled whole buckets
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


def _pool_ref(vec, lens, w, comb):
    bag = np.repeat(np.arange(lens.size), lens)
    wt = np.ones(bag.size) if w is None else w.astype(np.float64)
    out = np.zeros((lens.size, vec.shape[1]))
    np.add.at(out, bag, vec * wt[:, None])
    if comb == "mean":
        den = np.zeros(lens.size)
        np.add.at(den, bag, wt)
        out = out / np.where(den > 0, den, 1)[:, None]
    return out


@pytest.mark.parametrize("opt_name", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("comb", ["sum", "mean"])
@pytest.mark.parametrize("weighted", [False, True])
def test_training_through_lookup_sparse(opt_name, comb, weighted):
    """lookup_sparse + OptimizerWrapper.step against the oracle + the CPU optimizer; one step sees
    keys evicted between its lookup and step(): their gradients are dropped"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(7)
    D = 16
    var = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=512, seed=3)
    wrapper = sok.OptimizerWrapper(opt_name, lr=0.05)
    ns = {"sgd": 0, "adagrad": 1, "adam": 2}[opt_name]
    orc = LruTable(512, D, "", 128, seed=3, num_state=ns)
    for it in range(6):
        B = 64
        lens = rng.integers(1, 5, size=B)
        keys = rng.integers(0, 900, size=int(lens.sum())).astype(np.int64)
        w = rng.random(keys.size).astype(np.float32) + 0.5 if weighted else None
        G = rng.standard_normal((B, D)).astype(np.float32)
        ids = sok.Ragged(torch.from_numpy(keys).cuda(), torch.from_numpy(lens).cuda())
        sw = sok.Ragged(torch.from_numpy(w).cuda(), torch.from_numpy(lens).cuda()) if weighted \
            else None
        out = sok.lookup_sparse(var, ids, sw, combiners=comb)
        vec, _, _, _ = orc.lookup(keys, insert=True)
        assert np.allclose(out.detach().cpu().numpy(), _pool_ref(vec, lens, w, comb),
                           rtol=1e-5, atol=1e-5), it
        (out * torch.from_numpy(G).cuda()).sum().backward()
        if it == 3:
            # fresh keys evict some of this lookup's keys before the step
            fresh = torch.arange(5000, 5400, dtype=torch.int64, device="cuda")
            _, ek, _ = sok.sparse_read_and_evict(var, fresh)
            _, _, ok, _ = orc.lookup(fresh.cpu().numpy(), insert=True)
            assert np.array_equal(_u64(ek), ok)
            assert np.isin(ok.view(np.int64), keys).any()   # the case this step is about
        wrapper.step([var])
        _oracle_step(orc, keys, _keygrads(lens, w, G, comb), opt_name, wrapper)
        k, rows, sl, sc = var._lru.export(with_slots=True)
        occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
        assert np.array_equal(sl.cpu().numpy(), occ) and np.array_equal(_u64(k), orc.keys[occ])
        assert np.allclose(rows.cpu().numpy(), orc.rows[occ], rtol=1e-6, atol=1e-6), it
        cap = var._lru.capacity
        for j in range(ns):
            st = sok._view_f32(var._lru.state_ptr(j), (cap, D)).cpu().numpy()[occ]
            assert np.allclose(st, orc.states[j][occ], rtol=1e-6, atol=1e-6), (it, j)


def test_rejection_within_one_call():
    """one bucket of 128 slots, 200 new keys in one call: the 72 largest are rejected, read the
    initial value, and their gradients have no effect"""
    import torch
    from hugectr_amd import sok
    sok.init()
    D = 8
    var = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=128, seed=9)
    orc = LruTable(128, D, "", 128, seed=9)
    keys = np.arange(1000, 1200, dtype=np.int64)
    lens = np.ones(200, dtype=np.int64)
    ids = sok.Ragged(torch.from_numpy(keys).cuda(), torch.from_numpy(lens).cuda())
    out = sok.lookup_sparse(var, ids, combiners="sum")
    vec, slots, _, _ = orc.lookup(keys, insert=True)
    assert np.array_equal(out.detach().cpu().numpy(), vec)
    assert (slots < 0).sum() == 72 and np.array_equal(keys[slots < 0], keys[-72:])
    out.sum().backward()
    sok.OptimizerWrapper("sgd", lr=0.5).step([var])
    assert var.size == 128 and var._lru.rejected_count() == 72
    k, w = sok.export(var)
    assert set(k.cpu().tolist()) == set(keys[:128].tolist())
    order = np.argsort(k.cpu().numpy())
    assert np.array_equal(w.cpu().numpy()[order], vec[:128] - np.float32(0.5))
    again = var.sparse_read(torch.from_numpy(keys[-72:]).cuda())
    assert np.array_equal(again.cpu().numpy(), vec[-72:])       # still the initial value


def test_dump_load_restores_export(tmp_path):
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(5)
    D = 8
    var = sok.DynamicVariable(D, "0.25", var_type="hybrid", max_capacity=256, name="hyb")
    opt = sok.OptimizerWrapper("adagrad", lr=0.1)
    for _ in range(4):
        lens = rng.integers(1, 4, size=32)
        ids = sok.Ragged(torch.from_numpy(rng.integers(0, 600, size=int(lens.sum()))).cuda(),
                         torch.from_numpy(lens).cuda())
        out = sok.lookup_sparse(var, ids, combiners="sum")
        (out * out).sum().backward()
        opt.step([var])
    sok.dump(str(tmp_path), [var], opt)
    var2 = sok.DynamicVariable(D, "zeros", var_type="hybrid", max_capacity=256, name="hyb")
    sok.load(str(tmp_path), [var2], sok.OptimizerWrapper("adagrad", lr=0.1))
    k1, v1 = sok.export(var)
    k2, v2 = sok.export(var2)
    o1, o2 = torch.argsort(k1), torch.argsort(k2)
    assert torch.equal(k1[o1], k2[o2]) and torch.equal(v1[o1], v2[o2])
    a1 = sok._var_arrays(var, opt)[2][0]
    a2 = sok._var_arrays(var2, opt)[2][0]
    assert torch.equal(a1, a2)


def _worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from hugectr_amd import sok
        sok.init()
        rng = np.random.default_rng(21)               # same stream on both ranks
        D, B, cap = 8, 48, 256
        var = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=cap // world, seed=4)
        # the single-process computation: one oracle table per owner, capacity halved likewise
        orcs = [LruTable(cap // world, D, "", 128, seed=4) for _ in range(world)]
        opt = sok.OptimizerWrapper("sgd", lr=0.1)
        evicted = 0
        for step in range(4):
            lens = rng.integers(1, 4, size=B * world)
            vals = rng.integers(0, 2000, size=int(lens.sum())).astype(np.int64)
            G = rng.standard_normal((B * world, D)).astype(np.float32)
            off = np.concatenate([[0], np.cumsum(lens)])
            sl = slice(off[rank * B], off[(rank + 1) * B])
            ids = sok.Ragged(torch.from_numpy(vals[sl]).cuda(),
                             torch.from_numpy(lens[rank * B:(rank + 1) * B]).cuda())
            out = sok.lookup_sparse(var, ids, combiners="sum")
            vec = np.zeros((vals.size, D), dtype=np.float32)
            for r in range(world):
                own = vals % world == r
                v, _, ek, _ = orcs[r].lookup(vals[own], insert=True)
                vec[own] = v
                evicted += ek.size
            want = _pool_ref(vec, lens, None, "sum")[rank * B:(rank + 1) * B]
            assert np.allclose(out.detach().cpu().numpy(), want, rtol=1e-5, atol=1e-5), step
            (out * torch.from_numpy(G[rank * B:(rank + 1) * B]).cuda()).sum().backward()
            opt.step([var])
            kg = _keygrads(lens, None, G, "sum")
            for r in range(world):
                own = vals % world == r
                _oracle_step(orcs[r], vals[own], kg[own], "sgd", opt)
            k, w = sok.export(var)
            o = orcs[rank]
            occ = np.nonzero(o.keys != np.uint64(EMPTY))[0]
            assert np.array_equal(_u64(k), o.keys[occ]), step
            assert np.allclose(w.cpu().numpy(), o.rows[occ], rtol=1e-6, atol=1e-6), step
        assert evicted > 0
        ret[rank] = "ok"
    except Exception as e:  # pragma: no cover - reported by the parent
        import traceback
        ret[rank] = f"{e!r}\n{traceback.format_exc()}"
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = 29500 + (os.getpid() + 977) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    for r in range(2):
        if ret.get(r) != "ok":
            print(f"--- rank {r} ---\n{ret.get(r)}")
    assert ret.get(0) == "ok" and ret.get(1) == "ok"
