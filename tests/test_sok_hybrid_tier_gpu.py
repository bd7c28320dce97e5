"""GPU: hybrid DynamicVariables with the host-memory value tier (max_hbm_for_vectors).  Every
scenario runs the tiered variable beside an untiered twin of the same (capacity, bucket, dim, key
type, initializer, seed), at H = C / 2 and H = 0 HBM slots, and checks that everything observable
is bit-equal to the twin and to the sequential oracle (tests/lru_oracle.py)."""
import ctypes
import datetime as dt
import filecmp
import os

import numpy as np
import pytest

from lru_filter_oracle import FilterLruTable
from lru_oracle import EMPTY, LruTable

pytestmark = pytest.mark.gpu

FRACS = [0.5, 0.0]


def _u64(t):
    return t.cpu().numpy().astype(np.int64).view(np.uint64)


def _budget(hbm_slots, D):
    """the max_hbm_for_vectors (GiB) that gives exactly hbm_slots HBM slots"""
    return hbm_slots * D * 4 / 2**30


def _pair(D, init, cap, frac, seed=0, **kw):
    """(tiered variable, untiered twin)"""
    from hugectr_amd import sok
    h = int(cap * frac)
    var = sok.DynamicVariable(D, init, var_type="hybrid", max_capacity=cap, seed=seed,
                              max_hbm_for_vectors=_budget(h, D), **kw)
    twin = sok.DynamicVariable(D, init, var_type="hybrid", max_capacity=cap, seed=seed, **kw)
    assert var.tiered and not twin.tiered
    assert var._lru.hbm_slots == h and var._lru.placement()[2] == cap - h
    return var, twin


def _same_tables(var, twin, states=0):
    """export (keys, slots, scores, rows), size, rejected count and every state: bit-equal"""
    from hugectr_amd import sok
    a = var._lru.export(with_slots=True)
    b = twin._lru.export(with_slots=True)
    for x, y in zip(a, b):
        assert torch_equal(x, y)
    assert var.size == twin.size
    assert var._lru.rejected_count() == twin._lru.rejected_count()
    sl = b[2]
    for j in range(states):
        st = sok._view_f32(twin._lru.state_ptr(j), (twin._lru.capacity, twin.dimension))[sl]
        var._lru.state_ptr(j)
        assert torch_equal(var._lru.gather_slots(1 + j, a[2]), st), j


def torch_equal(x, y):
    import torch
    return x.shape == y.shape and torch.equal(x.cpu(), y.cpu())


def _check_oracle(var, orc: LruTable):
    k, w, sl, sc = var._lru.export(with_slots=True)
    occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
    assert np.array_equal(sl.cpu().numpy(), occ)
    assert np.array_equal(_u64(k), orc.keys[occ])
    assert np.array_equal(sc.cpu().numpy().astype(np.uint64), orc.scores[occ])
    assert np.array_equal(w.cpu().numpy(), orc.rows[occ])
    assert var.size == orc.size() and var._lru.rejected_count() == orc.rejected


def test_placement_and_host_memory():
    from hugectr_amd import sok
    from hugectr_amd.hybrid_table import hbm_slots_for
    sok.init()
    D, cap = 8, 1024
    for g in (_budget(512, D), 0, 0.1 * _budget(1024, D), 1.0):
        var = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=cap,
                                  max_hbm_for_vectors=g)
        h = hbm_slots_for(g, D, cap, 128)
        assert var._lru.hbm_slots == h and var.config_dict["max_hbm_for_vectors"] == g
        assert var.tiered == (h < cap)
        assert var._lru.rows_ptr()[1] == h
    assert var._lru.host_part_ptr() == 0          # 1 GiB: everything in HBM
    var, _ = _pair(D, "", cap, 0.5)
    var._lru.state_ptr(0)
    assert var._lru.host_part_ptr(0) and var._lru.host_part_ptr(1) and not var._lru.host_part_ptr(2)
    if os.environ.get("HCTR_EMU") == "1":
        return  # (the emulator has no HIP runtime to ask)
    hip = _hip_runtime()

    class Attr(ctypes.Structure):
        _fields_ = [("type", ctypes.c_int), ("device", ctypes.c_int),
                    ("devicePointer", ctypes.c_void_p), ("hostPointer", ctypes.c_void_p),
                    ("isManaged", ctypes.c_int), ("allocationFlags", ctypes.c_uint)]

    for arr, p in ((0, var._lru.host_part_ptr(0)), (1, var._lru.host_part_ptr(1)),
                   (-1, var._lru.rows_ptr()[0])):
        a = Attr()
        assert p
        assert hip.hipPointerGetAttributes(ctypes.byref(a), ctypes.c_void_p(p)) == 0
        assert a.type == (2 if arr < 0 else 1), (arr, a.type)   # hipMemoryTypeDevice / Host


def _hip_runtime():
    """the HIP runtime this process uses (torch's), found among the loaded libraries"""
    import torch
    torch.cuda.init()
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert paths
    return ctypes.CDLL(sorted(paths)[0])


@pytest.mark.skipif(os.environ.get("HCTR_EMU") == "1", reason="2 GiB of rows")
def test_a_table_larger_than_its_hbm_budget():
    """C = 2^22 slots of D = 128 (2 GiB of rows) with 0.125 GiB of HBM for values: creating it
    takes well under 1 GiB of device memory"""
    import torch
    from hugectr_amd import sok
    sok.init()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    var = sok.DynamicVariable(128, "", var_type="hybrid", max_capacity=1 << 22,
                              max_hbm_for_vectors=0.125)
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info()[0]
    assert var._lru.hbm_slots == 1 << 18
    assert used < (1 << 30), used
    keys = torch.arange(0, 1 << 16, dtype=torch.int64, device="cuda") * 7919
    vals, _, _ = sok.sparse_read_and_evict(var, keys)
    assert torch.equal(vals, var.sparse_read(keys))
    var._pending.clear()
    var._lru.close()


@pytest.mark.parametrize("frac", FRACS)
def test_reference_scenario_read_and_evict(frac):
    """sparse_read_evict.py, shrunk: 5 x 2048 fresh keys through a 4096-slot table, SGD lr 1"""
    import torch
    from hugectr_amd import sok
    sok.init()
    var, twin = _pair(16, "11", 4096, frac)
    orc = LruTable(4096, 16, "11", 128)
    opts = [sok.OptimizerWrapper("sgd", lr=1.0) for _ in range(2)]
    for it in range(5):
        keys = torch.arange(it * 2048, (it + 1) * 2048, dtype=torch.int64, device="cuda")
        outs = []
        for v, o in zip((var, twin), opts):
            vals, ek, ev = sok.sparse_read_and_evict(v, keys)
            vals.sum().backward()
            o.step([v])
            outs.append((vals.detach(), ek, ev))
        for x, y in zip(*outs):
            assert torch_equal(x, y), it
        wv, _, ok, orow = orc.lookup(keys.cpu().numpy(), insert=True)
        sl = orc.find(keys.cpu().numpy())
        orc.rows[sl[sl >= 0]] -= np.float32(1.0)            # SGD lr 1 on loss = sum
        assert np.array_equal(outs[0][0].cpu().numpy(), wv)
        assert np.array_equal(_u64(outs[0][1]), ok) and np.array_equal(outs[0][2].cpu().numpy(),
                                                                       orow)
        _same_tables(var, twin)
        _check_oracle(var, orc)
    assert orc.size() + orc.rejected < 5 * 2048      # evictions happened


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("initializer", ["", "11"])
def test_many_calls_power_law(frac, initializer):
    """power-law keys with repeats, training and read-only lookups mixed, one call that overflows
    buckets (rejections)"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(11)
    D = 8
    var, twin = _pair(D, initializer, 1024, frac, seed=5)
    orc = LruTable(1024, D, initializer, 128, seed=5)
    for call in range(16):
        n = int(rng.integers(50, 900)) if call != 9 else 3000
        keys = (rng.zipf(1.2, size=n) + (call // 4) * 500) % 6000
        kt = torch.from_numpy(keys.astype(np.int64)).cuda()
        train = call % 3 != 2
        if train:
            a = sok.sparse_read_and_evict(var, kt)
            b = sok.sparse_read_and_evict(twin, kt)
            for x, y in zip(a, b):
                assert torch_equal(x.detach(), y.detach()), call
        else:
            a = (var.sparse_read(kt),)
            assert torch_equal(a[0], twin.sparse_read(kt)), call
        wv, _, ok, orow = orc.lookup(keys, insert=train)
        assert np.array_equal(a[0].detach().cpu().numpy(), wv), call
        if train:
            assert np.array_equal(_u64(a[1]), ok) and np.array_equal(a[2].cpu().numpy(), orow)
        _same_tables(var, twin)
        _check_oracle(var, orc)
    assert orc.rejected > 0
    var._pending.clear()
    twin._pending.clear()


def _keygrads(lens, w, G, comb):
    bag = np.repeat(np.arange(lens.size), lens)
    wt = np.ones(bag.size, dtype=np.float32) if w is None else w
    kg = G[bag] * wt[:, None]
    if comb == "mean":
        den = np.zeros(lens.size, dtype=np.float32)
        np.add.at(den, bag, wt)
        kg = kg / den[bag][:, None]
    return kg.astype(np.float32)


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
    from oracle import pyoracle as orc
    slots = orc_t.find(keys)
    live = slots >= 0
    if not live.any():
        return
    st = orc_t.states + [None, None]
    orc.update_params(np.arange(int(live.sum()) + 1), slots[live].astype(np.uint64),
                      np.ascontiguousarray(kg[live]), _opt_params(name, wrapper), orc_t.rows,
                      st[0], st[1])


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("opt_name", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("comb,weighted", [("sum", False), ("mean", True), ("mean", False)])
def test_training_bit_equal_to_the_twin(frac, opt_name, comb, weighted):
    """lookup_sparse + OptimizerWrapper.step: pooled outputs, rows and states bit-equal to the twin
    and within the existing tolerance of the oracle; one key is evicted between lookup and step"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(7)
    D = 16
    var, twin = _pair(D, "", 512, frac, seed=3)
    wrappers = [sok.OptimizerWrapper(opt_name, lr=0.05) for _ in range(2)]
    ns = {"sgd": 0, "adagrad": 1, "adam": 2}[opt_name]
    orc = LruTable(512, D, "", 128, seed=3, num_state=ns)
    for it in range(6):
        B = 64
        lens = rng.integers(1, 5, size=B)
        keys = rng.integers(0, 900, size=int(lens.sum())).astype(np.int64)
        keys[:4] = keys[4:8]                                 # duplicates inside the batch
        w = rng.random(keys.size).astype(np.float32) + 0.5 if weighted else None
        G = rng.standard_normal((B, D)).astype(np.float32)
        ids = sok.Ragged(torch.from_numpy(keys).cuda(), torch.from_numpy(lens).cuda())
        sw = sok.Ragged(torch.from_numpy(w).cuda(), torch.from_numpy(lens).cuda()) if weighted \
            else None
        outs = [sok.lookup_sparse(v, ids, sw, combiners=comb) for v in (var, twin)]
        assert torch_equal(outs[0].detach(), outs[1].detach()), it
        slots = var._lru.find(ids.values)
        h = var._lru.hbm_slots
        if frac > 0:
            assert bool((slots < h).any()) and bool((slots >= h).any())   # both tiers in use
        vec, _, _, _ = orc.lookup(keys, insert=True)
        bag = np.repeat(np.arange(B), lens)
        wt = np.ones(keys.size) if w is None else w.astype(np.float64)
        ref = np.zeros((B, D))
        np.add.at(ref, bag, vec * wt[:, None])
        if comb == "mean":
            den = np.zeros(B)
            np.add.at(den, bag, wt)
            ref /= den[:, None]
        assert np.allclose(outs[0].detach().cpu().numpy(), ref, rtol=1e-5, atol=1e-5), it
        for o in outs:
            (o * torch.from_numpy(G).cuda()).sum().backward()
        if it == 3:
            fresh = torch.arange(5000, 5400, dtype=torch.int64, device="cuda")
            e1 = sok.sparse_read_and_evict(var, fresh)[1]
            e2 = sok.sparse_read_and_evict(twin, fresh)[1]
            assert torch_equal(e1, e2)
            _, _, ok, _ = orc.lookup(fresh.cpu().numpy(), insert=True)
            assert np.isin(ok.view(np.int64), keys).any()
        for v, wr in zip((var, twin), wrappers):
            wr.step([v])
        _oracle_step(orc, keys, _keygrads(lens, w, G, comb), opt_name, wrappers[0])
        _same_tables(var, twin, states=ns)
        k, rows, sl, _ = var._lru.export(with_slots=True)
        occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
        assert np.array_equal(sl.cpu().numpy(), occ) and np.array_equal(_u64(k), orc.keys[occ])
        assert np.allclose(rows.cpu().numpy(), orc.rows[occ], rtol=1e-6, atol=1e-6), it
        for j in range(ns):
            st = var._lru.gather_slots(1 + j, sl).cpu().numpy()
            assert np.allclose(st, orc.states[j][occ], rtol=1e-6, atol=1e-6), (it, j)


class _Clock:
    def __init__(self):
        self.s = 0

    def __call__(self):
        return self.s * 1_000_000_000


@pytest.mark.parametrize("frac", FRACS)
def test_filter_and_incremental_dump(frac):
    """the low-frequency filter at p = 0.3 with SGD, and incremental_model_dump: bit-equal to the
    twin; the filter's decisions and the table match the oracle"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(3)
    D = 8
    var, twin = _pair(D, "", 512, frac, seed=2, filter_ratio=0.3)
    clocks = [_Clock(), _Clock()]
    var._lru.clock, twin._lru.clock = clocks
    orc = FilterLruTable(512, D, "", 128, seed=2)
    wrs = [sok.OptimizerWrapper("sgd", lr=0.1) for _ in range(2)]
    for it in range(6):
        for c in clocks:
            c.s = 100 + it
        lens = rng.integers(1, 4, size=48)
        keys = rng.integers(0, 1500, size=int(lens.sum())).astype(np.int64)
        ids = sok.Ragged(torch.from_numpy(keys).cuda(), torch.from_numpy(lens).cuda())
        outs = [sok.lookup_sparse(v, ids, combiners="mean", use_low_frequency_filter=True)
                for v in (var, twin)]
        assert torch_equal(outs[0].detach(), outs[1].detach()), it
        orc.lookup(keys, insert=True, admit=0.3)
        for o, v, wr in zip(outs, (var, twin), wrs):
            (o * o).sum().backward()
            wr.step([v])
        assert var._lru.filtered_count() == twin._lru.filtered_count() == orc.filtered
        _same_tables(var, twin)
        k, _, sl, sc = var._lru.export(with_slots=True)
        occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
        assert np.array_equal(sl.cpu().numpy(), occ) and np.array_equal(_u64(k), orc.keys[occ])
    th = dt.datetime.fromtimestamp(103, tz=dt.timezone.utc)
    a = sok.incremental_model_dump([var], th)
    b = sok.incremental_model_dump([twin], th)
    assert a[0][0].size > 0
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1][0], b[1][0])


@pytest.mark.parametrize("frac", FRACS)
def test_slot_addressed_writes(frac):
    """assign, scatter_add, scatter_sub, scatter_update and sparse_read on keys of both tiers"""
    import torch
    from hugectr_amd import sok
    sok.init()
    D = 8
    var, twin = _pair(D, "0.5", 512, frac, seed=1)
    rng = np.random.default_rng(2)
    keys = torch.from_numpy(rng.permutation(3000)[:600].astype(np.int64)).cuda()   # overflows
    vals = torch.from_numpy(rng.standard_normal((600, D)).astype(np.float32)).cuda()
    for v in (var, twin):
        sok.assign(v, keys, vals)
    _same_tables(var, twin)
    assert bool((var._lru.find(keys) >= var._lru.hbm_slots).any())
    sub = keys[::3]
    d = torch.from_numpy(rng.standard_normal((sub.numel(), D)).astype(np.float32)).cuda()
    for v in (var, twin):
        v.scatter_add(sub, d)
    _same_tables(var, twin)
    for v in (var, twin):
        v.scatter_sub(keys[1::5], d[:keys[1::5].numel()])
    _same_tables(var, twin)
    for v in (var, twin):
        v.scatter_update(keys[::2], vals[1::2][:keys[::2].numel()])
    _same_tables(var, twin)
    probe = torch.cat([keys, torch.arange(90000, 90050, device="cuda")])
    assert torch_equal(var.sparse_read(probe), twin.sparse_read(probe))
    k, w = sok.export(var)
    got = var.sparse_read(k)
    assert torch_equal(got, w)


@pytest.mark.parametrize("frac", FRACS)
def test_dump_and_load_with_adam_state(frac, tmp_path):
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(5)
    D = 8
    var, twin = _pair(D, "0.25", 256, frac, seed=6, name=None)
    var.name, twin.name = "tier_t", "tier_t"
    wrs = [sok.OptimizerWrapper("adam", lr=0.1) for _ in range(2)]
    for _ in range(4):
        lens = rng.integers(1, 4, size=32)
        ids = sok.Ragged(torch.from_numpy(rng.integers(0, 600, size=int(lens.sum()))).cuda(),
                         torch.from_numpy(lens).cuda())
        for v, wr in zip((var, twin), wrs):
            out = sok.lookup_sparse(v, ids, combiners="sum")
            (out * out).sum().backward()
            wr.step([v])
    _same_tables(var, twin, states=2)
    pa, pb = tmp_path / "a", tmp_path / "b"
    sok.dump(str(pa), [var], wrs[0])
    sok.dump(str(pb), [twin], wrs[1])
    names = sorted(os.listdir(pa))
    assert names == sorted(os.listdir(pb)) and len(names) >= 4
    for n in names:
        assert filecmp.cmp(pa / n, pb / n, shallow=False), n
    h = int(256 * frac)
    var2 = sok.DynamicVariable(D, "zeros", var_type="hybrid", max_capacity=256, seed=6,
                               name="tier_t", max_hbm_for_vectors=_budget(h, D))
    sok.load(str(pa), [var2], sok.OptimizerWrapper("adam", lr=0.1))
    k1, v1 = sok.export(var)
    k2, v2 = sok.export(var2)
    o1, o2 = torch.argsort(k1), torch.argsort(k2)
    assert torch.equal(k1[o1], k2[o2]) and torch.equal(v1[o1], v2[o2])
    s1 = sok._var_arrays(var, wrs[0])[2]
    s2 = sok._var_arrays(var2, wrs[0])[2]
    assert len(s1) == len(s2) == 2
    for a, b in zip(s1, s2):
        assert torch.equal(a, b)


def _worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from hugectr_amd import sok
        sok.init()
        rng = np.random.default_rng(21)
        D, B, cap = 8, 48, 256
        var, twin = _pair(D, "", cap, 0.5, seed=4)
        wrs = [sok.OptimizerWrapper("adagrad", lr=0.1) for _ in range(2)]
        for step in range(4):
            lens = rng.integers(1, 4, size=B * world)
            vals = rng.integers(0, 2000, size=int(lens.sum())).astype(np.int64)
            G = rng.standard_normal((B * world, D)).astype(np.float32)
            off = np.concatenate([[0], np.cumsum(lens)])
            sl = slice(off[rank * B], off[(rank + 1) * B])
            ids = sok.Ragged(torch.from_numpy(vals[sl]).cuda(),
                             torch.from_numpy(lens[rank * B:(rank + 1) * B]).cuda())
            outs = []
            for v, wr in zip((var, twin), wrs):
                out = sok.lookup_sparse(v, ids, combiners="mean")
                (out * torch.from_numpy(G[rank * B:(rank + 1) * B]).cuda()).sum().backward()
                wr.step([v])
                outs.append(out.detach())
            assert torch_equal(outs[0], outs[1]), step
            _same_tables(var, twin, states=1)
        assert var.size > 0
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
    port = 29500 + (os.getpid() + 1409) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    for r in range(2):
        if ret.get(r) != "ok":
            print(f"--- rank {r} ---\n{ret.get(r)}")
    assert ret.get(0) == "ok" and ret.get(1) == "ok"
