"""GPU parity: embedding_collection on HYBRID tables (storage="hybrid": one bounded LRU table,
hctr_lru_*, per local table shard, optionally tiered to host memory) -- the two new entries
(hctr_ebc_group_segments, hctr_ebc_hybrid_row_ptrs) and the gradient expansion against numpy, the
forward / backward / update against the CPU restatements the static and dynamic paths are checked
with, the table's contents against the sequential LRU oracle (tests/lru_oracle.py,
tests/lru_grow_oracle.py), the tier's invisibility, the evaluation runtime and the refusals."""
import numpy as np
import pytest

from lru_grow_oracle import GrowLruTable
from lru_oracle import EMPTY, LruTable
from util import assert_close

pytestmark = pytest.mark.gpu


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the new entries alone --------------------------------------------------------------------

def _segment_case(rng, world, n_lookups, lookup_table, n_tables, bpg, max_len, empty_prob):
    """routed bucket offsets [n_seg * bpg + 1] with whole segments empty, and the numpy grouping"""
    n_seg = world * n_lookups
    lens = rng.integers(0, max_len + 1, size=(n_seg, bpg)).astype(np.int64)
    lens[rng.random(n_seg) < empty_prob] = 0
    br = np.zeros(n_seg * bpg + 1, np.int64)
    np.cumsum(lens.reshape(-1), out=br[1:])
    seg = br[::bpg]
    seg_table = np.array([lookup_table[s % n_lookups] for s in range(n_seg)], np.int32)
    dst = np.zeros(n_seg, np.int64)
    pos = 0
    for t in range(n_tables):           # grouped order: [table][peer][lookup]
        for s in range(n_seg):
            if seg_table[s] == t:
                dst[s] = pos
                pos += seg[s + 1] - seg[s]
    nnz = int(br[-1])
    perm = np.zeros(nnz, np.int64)      # routed position -> grouped position
    for s in range(n_seg):
        perm[seg[s]:seg[s + 1]] = dst[s] + np.arange(seg[s + 1] - seg[s])
    return br, seg_table, dst, perm, nnz


@pytest.mark.parametrize("case", ["random", "empty", "one_segment"])
def test_group_segments_and_row_ptrs(case):
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.default_rng(3)
    ev, n_tables = 8, 3
    if case == "random":     # 3 tables, world 3, 5 lookups, <= 200 keys
        world, n_lookups, lookup_table, bpg = 3, 5, [0, 1, 2, 1, 0], 4
        br, seg_table, dst, perm, nnz = _segment_case(rng, world, n_lookups, lookup_table, n_tables,
                                                      bpg, 6, 0.3)
        assert 0 < nnz <= 200 and (np.diff(br[::bpg]) == 0).any()
    elif case == "empty":    # nnz = 0
        world, n_lookups, lookup_table, bpg = 3, 5, [0, 1, 2, 1, 0], 4
        br, seg_table, dst, perm, nnz = _segment_case(rng, world, n_lookups, lookup_table, n_tables,
                                                      bpg, 0, 0.0)
        assert nnz == 0
    else:                    # a single segment
        world, n_lookups, lookup_table, bpg = 1, 1, [2], 7
        br, seg_table, dst, perm, nnz = _segment_case(rng, world, n_lookups, lookup_table, n_tables,
                                                      bpg, 5, 0.0)
        assert nnz > 0 and (perm == np.arange(nnz)).all()
    n_seg = world * n_lookups
    keys = rng.integers(-(1 << 62), 1 << 62, size=nnz).astype(np.int64)
    want_keys = np.zeros(nnz, np.int64)
    want_keys[perm] = keys
    t_br, t_dst, t_tab, t_keys = _cuda(br), _cuda(dst), _cuda(seg_table), _cuda(keys)
    out_keys = torch.full((max(nnz, 1),), -7, dtype=torch.int64, device="cuda")
    check(lib.hctr_ebc_group_segments(n_seg, bpg, ptr(t_br), ptr(t_dst), ptr(t_keys), nnz,
                                      ptr(out_keys), stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(out_keys.cpu().numpy()[:nnz], want_keys)
    # row numbers in grouped order, some of them not a row of their table -> NULL
    stores = [torch.zeros((n, ev), dtype=torch.float32, device="cuda") for n in (5, 9, 3)]
    counts = np.array([s.shape[0] for s in stores], np.int64)
    bases = np.array([s.data_ptr() for s in stores], np.int64)
    table_of_grouped = np.zeros(nnz, np.int64)
    seg = br[::bpg]
    for s in range(n_seg):
        table_of_grouped[dst[s]:dst[s] + seg[s + 1] - seg[s]] = seg_table[s]
    rows = rng.integers(0, 12, size=nnz).astype(np.int64)
    if nnz:
        rows[rng.integers(0, nnz)] = -1          # SIZE_MAX: "no row"
    desc = np.stack([bases, counts], axis=1).reshape(-1)
    ptrs = torch.full((max(nnz, 1),), -7, dtype=torch.int64, device="cuda")
    perm_out = torch.full((max(nnz, 1),), -7, dtype=torch.int32, device="cuda")
    t_rows, t_desc = _cuda(rows), _cuda(desc)
    check(lib.hctr_ebc_hybrid_row_ptrs(n_seg, bpg, ptr(t_br), ptr(t_dst), ptr(t_tab), n_tables,
                                       ptr(t_desc), ev, ptr(t_rows), nnz, ptr(ptrs), ptr(perm_out),
                                       stream_ptr()))
    torch.cuda.synchronize()
    r = rows[perm]
    t = table_of_grouped[perm]
    valid = (r >= 0) & (r < counts[t]) if nnz else np.zeros(0, bool)
    want_ptrs = np.where(valid, bases[t] + r * ev * 4, 0) if nnz else np.zeros(0, np.int64)
    assert np.array_equal(ptrs.cpu().numpy()[:nnz], want_ptrs)
    assert np.array_equal(perm_out.cpu().numpy()[:nnz].astype(np.int64), perm)
    if nnz:
        assert (~valid).any() and valid.any()
    else:   # nothing was written
        assert int(ptrs[0]) == -7 and int(perm_out[0]) == -7 and int(out_keys[0]) == -7


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("ev", [10, 16, 128, 260])
def test_hybrid_key_grads(dtype, mapped, ev):
    """key_grads[perm[j]] = fp32(grad[bucket of j]), through the batch-major address when mapped;
    ev 10: the element-wise loop, 16 / 128: four elements per access, 260: more words than lanes"""
    import torch
    from hugectr_amd import _lib
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.default_rng(4)
    samples, lookups = 6, 5
    buckets = samples * lookups
    lens = rng.integers(0, 4, size=buckets).astype(np.int64)
    br = np.zeros(buckets + 1, np.int64)
    np.cumsum(lens, out=br[1:])
    nnz = int(br[-1])
    perm = rng.permutation(nnz).astype(np.int32)
    tdt = getattr(torch, dtype)
    grad = torch.randn((buckets, ev), device="cuda").to(tdt)
    kg = torch.full((nnz, ev), -7.0, dtype=torch.float32, device="cuda")
    t_br, t_perm = _cuda(br), _cuda(perm)
    code = {"float32": _lib.F32, "float16": _lib.F16, "bfloat16": _lib.BF16}[dtype]
    check(lib.hctr_ebc_hybrid_key_grads(buckets, ev, ptr(t_br), ptr(t_perm), nnz, ptr(grad), code,
                                        samples if mapped else 0, lookups if mapped else 0, ptr(kg),
                                        stream_ptr()))
    torch.cuda.synchronize()
    g = grad.float().cpu().numpy()
    bucket_of = np.repeat(np.arange(buckets), lens)
    src = (bucket_of % samples) * lookups + bucket_of // samples if mapped else bucket_of
    want = np.zeros((nnz, ev), np.float32)
    want[perm] = g[src]
    assert np.array_equal(kg.cpu().numpy(), want)


# ---- 2. forward / backward / update against the oracle ---------------------------------------------

def _make_inputs(rng, B, vocabs, lookup_table, max_hot):
    L = len(lookup_table)
    lens = rng.integers(0, max_hot + 1, size=L * B).astype(np.int64)
    lens[rng.random(L * B) < 0.15] = 0
    br = np.zeros(L * B + 1, np.int64)
    np.cumsum(lens, out=br[1:])
    keys = np.concatenate([rng.integers(0, vocabs[lookup_table[l]],
                                        size=int(lens[l * B:(l + 1) * B].sum()))
                           for l in range(L)]).astype(np.int64)
    return keys, br


VOCABS = [50, 7, 300, 12]
LOOKUP_TABLE = [0, 1, 2, 3, 2]
COMBINERS = ["sum", "mean", "sum", "mean", "mean"]
OPT_NAMES = ["sgd", "adagrad", "adam", "momentum", "nesterov"]


def _opt_code(name):
    from hugectr_amd import _lib
    return {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "adam": _lib.OPT_ADAM,
            "momentum": _lib.OPT_MOMENTUM_SGD, "nesterov": _lib.OPT_NESTEROV}[name]


def _hybrid_ranks(world, shard, opt_name, B=32, ev=16, budget=None, initializer="0.5", **extra):
    import hugectr_amd as ha
    T, L = len(VOCABS), len(LOOKUP_TABLE)
    kw = dict(var_type="hybrid", max_capacity=1024, max_bucket_size=64, initializer=initializer)
    if budget is not None:
        kw["max_hbm_for_vectors"] = budget
    tcfg = [ha.EmbeddingTableConfig(f"t{i}", -1, ev, **kw) for i in range(T)]
    cfg = ha.EmbeddingCollectionConfig()
    for l in range(L):
        cfg.embedding_lookup(tcfg[LOOKUP_TABLE[l]], f"in{l}", f"out{l}", COMBINERS[l])
    if shard == "table":
        sm = [[1 if t % world == g else 0 for t in range(T)] for g in range(world)]
    elif shard == "row":
        sm = [[1] * T for _ in range(world)]
    else:
        sm = [[1 if g == 0 else 0, 1, 1, 1 if g == world - 1 else 0] for g in range(world)]
    cfg.shard(sm)
    return [ha.EmbeddingCollection.for_rank(r, world, cfg, B, lr=0.1, optimizer=_opt_code(opt_name),
                                            scaler=2.0, epsilon=1e-6, max_hotness=4, seed=9,
                                            **extra)
            for r in range(world)]


def _step(ranks, keys, br, grads):
    """one forward + backward + update of every rank's runtime, the collectives done by hand;
    returns the ranks' outputs"""
    import torch
    world = len(ranks)
    ev, bpg = ranks[0].ev, ranks[0].bpg
    gk, gbr = _cuda(keys), _cuda(br)
    sends = [e.route_and_pool(gk, gbr) for e in ranks]
    torch.cuda.synchronize()
    outs = []
    for d_, e in enumerate(ranks):
        blocks = []
        for s, es in enumerate(ranks):
            if es.n_local:
                blocks.append(sends[s].view(world, es.n_local, bpg, ev)[d_].reshape(-1, ev))
        recv = torch.cat(blocks) if blocks else torch.empty((0, ev), device="cuda")
        outs.append(e.network_forward(recv.contiguous()))
    if grads is None:
        return outs
    bsends = [ranks[d_].network_backward(_cuda(grads[d_])) for d_ in range(world)]
    torch.cuda.synchronize()
    for s, es in enumerate(ranks):
        if es.n_local == 0:
            continue
        base = sum(ranks[0].n_local_of[:s])
        tops = [bsends[d_].view(-1, bpg, ev)[base:base + es.n_local] for d_ in range(world)]
        es.apply_gradients(torch.stack(tops).contiguous())
    torch.cuda.synchronize()
    return outs


def _oracle_update(oracle, opt_name, it, B, world, ev, comb, keys, br, row_start, dense, states,
                   grads):
    """SGD / AdaGrad: the EBC oracle.  Adam / MomentumSGD / Nesterov, which it lacks: per-key
    gradients restated here, then the CPU sparse optimizer on (flat row, gradient) pairs."""
    if opt_name in ("sgd", "adagrad"):
        oracle.ebc_backward_update(B, LOOKUP_TABLE, ev, comb, keys, br, row_start, dense,
                                   np.stack([g.reshape(-1) for g in grads]),
                                   optimizer={"sgd": 0, "adagrad": 1}[opt_name], lr=0.1, scaler=2.0,
                                   epsilon=1e-6, accum=states[0], num_gpus=world)
        return
    bpg = B // world
    L = len(LOOKUP_TABLE)
    rows, kg = [], []
    for l in range(L):
        for b in range(B):
            ks = keys[br[l * B + b]:br[l * B + b + 1]]
            g = grads[b // bpg][l, b % bpg]
            if comb[l] == 1 and ks.size > 0:
                g = g / np.float32(ks.size)
            for k in ks:
                rows.append(row_start[LOOKUP_TABLE[l]] + int(k))
                kg.append(g)
    o = oracle.OptParamsC()
    o.optimizer = {"adam": oracle.OPT_ADAM, "momentum": oracle.OPT_MOMENTUM,
                   "nesterov": oracle.OPT_NESTEROV}[opt_name]
    o.update_type, o.lr, o.beta1, o.beta2, o.epsilon = 0, 0.1, 0.9, 0.999, 1e-6
    o.momentum_factor, o.scaler, o.times, o.state_half = 0.9, 2.0, it + 1, 0
    oracle.update_params(np.arange(len(rows) + 1), np.array(rows, np.uint64),
                         np.stack(kg).astype(np.float32), o, dense, states[0],
                         states[1] if opt_name == "adam" else None)


@pytest.mark.parametrize("world,shard", [(1, "table"), (2, "table"), (4, "row"), (2, "mixed")])
@pytest.mark.parametrize("opt_name", OPT_NAMES)
def test_ebc_hybrid_forward_backward_update(oracle, world, shard, opt_name):
    B, ev = 32, 16
    T, L = len(VOCABS), len(LOOKUP_TABLE)
    rng = np.random.default_rng(world * 11 + OPT_NAMES.index(opt_name))
    ranks = _hybrid_ranks(world, shard, opt_name, B, ev)
    assert all(e.hybrid and not e.dynamic for e in ranks)
    row_start = np.concatenate([[0], np.cumsum(VOCABS)[:-1]]).astype(np.int64)
    dense = np.full((sum(VOCABS), ev), 0.5, np.float32)     # the constant initializer
    states = [np.zeros_like(dense), np.zeros_like(dense)]
    seen = [set() for _ in range(T)]
    comb = [0 if c == "sum" else 1 for c in COMBINERS]
    for it in range(3):
        keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
        for l in range(L):
            seen[LOOKUP_TABLE[l]].update(keys[br[l * B]:br[(l + 1) * B]].tolist())
        want = oracle.ebc_forward(B, LOOKUP_TABLE, ev, comb, keys, br, row_start, dense,
                                  num_gpus=world)
        shape = (L, B // world, ev)
        grads = [rng.standard_normal(shape).astype(np.float32) for _ in range(world)]
        outs = _step(ranks, keys, br, grads)
        for d_ in range(world):
            assert_close(outs[d_].cpu().numpy().reshape(-1), want[d_], 1e-5, 1e-6,
                         f"fwd rank{d_} it{it}")
        _oracle_update(oracle, opt_name, it, B, world, ev, comb, keys, br, row_start, dense, states,
                       grads)
        for t in range(T):
            owners = ranks[0].owners[t]
            for sid, g in enumerate(owners):
                k, v = ranks[g].hyb[t].export()
                k, v = k.cpu().numpy(), v.cpu().numpy()
                assert np.unique(k).size == k.size
                # exactly the keys this shard has been asked for so far
                assert set(k.tolist()) == {x for x in seen[t] if x % len(owners) == sid}
                assert_close(v, dense[row_start[t] + k], 1e-5, 1e-6,
                             f"{opt_name} table {t} shard {sid} it{it}")
    for e in ranks:
        st = e.table_stats()
        assert set(st) == {e.tables[t].name for t in e.local_tables}
        for t in e.local_tables:
            s = st[e.tables[t].name]
            assert s["size"] == e.hyb[t].size() > 0 and s["rejected"] == 0
            assert s["capacity_now"] == s["max_capacity"] == s["hbm_slots"] == 1024
            assert s["doublings"] == 0


@pytest.mark.parametrize("batch_major", [False, True])
def test_one_gpu_direct_path_on_hybrid_tables_equals_staged(monkeypatch, batch_major):
    """one GPU: pooling straight into the (batch-major) output and the gradient read in place give
    the bits of the staged route -> pool -> network_forward / network_backward path"""
    import torch
    import hugectr_amd as ha
    from hugectr_amd import _lib
    rng = np.random.default_rng(31)
    B, ev = 32, 16
    L = len(LOOKUP_TABLE)
    tcfg = [ha.EmbeddingTableConfig(f"t{i}", -1, ev, var_type="hybrid", max_capacity=1024,
                                    max_bucket_size=64) for i in range(len(VOCABS))]
    cfg = ha.EmbeddingCollectionConfig()
    for l, t in enumerate(LOOKUP_TABLE):
        cfg.embedding_lookup(tcfg[t], f"in{l}", f"out{l}", "sum")
    kw = dict(lr=0.05, optimizer=_lib.OPT_ADAM, scaler=4.0, epsilon=1e-6,
              batch_major=batch_major, max_hotness=4, seed=3,
              out_dtype=torch.float16 if batch_major else torch.float32)
    monkeypatch.setenv("HCTR_EBC_DIRECT", "0")
    staged = ha.EmbeddingCollection.for_rank(0, 1, cfg, B, **kw)
    monkeypatch.setenv("HCTR_EBC_DIRECT", "1")
    direct = ha.EmbeddingCollection.for_rank(0, 1, cfg, B, **kw)
    assert direct._direct and direct.hybrid and not staged._direct
    for step in range(3):
        keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
        kt, brt = _cuda(keys), _cuda(br)
        a, b = staged.forward(kt, brt), direct.forward(kt, brt)
        assert a.shape == b.shape and torch.equal(a, b), step
        g = torch.randn(a.shape, device="cuda").to(a.dtype)
        staged.backward_and_update(g)
        direct.backward_and_update(g)
    torch.cuda.synchronize()
    for t in range(len(VOCABS)):
        for x, y in zip(staged.hyb[t].export(with_slots=True), direct.hyb[t].export(with_slots=True)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("world,shard", [(2, "mixed"), (4, "row")])
def test_a2a_key_route_on_hybrid_tables_equals_the_gathered_route(world, shard):
    """the reference's key route (bucket lengths a2a, keys a2a; route_send / route_recv, the two
    collectives done by hand) hands every owner the keys the gathered route finds: same bucket
    ranges, keys, pooled vectors and table contents"""
    import torch
    B, ev = 32, 16
    L = len(LOOKUP_TABLE)
    a = _hybrid_ranks(world, shard, "sgd", B, ev, initializer="")   # a2a route
    g = _hybrid_ranks(world, shard, "sgd", B, ev, initializer="")   # gathered
    rng = np.random.default_rng(world)
    bpg = B // world
    for it in range(2):
        keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
        gk, gbr = _cuda(keys), _cuda(br)
        want = [e.route_and_pool(gk, gbr) for e in g]
        sends = []
        for r in range(world):      # every rank's own share, feature-major
            lens, ks = [], []
            for l in range(L):
                for b in range(r * bpg, (r + 1) * bpg):
                    q0, q1 = br[l * B + b], br[l * B + b + 1]
                    lens.append(q1 - q0)
                    ks.append(keys[q0:q1])
            lbr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            sends.append(a[r].route_send(_cuda(np.concatenate(ks).astype(np.int64)), _cuda(lbr)))
        for p in range(world):
            a[p].route_recv(torch.cat([sends[s][0][p] for s in range(world)]),
                            torch.cat([sends[s][1][p] for s in range(world)]))
            got = a[p].pool_routed()
            nb, n = a[p].nb, g[p]._nnz_host
            assert a[p]._nnz_host == n
            assert torch.equal(a[p].out_range[:nb + 1], g[p].out_range[:nb + 1])
            assert torch.equal(a[p].indices[:n], g[p].indices[:n])
            assert torch.equal(got, want[p]), f"pooled vectors rank{p}"
            for t in a[p].local_tables:
                for x, y in zip(a[p].hyb[t].export(with_slots=True),
                                g[p].hyb[t].export(with_slots=True)):
                    assert torch.equal(x, y)


# ---- 3. the tier is invisible -----------------------------------------------------------------------

@pytest.mark.parametrize("hbm_slots", [512, 0])
def test_the_tier_is_invisible(hbm_slots):
    """max_hbm_for_vectors giving H = C / 2 and H = 0 beside an untiered twin: outputs, exports
    (keys, slots, scores, rows), optimizer states and table_stats (hbm_slots aside) bit-equal"""
    import torch
    B, ev, world = 32, 16, 2
    L = len(LOOKUP_TABLE)
    budget = hbm_slots * ev * 4 / 2**30
    tiered = _hybrid_ranks(world, "mixed", "adam", B, ev, budget=budget, initializer="")
    twin = _hybrid_ranks(world, "mixed", "adam", B, ev, initializer="")
    rng = np.random.default_rng(17)
    for it in range(3):
        keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
        grads = [rng.standard_normal((L, B // world, ev)).astype(np.float32) for _ in range(world)]
        a, b = _step(tiered, keys, br, grads), _step(twin, keys, br, grads)
        for x, y in zip(a, b):
            assert torch.equal(x, y), it
    for e, f in zip(tiered, twin):
        sa, sb = e.table_stats(), f.table_stats()
        for name in sa:
            assert sa[name].pop("hbm_slots") == hbm_slots and sb[name].pop("hbm_slots") == 1024
        assert sa == sb
        for t in e.local_tables:
            assert e.hyb[t].tiered and not f.hyb[t].tiered
            xa, xb = e.hyb[t].export(with_slots=True), f.hyb[t].export(with_slots=True)
            assert xa[0].numel() > 0
            for x, y in zip(xa, xb):
                assert torch.equal(x, y)
            for j in (1, 2):    # Adam's two states, at the slot numbers
                assert torch.equal(e.hyb[t].gather_slots(j, xa[2]), f.hyb[t].gather_slots(j, xb[2]))
                assert float(e.hyb[t].gather_slots(j, xa[2]).abs().sum()) > 0


# ---- 4. eviction and growth through the collection --------------------------------------------------

def _two_table_collection(B, ev, hot, **table_kw):
    import hugectr_amd as ha
    from hugectr_amd import _lib
    tcfg = [ha.EmbeddingTableConfig(f"t{i}", -1, ev, var_type="hybrid", **table_kw)
            for i in range(2)]
    cfg = ha.EmbeddingCollectionConfig()
    for l, t in enumerate([0, 1, 0]):
        cfg.embedding_lookup(tcfg[t], f"in{l}", f"out{l}", "sum")
    cfg.shard([[1, 1]])
    return ha.EmbeddingCollection.for_rank(0, 1, cfg, B, lr=0.1, optimizer=_lib.OPT_SGD,
                                           max_hotness=hot, seed=2)


def _u64(t):
    return t.cpu().numpy().astype(np.int64).view(np.uint64)


def _check_against_lru_oracle(e, orcs, what):
    for t, orc in enumerate(orcs):
        k, rows, sl, sc = e.hyb[t].export(with_slots=True)
        occ = np.nonzero(orc.keys != np.uint64(EMPTY))[0]
        assert np.array_equal(sl.cpu().numpy(), occ), what
        assert np.array_equal(_u64(k), orc.keys[occ]), what
        assert np.array_equal(sc.cpu().numpy().astype(np.uint64), orc.scores[occ]), what
        assert_close(rows.cpu().numpy(), orc.rows[occ], 1e-5, 1e-6, f"{what} table {t}")
        st = e.table_stats()[f"t{t}"]
        assert st["size"] == orc.size() and st["rejected"] == orc.rejected, what
        assert st["capacity_now"] == orc.C and st["doublings"] == getattr(orc, "doublings", 0), what


def _lru_step(e, orcs, lookup_table, B, ev, key_sets, rng, what):
    """one step: lookup l reads key_sets[l] (one key per bucket, the first buckets), summed; the
    oracle gets each table's keys in one inserting call and the SGD step restated in numpy"""
    L = len(lookup_table)
    lens = np.zeros(L * B, np.int64)
    for l, ks in enumerate(key_sets):
        per = -(-len(ks) // B) if len(ks) else 0
        full, rest = divmod(len(ks), max(per, 1)) if per else (0, 0)
        lens[l * B:l * B + full] = per
        if rest:
            lens[l * B + full] = rest
    br = np.zeros(L * B + 1, np.int64)
    np.cumsum(lens, out=br[1:])
    keys = np.concatenate(key_sets).astype(np.int64)
    out = e.forward(_cuda(keys), _cuda(br))
    grad = rng.standard_normal((L, B, ev)).astype(np.float32)
    want = np.zeros((L, B, ev), np.float32)
    per_table = [[] for _ in orcs]
    for l in range(L):
        per_table[lookup_table[l]].append(keys[br[l * B]:br[(l + 1) * B]])
    vec_of = {}
    slots_of = []
    for t, orc in enumerate(orcs):
        ks = np.concatenate(per_table[t])
        vec, slots, _, _ = orc.lookup(ks, insert=True)
        slots_of.append(dict(zip(ks.tolist(), slots.tolist())))
        for k, v in zip(ks.tolist(), vec):
            vec_of[(t, k)] = v
    gsum = {}
    for l in range(L):
        t = lookup_table[l]
        for b in range(B):
            for k in keys[br[l * B + b]:br[l * B + b + 1]].tolist():
                want[l, b] += vec_of[(t, k)]
                gsum[(t, k)] = gsum.get((t, k), np.zeros(ev, np.float32)) + grad[l, b]
    assert_close(out.cpu().numpy(), want, 1e-5, 1e-6, f"{what} forward")
    e.backward_and_update(_cuda(grad))
    for (t, k), g in gsum.items():      # SGD; a rejected key has no slot and gets no gradient
        s = slots_of[t][k]
        if s >= 0:
            orcs[t].rows[s] = (orcs[t].rows[s] - np.float32(0.1) * g).astype(np.float32)
    _check_against_lru_oracle(e, orcs, what)


def test_eviction_and_growth_through_the_collection():
    """2 tables of max_capacity 128 in buckets of 64, starting at 64 slots; 8 steps of <= 40 distinct
    fresh keys per table out of 10^4: the tables double, then evict, and every step's export equals
    the sequential oracle fed the same per-table key sets, one inserting call per step"""
    B, ev = 16, 8
    e = _two_table_collection(B, ev, 3, max_capacity=128, init_capacity=64, max_bucket_size=64)
    orcs = [GrowLruTable(64, 128, ev, "", 64, seed=2 * 1000003 + t) for t in range(2)]
    rng = np.random.default_rng(12)
    evicted = 0
    for step in range(8):
        pools = [rng.choice(10000, size=40, replace=False).astype(np.int64) for _ in range(2)]
        # table 0 is read by lookups 0 and 2 (a few keys in both), table 1 by lookup 1
        key_sets = [pools[0][:25], pools[1], pools[0][20:]]
        before = [set(o.where) for o in orcs]
        _lru_step(e, orcs, [0, 1, 0], B, ev, key_sets, rng, f"step {step}")
        evicted += sum(len(b - set(o.where)) for b, o in zip(before, orcs))
    assert evicted > 0                                         # on the oracle alone
    assert all(o.doublings == 1 and o.C == 128 and o.rejected == 0 for o in orcs)


def test_rejected_keys_read_the_initializer_and_get_no_gradient():
    """>= 65 fresh keys of ONE bucket in one call: the bucket's 64 slots fill, the other keys are
    rejected -- they read the initializer's value, get no gradient and are counted"""
    B, ev = 16, 8
    e = _two_table_collection(B, ev, 6, max_capacity=128, max_bucket_size=64)
    orcs = [LruTable(128, ev, "", 64, seed=2 * 1000003 + t) for t in range(2)]
    one_bucket = np.array([k for k in range(4000) if orcs[0].bucket(k) == 1][:70], np.int64)
    assert one_bucket.size == 70
    rng = np.random.default_rng(1)
    _lru_step(e, orcs, [0, 1, 0], B, ev, [one_bucket, np.arange(5, dtype=np.int64),
                                          one_bucket[:3]], rng, "overflow")
    assert orcs[0].rejected == 6 and orcs[1].rejected == 0
    assert e.table_stats()["t0"]["rejected"] == 6
    # the same keys again: the stored ones are found, the rejected ones try again and fail again
    _lru_step(e, orcs, [0, 1, 0], B, ev, [one_bucket, np.arange(5, dtype=np.int64),
                                          one_bucket[60:]], rng, "again")
    assert orcs[0].rejected == 12


# ---- 5. the evaluation runtime ------------------------------------------------------------------------

def test_eval_runtime_never_inserts():
    """tables_from= shares the tables; an evaluation lookup inserts nothing, changes no score and
    reads the initializer's value for a key the table does not hold"""
    import torch
    import hugectr_amd as ha
    from hugectr_amd import _lib
    B, ev = 16, 8
    e = _two_table_collection(B, ev, 3, max_capacity=128, max_bucket_size=64)
    cfg_tables = e.tables
    cfg = ha.EmbeddingCollectionConfig()
    for l, t in enumerate([0, 1, 0]):
        cfg.embedding_lookup(cfg_tables[t], f"in{l}", f"out{l}", "sum")
    cfg.shard([[1, 1]])
    ev_rt = ha.EmbeddingCollection.for_rank(0, 1, cfg, 8, lr=0.1, optimizer=_lib.OPT_SGD,
                                            max_hotness=3, seed=2, tables_from=e)
    ev_rt.training = False
    assert ev_rt.hyb is e.hyb
    orcs = [LruTable(128, ev, "", 64, seed=2 * 1000003 + t) for t in range(2)]
    rng = np.random.default_rng(6)
    _lru_step(e, orcs, [0, 1, 0], B, ev, [np.arange(10, dtype=np.int64),
                                          np.arange(100, 112, dtype=np.int64),
                                          np.arange(5, 15, dtype=np.int64)], rng, "train")
    before = [[x.clone() for x in e.hyb[t].export(with_slots=True)] for t in range(2)]
    # batch 8, one key per bucket: stored keys (3, 104) and unseen ones (777, 888)
    keys = np.array([3, 777, 1, 2, 4, 5, 6, 7,
                     104, 888, 100, 101, 102, 103, 105, 106,
                     777, 3, 8, 9, 10, 11, 12, 13], np.int64)
    br = np.arange(25, dtype=np.int64)
    out = ev_rt.forward(_cuda(keys), _cuda(br)).cpu().numpy()
    for l, t in enumerate([0, 1, 0]):
        vec, slots, _, _ = orcs[t].lookup(keys[l * 8:(l + 1) * 8], insert=False)
        assert np.array_equal(out[l], vec)
    assert np.array_equal(out[0, 1], orcs[0].init(777)) and np.array_equal(out[1, 1], orcs[1].init(888))
    for t in range(2):
        for x, y in zip(before[t], e.hyb[t].export(with_slots=True)):
            assert torch.equal(x, y)
        assert e.hyb[t].find(_cuda(np.array([777, 888], np.int64))).tolist() == [-1, -1]


# ---- 6. refusals ------------------------------------------------------------------------------------

def _refusal_config(ev=8, n=2):
    import hugectr_amd as ha
    tcfg = [ha.EmbeddingTableConfig(f"big{i}", -1, ev, var_type="hybrid", max_capacity=256)
            for i in range(n)]
    cfg = ha.EmbeddingCollectionConfig()
    for i, t in enumerate(tcfg):
        cfg.embedding_lookup(t, f"in{i}", f"out{i}", "sum")
    return cfg


def test_unique_on_two_gpus_is_refused():
    import hugectr_amd as ha
    cfg = _refusal_config()
    cfg.shard([[1, 1], [1, 1]], "mp", [("Unique", ["big0", "big1"])])
    with pytest.raises(RuntimeError, match=r"Unique.*big0.*big1.*hybrid"):
        ha.EmbeddingCollection.for_rank(0, 2, cfg, 8)
    # one GPU: nothing travels, the ordinary path serves the request
    cfg1 = _refusal_config()
    cfg1.shard([[1, 1]], "mp", [("Unique", ["big0", "big1"])])
    e = ha.EmbeddingCollection.for_rank(0, 1, cfg1, 8)
    assert e.hybrid and not e._unique


@pytest.mark.parametrize("name", ["Ftrl", "RMSProp"])
def test_unsupported_optimizers_are_refused(name):
    import hugectr_amd as ha
    from hugectr_amd import _lib
    code = {"Ftrl": _lib.OPT_FTRL, "RMSProp": _lib.OPT_RMSPROP}[name]
    with pytest.raises(RuntimeError, match=rf"{name}.*hybrid.*SGD, AdaGrad, Adam, MomentumSGD, Nesterov"):
        ha.EmbeddingCollection.for_rank(0, 1, _refusal_config(), 8, optimizer=code)


def test_more_than_2_24_keys_per_call_is_refused():
    import hugectr_amd as ha
    with pytest.raises(RuntimeError, match=r"big0.*keys in one call.*2\^24"):
        ha.EmbeddingCollection.for_rank(0, 1, _refusal_config(), 1 << 16, hotness=[257, 1])
    with pytest.raises(RuntimeError, match=r"2\^24"):
        ha.EmbeddingCollection.for_rank(0, 1, _refusal_config(), 1 << 16, max_hotness=257)
    e = ha.EmbeddingCollection.for_rank(0, 1, _refusal_config(), 16, hotness=[256, 1])
    assert e.hybrid


# ---- 7. sharding does not show in a key's first vector; the eval runtime of a mixed dynamic group ----

def test_initial_vectors_do_not_depend_on_the_sharding():
    """key-dependent initializer, fresh keys, one key per bucket: a 1-rank collection and a 4-rank
    row-sharded one give the same bits -- the table seed is a function of (collection seed, table
    position), never of the rank"""
    import torch
    B, ev = 32, 16
    L = len(LOOKUP_TABLE)
    one = _hybrid_ranks(1, "table", "sgd", B, ev, initializer="")
    four = _hybrid_ranks(4, "row", "sgd", B, ev, initializer="")
    rng = np.random.default_rng(21)
    keys = rng.integers(0, 1 << 40, size=L * B).astype(np.int64)
    br = np.arange(L * B + 1, dtype=np.int64)
    a = _step(one, keys, br, None)[0]                       # [L, B, ev]
    b = torch.cat(_step(four, keys, br, None), dim=1)       # ranks hold consecutive samples
    assert torch.equal(a, b)
    assert a.unique().numel() > L * B                       # not a constant
    rows = {}
    for e in four:          # every stored (table, key) -> row equals the 1-rank table's
        for t, tab in e.hyb.items():
            k, r = tab.export()
            rows.update({(t, int(x)): y.tobytes() for x, y in zip(k.cpu().numpy(), r.cpu().numpy())})
    want = {}
    for t, tab in one[0].hyb.items():
        k, r = tab.export()
        want.update({(t, int(x)): y.tobytes() for x, y in zip(k.cpu().numpy(), r.cpu().numpy())})
    assert rows == want


def test_eval_runtime_of_a_dynamic_group_that_holds_a_static_table():
    """tables_from= on a dynamic collection one of whose tables has a vocabulary (a mixed config's
    non-hybrid group): the evaluation runtime shares the table and reads what training stored"""
    import torch
    import hugectr_amd as ha
    tcfg = [ha.EmbeddingTableConfig("s", 40, 8), ha.EmbeddingTableConfig("d", -1, 8)]
    cfg = ha.EmbeddingCollectionConfig()
    for i, t in enumerate(tcfg):
        cfg.embedding_lookup(t, f"in{i}", f"out{i}", "sum")
    cfg.shard([[1, 1]])
    kw = dict(max_hotness=1, initializer="0.5", init_capacity=16)
    train = ha.EmbeddingCollection.for_rank(0, 1, cfg, 8, **kw)
    ev_rt = ha.EmbeddingCollection.for_rank(0, 1, cfg, 4, tables_from=train, **kw)
    ev_rt.training = False
    assert train.dynamic and ev_rt.det is train.det
    keys = np.arange(16, dtype=np.int64)
    out = train.forward(_cuda(keys), _cuda(np.arange(17, dtype=np.int64)))
    assert torch.equal(out, torch.full_like(out, 0.5))
    got = ev_rt.forward(_cuda(np.array([0, 1, 2, 99, 8, 9, 10, 99], np.int64)),
                        _cuda(np.arange(9, dtype=np.int64)))
    want = torch.full_like(got, 0.5)
    want[0, 3] = want[1, 3] = 0.0            # unseen keys read zeros on dynamic tables
    assert torch.equal(got, want)
