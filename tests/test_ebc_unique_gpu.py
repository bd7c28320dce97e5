"""GPU parity: CompressionStrategy.Unique of embedding_collection on several GPUs (distinct rows
travel once per destination, the receiver pools, per-row gradient sums travel back;
hugectr_amd/csrc/ebc_unique.hip) against the CPU oracle of the embedding_collection path, which
knows nothing of compression, and against the Reduction operator on the same tables.  All ranks are
played in one process (EmbeddingCollection.for_rank), the collectives emulated by slicing; the last
tests run two processes on one GPU over gloo."""
import os

import numpy as np
import pytest

import ebc_unique_oracle as uo
from util import assert_close

pytestmark = pytest.mark.gpu

VOCABS = [50, 7, 300, 12]
LOOKUP_TABLE = [0, 1, 2, 3, 2]       # two lookups share table 2
COMBINERS = ["sum", "mean", "sum", "mean", "mean"]


def _make_inputs(rng, B, vocabs, lookup_table, max_hot, one_hot=False):
    L = len(lookup_table)
    if one_hot:
        lens = np.ones(L * B, np.int64)
    else:
        lens = rng.integers(0, max_hot + 1, size=L * B).astype(np.int64)
        lens[rng.random(L * B) < 0.15] = 0
    br = np.zeros(L * B + 1, np.int64)
    np.cumsum(lens, out=br[1:])
    keys = np.concatenate([rng.integers(0, vocabs[lookup_table[l]], size=int(lens[l * B:(l + 1) * B].sum()))
                           for l in range(L)]).astype(np.int64)
    return keys, br


def _powerlaw(rng, n, vocab, alpha):
    """the reference's inverse-CDF key generator (data_generator.hpp:108-129)"""
    u = rng.random(n, dtype=np.float32).astype(np.float64)
    a = 1.0 - alpha
    y = ((float(vocab) ** a - 1.0) * u + 1.0) ** (1.0 / a)
    return np.clip(np.round(y) - 1, 0, vocab - 1).astype(np.int64)


def _shard_matrix(shard, world, T):
    if shard == "table":
        return [[1 if t % world == g else 0 for t in range(T)] for g in range(world)]
    if shard == "row":
        return [[1] * T for _ in range(world)]
    # table 0 and 3 table-wise, 1 and 2 row-wise over all ranks
    return [[1 if g == 0 else 0, 1, 1, 1 if g == world - 1 else 0] for g in range(world)]


def _config(ha, hugectr, world, shard, strategy, ev=16, vocabs=VOCABS, lookup_table=LOOKUP_TABLE,
            combiners=COMBINERS):
    tcfg = [ha.EmbeddingTableConfig(f"t{i}", v, ev) for i, v in enumerate(vocabs)]
    cfg = ha.EmbeddingCollectionConfig()
    for l, t in enumerate(lookup_table):
        cfg.embedding_lookup(tcfg[t], f"in{l}", f"out{l}", combiners[l])
    comp = None
    if strategy is not None:
        comp = [(getattr(hugectr.CompressionStrategy, strategy), [t.name for t in tcfg])]
    cfg.shard(_shard_matrix(shard, world, len(vocabs)), "mp", comp)
    return cfg


def _unique_forward(ranks, gk, gbr):
    """every rank's owner stage, the three all-to-alls emulated by slicing, the receiver stage"""
    import torch
    world = len(ranks)
    pk = [e.route_and_compress(gk, gbr) for e in ranks]
    outs = []
    for d, e in enumerate(ranks):
        rows, ridx, lens, u = [], [], [], []
        for s, es in enumerate(ranks):
            p = pk[s]
            uoff = np.concatenate([[0], np.cumsum(p["u_counts"])])
            koff = np.concatenate([[0], np.cumsum(p["k_counts"])])
            nbp = es.n_local * es.bpg
            rows.append(p["rows"][uoff[d]:uoff[d + 1]])
            ridx.append(p["ridx"][koff[d]:koff[d + 1]])
            lens.append(p["lens"][d * nbp:(d + 1) * nbp])
            u.append(p["u_counts"][d])
        outs.append(e.network_forward_unique(torch.cat(rows), torch.cat(ridx), torch.cat(lens), u))
    counts = [[list(p["u_counts"]) for p in pk], [list(p["k_counts"]) for p in pk]]
    assert world == len(outs)
    return counts, outs


def _unique_backward(ranks, counts, grads):
    """receiver sums, the variable all-to-all with the counts transposed, the owners' update"""
    import torch
    world = len(ranks)
    u = counts[0]  # u[owner][destination]
    sums = [ranks[d].network_backward_unique(grads[d]) for d in range(world)]
    for s, es in enumerate(ranks):
        parts = []
        for d in range(world):
            off = sum(u[o][d] for o in range(s))
            parts.append(sums[d][off:off + u[s][d]])
        es.apply_row_sums(torch.cat(parts).contiguous())
    return sums


def _reduction_step(ranks, gk, gbr, grads_of):
    """the Reduction operator driven as tests/test_ebc_gpu.py drives it"""
    import torch
    world, ev, bpg = len(ranks), ranks[0].ev, ranks[0].bpg
    sends = [e.route_and_pool(gk, gbr) for e in ranks]
    outs = []
    for d, e in enumerate(ranks):
        blocks = [sends[s].view(world, es.n_local, bpg, ev)[d].reshape(-1, ev)
                  for s, es in enumerate(ranks) if es.n_local]
        outs.append(e.network_forward(torch.cat(blocks).contiguous()))
    if grads_of is None:
        return outs
    grads = grads_of(outs)
    bsends = [ranks[d].network_backward(grads[d]) for d in range(world)]
    for s, es in enumerate(ranks):
        if es.n_local == 0:
            continue
        base = sum(ranks[0].n_local_of[:s])
        tops = [bsends[d].view(-1, bpg, ev)[base:base + es.n_local] for d in range(world)]
        es.apply_gradients(torch.stack(tops).contiguous())
    return outs


def _dense_from_shards(ranks, vocabs, ev):
    row_start = np.concatenate([[0], np.cumsum(vocabs)[:-1]]).astype(np.int64)
    dense = np.zeros((sum(vocabs), ev), np.float32)
    for t in range(len(vocabs)):
        owners = ranks[0].owners[t]
        for sid, g in enumerate(owners):
            e = ranks[g]
            s0 = e.row_start_of_table[t]
            ks = np.arange(sid, vocabs[t], len(owners))
            dense[row_start[t] + ks] = e.table[s0:s0 + ks.size].cpu().numpy()
    return row_start, dense


# ---- 1. the plan ------------------------------------------------------------------------------------
def _run_plan(torch, _lib, br, rows, world, bpp, positions, max_row):
    d_br = torch.from_numpy(br).cuda()
    d_rows = torch.from_numpy(rows.astype(np.uint64).view(np.int64)).cuda()
    urow = torch.full((max(positions, 1),), -1, dtype=torch.int64, device="cuda")
    ridx = torch.full((max(positions, 1),), -1, dtype=torch.int32, device="cuda")
    peer_off = torch.full((world + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(_lib.lib.hctr_ebc_uniq_plan_workspace_bytes(positions), dtype=torch.uint8,
                     device="cuda")
    _lib.check(_lib.lib.hctr_ebc_uniq_plan(positions, world, bpp, _lib.ptr(d_br), _lib.ptr(d_rows),
                                           max_row, _lib.ptr(urow), _lib.ptr(peer_off),
                                           _lib.ptr(ridx), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    return (urow.cpu().numpy().view(np.uint64), peer_off.cpu().numpy(),
            ridx.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("big_rows", [False, True])
def test_plan_equals_the_numpy_statement(world, big_rows):
    """urow / peer_off / ridx of hctr_ebc_uniq_plan equal the oracle exactly: ragged buckets with
    empty ones, row numbers beyond 2^31 handed straight to the entry (no table of that size is
    allocated), padding behind the live keys, a peer without keys"""
    import torch
    from hugectr_amd import _lib
    rng = np.random.default_rng(3 * world + big_rows)
    bpp = 3 * 8                                   # 3 local lookups x 8 samples per peer
    lens = rng.integers(0, 6, size=world * bpp).astype(np.int64)
    lens[rng.random(lens.size) < 0.3] = 0
    lens[bpp:2 * bpp] = 0                         # peer 1 gets no key at all
    br = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=br[1:])
    nnz = int(br[-1])
    max_row = 0xFFFFFFEF if big_rows else 40
    if big_rows:  # a few distinct values on both sides of 2^31, repeated
        pool = np.array([5, 2**31 - 1, 2**31, 2**31 + 7, 2**32 - 17, 3 * 2**30], np.uint64)
        rows = pool[rng.integers(0, pool.size, nnz)]
    else:
        rows = rng.integers(0, max_row + 1, nnz).astype(np.uint64)
    want_u, want_off, want_idx = uo.plan(br, rows, world, bpp)
    for pad in (0, 37):  # positions = a host upper bound of the key count
        padded = np.concatenate([rows, np.full(pad, 123456789, np.uint64)])
        urow, peer_off, ridx = _run_plan(torch, _lib, br, padded, world, bpp, nnz + pad, max_row)
        assert (peer_off == want_off).all(), (peer_off, want_off)
        assert (urow[:want_off[-1]] == want_u).all()
        assert (ridx[:nnz] == want_idx).all()
        for p in range(world):  # the whole claim about bytes: exact distinct counts
            seg = rows[br[p * bpp]:br[(p + 1) * bpp]]
            assert peer_off[p + 1] - peer_off[p] == np.unique(seg).size


@pytest.mark.parametrize("world,shard", [(2, "table"), (4, "row"), (2, "mixed")])
def test_plan_of_a_collection_counts_distinct_rows_per_destination(world, shard):
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    rng = np.random.default_rng(world)
    B = 32
    cfg = _config(ha, hugectr, world, shard, "Unique")
    ranks = [ha.EmbeddingCollection.for_rank(r, world, cfg, B, max_hotness=4) for r in range(world)]
    keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
    gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
    for e in ranks:
        p = e.route_and_compress(gk, gbr)
        nbp = e.n_local * e.bpg
        rng_h = e.out_range[:e.nb + 1].cpu().numpy()
        nnz = int(rng_h[-1])
        rows_h = e.indices[:nnz].cpu().numpy().view(np.uint64)
        want_u, want_off, want_idx = uo.plan(rng_h, rows_h, world, nbp)
        assert (e.peer_off.cpu().numpy() == want_off).all()
        assert (e.urow[:want_off[-1]].cpu().numpy().view(np.uint64) == want_u).all()
        assert (e.ridx[:nnz].cpu().numpy().view(np.uint32) == want_idx).all()
        for d in range(world):
            seg = rows_h[rng_h[d * nbp]:rng_h[(d + 1) * nbp]]
            assert p["u_counts"][d] == len(np.unique(seg)) and p["k_counts"][d] == seg.size
        # the gathered rows are the table's rows in the vector type
        got = p["rows"].cpu().numpy()
        assert (got == e.table[torch.from_numpy(want_u.view(np.int64)).cuda()].cpu().numpy()).all()


# ---- 2. forward / backward / update against the oracle ----------------------------------------------
@pytest.mark.parametrize("world,shard", [(2, "table"), (4, "row"), (2, "mixed")])
@pytest.mark.parametrize("batch_major", [False, True])
@pytest.mark.parametrize("opt_name", ["sgd", "adagrad", "ftrl"])
def test_unique_forward_backward_update(oracle, world, shard, batch_major, opt_name):
    _oracle_case(oracle, world, shard, batch_major, opt_name, 16)


@pytest.mark.parametrize("world,shard", [(4, "row"), (2, "mixed")])
@pytest.mark.parametrize("batch_major", [False, True])
@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
def test_unique_vector_size_off_the_16_byte_path(oracle, world, shard, batch_major, opt_name):
    """ev = 6: the element-wise gather and receiver kernels and the updater's generic reduce"""
    _oracle_case(oracle, world, shard, batch_major, opt_name, 6)


def _oracle_case(oracle, world, shard, batch_major, opt_name, ev):
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    rng = np.random.default_rng(world * 7 + (1 if batch_major else 0))
    B = 32
    T = len(VOCABS)
    cfg = _config(ha, hugectr, world, shard, "Unique", ev)
    opt = {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "ftrl": _lib.OPT_FTRL}[opt_name]
    ftrl = (0.02, 0.05, 0.3)
    ranks = [ha.EmbeddingCollection.for_rank(r, world, cfg, B, lr=0.1, optimizer=opt, scaler=2.0,
                                             epsilon=1e-6, batch_major=batch_major, max_hotness=4,
                                             ftrl=ftrl)
             for r in range(world)]
    assert all(e._unique for e in ranks)
    row_start, dense = _dense_from_shards(ranks, VOCABS, ev)
    accum, ftrl_z = np.zeros_like(dense), np.zeros_like(dense)
    comb = [0 if c == "sum" else 1 for c in COMBINERS]
    for it in range(2):
        keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
        gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
        counts, outs = _unique_forward(ranks, gk, gbr)
        want = oracle.ebc_forward(B, LOOKUP_TABLE, ev, comb, keys, br, row_start, dense,
                                  num_gpus=world, batch_major=batch_major)
        for d in range(world):
            assert_close(outs[d].cpu().numpy().reshape(-1), want[d], 1e-5, 1e-6, f"fwd rank{d}")
        grads = [rng.standard_normal(outs[d].shape).astype(np.float32) for d in range(world)]
        _unique_backward(ranks, counts, [torch.from_numpy(g).cuda() for g in grads])
        torch.cuda.synchronize()
        oracle.ebc_backward_update(B, LOOKUP_TABLE, ev, comb, keys, br, row_start, dense,
                                   np.stack([g.reshape(-1) for g in grads]),
                                   optimizer={"sgd": 0, "adagrad": 1, "ftrl": 2}[opt_name], lr=0.1,
                                   scaler=2.0, epsilon=1e-6, accum=accum, num_gpus=world,
                                   batch_major=batch_major, ftrl=ftrl, ftrl_z=ftrl_z)
        for t in range(T):
            owners = ranks[0].owners[t]
            for sid, g in enumerate(owners):
                e = ranks[g]
                s0 = e.row_start_of_table[t]
                ks = np.arange(sid, VOCABS[t], len(owners))
                assert_close(e.table[s0:s0 + ks.size].cpu().numpy(), dense[row_start[t] + ks],
                             1e-5, 1e-6, f"table {t} shard {sid} it{it}")


@pytest.mark.parametrize("world", [2, 4])
def test_unique_power_law_keys_take_the_split_path_of_the_backward(oracle, world):
    """one table of 10^5 rows, B = 4096, power-law keys (alpha = 1.1): a median of one position
    per row next to a row with hundreds per destination, whose sum the segmented reduce of the
    backward splits over several lane groups (tiles of 32 positions, partials added in tile order)"""
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    rng = np.random.default_rng(0)
    B, ev, V, max_hot = 4096, 16, 100000, 8
    vocabs, lookup_table, combiners = [V], [0], ["sum"]
    lens = rng.integers(0, max_hot + 1, size=B).astype(np.int64)
    lens[rng.random(B) < 0.15] = 0
    br = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=br[1:])
    keys = _powerlaw(rng, int(br[-1]), V, 1.1)
    bpg = B // world
    heaviest = min(np.bincount(keys[br[d * bpg]:br[(d + 1) * bpg]]).max() for d in range(world))
    print(f"keys {keys.size}, distinct {np.unique(keys).size}, heaviest row per destination >= {heaviest}")
    assert heaviest >= 200  # 128 positions is the longest chunk one lane group may sum alone
    cfg = _config(ha, hugectr, world, "row", "Unique", ev, vocabs, lookup_table, combiners)
    ranks = [ha.EmbeddingCollection.for_rank(r, world, cfg, B, lr=0.1, optimizer=_lib.OPT_SGD,
                                             scaler=2.0, max_hotness=max_hot) for r in range(world)]
    row_start, dense = _dense_from_shards(ranks, vocabs, ev)
    gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
    counts, outs = _unique_forward(ranks, gk, gbr)
    want = oracle.ebc_forward(B, lookup_table, ev, [0], keys, br, row_start, dense, num_gpus=world)
    for d in range(world):
        assert_close(outs[d].cpu().numpy().reshape(-1), want[d], 1e-5, 1e-6, f"fwd rank{d}")
    grads = [rng.standard_normal(outs[d].shape).astype(np.float32) for d in range(world)]
    _unique_backward(ranks, counts, [torch.from_numpy(g).cuda() for g in grads])
    oracle.ebc_backward_update(B, lookup_table, ev, [0], keys, br, row_start, dense,
                               np.stack([g.reshape(-1) for g in grads]), optimizer=0, lr=0.1,
                               scaler=2.0, epsilon=1e-6, accum=np.zeros_like(dense), num_gpus=world)
    for sid, e in enumerate(ranks):
        ks = np.arange(sid, V, world)
        assert_close(e.table[:ks.size].cpu().numpy(), dense[ks], 1e-5, 1e-6, f"shard {sid}")


# ---- 3. against the Reduction operator on the same tables -------------------------------------------
def _twins(ha, hugectr, world, shard, B, **kw):
    uq = [ha.EmbeddingCollection.for_rank(r, world, _config(ha, hugectr, world, shard, "Unique"),
                                          B, **kw) for r in range(world)]
    rd = [ha.EmbeddingCollection.for_rank(r, world, _config(ha, hugectr, world, shard, "Reduction"),
                                          B, **kw) for r in range(world)]
    assert all(e._unique for e in uq) and not any(e._unique for e in rd)
    for a, b in zip(uq, rd):
        if a.table is not None:
            assert a.table.data_ptr() != b.table.data_ptr()
            a.table.copy_(b.table)
    return uq, rd


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("world,shard", [(2, "table"), (4, "row"), (2, "mixed")])
def test_unique_one_hot_forward_equals_reduction_bit_for_bit(world, shard, dtype):
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    rng = np.random.default_rng(11)
    B = 32
    uq, rd = _twins(ha, hugectr, world, shard, B, out_dtype=getattr(torch, dtype), max_hotness=1,
                    batch_major=True)
    keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 1, one_hot=True)
    gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
    _, outs = _unique_forward(uq, gk, gbr)
    want = _reduction_step(rd, gk, gbr, None)
    for d in range(world):
        assert torch.equal(outs[d], want[d]), f"rank {d}"


@pytest.mark.parametrize("world,shard", [(2, "table"), (4, "row"), (2, "mixed")])
@pytest.mark.parametrize("opt_name", ["sgd", "adagrad"])
def test_unique_multi_hot_equals_reduction_within_tolerance(world, shard, opt_name):
    """the association of the gradient sums differs (per destination first, then across
    destinations), so tables agree to the oracle tolerance, not bit for bit"""
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    rng = np.random.default_rng(13 + world)
    B = 32
    opt = {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD}[opt_name]
    uq, rd = _twins(ha, hugectr, world, shard, B, lr=0.1, optimizer=opt, scaler=2.0, epsilon=1e-6,
                    max_hotness=4)
    for it in range(2):
        keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
        gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
        counts, outs = _unique_forward(uq, gk, gbr)
        grads = [torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float32)).cuda()
                 for o in outs]
        want = _reduction_step(rd, gk, gbr, lambda _: grads)
        for d in range(world):
            assert_close(outs[d].cpu().numpy().reshape(-1), want[d].cpu().numpy().reshape(-1),
                         1e-5, 1e-6, f"fwd rank{d} it{it}")
        _unique_backward(uq, counts, grads)
        for r, (a, b) in enumerate(zip(uq, rd)):
            assert_close(a.table.cpu().numpy(), b.table.cpu().numpy(), 1e-5, 1e-6,
                         f"table rank{r} it{it}")


# ---- 4. 16-bit vectors: fp32 accumulate, one rounding ----------------------------------------------
@pytest.mark.parametrize("dtype,ulp", [("float16", 2.0 ** -10), ("bfloat16", 2.0 ** -7)])
@pytest.mark.parametrize("world,shard", [(4, "row"), (2, "mixed")])
@pytest.mark.parametrize("ev", [16, 6])
def test_unique_16_bit_output_is_the_fp32_sum_rounded_once(world, shard, dtype, ulp, ev):
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    rng = np.random.default_rng(17)
    B = 32
    tdt = getattr(torch, dtype)
    cfg = _config(ha, hugectr, world, shard, "Unique", ev)
    ranks = [ha.EmbeddingCollection.for_rank(r, world, cfg, B, out_dtype=tdt, max_hotness=4)
             for r in range(world)]
    for e in ranks:  # values of order one, so that the 16-bit grid is coarse next to fp32 noise
        e.table.normal_()
    row_start, dense = _dense_from_shards(ranks, VOCABS, ev)
    sent = torch.from_numpy(dense).to(tdt).float().numpy()  # the rows as they travel
    keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
    gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
    _, outs = _unique_forward(ranks, gk, gbr)
    bpg = B // world
    for l, t in enumerate(LOOKUP_TABLE):
        ns = len(ranks[0].owners[t])
        for b in range(B):
            ks = keys[br[l * B + b]:br[l * B + b + 1]]
            by_shard = [sent[row_start[t] + ks[ks % ns == s]] for s in range(ns)]
            acc = uo.pool(by_shard, ks.size, COMBINERS[l] == "mean")
            want = torch.from_numpy(np.broadcast_to(acc, (ev,)).copy()).to(tdt).float().numpy()
            got = outs[b // bpg][l, b % bpg].float().cpu().numpy()
            assert (np.abs(got - want) <= ulp * np.abs(want)).all(), (l, b, got, want)


# ---- 5. dynamic tables --------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["sgd", "adagrad", "adam", "momentum"])
@pytest.mark.parametrize("world,shard", [(2, "table"), (4, "row")])
def test_unique_on_dynamic_tables_equals_a_reduction_twin(world, shard, opt_name):
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    rng = np.random.default_rng(19 + world)
    B = 32
    opt = {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "adam": _lib.OPT_ADAM,
           "momentum": _lib.OPT_MOMENTUM_SGD}[opt_name]
    uq, rd = _twins(ha, hugectr, world, shard, B, lr=0.05, optimizer=opt, scaler=2.0, epsilon=1e-6,
                    max_hotness=4, storage="dynamic", initializer="", init_capacity=8)
    # a known, distinct vector for every key of both twins, pushed through the table's own verbs:
    # a forward that gathered the wrong row cannot match
    full = [rng.standard_normal((v, 16)).astype(np.float32) for v in VOCABS]
    for ranks in (uq, rd):
        for g, e in enumerate(ranks):
            for t in e.local_tables:
                ks = np.arange(e.owners[t].index(g), VOCABS[t], len(e.owners[t])).astype(np.int64)
                c = e.class_of_table[t]
                tk = torch.from_numpy(ks).cuda()
                e.det.lookup(tk, [c], [0, ks.size])
                e.det.scatter_update(tk, torch.from_numpy(full[t][ks]).cuda().view(-1), [c],
                                     [0, ks.size])
    for it in range(3):
        keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
        gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
        counts, outs = _unique_forward(uq, gk, gbr)
        grads = [torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float32)).cuda()
                 for o in outs]
        want = _reduction_step(rd, gk, gbr, lambda _: grads)
        for d in range(world):
            assert_close(outs[d].cpu().numpy().reshape(-1), want[d].cpu().numpy().reshape(-1),
                         1e-5, 1e-6, f"fwd rank{d} it{it}")
        _unique_backward(uq, counts, grads)
        for r, (a, b) in enumerate(zip(uq, rd)):
            for t in a.local_tables:
                (ka, va), (kb, vb) = (x.det.export(x.class_of_table[t]) for x in (a, b))
                ka, kb = ka.cpu().numpy(), kb.cpu().numpy()
                oa, ob = np.argsort(ka), np.argsort(kb)
                assert (ka[oa] == kb[ob]).all(), f"keys of table {t} rank{r} it{it}"
                assert_close(va.cpu().numpy()[oa], vb.cpu().numpy()[ob], 2e-5, 2e-6,
                             f"{opt_name} table {t} rank{r} it{it}")


def test_unique_on_dynamic_tables_refuses_the_unique_key_optimizers_by_name():
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    cfg = _config(ha, hugectr, 2, "table", "Unique")
    with pytest.raises(_lib.HugeCTRAmdError, match="Nesterov, RMSProp and Ftrl"):
        ha.EmbeddingCollection.for_rank(0, 2, cfg, 32, optimizer=_lib.OPT_RMSPROP, storage="dynamic",
                                        init_capacity=8)


# ---- 6. concat ----------------------------------------------------------------------------------------
def test_unique_multi_hot_concat_lookup():
    """Combiner::Concat with several keys per bucket under Unique: the expectation of
    test_multi_hot_concat_combiner (key r of the bucket in slot r, missing keys zero)"""
    import torch
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    from hugectr_amd.embedding_collection import (EmbeddingCollection, EmbeddingCollectionConfig,
                                                  EmbeddingTableConfig)
    world = 2
    rng = np.random.default_rng(4)
    ev, B = 8, 16
    bpg = B // world
    rows = [40, 9]
    tabs = [EmbeddingTableConfig(f"t{i}", r, ev) for i, r in enumerate(rows)]
    cfg = EmbeddingCollectionConfig()
    spec = [(0, "concat", 3), (1, "sum", 4), (0, "mean", 2), (1, "concat", 2)]
    cfg.embedding_lookup(table_config=[tabs[t] for t, _, _ in spec],
                         bottom_name=[f"d{i}" for i in range(len(spec))], top_name="emb",
                         combiner=[c for _, c, _ in spec])
    cfg.shard(shard_matrix=[["t0", "t1"]] * world, shard_strategy=[("mp", ["t0", "t1"])],
              compression_strategy=[(hugectr.CompressionStrategy.Unique, ["t0", "t1"])])
    hot = [h for _, _, h in spec]
    shards = [EmbeddingCollection.for_rank(r, world, cfg, B, lr=0.5, optimizer=_lib.OPT_SGD,
                                           batch_major=True, max_hotness=max(hot), hotness=hot)
              for r in range(world)]
    assert all(e._unique for e in shards)
    full = [rng.standard_normal((r, ev)).astype(np.float32) for r in rows]
    for r, e in enumerate(shards):
        for t in e.local_tables:
            ns = len(e.owners[t])
            sid = e.owners[t].index(r)
            n = -(-rows[t] // ns)
            blk = np.zeros((n, ev), np.float32)
            own = np.arange(sid, rows[t], ns)
            blk[:own.size] = full[t][own]
            s0 = e.row_start_of_table[t]
            e.table[s0:s0 + n] = torch.from_numpy(blk).cuda()
    lens = np.concatenate([rng.integers(0, h + 1, B) for h in hot])
    br = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = np.concatenate([rng.integers(0, rows[t], int(lens[l * B:(l + 1) * B].sum()))
                           for l, (t, _, _) in enumerate(spec)]).astype(np.int64)
    widths = [ev * (h if c == "concat" else 1) for (_, c, h) in spec]
    off = np.concatenate([[0], np.cumsum(widths)])
    want = np.zeros((B, off[-1]), np.float32)
    for l, (t, c, h) in enumerate(spec):
        for b in range(B):
            ks = keys[br[l * B + b]:br[l * B + b + 1]]
            if c == "concat":
                for r, k in enumerate(ks):
                    want[b, off[l] + r * ev:off[l] + (r + 1) * ev] = full[t][k]
            elif len(ks):
                v = full[t][ks].sum(0, dtype=np.float32)
                want[b, off[l]:off[l] + ev] = v / np.float32(len(ks)) if c == "mean" else v
    gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
    counts, outs = _unique_forward(shards, gk, gbr)
    got = torch.cat([o.reshape(bpg, -1) for o in outs]).float().cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    # backward + SGD: slot r's gradient reaches key r
    g = rng.standard_normal((B, off[-1])).astype(np.float32)
    ref = [f.astype(np.float64) for f in full]
    for l, (t, c, h) in enumerate(spec):
        for b in range(B):
            ks = keys[br[l * B + b]:br[l * B + b + 1]]
            for r, k in enumerate(ks):
                if c == "concat":
                    ref[t][k] -= 0.5 * g[b, off[l] + r * ev:off[l] + (r + 1) * ev]
                else:
                    ref[t][k] -= 0.5 * g[b, off[l]:off[l] + ev] / (len(ks) if c == "mean" else 1)
    grads = [torch.from_numpy(g[d * bpg:(d + 1) * bpg].reshape(tuple(outs[d].shape))).cuda()
             for d in range(world)]
    _unique_backward(shards, counts, grads)
    for r, e in enumerate(shards):
        for t in e.local_tables:
            ns = len(e.owners[t])
            own = np.arange(e.owners[t].index(r), rows[t], ns)
            s0 = e.row_start_of_table[t]
            np.testing.assert_allclose(e.table[s0:s0 + own.size].cpu().numpy(), ref[t][own],
                                       rtol=1e-5, atol=1e-5)


# ---- 7. determinism ---------------------------------------------------------------------------------
def test_unique_two_runs_give_identical_bits():
    import torch
    import hugectr_amd as ha
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib
    world, B = 4, 256
    results = []
    for run in range(2):
        rng = np.random.default_rng(23)
        cfg = _config(ha, hugectr, world, "row", "Unique")
        ranks = [ha.EmbeddingCollection.for_rank(r, world, cfg, B, lr=0.1, optimizer=_lib.OPT_ADAGRAD,
                                                 out_dtype=torch.float16, scaler=128.0, max_hotness=8,
                                                 seed=5) for r in range(world)]
        kept = []
        for it in range(2):
            keys, br = _make_inputs(rng, B, [20, 7, 30, 12], LOOKUP_TABLE, 8)  # keys repeat a lot
            gk, gbr = torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda()
            counts, outs = _unique_forward(ranks, gk, gbr)
            grads = [torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float16)).cuda()
                     for o in outs]
            _unique_backward(ranks, counts, grads)
            kept += [o.clone() for o in outs]
        results.append(kept + [e.table.clone() for e in ranks])
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ---- 8. two processes on one GPU over gloo ------------------------------------------------------------
def _local_share(keys, br, rank, B, bpg, L):
    lens, ks = [], []
    for l in range(L):
        for b in range(rank * bpg, (rank + 1) * bpg):
            q0, q1 = br[l * B + b], br[l * B + b + 1]
            lens.append(q1 - q0)
            ks.append(keys[q0:q1])
    return (np.concatenate(ks).astype(np.int64),
            np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


def _unique_worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        import hugectr_amd as ha
        import hugectr_amd.hugectr as hugectr
        rng = np.random.default_rng(5)                      # same stream on both ranks
        B, ev = 64, 16
        L = len(LOOKUP_TABLE)

        def cfg(strategy):
            tcfg = [ha.EmbeddingTableConfig(f"t{i}", v, ev) for i, v in enumerate(VOCABS)]
            c = ha.EmbeddingCollectionConfig()
            for l in range(L):
                c.embedding_lookup(tcfg[LOOKUP_TABLE[l]], f"in{l}", f"out{l}", "sum" if l % 2 else "mean")
            c.shard([[1, 1, 1, 0], [0, 1, 1, 1]], "mp",   # tables 1, 2 row-sharded over both
                    [(getattr(hugectr.CompressionStrategy, strategy), [t.name for t in tcfg])])
            return c
        kw = dict(lr=0.1, max_hotness=4, seed=3)
        ea = ha.EmbeddingCollection(cfg("Unique"), B, key_route="a2a", **kw)
        eg = ha.EmbeddingCollection(cfg("Unique"), B, key_route="allgather", **kw)
        er = ha.EmbeddingCollection(cfg("Reduction"), B, key_route="allgather", **kw)
        assert ea._unique and eg._unique and not er._unique
        assert torch.equal(ea.table, eg.table) and torch.equal(ea.table, er.table)
        bpg = B // world
        for it in range(3):
            keys, br = _make_inputs(rng, B, VOCABS, LOOKUP_TABLE, 4)
            lk, lbr = _local_share(keys, br, rank, B, bpg, L)
            lk, lbr = torch.from_numpy(lk).cuda(), torch.from_numpy(lbr).cuda()
            oa, og, orr = ea.forward(lk, lbr), eg.forward(lk, lbr), er.forward(lk, lbr)
            assert torch.equal(oa, og), f"forward it{it}: the two key routes differ"
            assert_close(oa.cpu().numpy().reshape(-1), orr.cpu().numpy().reshape(-1), 1e-5, 1e-6,
                         f"forward it{it} vs Reduction")
            grad = torch.from_numpy(rng.standard_normal((world,) + tuple(oa.shape)).astype(np.float32))[rank].cuda()
            for e in (ea, eg, er):
                e.backward_and_update(grad)
            assert torch.equal(ea.table, eg.table), f"tables it{it}: the two key routes differ"
            assert_close(ea.table.cpu().numpy(), er.table.cpu().numpy(), 1e-5, 1e-6,
                         f"tables it{it} vs Reduction")
            x = eg.last_exchange
            assert x["distinct_rows_out"] <= x["keys_out"] and x["bytes_out_forward"] > 0
        ret[rank] = "ok"
    except Exception as ex:
        import traceback
        ret[rank] = "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))
    finally:
        dist.destroy_process_group()


def _spawn(target, args_of, world=2, timeout=600):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=target, args=args_of(r, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
    for r in range(world):
        if ret.get(r) != "ok":
            print(f"--- rank {r} ---\n{ret.get(r)}")
    assert all(ret.get(r) == "ok" for r in range(world))
    return ret


def test_unique_two_ranks_on_one_gpu_both_key_routes():
    """EmbeddingCollection.forward / backward_and_update under Unique on 2 processes (gloo, both on
    this GPU): the two key routes give identical bits, a Reduction twin agrees within tolerance"""
    port = 29500 + os.getpid() % 2000 + 41
    _spawn(_unique_worker, lambda r, ret: (r, 2, port, ret))


MODEL_HOT = [1, 2, 1, 2, 6, 1, 1, 1, 1, 7, 3, 8, 1, 6, 9, 5, 1, 1, 1, 12, 10, 7, 4, 3, 1, 1]


def _model_worker(rank, world, port, folder, ret, mixed):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import hugectr_amd.hugectr as hugectr
        from test_model_gpu import SIZES
        hot = MODEL_HOT
        solver = hugectr.CreateSolver(batchsize=256, batchsize_eval=256, lr=0.05, vvgpu=[[0, 1]],
                                      i64_input_key=True, max_eval_batches=1,
                                      use_embedding_collection=True)
        reader = hugectr.DataReaderParams(
            data_reader_type=hugectr.DataReaderType_t.Parquet,
            source=[os.path.join(folder, "train", "_file_list.txt")],
            eval_source=os.path.join(folder, "val", "_file_list.txt"), slot_size_array=SIZES,
            check_type=hugectr.Check_t.Non)
        # (plain SGD: AdaGrad from zero accumulators steps by +-lr whatever a gradient's size, which
        #  turns a last-bit difference of a near-zero gradient into a difference of the step)
        opt = hugectr.CreateOptimizer(optimizer_type=hugectr.Optimizer_t.SGD,
                                      update_type=hugectr.Update_t.Local)
        model = hugectr.Model(solver, reader, opt)
        model.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=13, dense_name="dense",
                                data_reader_sparse_param_array=[
                                    hugectr.DataReaderSparseParam(f"data{i}", hot[i], True, 1)
                                    for i in range(26)]))
        tables = [hugectr.EmbeddingTableConfig(name=str(i), max_vocabulary_size=SIZES[i], ev_size=16)
                  for i in range(26)]
        names = [t.name for t in tables]
        S = hugectr.CompressionStrategy
        # every table row-sharded over both ranks; every other table under Unique
        comp = [(S.Unique, names[0::2]), (S.Reduction, names[1::2])] if mixed else \
            [(S.Reduction, names)]
        ebc = hugectr.EmbeddingCollectionConfig()
        ebc.embedding_lookup(table_config=tables, bottom_name=[f"data{i}" for i in range(26)],
                             top_name="sparse_embedding",
                             combiner=["concat" if h == 1 else "sum" for h in hot])
        ebc.shard(shard_matrix=[names, names], shard_strategy=[("mp", names)],
                  compression_strategy=comp)
        model.add(ebc)
        D, T = hugectr.DenseLayer, hugectr.Layer_t
        model.add(D(layer_type=T.Reshape, bottom_names=["sparse_embedding"],
                    top_names=["sparse_embedding1"], shape=[-1, 26, 16]))
        model.add(D(layer_type=T.MLP, bottom_names=["dense"], top_names=["mlp1"], num_outputs=[32, 16],
                    act_type=hugectr.Activation_t.Relu))
        model.add(D(layer_type=T.Interaction, bottom_names=["mlp1", "sparse_embedding1"],
                    top_names=["interaction1"]))
        model.add(D(layer_type=T.MLP, bottom_names=["interaction1"], top_names=["mlp2"],
                    num_outputs=[64, 1],
                    activations=[hugectr.Activation_t.Relu, hugectr.Activation_t.Non]))
        model.add(D(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["mlp2", "label"],
                    top_names=["loss"]))
        model.compile()
        kinds = sorted(bool(rt["train"]._unique) for rt in model._ebc)
        assert kinds == ([False, True] if mixed else [False]), kinds
        # the same starting rows in both models: a collection draws its tables from its own
        # generator, so splitting the config changes the draw; here every table gets values that
        # depend on its name alone
        import torch
        for rt in model._ebc:
            e = rt["train"]
            for t in e.local_tables:
                V = e.tables[t].max_vocabulary_size
                full = np.random.default_rng(1000 + int(e.tables[t].name)).uniform(
                    -0.1, 0.1, (V, 16)).astype(np.float32)
                own = np.arange(e.owners[t].index(rank), V, len(e.owners[t]))
                s0 = e.row_start_of_table[t]
                e.table[s0:s0 + own.size] = torch.from_numpy(full[own]).cuda()
        losses = []
        for _ in range(5):
            model.train()
            losses.append(float(model.get_current_loss()))
        if mixed:
            u = [v for v in model.exchange_report().values() if v.get("payload") == "unique rows"]
            assert len(u) == 1 and u[0]["distinct_rows_out"] > 0 and u[0]["bytes_out_backward"] > 0
        ret[(rank, "loss")] = losses
        ret[rank] = "ok"
    except Exception as ex:
        import traceback
        ret[rank] = "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))
    finally:
        dist.destroy_process_group()


def test_unique_and_reduction_tables_in_one_model_two_ranks(tmp_path):
    """hugectr.Model splits a config by (placement, vector size, strategy): one Unique and one
    Reduction table train on 2 ranks; the loss of each of 5 steps is within 1e-3 of the
    all-Reduction model (the project's bound for whole-model loss parity)"""
    import hugectr_amd.hugectr as hugectr
    from test_model_gpu import _gen
    _gen(tmp_path, hugectr, n_train=4096, n_eval=512, nnz=MODEL_HOT)
    losses = {}
    for k, mixed in enumerate((False, True)):
        port = 29500 + os.getpid() % 2000 + 47 + k
        ret = _spawn(_model_worker, lambda r, ret: (r, 2, port, str(tmp_path), ret, mixed))
        losses[mixed] = ret[(0, "loss")]
    print("all-Reduction:", losses[False], "\nUnique + Reduction:", losses[True])
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 1e-3, (losses[False], losses[True])
