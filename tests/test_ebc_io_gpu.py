"""GPU: embedding_dump / embedding_load below the Model -- the kernels of csrc/ebc_io.hip through the
C ABI against numpy, and export_table / import_table of the runtime collections.  Everything is a
copy: every comparison is exact."""
import ctypes
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 64
N_KEYS = 1000   # 16 chunks of 64, the last one partial (40)
VOCAB = 1500


def _feed(io, w, start, m, keys, rows, states):
    io.wait(w)
    io.keys[w][:m] = keys[start:start + m]
    io.rows[w][:m] = rows[start:start + m]
    for a, s in enumerate(states):
        io.state[w][a][:m] = s[start:start + m]


def _file_like(rng, ev, nstate, key_dtype, n=N_KEYS, vocab=VOCAB):
    keys = rng.permutation(vocab)[:n].astype(key_dtype)
    rows = rng.standard_normal((n, ev)).astype(np.float32)
    states = [rng.standard_normal((n, ev)).astype(np.float32) for _ in range(nstate)]
    return keys, rows, states


@pytest.mark.parametrize("nstate", [0, 1, 2])
@pytest.mark.parametrize("num_shards,shard_id", [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
@pytest.mark.parametrize("ev", [128, 16, 3])
def test_check_and_static_import(ev, num_shards, shard_id, nstate):
    """1000 keys in random order through 64-row chunks (ev 3: the element-wise path; ev 16 with
    uint32 keys): counts exact, every owned key's row and state rows at row_start + key /
    num_shards, every other row of the destination -- foreign keys, keys outside the vocab, rows
    whose key is not in the file, the padding around the shard -- untouched."""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    from hugectr_amd.ebc_io import IoChunks
    rng = np.random.default_rng(ev * 100 + num_shards * 10 + shard_id)
    kd = np.dtype("<u4") if ev == 16 else np.dtype("<i8")
    keys, rows, states = _file_like(rng, ev, nstate, kd)
    bad = [5, 70, 999]  # keys outside [0, vocab): >= vocab, far beyond, negative (int64 only)
    keys[bad[0]], keys[bad[1]] = VOCAB, VOCAB + 12345
    keys[bad[2]] = -3 if kd.itemsize == 8 else 0xFFFFFFFF
    row_start, pad = 5, 3
    shard_rows = -(-VOCAB // num_shards)
    dst = [torch.from_numpy(rng.standard_normal((row_start + shard_rows + pad, ev))
                            .astype(np.float32)).cuda() for _ in range(1 + nstate)]
    before = [d.cpu().numpy().copy() for d in dst]
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    sp = [ptr(d) for d in dst[1:]] + [None, None]
    with IoChunks(CHUNK, ev, kd) as io:
        w = 0
        for start in range(0, N_KEYS, CHUNK):
            m = min(CHUNK, N_KEYS - start)
            _feed(io, w, start, m, keys, rows, states)
            check(lib.hctr_ebc_io_check(io._h, w, m, num_shards, shard_id, VOCAB, ptr(counts),
                                        stream_ptr()))
            check(lib.hctr_ebc_io_import_static(io._h, w, m, num_shards, shard_id, VOCAB, row_start,
                                                ptr(dst[0]), sp[0], sp[1], stream_ptr()))
            w ^= 1
        io.wait(0)
        io.wait(1)
    torch.cuda.synchronize()
    k = keys.astype(np.int64) if kd.itemsize == 8 else keys.astype(np.uint32).astype(np.int64)
    inside = (k >= 0) & (k < VOCAB)
    own = inside & (k % num_shards == shard_id)
    assert counts.cpu().tolist() == [int(own.sum()), int((inside & ~own).sum()), 3]
    for d, b, src in zip(dst, before, [rows] + states):
        want = b.copy()
        want[row_start + k[own] // num_shards] = src[own]
        assert np.array_equal(d.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_a_chunk_without_an_owned_key():
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    from hugectr_amd.ebc_io import IoChunks
    rng = np.random.default_rng(7)
    ev, n = 16, 3 * CHUNK
    keys = rng.permutation(VOCAB // 2)[:n].astype(np.int64) * 2 + 1     # odd: shard 1 of 2
    keys[CHUNK:2 * CHUNK] -= 1                                          # chunk 1: even keys only
    rows = rng.standard_normal((n, ev)).astype(np.float32)
    table = torch.zeros((VOCAB // 2 + 1, ev), dtype=torch.float32, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    okeys = torch.full((CHUNK,), -1, dtype=torch.int64, device="cuda")
    orows = torch.zeros((CHUNK, ev), dtype=torch.float32, device="cuda")
    sel = []
    with IoChunks(CHUNK, ev, np.dtype("<i8")) as io:
        for c in range(3):
            w = c & 1
            _feed(io, w, c * CHUNK, CHUNK, keys, rows, [])
            one = torch.zeros(3, dtype=torch.int64, device="cuda")
            check(lib.hctr_ebc_io_check(io._h, w, CHUNK, 2, 1, VOCAB, ptr(one), stream_ptr()))
            check(lib.hctr_ebc_io_import_static(io._h, w, CHUNK, 2, 1, VOCAB, 0, ptr(table), None,
                                                None, stream_ptr()))
            got = ctypes.c_size_t(99)
            check(lib.hctr_ebc_io_select(io._h, w, CHUNK, 2, 1, VOCAB, ptr(okeys), ptr(orows), None,
                                         None, ctypes.byref(got), stream_ptr()))
            sel.append(got.value)
            assert one.cpu().tolist() == ([0, CHUNK, 0] if c == 1 else [CHUNK, 0, 0])
            counts += one
    assert sel == [CHUNK, 0, CHUNK] and counts.cpu().tolist() == [2 * CHUNK, CHUNK, 0]
    want = np.zeros((VOCAB // 2 + 1, ev), np.float32)
    own = keys % 2 == 1
    want[keys[own] // 2] = rows[own]
    assert np.array_equal(table.cpu().numpy(), want)


@pytest.mark.parametrize("ev,nstate,key_dtype", [(16, 2, "<i8"), (3, 1, "<i8"), (128, 0, "<u4")])
def test_dynamic_select_is_a_stable_compaction(ev, nstate, key_dtype):
    """order kept, count exact, keys above 2^40 (int64), rows and state rows follow their keys"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    from hugectr_amd.ebc_io import IoChunks
    rng = np.random.default_rng(ev)
    kd = np.dtype(key_dtype)
    keys, rows, states = _file_like(rng, ev, nstate, kd)
    if kd.itemsize == 8:
        keys[::3] += (1 << 40) + 7
    ns, sid = 3, 1
    okeys = torch.empty(CHUNK, dtype=torch.int64, device="cuda")
    obuf = [torch.empty((CHUNK, ev), dtype=torch.float32, device="cuda") for _ in range(1 + nstate)]
    so = [ptr(b) for b in obuf[1:]] + [None, None]
    got_k, got = [], [[] for _ in range(1 + nstate)]
    with IoChunks(CHUNK, ev, kd) as io:
        w = 0
        for start in range(0, N_KEYS, CHUNK):
            m = min(CHUNK, N_KEYS - start)
            _feed(io, w, start, m, keys, rows, states)
            n = ctypes.c_size_t()
            check(lib.hctr_ebc_io_select(io._h, w, m, ns, sid, 1 << 63, ptr(okeys), ptr(obuf[0]),
                                         so[0], so[1], ctypes.byref(n), stream_ptr()))
            torch.cuda.synchronize()
            got_k.append(okeys[:n.value].cpu().numpy())
            for g, b in zip(got, obuf):
                g.append(b[:n.value].cpu().numpy())
            w ^= 1
    k = keys.astype(np.int64)
    own = k % ns == sid
    assert 200 < own.sum() < 500
    assert np.array_equal(np.concatenate(got_k), k[own])
    for g, src in zip(got, [rows] + states):
        assert np.array_equal(np.concatenate(g), src[own])


# ---- collections ---------------------------------------------------------------------------------

VOCABS = [1000, 37, 4096]
EV, B = 16, 64


def _config(world, placement="all", vocabs=VOCABS, ev=EV):
    import hugectr_amd as ha
    tcfg = [ha.EmbeddingTableConfig(f"t{i}", v, ev) for i, v in enumerate(vocabs)]
    cfg = ha.EmbeddingCollectionConfig()
    for l, t in enumerate(tcfg):
        cfg.embedding_lookup(t, f"in{l}", f"out{l}", "sum")
    if world == 2 and placement == "mixed":  # t0 on both ranks, t1 on rank 0 only, t2 on rank 1 only
        cfg.shard([[1, 1, 0], [1, 0, 1]])
    return cfg


def _shard_equals_source(shard, src):
    """every row of every local table of `shard` equals the row of its key in the one-GPU `src`"""
    for t in shard.local_tables:
        lay = shard._io_layout(t)
        n = -(-(VOCABS[t] - lay["shard_id"]) // lay["num_shards"])
        keys = lay["shard_id"] + np.arange(n) * lay["num_shards"]
        got = shard.table[lay["row_start"]:lay["row_start"] + n].cpu().numpy()
        want = src.table.cpu().numpy()[src.row_start_of_table[t] + keys]
        assert np.array_equal(got, want), t


@pytest.mark.parametrize("placement", ["all", "mixed"])
def test_static_reshard_one_to_two_and_back(tmp_path, placement):
    import hugectr_amd as ha
    from hugectr_amd import ebc_io
    src = ha.EmbeddingCollection.for_rank(0, 1, _config(1), B, seed=1)
    p1, p2 = str(tmp_path / "w1"), str(tmp_path / "w2")
    ebc_io.dump_shards(p1, 0, [src], chunk_rows=100)          # 41 chunks for the largest table
    shards = [ha.EmbeddingCollection.for_rank(r, 2, _config(2, placement), B, seed=7 + r)
              for r in range(2)]
    for s in shards:
        ebc_io.load_shard(p1, 0, s, chunk_rows=100)
        _shard_equals_source(s, src)
    ebc_io.dump_shards(p2, 0, shards, chunk_rows=100)
    back = ha.EmbeddingCollection.for_rank(0, 1, _config(1), B, seed=99)
    assert not np.array_equal(back.table.cpu().numpy(), src.table.cpu().numpy())
    ebc_io.load_shard(p2, 0, back, chunk_rows=100)
    assert np.array_equal(back.table.cpu().numpy(), src.table.cpu().numpy())
    # the two dumps hold the same (key, row) pairs; in p2 rank 0's keys come first
    from hugectr_amd import embedding_io as eio
    with eio.TableFiles(p2, 0, 1) as f:
        assert f.key_num == 37
        want = np.arange(37) if placement == "mixed" else np.r_[np.arange(0, 37, 2), np.arange(1, 37, 2)]
        assert np.array_equal(f.read_keys(), want)


def test_data_parallel_replicas_load_rank_0s_dump(tmp_path):
    import torch
    import hugectr_amd as ha
    from hugectr_amd import _lib, ebc_io
    from hugectr_amd.embedding_collection import DataParallelCollection
    cfg = _config(1, vocabs=[37, 300])
    reps = [DataParallelCollection(cfg, B, optimizer=_lib.OPT_ADAGRAD, seed=3, rank=r, world=2)
            for r in range(2)]
    reps[0].table.copy_(torch.randn_like(reps[0].table))
    reps[0].accum.copy_(torch.rand_like(reps[0].accum))
    ebc_io.dump_shards(str(tmp_path), 0, reps, optimizer_states=True, chunk_rows=50)
    assert [reps[r].table_key_count(0) for r in range(2)] == [37, 0]
    new = [DataParallelCollection(cfg, B, optimizer=_lib.OPT_ADAGRAD, seed=50 + r, rank=r, world=2)
           for r in range(2)]
    for e in new:
        ebc_io.load_shard(str(tmp_path), 0, e, chunk_rows=50)
        assert torch.equal(e.table, reps[0].table) and torch.equal(e.accum, reps[0].accum)


def _as_map(e, t):
    k, v = e.det.export(e.class_of_table[t])
    k, v = k.cpu().numpy(), v.cpu().numpy()
    o = np.argsort(k)
    return k[o], v[o]


def _dynamic(cfg, seed, **kw):
    import hugectr_amd as ha
    return ha.EmbeddingCollection.for_rank(0, 1, cfg, B, seed=seed, storage="dynamic",
                                           init_capacity=64, max_hotness=4, **kw)


def _insert_keys(e, rng, n_tables, per_lookup=4):
    import torch
    keys = rng.integers(0, 3000, size=n_tables * B * per_lookup).astype(np.int64)
    keys[::5] += (1 << 40) + 11
    br = np.arange(0, keys.size + 1, per_lookup, dtype=np.int64)
    e.forward(torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda())
    return keys


def test_dynamic_dump_and_load_are_equal_as_maps(tmp_path):
    from hugectr_amd import ebc_io
    rng = np.random.default_rng(11)
    cfg = _config(1, vocabs=[-1, -1])
    a = _dynamic(cfg, 1)
    keys = _insert_keys(a, rng, 2)
    assert 400 < np.unique(keys).size < 600 and a.det.size() > 400
    ebc_io.dump_shards(str(tmp_path), 0, [a], chunk_rows=100)
    b = _dynamic(cfg, 2)
    ebc_io.load_shard(str(tmp_path), 0, b, chunk_rows=100)
    for t in range(2):
        (ka, va), (kb, vb) = _as_map(a, t), _as_map(b, t)
        assert ka.max() > 1 << 40
        assert np.array_equal(ka, kb) and np.array_equal(va, vb)


def test_static_dump_loads_into_a_dynamic_table_and_back(tmp_path):
    import hugectr_amd as ha
    from hugectr_amd import ebc_io
    vocabs = [1000, 37]
    src = ha.EmbeddingCollection.for_rank(0, 1, _config(1, vocabs=vocabs), B, seed=1)
    p1, p2 = str(tmp_path / "s"), str(tmp_path / "d")
    ebc_io.dump_shards(p1, 0, [src], chunk_rows=100)
    dyn = _dynamic(_config(1, vocabs=[-1, -1]), 5)
    ebc_io.load_shard(p1, 0, dyn, chunk_rows=100)
    table = src.table.cpu().numpy()
    for t, v in enumerate(vocabs):
        k, rows = _as_map(dyn, t)
        assert np.array_equal(k, np.arange(v))
        r0 = src.row_start_of_table[t]
        assert np.array_equal(rows, table[r0:r0 + v])
    ebc_io.dump_shards(p2, 0, [dyn], chunk_rows=100)
    back = ha.EmbeddingCollection.for_rank(0, 1, _config(1, vocabs=vocabs), B, seed=77)
    ebc_io.load_shard(p2, 0, back, chunk_rows=100)
    assert np.array_equal(back.table.cpu().numpy(), table)


def _steps(e, rng_seed, first, count, n_tables, vocab_hi):
    """`count` forward / backward_and_update steps with keys and gradients fixed by the seed"""
    import torch
    for s in range(first, first + count):
        rng = np.random.default_rng(rng_seed * 1000 + s)
        keys = rng.integers(0, vocab_hi, size=n_tables * B).astype(np.int64)
        br = np.arange(n_tables * B + 1, dtype=np.int64)
        out = e.forward(torch.from_numpy(keys).cuda(), torch.from_numpy(br).cuda())
        g = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        e.backward_and_update(torch.from_numpy(g).cuda())


@pytest.mark.parametrize("case", ["adagrad", "ftrl", "dynamic-adagrad"])
def test_resume_with_optimizer_state(tmp_path, case):
    """three steps, dump with the optimizer state, load into a fresh collection: one more identical
    step leaves tables and state bit-equal; the same dump WITHOUT its opt_state files gives
    another table after that step (the state files are read)"""
    import torch
    import hugectr_amd as ha
    from hugectr_amd import _lib, ebc_io
    dynamic = case.startswith("dynamic")
    vocabs = [-1, -1, -1] if dynamic else [37, 37, 37]
    cfg = _config(1, vocabs=vocabs)
    kw = dict(lr=0.1, optimizer=_lib.OPT_FTRL if case == "ftrl" else _lib.OPT_ADAGRAD,
              initial_accu_value=0.0, ftrl=(0.01, 0.02, 0.5))

    def make(seed):
        if dynamic:
            # ("ones": a key first met in the step after the load starts from the same row in
            #  every collection; the default initializer draws from the collection's seed)
            return _dynamic(cfg, seed, initializer="ones",
                            **{k: v for k, v in kw.items() if k != "initial_accu_value"})
        return ha.EmbeddingCollection.for_rank(0, 1, cfg, B, seed=seed, **kw)

    def state(e):
        if dynamic:
            return [x for t in range(3) for x in _as_map(e, t)]
        return [a.cpu().numpy() for a in (e.table, e.accum, e.ftrl_z) if a is not None]

    a = make(1)
    _steps(a, 5, 0, 3, 3, 37)
    full, bare = str(tmp_path / "full"), str(tmp_path / "bare")
    ebc_io.dump_shards(full, 0, [a], optimizer_states=True, chunk_rows=16)
    shutil.copytree(full, bare)
    removed = [os.remove(os.path.join(bare, "embedding_collection_0", f))
               for f in os.listdir(os.path.join(bare, "embedding_collection_0"))
               if f.startswith("opt_state")]
    assert len(removed) == 3
    b, c = make(2), make(3)
    ebc_io.load_shard(full, 0, b, chunk_rows=16)
    ebc_io.load_shard(bare, 0, c, chunk_rows=16)
    assert all(np.array_equal(x, y) for x, y in zip(state(a)[:1], state(b)[:1]))
    for e in (a, b, c):
        _steps(e, 5, 3, 1, 3, 37)
    torch.cuda.synchronize()
    sa, sb, sc = state(a), state(b), state(c)
    assert len(sa) == (6 if dynamic else 3 if case == "ftrl" else 2)
    for x, y in zip(sa, sb):
        assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else x.dtype),
                              y.view(np.uint32 if y.dtype == np.float32 else y.dtype))
    table_of = (lambda s: s[1]) if dynamic else (lambda s: s[0])
    assert not np.array_equal(table_of(sa), table_of(sc))


def test_refusals(tmp_path):
    import hugectr_amd as ha
    from hugectr_amd import _lib, ebc_io
    from hugectr_amd import embedding_io as eio
    rng = np.random.default_rng(3)
    cfg = _config(1, vocabs=[37, 300])
    e = ha.EmbeddingCollection.for_rank(0, 1, cfg, B, seed=1)
    before = e.table.cpu().numpy().copy()
    good = (np.arange(37), rng.standard_normal((37, EV)).astype(np.float32))
    # a key AT the vocab in the second table: raises, names the table, and the first table's rows
    # (valid, earlier in the folder) were not written either
    keys = rng.permutation(300)[:200]
    keys[150] = 300
    eio.write_collection(str(tmp_path / "a"), 0,
                         {0: good, 1: (keys, rng.standard_normal((200, EV)).astype(np.float32))})
    with pytest.raises(_lib.HugeCTRAmdError, match=r"'t1'.*1 of 200 keys"):
        ebc_io.load_shard(str(tmp_path / "a"), 0, e, chunk_rows=64)
    assert np.array_equal(e.table.cpu().numpy(), before)
    # ev_size mismatch
    eio.write_collection(str(tmp_path / "b"), 0,
                         {0: (np.arange(37), np.zeros((37, 8), np.float32)), 1: good})
    with pytest.raises(_lib.HugeCTRAmdError, match="ev_size 8"):
        ebc_io.load_shard(str(tmp_path / "b"), 0, e)
    assert np.array_equal(e.table.cpu().numpy(), before)
    # a state file for another optimizer
    eio.write_collection(str(tmp_path / "c"), 0, {0: good + ([good[1]],)}, optimizer=_lib.OPT_ADAGRAD)
    with pytest.raises(_lib.HugeCTRAmdError, match="opt_state0"):
        ebc_io.load_shard(str(tmp_path / "c"), 0, e, table_ids=[0])
    assert np.array_equal(e.table.cpu().numpy(), before)
    # optimizer state of a dynamic table on the unique-key flow: refused, no folder created
    d = _dynamic(_config(1, vocabs=[-1]), 1, optimizer=_lib.OPT_NESTEROV)
    _insert_keys(d, rng, 1)
    with pytest.raises(_lib.HugeCTRAmdError, match="unique-key flow"):
        ebc_io.dump_shards(str(tmp_path / "n"), 0, [d], optimizer_states=True)
    assert not os.path.exists(str(tmp_path / "n"))
    ebc_io.dump_shards(str(tmp_path / "n"), 0, [d])  # (without the state it dumps)
    assert os.path.exists(str(tmp_path / "n" / "embedding_collection_0" / "weight0"))
