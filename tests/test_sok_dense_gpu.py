"""GPU: the SOK dense lookups -- hctr_dist_select and hctr_indexed_row_copy bit for bit against the
numpy oracle (tests/dense_lookup_oracle.py), sok.group_lookup on the reference's own op-test data,
sok.all2all_dense_embedding on one rank against plain indexing and against lookup_sparse with one
key per row, the reference's training scenario with its own criterion, and two ranks over gloo on
the one GPU.  Expected values never come from the kernels under test."""
import os

import numpy as np
import pytest

import dense_lookup_oracle as orc

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"


# ---- hctr_dist_select ---------------------------------------------------------------------------
def _keys(rng, n, dtype, kind, N):
    hi = 1 << 30
    if kind == "uniform":
        k = rng.integers(0, hi, size=n)
    elif kind == "powerlaw":
        k = np.minimum((rng.pareto(1.05, size=n) * 3).astype(np.int64), hi)
    elif kind == "one_owner":
        k = rng.integers(0, hi // 256, size=n) * N + (N - 1)
    else:  # keys above 2^32 (int64 only)
        k = rng.integers(1 << 32, 1 << 62, size=n)
    return k.astype(dtype)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 8192, 1 << 20])
@pytest.mark.parametrize("N", [1, 2, 3, 8, 64, 256])
def test_dist_select_is_the_stable_partition(N, n):
    if EMU and n > (1 << 16):
        pytest.skip("more than 2^16 keys on the host interpreter")
    import torch
    from hugectr_amd import sok
    rng = np.random.default_rng(1000 * N + n % 997)
    for dtype, kinds in ((np.int32, ("uniform", "powerlaw", "one_owner")),
                         (np.int64, ("uniform", "powerlaw", "one_owner", "big"))):
        for kind in kinds:
            keys = _keys(rng, n, dtype, kind, N)
            out, order, splits = sok._dist_select(torch.from_numpy(keys).cuda(), N)
            wk, wo, ws = orc.dist_select(keys, N)
            what = (N, n, dtype.__name__, kind)
            assert np.array_equal(splits.cpu().numpy(), ws), what
            assert np.array_equal(order.cpu().numpy(), wo), what
            assert np.array_equal(out.cpu().numpy(), wk), what
            assert out.dtype == torch.from_numpy(keys).dtype and order.dtype == torch.int32


# ---- hctr_indexed_row_copy ----------------------------------------------------------------------
_NP = {"f32": np.float32, "f16": np.float16}


def _code(name):
    from hugectr_amd import _lib
    return {"f32": _lib.F32, "f16": _lib.F16}[name]


def _run_copy(torch, sok, cases, sd, dd):
    """cases: dicts(src, index, div, n, dst_rows, dst_pos, src_rows) in numpy; one call for all;
    compares every destination with the oracle (untouched rows keep their fill)"""
    tasks, keep = [], []
    for c in cases:
        src = c.get("src_t")
        if src is None:
            src = torch.from_numpy(c["src"]).cuda()
        dim = c["src"].shape[1]
        dst0 = np.full((c["dst_rows"], dim), 7, dtype=_NP[dd])
        dst = torch.from_numpy(dst0.copy()).cuda()
        idx = torch.from_numpy(c["index"]).cuda() if c["index"] is not None else None
        pos = torch.from_numpy(c["dst_pos"]).cuda() if c["dst_pos"] is not None else None
        src_rows = c["src"].shape[0] if c.get("src_rows") is None else c["src_rows"]
        tasks.append((src, src_rows, dim, idx, c["div"], c["n"], dst, pos))
        keep.append((dst, dst0))
    sok._row_copy(tasks, _code(sd), _code(dd))
    for c, (dst, dst0) in zip(cases, keep):
        want = orc.indexed_row_copy(c["src"], c["index"], c["div"], c["n"], dst0, c["dst_pos"],
                                    c.get("src_rows"))
        got = dst.cpu().numpy()
        assert got.dtype == want.dtype
        assert np.array_equal(got.view(np.uint16 if dd == "f16" else np.uint32),
                              want.view(np.uint16 if dd == "f16" else np.uint32)), \
            (c["src"].shape, c["div"], c["n"], sd, dd)


def _case(rng, rows, dim, n, sd, index="i64", div=1, perm=False, src_rows=None, bad=True):
    src = rng.standard_normal((rows, dim)).astype(_NP[sd])
    idx = None
    if index is not None:
        idx = rng.integers(0, rows * div, size=n)
        if bad and n >= 4:
            idx[rng.integers(0, n, size=max(1, n // 16))] = rows * div + rng.integers(0, 50)
            if index == "i64":
                idx[rng.integers(0, n, size=max(1, n // 16))] = -1
                idx[rng.integers(0, n)] = -(1 << 40)
        idx = idx.astype(np.int64 if index == "i64" else np.int32)
    pos = rng.permutation(n).astype(np.int32) if perm else None
    return dict(src=src, index=idx, div=div, n=n, dst_rows=n, dst_pos=pos, src_rows=src_rows)


@pytest.mark.parametrize("sd,dd", [("f32", "f32"), ("f32", "f16"), ("f16", "f32")])
@pytest.mark.parametrize("dim", [1, 3, 4, 16, 64, 128, 130, 256])
def test_indexed_row_copy_equals_the_oracle(dim, sd, dd):
    import torch
    from hugectr_amd import sok
    rng = np.random.default_rng(dim * 7 + len(sd + dd))
    rows, n = 97, 150 if EMU else 333
    for index in ("i64", "u32", None):
        for div in ((1, 2, 8) if index else (1,)):
            for perm in (False, True):
                c = _case(rng, rows, dim, min(n, rows) if index is None else n, sd, index, div,
                          perm)
                _run_copy(torch, sok, [c], sd, dd)
    # src_rows = 0: only the sign of a row is checked
    c = _case(rng, rows, dim, n, sd, "i64", 1, True, src_rows=0, bad=False)
    c["index"][::5] = -1
    _run_copy(torch, sok, [c], sd, dd)


def test_indexed_row_copy_26_tasks_of_mixed_shape_in_one_call():
    import torch
    from hugectr_amd import sok
    rng = np.random.default_rng(26)
    dims = [1, 3, 4, 8, 12, 16, 32, 64, 128, 130, 256, 20, 100] * 2
    cases = []
    for t, dim in enumerate(dims):
        n = 0 if t == 7 else int(rng.integers(1, 90 if EMU else 400))
        cases.append(_case(rng, int(rng.integers(1, 60)), dim, n, "f32",
                           ("i64", "u32")[t % 2], (1, 2, 8)[t % 3], perm=t % 4 == 0))
    assert len(cases) == 26
    for dd in ("f32", "f16"):
        _run_copy(torch, sok, cases, "f32", dd)


def test_indexed_row_copy_misaligned_views_take_the_element_path():
    import torch
    from hugectr_amd import sok
    rng = np.random.default_rng(5)
    for dim in (4, 128):
        c = _case(rng, 50, dim, 120, "f32", "i64", 1, True)
        base = torch.zeros(50 * dim + 1, dtype=torch.float32).cuda()
        view = base[1:].view(50, dim)          # 4 bytes off a 16-byte boundary
        view.copy_(torch.from_numpy(c["src"]).cuda())
        assert view.data_ptr() % 16 == 4
        c["src_t"] = view
        _run_copy(torch, sok, [c], "f32", "f32")


# ---- group_lookup -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("plain", [False, True])
def test_group_lookup_on_the_reference_op_test_data(dtype, plain):
    """R/sparse_operation_kit/sparse_operation_kit/test/op_test/lookup/group_lookup_test.py:22-37"""
    import torch
    from hugectr_amd import sok
    sok.init()
    dt = getattr(torch, dtype)
    t1 = np.arange(12, dtype=np.float32).reshape(3, 4)
    t2 = np.arange(15, dtype=np.float32).reshape(5, 3)
    if plain:
        params = [torch.from_numpy(t1).cuda(), torch.from_numpy(t2).cuda()]
    else:
        params = [sok.Variable(t1), sok.Variable(t2)]
    i1 = torch.tensor([0, 1], dtype=torch.int32).cuda()
    i2 = torch.tensor([1, 2, 3], dtype=torch.int32).cuda()
    outs = sok.group_lookup(params, [i1, i2], dtype=dt)
    assert isinstance(outs, list) and len(outs) == 2
    assert outs[0].dtype == dt and outs[1].dtype == dt
    assert outs[0].detach().cpu().numpy().tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert outs[1].detach().cpu().numpy().tolist() == [[3, 4, 5], [6, 7, 8], [9, 10, 11]]
    one = sok.group_lookup(params[0], i1, dtype=dt)   # one item: still a list
    assert isinstance(one, list) and torch.equal(one[0].detach(), outs[0].detach())


def test_group_lookup_shapes_and_gradients():
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(8)
    tabs = [rng.standard_normal((40, 8)).astype(np.float32),
            rng.standard_normal((9, 130)).astype(np.float32),
            rng.standard_normal((25, 16)).astype(np.float32)]
    vs = [sok.Variable(tabs[0]), sok.Variable(tabs[1])]
    plain = torch.nn.Parameter(torch.from_numpy(tabs[2]).cuda())
    twin = torch.nn.Parameter(torch.from_numpy(tabs[2]).cuda())
    refs = [torch.from_numpy(t).cuda().requires_grad_() for t in tabs[:2]]
    idx = [torch.from_numpy(rng.integers(0, 40, size=(6, 5))).cuda(),
           torch.from_numpy(rng.integers(0, 9, size=17).astype(np.int32)).cuda(),
           torch.from_numpy(rng.integers(0, 25, size=(3, 2, 4))).cuda()]
    outs = sok.group_lookup(vs + [plain], idx)
    want = [r[i.long()] for r, i in zip(refs, idx)] + \
        [torch.nn.functional.embedding(idx[2], twin, sparse=True)]
    gs = []
    for o, w, i in zip(outs, want, idx):
        assert tuple(o.shape) == tuple(i.shape) + (w.shape[-1],)
        assert torch.equal(o.detach(), w.detach())
        gs.append(torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float32)).cuda())
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    sum((w * g).sum() for w, g in zip(want, gs)).backward()
    # the plain parameter: a sparse gradient, as nn.Embedding(sparse=True) gives
    assert plain.grad.is_sparse and twin.grad.is_sparse
    assert plain.grad._nnz() == idx[2].numel()         # uncoalesced
    assert torch.equal(plain.grad.coalesce().indices(), twin.grad.coalesce().indices())
    assert torch.allclose(plain.grad.to_dense(), twin.grad.to_dense(), rtol=1e-6, atol=1e-6)
    # the SOK variables: applied by OptimizerWrapper.step
    sok.OptimizerWrapper("sgd", lr=0.1).step(vs)
    for v, r in zip(vs, refs):
        new = (r - 0.1 * r.grad).detach()
        assert torch.allclose(v.weight, new, rtol=1e-5, atol=1e-6)
    # fp16 output carries gradients too
    o16 = sok.group_lookup(vs[0], idx[0], dtype=torch.float16)[0]
    assert torch.equal(o16.detach(), vs[0].weight[idx[0]].half())
    o16.float().sum().backward()
    assert len(vs[0]._pending) == 1
    vs[0]._pending.clear()


# ---- all2all_dense_embedding, one rank ----------------------------------------------------------
@pytest.mark.parametrize("shape", [(50,), (7, 9)])
@pytest.mark.parametrize("idt", ["int32", "int64"])
def test_all2all_dense_static_variable_equals_indexing(shape, idt):
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(len(shape) + len(idt))
    tab = rng.standard_normal((64, 20)).astype(np.float32)
    var = sok.Variable(tab)
    full = torch.from_numpy(tab).cuda().requires_grad_()
    idx = torch.from_numpy(rng.integers(0, 64, size=shape).astype(idt)).cuda()
    out = sok.all2all_dense_embedding(var, idx)
    want = full[idx.long()]
    assert tuple(out.shape) == shape + (20,) and out.dtype == torch.float32
    assert torch.equal(out.detach(), want.detach())
    g = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).cuda()
    (out * g).sum().backward()
    (want * g).sum().backward()
    sok.OptimizerWrapper("sgd", lr=0.5).step([var])
    assert torch.allclose(var.weight, (full - 0.5 * full.grad).detach(), rtol=1e-5, atol=1e-6)


def _dyn(sok, kind, D):
    C, S = 1024, 128
    if kind == "hbm":
        return sok.DynamicVariable(D, "")
    if kind == "hybrid":
        return sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=C, max_bucket_size=S)
    gib = (C // 2) * D * 4 / float(1 << 30)     # H = C / 2 slots in HBM, the rest in host memory
    v = sok.DynamicVariable(D, "", var_type="hybrid", max_capacity=C, max_bucket_size=S,
                            max_hbm_for_vectors=gib)
    assert v.tiered and v._lru.hbm_slots == C // 2
    return v


@pytest.mark.parametrize("kind", ["hbm", "hybrid", "tiered"])
def test_all2all_dense_dynamic_variable_equals_lookup_sparse_with_one_key_per_row(kind):
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(31)
    D = 16
    a, b = _dyn(sok, kind, D), _dyn(sok, kind, D)
    opt_a, opt_b = sok.OptimizerWrapper("sgd", lr=0.1), sok.OptimizerWrapper("sgd", lr=0.1)
    for step in range(3):
        shape = (40, 6) if step % 2 else (300,)
        keys = torch.from_numpy(rng.integers(0, 700, size=shape) * 7919).cuda()
        out = sok.all2all_dense_embedding(a, keys)
        flat = keys.reshape(-1)
        ref = sok.lookup_sparse(b, sok.Ragged(flat, torch.ones_like(flat)), combiners="sum")
        assert tuple(out.shape) == shape + (D,)
        assert torch.equal(out.detach().reshape(-1, D), ref.detach()), (kind, step)
        assert float(out.detach().std()) > 0          # (not a table of one value)
        assert a.size == b.size
        g = torch.from_numpy(rng.standard_normal((flat.numel(), D)).astype(np.float32)).cuda()
        (out.reshape(-1, D) * g).sum().backward()
        (ref * g).sum().backward()
        opt_a.step([a])
        opt_b.step([b])
    # evaluation lookup: stored keys as they are, unknown keys zero, nothing inserted
    size = a.size
    unk = torch.tensor([10**12, 3, 10**12 + 5], dtype=torch.int64).cuda()
    z = sok.all2all_dense_embedding(a, unk, training=False)
    assert float(z.detach().abs().max()) == 0.0 and a.size == size
    known = flat[:20].contiguous()
    assert torch.equal(sok.all2all_dense_embedding(a, known, training=False).detach(),
                       sok.lookup_sparse(b, sok.Ragged(known, torch.ones_like(known)),
                                         combiners="sum", training=False).detach())
    assert a.size == b.size == size


@pytest.mark.skipif(EMU, reason="81920 x 128 table, 8192 keys per step")
def test_all2all_dense_reference_training_scenario():
    """R/sparse_operation_kit/sparse_operation_kit/test/function_test/tf2/lookup/
    all2all_dense_embedding_test.py: table 81920 x 128, 8192 keys per step, loss = sum, SGD lr 1.0
    (5 steps here, 100 there), against index_add_ in fp32, with that test's own criterion (:111-121)"""
    import torch
    from hugectr_amd import sok
    sok.init()
    rng = np.random.default_rng(0)
    row, col, batch, iters = 8192 * 10, 128, 8192, 5
    weight = rng.random((row, col)).astype(np.float32)
    var = sok.Variable(weight)
    ref = torch.from_numpy(weight).cuda()
    total = torch.from_numpy(rng.integers(0, row, size=(iters, batch))).cuda()
    opt = sok.OptimizerWrapper("sgd", lr=1.0)
    loss1, loss2 = [], []
    for i in range(iters):
        loss = sok.all2all_dense_embedding(var, total[i]).sum()
        loss.backward()
        opt.step([var])
        loss1.append(float(loss.detach()))
        loss2.append(float(ref[total[i]].sum()))
        ref.index_add_(0, total[i], torch.full((batch, col), -1.0, device=ref.device))
    out1, out2 = var.weight.double(), ref.double()
    diff = float(((out1 - out2) ** 2 / (out1 ** 2 + out2 ** 2 + 1e-8)).sum())
    ldiff = sum((a - b) ** 2 / (a ** 2 + b ** 2 + 1e-8) for a, b in zip(loss1, loss2))
    print(f"table diff {diff:.3e}  loss diff {ldiff:.3e}")
    assert diff < 1e-6
    assert ldiff < 1e-6


# ---- refusals -----------------------------------------------------------------------------------
def test_dense_lookups_refuse_what_they_cannot_serve():
    import torch
    from hugectr_amd import sok
    sok.init()
    tab = np.zeros((8, 4), dtype=np.float32)
    idx = torch.arange(4).cuda()
    with pytest.raises(TypeError):
        sok.all2all_dense_embedding(sok.Variable(tab, mode="localized:0"), idx)
    with pytest.raises(TypeError):
        sok.all2all_dense_embedding(sok.Variable(tab), idx.float())
    with pytest.raises(TypeError):
        sok.all2all_dense_embedding(torch.from_numpy(tab).cuda(), idx)
    with pytest.raises(TypeError):
        sok.group_lookup(sok.Variable(tab), idx.float())
    with pytest.raises(TypeError):
        sok.group_lookup(sok.DynamicVariable(4), idx)
    with pytest.raises(TypeError):
        sok.group_lookup(sok.Variable(tab), idx, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        sok.group_lookup([sok.Variable(tab)], [idx, idx])
    # a variable localized on this GPU is wholly held here
    out = sok.group_lookup(sok.Variable(tab + 1, mode="localized:0"), idx)[0]
    assert float(out.detach().min()) == 1.0


# ---- two ranks over gloo, both on this GPU ------------------------------------------------------
def _worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from hugectr_amd import sok
        sok.init()
        rng = np.random.default_rng(77)               # the same stream on both ranks
        R, D, lr = 41, 12, 0.1
        tab = rng.standard_normal((R, D)).astype(np.float32)
        var = sok.Variable(tab)                        # rows r % 2 == rank live here
        dyn = sok.DynamicVariable(D, initializer="ones")
        full = torch.from_numpy(tab).cuda().requires_grad_()
        with pytest.raises(TypeError):
            sok.group_lookup(var, torch.arange(3).cuda())
        with pytest.raises(TypeError):
            sok.all2all_dense_embedding(sok.Variable(tab, mode="localized:1"),
                                        torch.arange(3).cuda())
        opt = sok.OptimizerWrapper("sgd", lr=lr)
        seen, dyn_ref = set(), {}
        shapes = [((5, 3), (5, 3)), ((16,), (4, 2)), ((6,), (9,))]
        for step, shp in enumerate(shapes):
            idx_all = [rng.integers(0, R, size=s) for s in shp]
            if step == 2:
                idx_all[0] = idx_all[0] // 2 * 2       # rank 0 asks for even keys only: it sends
                #                                        nothing to rank 1
            g_all = [rng.standard_normal(s + (D,)).astype(np.float32) for s in shp]
            idx = torch.from_numpy(idx_all[rank]).cuda()
            g = torch.from_numpy(g_all[rank]).cuda()
            out = sok.all2all_dense_embedding(var, idx)
            assert tuple(out.shape) == shp[rank] + (D,)
            assert torch.equal(out.detach(), full.detach()[idx]), ("forward", step)
            (out * g).sum().backward()
            for r in range(world):
                (full[torch.from_numpy(idx_all[r]).cuda()]
                 * torch.from_numpy(g_all[r]).cuda()).sum().backward()
            opt.step([var])
            new_full = (full - lr * full.grad).detach()
            full.grad = None
            assert torch.allclose(var.weight, new_full[rank::world], rtol=1e-5, atol=1e-6), step
            with torch.no_grad():                      # keep the copies of the table in step
                full.copy_(new_full)
                var.weight.copy_(new_full[rank::world])
            # dynamic variable: all-ones rows; every key lives on the rank key % 2
            want = np.stack([dyn_ref.get(int(k), np.ones(D, np.float32))
                             for k in idx_all[rank].reshape(-1)]).reshape(shp[rank] + (D,))
            out = sok.all2all_dense_embedding(dyn, idx)
            assert np.allclose(out.detach().cpu().numpy(), want, rtol=1e-5, atol=1e-6), step
            (out * g).sum().backward()
            opt.step([dyn])
            sums = {}
            for r in range(world):
                for k, gr in zip(idx_all[r].reshape(-1), g_all[r].reshape(-1, D)):
                    sums[int(k)] = sums.get(int(k), 0) + gr.astype(np.float64)
            for k, s in sums.items():
                dyn_ref[k] = dyn_ref.get(k, np.ones(D, np.float32)) - lr * s.astype(np.float32)
            seen |= {int(k) for r in range(world) for k in idx_all[r].reshape(-1)
                     if k % world == rank}
            assert dyn.size == len(seen), (dyn.size, len(seen))
        ks, vals = sok.export(dyn)
        assert sorted(ks.cpu().numpy().tolist()) == sorted(seen)
        for k, x in zip(ks.cpu().numpy().tolist(), vals.cpu().numpy()):
            assert np.allclose(x, dyn_ref[k], rtol=1e-5, atol=1e-6), k
        # an evaluation lookup of keys nobody holds: zeros, nothing inserted, on both ranks
        z = sok.all2all_dense_embedding(dyn, torch.tensor([10**9 + rank, 10**9 + 7]).cuda(),
                                        training=False)
        assert float(z.detach().abs().max()) == 0.0 and dyn.size == len(seen)
        # a rank without indices still takes part
        n0 = 0 if rank == 1 else 5
        e = sok.all2all_dense_embedding(var, torch.arange(n0).cuda())
        assert tuple(e.shape) == (n0, D) and torch.equal(e.detach(), full.detach()[:n0])
        ret[rank] = "ok"
    except BaseException as e:  # surface the failure in the parent
        import traceback
        ret[rank] = "".join(traceback.format_exception(type(e), e, e.__traceback__))
    finally:
        dist.destroy_process_group()


def test_all2all_dense_two_ranks_on_one_gpu_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    for p in procs:
        if p.is_alive():
            p.terminate()
    for r in range(2):
        if ret.get(r) != "ok":
            print(f"--- rank {r} ---\n{ret.get(r)}")
    assert ret.get(0) == "ok" and ret.get(1) == "ok"
