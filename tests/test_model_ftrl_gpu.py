"""hugectr.Model on Optimizer_t.Ftrl trains its DENSE layers with Ftrl (FtrlOptimizer of the
reference, R/HugeCTR/src/optimizers/ftrl_optimizer.cu; R/samples/ftrl/dlrm_train_ftrl.py:185-192):
on the generic path (fp32, InnerProduct + ReLU: dense.DenseFtrl, one hctr_ftrl_segments launch per
step) and on the flat path (use_mixed_precision, Layer_t.MLP: hctr_ftrl_shadow per MLP).  Models
are built as the sample builds them: static embedding_collection tables, per-lookup top names and
a Concat.  Batches are handed over resident in HBM (Model.reader_override).  The step oracle and
its tolerance are those of tests/test_dense_ftrl_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dense_ftrl_gpu as K  # noqa: E402  (oracle_step, close, check_step)

pytestmark = pytest.mark.gpu

S, EV, ROWS, B = 4, 16, 50, 256
EPS = K.EPS


class _Cycle:
    def __init__(self, batches):
        self.b, self.i = batches, 0

    def next_batch(self, train: bool):
        self.i += 1
        return self.b[(self.i - 1) % len(self.b)]

    def has_eval(self):
        return False


def _batches(n, seed=3, world=1, rank=0):
    """n batches of B samples: the sparse CSR of the whole batch (every rank routes it), this
    rank's share of the dense features and labels; the label is a function of a dense feature and
    a key"""
    g = torch.Generator().manual_seed(seed)
    bl = B // world
    sl = slice(rank * bl, (rank + 1) * bl)
    ro = torch.arange(B + 1, dtype=torch.int64).cuda()
    out = []
    for _ in range(n):
        keys = torch.randint(0, ROWS, (B, S), generator=g)
        dense = torch.rand((B, 13), generator=g)
        lab = ((dense[:, 0] + 0.25 * (keys[:, 0] % 2).float()) > 0.6).float().view(B, 1)
        out.append({"dense": dense[sl].cuda(), "label": lab[sl].cuda(),
                    "sparse": {f"data{i}": (ro, keys[:, i].contiguous().cuda())
                               for i in range(S)}})
    return out


def _build(batches, mixed, lr=0.05, beta=0.0, lambda1=0.0, lambda2=0.0, world=1, **solver_kw):
    """the sample's model in small: generic path = fp32 InnerProduct + ReLU, flat path =
    use_mixed_precision + Layer_t.MLP.  The same seed gives every model the same initial weights."""
    import hugectr_amd.hugectr as hugectr
    torch.manual_seed(11)
    solver = hugectr.CreateSolver(max_eval_batches=1, batchsize_eval=B, batchsize=B, lr=lr,
                                  vvgpu=[list(range(world))], repeat_dataset=True,
                                  i64_input_key=True, use_mixed_precision=mixed,
                                  scaler=1024.0 if mixed else 1.0, **solver_kw)
    reader = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet,
                                      source=["(batches resident in HBM)"], eval_source="",
                                      check_type=hugectr.Check_t.Non)
    opt = hugectr.CreateOptimizer(optimizer_type=hugectr.Optimizer_t.Ftrl,
                                  update_type=hugectr.Update_t.Global, beta=beta, lambda1=lambda1,
                                  lambda2=lambda2)
    m = hugectr.Model(solver, reader, opt)
    m.add(hugectr.Input(label_dim=1, label_name="label", dense_dim=13, dense_name="dense",
                        data_reader_sparse_param_array=[
                            hugectr.DataReaderSparseParam(f"data{i}", 1, True, 1)
                            for i in range(S)]))
    names = [str(i) for i in range(S)]
    ebc = hugectr.EmbeddingCollectionConfig(use_exclusive_keys=True)
    for i in range(S):
        ebc.embedding_lookup(table_config=hugectr.EmbeddingTableConfig(names[i], ROWS, EV),
                             bottom_name=f"data{i}", top_name=f"emb_vec{i}", combiner="sum")
    per = S // world
    ebc.shard(shard_matrix=[names[r * per:(r + 1) * per] for r in range(world)],
              shard_strategy=[("mp", names)])
    m.add(ebc)
    L, T, A = hugectr.DenseLayer, hugectr.Layer_t, hugectr.Activation_t
    embs = [f"emb_vec{i}" for i in range(S)]
    if mixed:
        m.add(L(layer_type=T.MLP, bottom_names=["dense"], top_names=["mlp1"], num_outputs=[32, 16],
                act_type=A.Relu))
        m.add(L(layer_type=T.Concat, bottom_names=embs + ["mlp1"], top_names=["concat1"]))
        m.add(L(layer_type=T.MLP, bottom_names=["concat1"], top_names=["fc2"], num_outputs=[32, 1],
                activations=[A.Relu, A.Non]))
    else:
        m.add(L(layer_type=T.Concat, bottom_names=embs + ["dense"], top_names=["concat1"]))
        m.add(L(layer_type=T.InnerProduct, bottom_names=["concat1"], top_names=["fc1"],
                num_output=32))
        m.add(L(layer_type=T.ReLU, bottom_names=["fc1"], top_names=["relu1"]))
        m.add(L(layer_type=T.InnerProduct, bottom_names=["relu1"], top_names=["fc2"], num_output=1))
    m.add(L(layer_type=T.BinaryCrossEntropyLoss, bottom_names=["fc2", "label"], top_names=["loss"]))
    m.reader_override = _Cycle(batches)
    m.compile()
    assert len(m._ebc) == 1
    assert bool(m._flat_mlps) == (mixed and os.environ.get("HCTR_MODEL_FUSED_DENSE", "1") != "0")
    return m


def _dense(m):
    return [q.detach().clone() for q in m._dense_params]


# -- 1. known answer -------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["generic_fp32", "flat_mixed"])
def test_huge_lambda1_leaves_every_dense_parameter_zero(mixed):
    """lambda1 = 1e6: |z'| never exceeds it, so ONE Ftrl step leaves every dense parameter exactly
    0.0 (and the flat path's 16-bit copies).  Plain SGD, what the dense layers of a Ftrl model were
    trained with before, leaves them non-zero."""
    m = _build(_batches(1), mixed, lambda1=1e6)
    before = _dense(m)
    assert all(bool((q != 0).any()) for q in before)
    assert m.train()
    torch.cuda.synchronize()
    for q in m._dense_params:
        assert q.numel() > 0 and bool((q == 0).all())
    if mixed:
        for mlp in m._flat_mlps:
            assert bool((mlp.flat_w16 == 0).all()) and bool((mlp.flat_w == 0).all())
    else:
        from hugectr_amd.dense import DenseFtrl
        assert isinstance(m._dense_opt, DenseFtrl)


def test_ftrl_models_stay_out_of_the_captured_step():
    """solver.use_cuda_graph is on by default; a model with dense Ftrl is kept out of the captured
    step at compile (DESIGN.md "Dense-tower glue") and runs eager launches"""
    m = _build(_batches(1), False)
    assert m.solver.use_cuda_graph and m._graph_ok is False


# -- 2. loss curve ---------------------------------------------------------------------------------
class _Tower:
    """the dense layers of the graph in plain torch fp32 on the CPU, formulas written out (the
    independent-path pattern of tests/test_loss_curve_gpu.py)"""

    def __init__(self, m, params=None):
        import hugectr_amd.hugectr as hugectr
        self.T, self.layers, self.p = hugectr.Layer_t, m.layers, {}
        for i, L in enumerate(m.layers):
            mod = m._mods[f"l{i}"] if f"l{i}" in m._mods else None
            if L.layer_type == self.T.InnerProduct:
                self.p[i] = [mod.weight, mod.bias]
            elif L.layer_type == self.T.MLP:
                self.p[i] = [w for pair in zip(mod.weights, mod.biases) for w in pair]
        for i in self.p:
            self.p[i] = [q.detach().float().cpu().clone().requires_grad_(True) for q in self.p[i]]
        self.params = [q for i in sorted(self.p) for q in self.p[i]]

    def loss(self, tensors):
        T = self.T
        for i, L in enumerate(self.layers):
            x = [tensors[b] for b in L.bottom_names]
            if L.layer_type == T.InnerProduct:
                y = x[0] @ self.p[i][0].t() + self.p[i][1]
            elif L.layer_type == T.MLP:
                y, ps = x[0], self.p[i]
                acts = L.activations or [L.act_type] * len(L.num_outputs)
                for k in range(len(ps) // 2):
                    y = y @ ps[2 * k].t() + ps[2 * k + 1]
                    if getattr(acts[k], "name", "") == "Relu":
                        y = torch.relu(y)
            elif L.layer_type == T.ReLU:
                y = torch.relu(x[0])
            elif L.layer_type == T.Concat:
                y = torch.cat(x, dim=1)
            elif L.layer_type == T.BinaryCrossEntropyLoss:
                return torch.nn.functional.binary_cross_entropy_with_logits(x[0], x[1])
            else:
                raise AssertionError(L.layer_type)
            tensors[L.top_names[0]] = y


class _TorchFtrl:
    """the step of ftrl_update_kernel with elementwise torch ops (fp32, CPU)"""

    def __init__(self, params, lr, beta, l1, l2):
        self.params, self.h = params, (lr, beta, l1, l2)
        self.z = [torch.zeros_like(p) for p in params]
        self.n = [torch.zeros_like(p) for p in params]

    @torch.no_grad()
    def step(self):
        lr, beta, l1, l2 = self.h
        for p, z, n in zip(self.params, self.z, self.n):
            g = p.grad
            n1 = n + g * g
            z1 = z + g + ((n + EPS).sqrt() - (n1 + EPS).sqrt()) * p / lr
            sgn = torch.where(torch.signbit(z1), -torch.ones_like(z1), torch.ones_like(z1))
            w = (l1 * sgn - z1) / ((n1 + EPS).sqrt() / lr + (l2 + beta / lr))
            p.copy_(torch.where(z1.abs() > l1, w, torch.zeros_like(w)))
            z.copy_(z1)
            n.copy_(n1)
            p.grad = None


LOSS_STEPS = 24
LOSS_HP = dict(lr=0.02, beta=0.0, lambda1=0.0, lambda2=0.0)


@pytest.mark.parametrize("mixed", [False, True], ids=["generic_fp32", "flat_mixed"])
def test_loss_curve_follows_an_independent_ftrl_tower(mixed):
    """24 steps: the model's per-step loss against a plain-torch fp32 replica of the dense tower
    stepped by a Ftrl written here with elementwise torch ops, within the tolerances of
    tests/test_loss_curve_gpu.py (1e-3 fp32, 1e-2 mixed).  The replica reads the embedding vectors
    the model looked up in that step (the sparse side is not what this test is about), everything
    behind them is its own.

    The same replica stepped by plain SGD (what the model's dense layers did before) leaves the
    band: Ftrl's first step forgets the initial weights (z starts at 0) and, with lambda2 = beta
    = 0, then moves every weight by up to lr per step, while SGD at lr = 0.02 hardly moves them.
    Observed with the replicas alone on these inputs (CPU): max relative distance SGD replica /
    Ftrl replica 1.9e-1 (the fp32 model's tower) and 5.4e-1 (the mixed model's) over the 24
    steps; the test asserts at least 2x the band."""
    batches = _batches(LOSS_STEPS)
    m = _build(batches, mixed, **LOSS_HP)
    seen = []
    fwd = m._ebc_forward

    def spy(rt, batch, train):
        E = fwd(rt, batch, train)
        seen.append(E.detach().float().cpu())
        return E
    m._ebc_forward = spy
    ftrl_tower, sgd_tower = _Tower(m), _Tower(m)
    ftrl = _TorchFtrl(ftrl_tower.params, LOSS_HP["lr"], LOSS_HP["beta"], LOSS_HP["lambda1"],
                      LOSS_HP["lambda2"])
    sgd = torch.optim.SGD(sgd_tower.params, lr=LOSS_HP["lr"])
    got, want, other = [], [], []
    for s in range(LOSS_STEPS):
        assert m.train()
        got.append(m.get_current_loss())
        E = seen[-1]
        for tower, out in ((ftrl_tower, want), (sgd_tower, other)):
            tensors = {"dense": batches[s]["dense"].cpu(), "label": batches[s]["label"].cpu()}
            tensors.update({f"emb_vec{i}": E[:, i, :] for i in range(S)})
            loss = tower.loss(tensors)
            loss.backward()
            out.append(float(loss.detach()))
        ftrl.step()
        sgd.step()
        sgd.zero_grad()
    got, want, other = np.array(got), np.array(want), np.array(other)
    tol = 1e-2 if mixed else 1e-3
    rel = np.abs(got - want) / np.abs(want)
    sep = np.abs(other - want) / np.abs(want)
    print(f"max rel distance model / Ftrl replica {rel.max():.2e}, SGD replica / Ftrl replica "
          f"{sep.max():.2e}")
    assert sep.max() > 2 * tol, f"the SGD replica stays within the band: {sep.max():.2e}"
    assert rel.max() < tol, f"max rel loss difference {rel.max():.2e} at step {rel.argmax()}"


# -- the step of a model against the oracle ---------------------------------------------------------
def _spy_steps(m):
    """records (lr, grad_scale, [w, z, n, g] before, [w, z, n] after) of every dense Ftrl launch
    of the model, as fp32 numpy over the parameters' elements"""
    log = []
    if m._flat_mlps:
        for mlp in m._flat_mlps:
            def spy(lr, beta, l1, l2, gs, mlp=mlp, real=mlp.ftrl_step):
                pre = [t.detach().cpu().numpy().copy()
                       for t in (mlp.flat_w, mlp.flat_z, mlp.flat_n, mlp.flat_g)]
                real(lr, beta, l1, l2, gs)
                assert torch.equal(mlp.flat_w16, mlp.flat_w.to(mlp.dtype))
                log.append((lr, gs, pre, [t.detach().cpu().numpy().copy()
                                          for t in (mlp.flat_w, mlp.flat_z, mlp.flat_n)]))
            mlp.ftrl_step = spy
        return log
    opt = m._dense_opt

    def spy(real=opt.step):
        pre = _opt_state(opt) + [_opt_grads(opt)]
        real()
        log.append((opt.param_groups[0]["lr"], 1.0 / opt.scaler, pre, _opt_state(opt)))
    opt.step = spy
    return log


def _opt_state(opt):
    w = np.concatenate([p.detach().flatten().cpu().numpy() for p in opt._params])
    z = np.concatenate([z.cpu().numpy() for z, _ in opt.ftrl_state()])
    n = np.concatenate([n.cpu().numpy() for _, n in opt.ftrl_state()])
    return [w, z, n]


def _opt_grads(opt):
    return np.concatenate([p.grad.detach().flatten().cpu().numpy() for p in opt._params])


def _check_logged(entry, hp, what):
    lr, gs, (w, z, n, g), (w1, z1, n1) = entry
    want = K.oracle_step(w, z, n, g, lr=lr, beta=hp["beta"], l1=hp["lambda1"], l2=hp["lambda2"],
                         gs=gs)
    ww, wz, wn = want
    assert K.close(z1, wz).all(), f"{what}: z"
    assert K.close(n1, wn).all(), f"{what}: n"
    # w: every element is compared; one may miss only on the branch edge, and 0.1 % at the most
    bad = ~K.close(w1, ww)
    edge = np.abs(np.abs(wz) - hp["lambda1"]) <= 1e-5 * (1 + np.abs(wz))
    assert not (bad & ~edge).any(), f"{what}: w"
    assert bad.mean() <= 1e-3, f"{what}: {bad.mean():.2%} of w off on the branch edge"
    assert (ww != 0).mean() > 0.2, f"{what}: the step left next to nothing"


# -- 3. set_learning_rate -----------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["generic_fp32", "flat_mixed"])
def test_set_learning_rate_reaches_the_dense_ftrl_step(mixed):
    """two models fed the same batches, one given set_learning_rate(lr / 4) after step 1: the
    launches of step 2 carry lr and lr / 4, each step matches the oracle on the state and the
    gradient it was given, and the dense weights differ after step 2.  (Ftrl models stay out of
    the captured step, so there is no use_cuda_graph case.)"""
    hp = dict(lr=0.05, beta=0.9, lambda1=1e-5, lambda2=0.1)
    a = _build(_batches(2), mixed, **hp)
    b = _build(_batches(2), mixed, **hp)
    for x, y in zip(_dense(a), _dense(b)):
        assert torch.equal(x, y)
    la, lb = _spy_steps(a), _spy_steps(b)
    assert a.train() and b.train()
    for x, y in zip(_dense(a), _dense(b)):
        assert torch.equal(x, y)
    b.set_learning_rate(hp["lr"] / 4)
    assert a.train() and b.train()
    torch.cuda.synchronize()
    per = len(la) // 2
    assert per >= 1 and len(la) == len(lb) == 2 * per
    assert {e[0] for e in la} == {hp["lr"]}
    assert [e[0] for e in lb] == [hp["lr"]] * per + [hp["lr"] / 4] * per
    assert all(e[1] == 1.0 / a.solver.scaler for e in la + lb)
    for k, e in enumerate(la + lb):
        _check_logged(e, hp, f"launch {k}")
    assert any(not torch.equal(x, y) for x, y in zip(_dense(a), _dense(b)))


# -- 4. DenseFtrl alone ------------------------------------------------------------------------------
def test_dense_ftrl_optimizer_alone():
    """DenseFtrl on parameters of shapes (1,), (3, 5), (64, 13), (7,) with .grad written by the
    test and scaler = 1024: three steps against the oracle; .grad is the same storage before and
    after zero_grad(set_to_none=True) and zero after it; state_dict -> a fresh DenseFtrl ->
    load_state_dict -> the next step is bit-identical to continuing"""
    from hugectr_amd.dense import DenseFtrl
    hp = dict(lr=K.LR, beta=K.BETA, lambda1=K.L1, lambda2=K.L2)
    shapes = [(1,), (3, 5), (64, 13), (7,)]
    rng = np.random.default_rng(5)
    w0 = [rng.uniform(-0.1, 0.1, s).astype(np.float32) for s in shapes]
    grads = [[(0.1 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
             for _ in range(4)]
    grads[0][2][:2] = 0.0
    params = [torch.nn.Parameter(torch.tensor(w).cuda()) for w in w0]
    opt = DenseFtrl(params, scaler=1024.0, **hp)
    views = [p.grad for p in params]
    assert all(v is not None and v.data_ptr() % 16 == 0 for v in views)
    w = np.concatenate([a.ravel() for a in w0]).astype(np.float64)
    z, n = np.zeros_like(w), np.zeros_like(w)

    def give(step, to):
        for p, g in zip(to, grads[step]):
            p.grad.add_(torch.tensor(g).cuda() * 1024.0)  # (autograd accumulates in place)

    for s in range(3):
        give(s, params)
        opt.step()
        g = np.concatenate([a.ravel() for a in grads[s]])
        w, z, n = K.oracle_step(w, z, n, g)
        got = _opt_state(opt)
        K.check_step(got[0], got[1], got[2], (w, z, n), f"step {s + 1}")
        if s == 0:  # the zero-gradient elements
            assert bool((params[2].detach().flatten()[:26] == 0).all())
        opt.zero_grad(set_to_none=True)
        for p, v in zip(params, views):
            assert p.grad is v and bool((v == 0).all())
        assert bool((opt.flat_g == 0).all())
    # a .grad somebody dropped or replaced comes back into its view
    params[1].grad = None
    params[3].grad = torch.ones_like(params[3])
    opt.zero_grad()
    assert params[1].grad is views[1] and params[3].grad is views[3]
    # state_dict -> fresh optimizer on copies of the parameters -> the next step
    sd = opt.state_dict()
    assert [t.numel() for t in sd["z"]] == [1, 15, 832, 7] == [t.numel() for t in sd["n"]]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = DenseFtrl(twins, scaler=1024.0, **hp)
    opt2.load_state_dict(sd)
    give(3, params)
    give(3, twins)
    opt.step()
    opt2.step()
    torch.cuda.synchronize()
    for p, q in zip(params, twins):
        assert torch.equal(p, q)
    for (z1, n1), (z2, n2) in zip(opt.ftrl_state(), opt2.ftrl_state()):
        assert torch.equal(z1, z2) and torch.equal(n1, n2)
    with pytest.raises(ValueError):
        DenseFtrl(twins[:2], **hp).load_state_dict(sd)


# -- 5. checkpoint -----------------------------------------------------------------------------------
def _sparse_state(m):
    e = m._ebc[0]["train"]
    return [t.detach().clone() for t in (e.table, e.accum, e.ftrl_z)]


def _put_sparse_state(m, state):
    e = m._ebc[0]["train"]
    for dst, src in zip((e.table, e.accum, e.ftrl_z), state):
        dst.copy_(src)


@pytest.mark.parametrize("target", ["flat", "unfused"])
def test_dense_ftrl_state_travels_through_the_checkpoint(tmp_path, monkeypatch, target):
    """3 steps on the flat path, save_params_to_files, a new model + load_dense_weights +
    load_dense_optimizer_states: its step 4 equals the original's step 4 on the same batch.
    flat -> flat: bit for bit.  flat -> HCTR_MODEL_FUSED_DENSE=0 (DenseFtrl on the unflattened
    MLPs): the state loads exactly (asserted bit for bit), the step is compared within the 16-bit
    path's tolerance (1e-2 of each tensor's largest element) -- unfused, the logit layer's
    gradients come from library GEMMs instead of the fused head, in another summation order.
    The embedding table and its Ftrl state are carried over by hand: the sparse side is not what
    this test is about."""
    hp = dict(lr=0.05, beta=0.9, lambda1=1e-5, lambda2=0.1)
    batches = _batches(4)
    a = _build(batches, True, **hp)
    for _ in range(3):
        assert a.train()
    prefix = str(tmp_path / "ck")
    a.save_params_to_files(prefix, 3)
    assert os.path.exists(f"{prefix}_opt_dense_3.model")
    sparse3 = _sparse_state(a)
    state3 = [(z.clone(), n.clone()) for z, n in a._flat_ftrl_state()]
    assert any(bool((n != 0).any()) for _, n in state3)
    assert a.train()
    if target == "unfused":
        monkeypatch.setenv("HCTR_MODEL_FUSED_DENSE", "0")
    b = _build(batches[3:], True, **hp)
    b.load_dense_weights(f"{prefix}_dense_3.model")
    b.load_dense_optimizer_states(f"{prefix}_opt_dense_3.model")
    _put_sparse_state(b, sparse3)
    got = b._flat_ftrl_state() if target == "flat" else b._dense_opt.ftrl_state()
    for (z, n), (z3, n3) in zip(got, state3):
        assert torch.equal(z, z3) and torch.equal(n, n3)
    assert b.train()
    torch.cuda.synchronize()
    for x, y in zip(_dense(a), _dense(b)):
        if target == "flat":
            assert torch.equal(x, y)
        else:
            assert float((x - y).abs().max()) <= 1e-2 * float(x.abs().max()) + 1e-7
    if target == "unfused":  # and the other way round: the unfused model's file loads into a flat one
        b.save_params_to_files(prefix + "_u", 4)
        monkeypatch.delenv("HCTR_MODEL_FUSED_DENSE")
        c = _build(batches, True, **hp)
        c.load_dense_optimizer_states(f"{prefix}_u_opt_dense_4.model")
        for (z, n), (z4, n4) in zip(c._flat_ftrl_state(), b._dense_opt.ftrl_state()):
            assert torch.equal(z, z4) and torch.equal(n, n4)


# -- 6. two ranks --------------------------------------------------------------------------------------
TWO_RANK_HP = dict(lr=0.05, beta=0.9, lambda1=1e-5, lambda2=0.1)


def _same_tables(m):
    """the same embedding rows however the tables are sharded (a rank's shard holds its tables'
    rows one table after the other; the initializer is seeded per shard)"""
    e = m._ebc[0]["train"]
    G = torch.rand((S * ROWS, EV), generator=torch.Generator().manual_seed(17)) * 0.1 - 0.05
    rows = S // m.world * ROWS
    assert tuple(e.table.shape) == (rows, EV)
    e.table.copy_(G[m.rank * rows:(m.rank + 1) * rows])


def _two_rank_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for mixed in (False, True):
            m = _build(_batches(3, world=world, rank=rank), mixed, world=world, **TWO_RANK_HP)
            _same_tables(m)
            for _ in range(3):
                assert m.train()
            torch.cuda.synchronize()
            ret[(rank, mixed)] = [q.detach().float().cpu().numpy() for q in m._dense_params]
        ret[rank] = "ok"
    except Exception as ex:
        import traceback
        ret[rank] = "".join(traceback.format_exception(type(ex), ex, ex.__traceback__))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_take_one_step_on_the_summed_gradient():
    """2 processes over gloo on this one GPU (the harness of
    test_legacy_embedding_model_two_ranks_on_one_gpu), generic and flat path: after 3 steps the
    ranks hold the same dense weights bit for bit (what that test asserts), and they equal the
    1-rank run on the same global batch within 1e-4 (fp32) / 1e-2 (mixed: the 16-bit path's
    tolerance, its split-K partial products are rounded to fp16) of each tensor's largest element
    -- the two runs differ in the summation order of the gradients only (two half-batch sums added
    by the all-reduce against one full-batch sum), while a Ftrl step per rank instead of ONE step
    on the summed gradient would accumulate n from the halves' squares and miss by tens of
    percent."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = 29500 + os.getpid() % 2000 + 31
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    single = {}
    for mixed in (False, True):
        m = _build(_batches(3), mixed, **TWO_RANK_HP)
        _same_tables(m)
        for _ in range(3):
            assert m.train()
        torch.cuda.synchronize()
        single[mixed] = [q.detach().float().cpu().numpy() for q in m._dense_params]
    for p in procs:
        p.join(600)
    for r in range(2):
        assert ret.get(r) == "ok", ret.get(r)
    for mixed in (False, True):
        r0, r1 = ret[(0, mixed)], ret[(1, mixed)]
        for x, y, one in zip(r0, r1, single[mixed]):
            assert (x == y).all()
            tol = 1e-2 if mixed else 1e-4
            assert np.abs(x - one).max() <= tol * np.abs(one).max() + 1e-7, (mixed, x.shape)
            assert np.abs(one).max() > 0
