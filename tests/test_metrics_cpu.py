"""CPU: the evaluation metrics' oracle (tests/metrics_oracle.py) against the two definitions it must
agree with -- `_auc` of hugectr.py (the parent's metric) and scikit-learn, which the reference's own
test/utest/metrics/python_sklearn.py checks against -- the argument checks of the hctr_metric_*
entry points, the naming / order of get_eval_metrics, and the kernels' logic under the host
interpreter of tests/emu."""
import ctypes

import numpy as np
import pytest

import metrics_oracle as mo


def _case(n, C, seed, ties=True):
    rng = np.random.default_rng(seed)
    p = rng.random((n, C), dtype=np.float32)
    if ties:
        p = np.round(p * 50) / np.float32(50)
    y = (rng.random((n, C)) < 0.35).astype(np.float32)
    return p.astype(np.float32), y


@pytest.mark.parametrize("n,ties", [(2, False), (100, True), (5000, True), (5000, False)])
def test_oracle_agrees_with_auc_of_hugectr(n, ties):
    import torch
    from hugectr_amd.hugectr import _auc
    p, y = _case(n, 1, n + ties, ties)
    got = mo.auc(p[:, 0], y[:, 0])
    want = _auc(torch.from_numpy(p[:, 0]), torch.from_numpy(y[:, 0]))
    assert abs(got - want) <= 1e-12
    assert mo.auc(p[:, 0], np.ones(n, np.float32)) == 0.5 == _auc(
        torch.from_numpy(p[:, 0]), torch.ones(n))


def test_oracle_agrees_with_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    for n, ties in ((100, True), (5000, True), (5000, False)):
        p, y = _case(n, 1, 7 * n + ties, ties)
        assert abs(mo.auc(p[:, 0], y[:, 0]) - sk.roc_auc_score(y[:, 0], p[:, 0])) <= 1e-12
    # the multi-class mean: what the reference's python_sklearn.py computes on [n, C] input
    p, y = _case(3000, 4, 99)
    mean, per = mo.auc_mean(p, y)
    assert len(per) == 4 and abs(mean - sk.roc_auc_score(y, p)) <= 1e-12
    # NDCG on tie-free scores
    rng = np.random.default_rng(3)
    p = rng.permutation(2000).astype(np.float32) / np.float32(2000)
    y = rng.integers(0, 5, 2000).astype(np.float32)
    assert abs(mo.ndcg(p, y) - sk.ndcg_score(y[None, :], p[None, :])) <= 1e-12


def test_keys_preserve_the_order_of_the_scores():
    f = np.array([-np.inf, -3.0e38, -1.5, -1.1e-38, -1e-45, -0.0, 0.0, 1e-45, 1.1e-38, 0.25, 1.5,
                  3.0e38, np.inf, np.nan], np.float32)
    k = mo.keys_of(f).astype(np.int64)
    assert k[5] == k[6] == 0x80000000, "-0.0 and +0.0 share a key"
    assert (np.diff(np.delete(k, 5)) > 0).all()
    assert k[-1] == 0xFFFFFFFF == mo.keys_of(np.array([-np.nan], np.float32))[0]


def test_oracle_small_case_by_hand():
    # scores 0.1 0.4 0.4 0.8, labels 0 1 0 1: pairs (pos, neg): (0.4,0.1)=1 (0.4,0.4)=1/2
    # (0.8,0.1)=1 (0.8,0.4)=1 -> U = 3.5, 2U = 7, AUC = 7 / 8
    w = mo.auc_words([0.1, 0.4, 0.4, 0.8], [0, 1, 0, 1])
    assert w == (7, 2, 2) and mo.auc_value(w) == 0.875
    assert mo.hitrate_words([np.float32(0.8), 0.9, 0.5], [1, 0, 1]) == (2, 1)
    assert mo.smape_words([0.0, 1.0], [0.0, 3.0]) == (1.0, 2)


def test_entry_points_validate_before_touching_the_device():
    from hugectr_amd import _lib
    L = _lib.lib
    buf = ctypes.create_string_buffer(64)
    q = ctypes.cast(buf, ctypes.c_void_p)  # a non-null pointer that is never followed
    tb = L.hctr_metric_accumulate_temp_bytes()
    assert tb > 0 and L.hctr_metric_auc_temp_bytes(1000) > 8000 < L.hctr_metric_ndcg_temp_bytes(1000)

    def acc(pred=q, label=q, n=4, C=1, keys=q, labels=q, cap=8, off=0, ct=q, tmp=q):
        rc = L.hctr_metric_accumulate(pred, 0, label, n, C, keys, labels, cap, off, ct, tmp, tb, None)
        return rc, _lib.last_error()

    for kw in ({"pred": None}, {"label": None}, {"keys": None}, {"labels": None}, {"ct": None},
               {"tmp": None}):
        rc, msg = acc(**kw)
        assert rc == -1 and "null" in msg, kw
    for C in (0, 257, -1):
        rc, msg = acc(C=C)
        assert rc == -1 and "C must be" in msg
    rc, msg = acc(n=5, cap=8, off=4)
    assert rc == -1 and "offset + n > cap" in msg
    rc, msg = acc(n=1, cap=8, off=9)
    assert rc == -1 and "offset + n > cap" in msg
    rc, msg = acc(n=2 ** 31, cap=2 ** 32)
    assert rc == -1 and "2^31" in msg
    rc = L.hctr_metric_accumulate(q, 7, q, 4, 1, q, q, 8, 0, q, q, tb, None)
    assert rc == -1 and "dtype" in _lib.last_error()
    for fn in (L.hctr_metric_auc, L.hctr_metric_ndcg):
        assert fn(q, 1 << 40, q, q, 2 ** 31, q, None) == -1 and "2^31" in _lib.last_error()
        for args in ((None, 1 << 40, q, q, 10, q), (q, 1 << 40, None, q, 10, q),
                     (q, 1 << 40, q, None, 10, q), (q, 1 << 40, q, q, 10, None)):
            assert fn(*args, None) == -1 and "null" in _lib.last_error()
        assert fn(q, 16, q, q, 10, q, None) == -1 and "workspace" in _lib.last_error()


class _MT:  # stands in for hugectr.MetricsType members where only .name matters
    def __init__(self, name):
        self.name = name


@pytest.mark.parametrize("spec,names", [
    (["AUC"], ["AUC", "AverageLoss"]),
    (["AverageLoss", "AUC"], ["AUC", "AverageLoss"]),
    (["SMAPE", "NDCG", "HitRate", "AverageLoss", "AUC"],
     ["AUC", "AverageLoss", "HitRate", "NDCG", "SMAPE"]),
    (["HitRate"], ["HitRate", "AverageLoss"]),
    (["SMAPE", "AUC", "NDCG"], ["AUC", "NDCG", "SMAPE", "AverageLoss"]),
])
def test_names_and_order_of_the_result(spec, names):
    from hugectr_amd.hugectr import MetricsType
    from hugectr_amd.metrics import EvalMetrics

    class Stub(EvalMetrics):
        def _values(self):
            return {"AUC": 0.75, "AverageLoss": 0.5, "HitRate": 0.25, "NDCG": 0.9, "SMAPE": 1.5}

    for keys in ([MetricsType[s] for s in spec], [_MT(s) for s in spec]):
        m = Stub({k: 1.0 for k in keys}, 1, 512, 2)
        assert m.result() == [] and not m, "nothing accumulated: empty and falsy"
        m.n = m.batches = 1
        assert [n for n, _ in m.result()] == names
        assert m.result() == m.result()
        m.reset()
        assert m.result() == [] and not m
    assert MetricsType.SMAPE.value == 4
    assert [t.name for t in sorted(MetricsType, key=lambda t: t.value)] == \
        ["AUC", "AverageLoss", "HitRate", "NDCG", "SMAPE"]


def test_multi_task_models_take_auc_only():
    from hugectr_amd.metrics import EvalMetrics
    EvalMetrics({_MT("AUC"): 0.8}, 2, 512, 2, num_loss_layers=2)
    with pytest.raises(RuntimeError, match="Metrics besides AUC are not supported for multi-task"):
        EvalMetrics({_MT("AUC"): 0.8, _MT("HitRate"): 0.0}, 2, 512, 2, num_loss_layers=2)
    with pytest.raises(RuntimeError, match="label columns"):
        EvalMetrics({_MT("AUC"): 0.8}, 257, 512, 2)


# ---- the kernels' logic under the host interpreter (device memory = numpy arrays) -------------------
@pytest.fixture(scope="module")
def emulib():
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import emu
    if not emu.available():
        pytest.skip("no host compiler for the interpreter")
    return emu, emu.load_under_test()


def _emu_store(emu, lib, p, y, pieces):
    n, C = y.shape
    cap = n + 3
    keys = np.full((C, cap), 0xFFFFFFFF, np.uint32)
    labs = np.full((C, cap), -7.0, np.float32)
    ct = np.zeros(264, np.uint64)
    tmp = np.zeros(lib.hctr_metric_accumulate_temp_bytes(), np.uint8)
    off = 0
    for k in pieces:
        pp, yy = np.ascontiguousarray(p[off:off + k]), np.ascontiguousarray(y[off:off + k])
        emu.check(lib, lib.hctr_metric_accumulate(emu.ptr(pp), 0, emu.ptr(yy), k, C, emu.ptr(keys),
                                                  emu.ptr(labs), cap, off, emu.ptr(ct), emu.ptr(tmp),
                                                  tmp.size, None))
        off += k
    return keys, labs, ct, cap


@pytest.mark.parametrize("n,C,pieces", [(1, 1, [1]), (65, 3, [64, 1]), (4097, 1, [1000, 1, 3096]),
                                        (9000, 2, [4097, 4903])])
def test_kernels_under_the_host_interpreter(emulib, n, C, pieces):
    emu, lib = emulib
    rng = np.random.default_rng(n)
    p = rng.choice(np.array([0.1, 0.2, 0.5, -0.0, 0.0, 0.9, np.nan, -2.0], np.float32), (n, C))
    p[::5] = rng.random((len(p[::5]), C), dtype=np.float32)
    y = (rng.random((n, C)) < 0.4).astype(np.float32)
    keys, labs, ct, cap = _emu_store(emu, lib, p, y, pieces)
    assert (ct[0], ct[1]) == mo.hitrate_words(p, y) and ct[2] == n * C and ct[4] == 0
    ok = ~np.isnan(p)  # (a NaN score makes the SMAPE sum NaN: checked on the rest)
    assert np.isnan(ct[3:4].view(np.float64)[0]) == (not ok.all())
    if not ok.all():
        ct2 = _emu_store(emu, lib, np.where(ok, p, np.float32(0.3)), y, pieces)[2]
        want = mo.smape_words(np.where(ok, p, np.float32(0.3)), y)[0]
        assert abs(ct2[3:4].view(np.float64)[0] - want) <= 1e-9 * abs(want)
    for c in range(C):
        assert (keys[c, :n] == mo.keys_of(p[:, c])).all() and (keys[c, n:] == 0xFFFFFFFF).all()
        out = np.full(3, 99, np.uint64)
        tb = lib.hctr_metric_auc_temp_bytes(n)
        tmp = np.zeros(tb, np.uint8)
        emu.check(lib, lib.hctr_metric_auc(emu.ptr(tmp), tb, ctypes.c_void_p(keys[c].ctypes.data),
                                           ctypes.c_void_p(labs[c].ctypes.data), n, emu.ptr(out), None))
        assert tuple(int(v) for v in out) == mo.auc_words(p[:, c], y[:, c])
        d = np.zeros(2, np.float64)
        tb = lib.hctr_metric_ndcg_temp_bytes(n)
        tmp = np.zeros(tb, np.uint8)
        emu.check(lib, lib.hctr_metric_ndcg(emu.ptr(tmp), tb, ctypes.c_void_p(keys[c].ctypes.data),
                                            ctypes.c_void_p(labs[c].ctypes.data), n, emu.ptr(d), None))
        want = mo.ndcg_words(p[:, c], y[:, c])
        assert abs(d[0] - want[0]) <= 1e-9 * abs(want[0]) and abs(d[1] - want[1]) <= 1e-9 * abs(want[1])
