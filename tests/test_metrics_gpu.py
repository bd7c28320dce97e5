"""Evaluation metrics through the C ABI (csrc/metrics.hip): hctr_metric_accumulate / _auc / _ndcg
against tests/metrics_oracle.py.  The AUC words (2U, P, N) are integers and must EQUAL the oracle's;
HitRate's counters are exact; NDCG and SMAPE are fp64 sums in a fixed order: within 1e-9 relative
(n * 2^-53 for n <= 2^20, with a decade of room for log2) and bit-identical between two calls."""
import numpy as np
import pytest

import metrics_oracle as mo

pytestmark = pytest.mark.gpu

NS = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 100_003]  # the sort's tile edges (test_sort_gpu.py)
F32, F16, BF16 = 0, 1, 2
WORDS = 264


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:  # bf16 bits
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a).cuda()


class Store:
    """the caller's side of the ABI: class-major store, counter block, workspace"""

    def __init__(self, C, cap):
        import torch
        from hugectr_amd._lib import lib
        self.C, self.cap, self.n = C, max(cap, 1), 0
        self.keys = torch.full((C, self.cap), -1, dtype=torch.int32, device="cuda")
        self.labels = torch.full((C, self.cap), -7.0, dtype=torch.float32, device="cuda")
        self.counters = torch.zeros(WORDS, dtype=torch.int64, device="cuda")
        self.tmp = torch.empty(lib.hctr_metric_accumulate_temp_bytes(), dtype=torch.uint8,
                               device="cuda")

    def add(self, pred, label, dtype=F32):
        from hugectr_amd._lib import check, lib, ptr, stream_ptr
        p, l = _dev(pred), _dev(np.asarray(label, np.float32))
        n = int(l.shape[0])
        check(lib.hctr_metric_accumulate(ptr(p), dtype, ptr(l), n, self.C, ptr(self.keys),
                                         ptr(self.labels), self.cap, self.n, ptr(self.counters),
                                         ptr(self.tmp), self.tmp.numel(), stream_ptr()))
        self.n += n

    def host(self):
        import torch
        torch.cuda.synchronize()
        return (self.keys.cpu().numpy().view(np.uint32).copy(), self.labels.cpu().numpy().copy(),
                self.counters.cpu().numpy().copy())

    def _cls(self, t, c):
        from ctypes import c_void_p
        return c_void_p(t.data_ptr() + c * self.cap * 4)

    def auc(self, c):
        import torch
        from hugectr_amd._lib import check, lib, ptr, stream_ptr
        tb = lib.hctr_metric_auc_temp_bytes(self.n)
        tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
        out = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        check(lib.hctr_metric_auc(ptr(tmp), tb, self._cls(self.keys, c), self._cls(self.labels, c),
                                  self.n, ptr(out), stream_ptr()))
        return tuple(int(v) for v in out.cpu().numpy())

    def ndcg(self, c):
        import torch
        from hugectr_amd._lib import check, lib, ptr, stream_ptr
        tb = lib.hctr_metric_ndcg_temp_bytes(self.n)
        tmp = torch.empty(tb, dtype=torch.uint8, device="cuda")
        out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        check(lib.hctr_metric_ndcg(ptr(tmp), tb, self._cls(self.keys, c), self._cls(self.labels, c),
                                   self.n, ptr(out), stream_ptr()))
        return out.cpu().numpy().copy()


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1e-38, -1.1e-38, -1.5, -0.25, 0.25,
                    1.5, np.nan, -np.nan, 3.0e38, -3.0e38], np.float32)


def _scores(pattern, n, C, rng):
    if pattern == "uniform":
        return rng.random((n, C), dtype=np.float32)
    if pattern == "equal":
        return np.full((n, C), 0.625, np.float32)
    if pattern == "six":  # tie runs that span several workgroups
        return rng.choice(np.array([0.1, 0.2, 0.5, 0.7, 0.9, -0.3], np.float32), (n, C))
    if pattern == "special":  # +-0.0, +-inf, denormals, negatives, NaN
        return rng.choice(SPECIAL, (n, C))
    raise AssertionError(pattern)


def _labels(kind, n, C, rng):
    if kind == "pos":
        return np.ones((n, C), np.float32)
    if kind == "neg":
        return np.zeros((n, C), np.float32)
    return (rng.random((n, C)) < 0.3).astype(np.float32)


def _check_auc(p32, pdev, y, dtype, C):
    n = y.shape[0]
    st = Store(C, n)
    st.add(pdev, y, dtype)
    keys, labs, _ = st.host()
    for c in range(C):
        assert (keys[c, :n] == mo.keys_of(p32[:, c])).all(), "keys differ from the oracle's"
        assert (labs[c, :n] == y[:, c]).all()
        want = mo.auc_words(p32[:, c], y[:, c])
        got = st.auc(c)
        print(f"n={n} C={C} class {c}: (2U, P, N) = {got}, oracle {want}")
        assert got == want
    return st


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_auc_words_equal_the_oracle(n, C):
    rng = np.random.default_rng(1000 * C + n)
    for pattern in ("uniform", "equal", "six", "special"):
        p = _scores(pattern, n, C, rng)
        _check_auc(p, p, _labels("mixed", n, C, rng), F32, C)


@pytest.mark.parametrize("kind", ["pos", "neg"])
@pytest.mark.parametrize("n", [1, 4097])
def test_auc_one_class_absent(n, kind):
    rng = np.random.default_rng(n)
    p = _scores("six", n, 1, rng)
    st = _check_auc(p, p, _labels(kind, n, 1, rng), F32, 1)
    two_u, P, N = st.auc(0)
    assert two_u == 0 and (P, N) == ((n, 0) if kind == "pos" else (0, n))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_auc_16bit_scores_heavy_ties(dtype, C):
    n = 100_003
    rng = np.random.default_rng(dtype * 10 + C)
    p = rng.random((n, C), dtype=np.float32)
    if dtype == F16:
        pdev = p.astype(np.float16)
        p32 = pdev.astype(np.float32)
    else:
        pdev = (p.view(np.uint32) >> 16).astype(np.uint16)
        p32 = (pdev.astype(np.uint32) << 16).view(np.float32)
    _check_auc(p32, pdev, _labels("mixed", n, C, rng), dtype, C)


@pytest.mark.parametrize("C", [1, 3])
def test_uneven_pieces_give_the_same_store_and_words(C):
    pieces = [1000, 1, 3095, 4097, 0, 64, 7]
    n = sum(pieces)
    rng = np.random.default_rng(C)
    p = _scores("six", n, C, rng)
    p[::3] = rng.random((len(p[::3]), C), dtype=np.float32)
    y = _labels("mixed", n, C, rng)
    one, many = Store(C, n + 5), Store(C, n + 5)
    one.add(p, y)
    off = 0
    for k in pieces:
        many.add(p[off:off + k], y[off:off + k])
        off += k
    a, b = one.host(), many.host()
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), "stores differ"
    assert (a[2][[0, 1, 2, 4]] == b[2][[0, 1, 2, 4]]).all() and a[2][4] == 0
    assert (a[0][:, n:] == 0xFFFFFFFF).all() and (a[1][:, n:] == -7.0).all(), "wrote past offset + n"
    for c in range(C):
        assert one.auc(c) == many.auc(c) == mo.auc_words(p[:, c], y[:, c])


def test_finalise_twice_is_identical_and_leaves_the_store():
    n, C = 4097, 3
    rng = np.random.default_rng(5)
    p, y = _scores("six", n, C, rng), _labels("mixed", n, C, rng)
    st = Store(C, n)
    st.add(p, y)
    before = st.host()
    first = [st.auc(c) for c in range(C)]
    nd = [st.ndcg(c) for c in range(C)]
    assert [st.auc(c) for c in range(C)] == first
    for c in range(C):
        assert st.ndcg(c).tobytes() == nd[c].tobytes()
    after = st.host()
    assert all((a == b).all() for a, b in zip(before, after)), "the finalise wrote into the store"


def test_hitrate_counters_are_exact():
    p8 = np.float32(0.8)                       # > the double 0.8: checked
    below = np.nextafter(p8, np.float32(0))    # its fp32 predecessor: not checked
    rng = np.random.default_rng(11)
    p = rng.random((5000, 1), dtype=np.float32)
    p[:6, 0] = [p8, below, 0.9, 0.95, 0.8000001, 0.1]
    y = _labels("mixed", 5000, 1, rng)
    y[:3, 0] = [1.0, 1.0, 0.0]
    st = Store(1, 5000)
    st.add(p, y)
    ct = st.host()[2]
    want = mo.hitrate_words(p, y)
    print("hitrate (checked, hits):", (int(ct[0]), int(ct[1])), "oracle", want)
    assert (int(ct[0]), int(ct[1])) == want
    assert float(p8) > 0.8 and float(below) < 0.8
    # float16(0.8) = 0.7998046875: not checked
    for scores, dtype, exp in ((np.array([[p8]], np.float32), F32, (1, 1)),
                               (np.array([[below]], np.float32), F32, (0, 0)),
                               (np.array([[0.8]], np.float16), F16, (0, 0))):
        s1 = Store(1, 1)
        s1.add(scores, np.ones((1, 1), np.float32), dtype)
        ct = s1.host()[2]
        assert (int(ct[0]), int(ct[1])) == exp


def test_labels_that_are_not_0_or_1_are_counted_per_class():
    y = np.array([[0, 1, 0.5], [1, 2, 0], [1, 0, -1], [0, 0, 1]], np.float32)
    st = Store(3, 4)
    st.add(np.full((4, 3), 0.5, np.float32), y)
    assert st.host()[2][8:11].tolist() == [0, 1, 2]


@pytest.mark.parametrize("n", [0, 1, 65, 4097, 100_003, 300_000])
def test_smape_and_ndcg_within_1e_9_and_reproducible(n):
    rng = np.random.default_rng(n)
    p = rng.random((n, 1), dtype=np.float32)
    p[::7] = p[:len(p[::7])]  # some ties
    y = rng.integers(0, 5, (n, 1)).astype(np.float32)  # graded relevance, >= 0
    if n > 2:
        p[1], y[1] = 0.0, 0.0   # p + l == 0: the term counts 0
    res = []
    for _ in range(2):
        st = Store(1, n)
        half = n // 3
        st.add(p[:half], y[:half])
        st.add(p[half:], y[half:])
        ct = st.host()[2]
        res.append((ct[2:4].tobytes(), st.ndcg(0).tobytes()))
    assert res[0] == res[1], "not bit-identical between two calls"
    s_sum, s_cnt = float(ct[3:4].view(np.float64)[0]), int(ct[2])
    w_sum, w_cnt = mo.smape_words(p, y)
    dcg = np.frombuffer(res[0][1], np.float64)
    w_dcg = mo.ndcg_words(p, y)
    print(f"n={n}: smape sum {s_sum!r} oracle {w_sum!r}; dcg {dcg.tolist()} oracle {w_dcg}")
    assert s_cnt == w_cnt
    assert abs(s_sum - w_sum) <= 1e-9 * abs(w_sum)
    assert abs(dcg[0] - w_dcg[0]) <= 1e-9 * abs(w_dcg[0])
    assert abs(dcg[1] - w_dcg[1]) <= 1e-9 * abs(w_dcg[1])
