"""numpy oracle of the evaluation metrics (hugectr_amd/csrc/metrics.hip, hugectr_amd/metrics.py):
keys and the AUC words in integers, NDCG / SMAPE / HitRate in fp64.  Test infrastructure only."""
import numpy as np


def keys_of(scores):
    """order-preserving uint32 image of the scores' exact fp32 values: sign bit flipped for
    non-negatives, all bits for negatives, -0.0 as +0.0, every NaN 0xFFFFFFFF"""
    f = np.ascontiguousarray(np.asarray(scores).astype(np.float32))
    b = f.view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    k = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(f)] = np.uint32(0xFFFFFFFF)
    return k


def auc_words(scores, labels):
    """(2U, P, N) as Python integers: P / N = labels that are / are not 1.0,
    2U = sum over runs of equal key of pos_run * (2 * neg_below_run + neg_run)"""
    k = keys_of(scores).reshape(-1)
    y = np.asarray(labels, dtype=np.float32).reshape(-1)
    if k.size == 0:
        return 0, 0, 0
    _, inv = np.unique(k, return_inverse=True)
    inv = inv.reshape(-1)
    pos = np.bincount(inv, weights=(y == 1.0)).astype(np.int64)
    neg = np.bincount(inv, weights=(y != 1.0)).astype(np.int64)
    two_u, below = 0, 0
    for p, n in zip(pos.tolist(), neg.tolist()):
        two_u += p * (2 * below + n)
        below += n
    return two_u, int(pos.sum()), int(neg.sum())


def auc_value(words):
    two_u, p, n = words
    if p == 0 or n == 0:
        return 0.5
    return float(np.float64(two_u) / np.float64(2 * p * n))


def auc(scores, labels):
    return auc_value(auc_words(scores, labels))


def auc_mean(scores, labels):
    """[n, C] input: per-column AUCs and their mean (R/HugeCTR/src/metrics.cu:940-998)"""
    s, y = np.asarray(scores), np.asarray(labels)
    per = [auc(s[:, c], y[:, c]) for c in range(s.shape[1])]
    return float(np.mean(np.array(per, dtype=np.float64))), per


def _dcg(lab_sorted_ascending):
    n = lab_sorted_ascending.size
    i = np.arange(n, dtype=np.float64)
    return float(np.sum(lab_sorted_ascending.astype(np.float64) / np.log2(2.0 + (n - 1 - i))))


def ndcg_words(scores, labels):
    """(DCG, ideal DCG): samples sorted ascending and stable by key, the last one ranked first"""
    k = keys_of(scores).reshape(-1)
    y = np.asarray(labels, dtype=np.float32).reshape(-1)
    if k.size == 0:
        return 0.0, 0.0
    order = np.argsort(k, kind="stable")
    return _dcg(y[order]), _dcg(y[np.argsort(keys_of(y), kind="stable")])


def ndcg(scores, labels):
    d, i = ndcg_words(scores, labels)
    return d / i


def smape_words(scores, labels):
    """(sum, count): sum of |p - l| / ((p + l) / 2) in fp64, a term with p + l == 0 counting 0"""
    p = np.asarray(scores).astype(np.float32).astype(np.float64).reshape(-1)
    l = np.asarray(labels, dtype=np.float32).astype(np.float64).reshape(-1)
    s = p + l
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(s != 0.0, np.abs(p - l) / (s / 2.0), 0.0)
    return float(np.sum(t)), int(p.size)


def smape(scores, labels):
    s, n = smape_words(scores, labels)
    return s / n if n else 0.0


def hitrate_words(scores, labels):
    """(checked, hits): (double)pred > 0.8, and label == 1 among those"""
    p = np.asarray(scores).astype(np.float32).astype(np.float64).reshape(-1)
    l = np.asarray(labels, dtype=np.float32).reshape(-1)
    c = p > 0.8
    return int(c.sum()), int((c & (l == 1.0)).sum())


def hitrate(scores, labels):
    c, h = hitrate_words(scores, labels)
    return h / c if c else 0.0
