"""Attention with lengths = (len_from, len_to) in the place of the dense mask (the *_len_* entries of
both kernel families) through MultiHeadAttentionLayer: forward and the three gradients against the
float64 restatement of tests/test_mha_gpu.py given the mask numpy builds from the same lengths, its
tolerances unchanged.  One sample per length pair; every case runs twice for equal bits; where all
rows of a sample are valid and 1 <= nv < n keys are, dk and dv past nv are exactly 0 (a skipped key
block that was not written would show there)."""
import numpy as np
import pytest

from test_mha_gpu import _np64, _ref, _tol
from util import assert_close

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16", "bfloat16"]
# tiled family, (m, n, d) -> (len_from, len_to): a workgroup owns 128 rows, a tile holds 64, a
# wavefront skips sub-tiles of 32 keys; the dkv sweep has two key blocks at n 129
TILED = {
    (130, 200, 32): [(130, 200), (128, 64), (129, 65), (40, 33), (0, 100), (70, 0), (130, 1),
                     (2.5, 2.5)],
    (40, 129, 64): [(40, 129), (40, 128), (20, 128), (40, 5), (1, 129)],
    (129, 70, 128): [(129, 70), (128, 64), (1, 1), (0, 0)],
}
FIRST = [(10, 10, 8), (40, 97, 24), (97, 40, 56), (128, 128, 64)]


def _check(dtype_name, H, m, n, d, pairs, len_dtype="float32"):
    import torch
    import hugectr_amd as ha
    dt, B = getattr(torch, dtype_name), len(pairs)
    rng = np.random.default_rng([B, H, m, n, d])
    q, k, v, top = (torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda().to(dt)
                    for s in ((B, m, H * d), (B, n, H * d), (B, n, H * d), (B, m, H * d)))
    lf, lt = (np.array(x, dtype=np.float32) for x in zip(*pairs))
    mask = (np.arange(m)[None, :, None] < lf[:, None, None]) & \
        (np.arange(n)[None, None, :] < lt[:, None, None])
    want = _ref(_np64(q), _np64(k), _np64(v), mask[:, None].astype(np.float64), _np64(top), H)
    lengths = tuple(torch.from_numpy(x).cuda().to(getattr(torch, len_dtype)) for x in (lf, lt))

    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    runs = []
    for _ in range(2):
        q.grad = k.grad = v.grad = None
        out = ha.MultiHeadAttentionLayer(H)(q, k, v, lengths=lengths)
        out.backward(top)
        torch.cuda.synchronize()
        runs.append([_np64(t) for t in (out, q.grad, k.grad, v.grad)])
    what = f"{dtype_name} B={B} H={H} m={m} n={n} d={d} lengths {len_dtype}"
    for got, w, name in zip(runs[0], want, ("out", "dq", "dk", "dv")):
        assert_close(got, w, *_tol(dtype_name, name != "out"), f"{what} {name}")
    for a, b in zip(*runs):  # no atomics: the same bits again
        assert np.array_equal(a, b)
    nv = np.clip(np.ceil(lt), 0, n).astype(int)
    for b in np.flatnonzero((lf >= m) & (nv >= 1) & (nv < n)):
        assert not runs[0][2][b, nv[b]:].any() and not runs[0][3][b, nv[b]:].any(), f"{what} b={b}"


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("shape", TILED)
def test_tiled_family(shape, dtype_name):
    _check(dtype_name, 2, *shape, TILED[shape])


@pytest.mark.parametrize("len_dtype", ["element", "float32"])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("m,n,d", FIRST)
def test_first_family(m, n, d, dtype_name, len_dtype):
    pairs = [(m, n), (m // 2, n // 2), (0, n), (m, 0), (m, 1)]  # (all exact in bf16)
    _check(dtype_name, 2, m, n, d, pairs, dtype_name if len_dtype == "element" else len_dtype)


def test_first_family_past_the_grid():
    """B H = 2100 heads over the grid of 2048 workgroups: the lengths follow the sample"""
    pairs = [(5, 3), (2, 1), (0, 3), (5, 0), (5, 1)]
    _check("float16", 3, 5, 3, 8, [pairs[b % 5] for b in range(700)])


def test_lengths_are_validated():
    import torch
    import hugectr_amd as ha
    q = torch.zeros(3, 10, 16, device="cuda")
    ones = torch.ones(3, device="cuda")
    with pytest.raises(ValueError):
        ha.multi_head_attention(q, q, q, torch.ones(3, 1, 10, 10, device="cuda"), 2,
                                lengths=(ones, ones))
    with pytest.raises(ValueError):
        ha.MultiHeadAttentionLayer(2)(q, q, q, lengths=(torch.ones(4, device="cuda"), ones))
