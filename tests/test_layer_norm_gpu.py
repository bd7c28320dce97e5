"""LayerNorm with the residual add folded in (hugectr_amd/csrc/layer_norm.hip) through LayerNormLayer,
against a numpy float64 restatement of the formulas (`_ref`) computed from the device inputs, so that
their rounding to the element type is not charged.  Tolerances are `_tol` of tests/test_mha_gpu.py;
dgamma / dbeta are fp32 outputs and take the fp32 pair."""
import numpy as np
import pytest

from test_mha_gpu import _np64, _tol
from util import assert_close

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _ref(x, res, gamma, beta, top):
    """float64: y, dz, dgamma, dbeta"""
    z = x if res is None else x + res
    mean = z.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((z - mean) ** 2).mean(-1, keepdims=True) + EPS)
    xh = (z - mean) * rstd
    t = top * gamma
    dz = rstd * (t - t.mean(-1, keepdims=True) - xh * (t * xh).mean(-1, keepdims=True))
    lead = tuple(range(x.ndim - 1))
    return xh * gamma + beta, dz, (top * xh).sum(lead), top.sum(lead)


def _run(dtype_name, shape, hidden, with_res, loc=0.0, scale=1.0):
    """-> (y, dx, dgamma, dbeta, dresidual or None) of the layer, and the float64 expectation"""
    import torch
    import hugectr_amd as ha
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng([hidden, *shape])
    normal = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()  # noqa: E731
    x = (loc + scale * normal(*shape, hidden)).to(dt).requires_grad_(True)
    res = normal(*shape, hidden).to(dt).requires_grad_(True) if with_res else None
    top = normal(*shape, hidden).to(dt)
    layer = ha.LayerNormLayer(hidden, EPS).cuda()
    with torch.no_grad():
        layer.gamma.copy_(1 + 0.5 * normal(hidden))
        layer.beta.copy_(normal(hidden))
    y = layer(x, res)
    y.backward(top)
    torch.cuda.synchronize()
    want = _ref(_np64(x), None if res is None else _np64(res), _np64(layer.gamma), _np64(layer.beta),
                _np64(top))
    return (y, x.grad, layer.gamma.grad, layer.beta.grad, None if res is None else res.grad), want


def _check(dtype_name, shape, hidden, with_res, **kw):
    got, want = _run(dtype_name, shape, hidden, with_res, **kw)
    what = f"{dtype_name} {shape} x {hidden} residual={with_res}"
    assert got[0].shape == (*shape, hidden) and got[0].dtype == got[1].dtype
    assert_close(_np64(got[0]), want[0], *_tol(dtype_name, False), what + " y")
    assert_close(_np64(got[1]), want[1], *_tol(dtype_name, True), what + " dx")
    assert_close(_np64(got[2]), want[2], *_tol("float32", True), what + " dgamma")
    assert_close(_np64(got[3]), want[3], *_tol("float32", True), what + " dbeta")
    if with_res:
        assert_close(_np64(got[4]), want[1], *_tol(dtype_name, True), what + " dresidual")


# A row belongs to G lanes of E elements each, in 16-byte chunks of V = 4 (fp32) or 8 (16-bit)
# elements: G = 1, 2 .. 64 with E = V up to hidden = 64 V, then (G, E) = (64, 16), (64, 32),
# (256, 16), (256, 32) up to 1024, 2048, 4096, 8192.  Every boundary is walked (below, at, above)
# in one element type; a workgroup takes 256 / G rows a trip and a wavefront 64 / G, and the row
# counts are multiples of neither and more than one workgroup's.  hidden = 1: variance 0, y = beta,
# dx = 0.  262221 rows of 9: G = 2, 128 rows a workgroup, more than the forward's 2048 and the
# backward's 1024 workgroups take in one trip.
CASES = [
    ("float32", (301,), 1, True), ("bfloat16", (1,), 1, False), ("float16", (301,), 7, True),
    ("float32", (301,), 3, False), ("float32", (301,), 4, True), ("float32", (301,), 5, False),
    ("float16", (3, 67), 15, True), ("float16", (3, 67), 16, False), ("float16", (3, 67), 17, True),
    ("bfloat16", (150,), 31, False), ("bfloat16", (150,), 32, True), ("bfloat16", (150,), 33, False),
    ("float32", (75,), 31, True), ("float32", (75,), 32, False), ("float32", (75,), 33, True),
    ("float16", (2, 3, 13), 127, False), ("float16", (2, 3, 13), 128, True),
    ("float16", (2, 3, 13), 129, False),
    ("float32", (37,), 127, True), ("float32", (37,), 128, False), ("float32", (37,), 129, True),
    ("bfloat16", (1,), 256, True), ("bfloat16", (19,), 255, False), ("bfloat16", (19,), 257, True),
    ("float16", (9,), 511, True), ("float16", (9,), 512, False), ("float16", (9,), 513, True),
    ("float32", (9,), 255, False), ("float32", (9,), 256, True), ("float32", (9,), 257, False),
    ("bfloat16", (9,), 1023, False), ("bfloat16", (9,), 1024, True), ("float32", (9,), 1025, True),
    ("float32", (5,), 2047, False), ("float16", (5,), 2048, True), ("float16", (5,), 2049, False),
    ("float16", (3,), 4095, True), ("bfloat16", (3,), 4096, False), ("float32", (3,), 4097, True),
    ("float32", (1,), 8192, True), ("float16", (3,), 8192, False), ("bfloat16", (3,), 8191, True),
    ("bfloat16", (262221,), 9, True),
]


@pytest.mark.parametrize("dtype_name,shape,hidden,with_res", CASES)
def test_forward_and_gradients(dtype_name, shape, hidden, with_res):
    _check(dtype_name, shape, hidden, with_res)


def test_rows_far_from_zero_need_the_variance_around_the_mean():
    """x = 100 + 0.5 N(0, 1): E[z^2] - E[z]^2 in fp32 loses the variance here (a third of y, half of
    dx and 916 of 1000 dgamma miss the fp32 bound), the two-pass form stays inside it"""
    _check("float32", (390,), 1000, False, loc=100.0, scale=0.5)


def test_two_runs_give_the_same_bits():
    import torch
    a, _ = _run("float16", (40, 50), 72, True)
    b, _ = _run("float16", (40, 50), 72, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
