"""BatchNorm and PReLU_Dice (hugectr_amd/csrc/batch_norm.hip) through BatchNormLayer / PReLUDiceLayer,
against numpy float64 restatements of the formulas (`_bn_ref`, `_dice_ref`) computed from the device
inputs, so that their rounding to the element type is not charged.  Tolerances are `_tol` of
tests/test_mha_gpu.py; dgamma / dbeta and the running statistics are fp32 outputs and take the fp32
pair (the saved statistics are checked through the running ones and through dx)."""
import numpy as np
import pytest

from test_mha_gpu import _np64, _tol
from util import assert_close

pytestmark = pytest.mark.gpu

EPS, DICE_EPS, ALPHA = 1e-5, 1e-8, 0.2
F32 = _tol("float32", True)


def _bn_ref(x, gamma, beta, top, eps=EPS):
    """float64, x [rows][n]: y, dx, dgamma, dbeta, mean, unbiased var"""
    m = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * rstd
    dbeta, dgamma = top.sum(0), (top * xh).sum(0)
    dx = gamma * rstd * (top - dbeta / m - xh * dgamma / m)
    return xh * gamma + beta, dx, dgamma, dbeta, mean, var * m / max(m - 1, 1)


def _dice_ref(x, top, alpha, eps):
    """float64, x [rows][n]: y and the reference's diagonal dx (its guard compares in fp32)"""
    m = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    p = 1.0 / (1.0 + np.exp((mean - x) / np.sqrt(var + eps)))
    small = var.astype(np.float32) + np.float32(eps) < np.float32(1e-8)
    r1 = np.where(small, 0.0, 1.0 / np.sqrt(var + eps))
    ys = (mean - x) * r1
    ys_x = (1.0 / m - 1.0) * r1 + (mean - x) ** 2 * r1 ** 3 / m
    q = 1.0 / (1.0 + np.exp(ys))
    return p * x + (1 - p) * alpha * x, ((-q * (1 - q) * ys_x * x + q) * (1 - alpha) + alpha) * top


def _inputs(dtype_name, shape, loc=0.0, scale=1.0):
    import torch
    rng = np.random.default_rng(list(shape))
    normal = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()  # noqa: E731
    dt = getattr(torch, dtype_name)
    return (loc + scale * normal(*shape)).to(dt).requires_grad_(True), normal(*shape).to(dt), normal


def _run_bn(dtype_name, shape, **kw):
    """-> (y, dx, dgamma, dbeta, running_mean, running_var) of a training step and the expectation"""
    import torch
    import hugectr_amd as ha
    x, top, normal = _inputs(dtype_name, shape, **kw)
    n = int(np.prod(shape[1:]))
    layer = ha.BatchNormLayer(n, eps=EPS).cuda()
    with torch.no_grad():
        layer.gamma.copy_(1 + 0.5 * normal(n))
        layer.beta.copy_(normal(n))
    y = layer(x)
    y.backward(top)
    torch.cuda.synchronize()
    flat = lambda t: _np64(t).reshape(shape[0], n)  # noqa: E731
    want = _bn_ref(flat(x), _np64(layer.gamma), _np64(layer.beta), flat(top))
    want = (want[0].reshape(shape), want[1].reshape(shape)) + want[2:]
    return (y, x.grad, layer.gamma.grad, layer.beta.grad, layer.running_mean, layer.running_var), want


def _run_dice(dtype_name, shape, alpha=ALPHA, eps=DICE_EPS, const_col=None, **kw):
    import torch
    import hugectr_amd as ha
    x, top, _ = _inputs(dtype_name, shape, **kw)
    if const_col is not None:
        with torch.no_grad():
            x[:, const_col] = 3.0
    y = ha.PReLUDiceLayer(alpha, eps)(x)
    y.backward(top)
    torch.cuda.synchronize()
    flat = lambda t: _np64(t).reshape(shape[0], -1)  # noqa: E731
    want = _dice_ref(flat(x), flat(top), alpha, eps)
    return (y, x.grad, x, top), tuple(w.reshape(shape) for w in want)


def _check_bn(dtype_name, shape, **kw):
    got, want = _run_bn(dtype_name, shape, **kw)
    what = f"batch_norm {dtype_name} {shape}"
    assert got[0].shape == shape and got[0].dtype == got[1].dtype
    assert_close(_np64(got[0]), want[0], *_tol(dtype_name, False), what + " y")
    assert_close(_np64(got[1]), want[1], *_tol(dtype_name, True), what + " dx")
    for g, w, name in zip(got[2:], want[2:], ("dgamma", "dbeta", "running_mean", "running_var")):
        assert_close(_np64(g), w, *F32, f"{what} {name}")


def _check_dice(dtype_name, shape, **kw):
    got, want = _run_dice(dtype_name, shape, **kw)
    what = f"prelu_dice {dtype_name} {shape}"
    assert got[0].shape == shape and got[0].dtype == got[1].dtype
    assert_close(_np64(got[0]), want[0], *_tol(dtype_name, False), what + " y")
    assert_close(_np64(got[1]), want[1], *_tol(dtype_name, True), what + " dx")


# rows = shape[0], n = the product of the rest.  A row is cut into 16-byte chunks of V = 4 (fp32) or
# 8 (16-bit) columns; G = 1, 2, 4 .. 64 lanes cover a panel of G V columns: G doubles above
# n = V, 2 V .. 32 V, and above 64 V columns a second panel begins.  Every boundary is walked (below,
# at, above) in one element type, which also gives each type widths that are no multiple of V (the
# element path).  A workgroup takes 256 / G rows a trip; the slab count is min(64, 1024 / panels,
# trips): the row counts are multiples of neither, 301 rows of >= 128 columns give 61 slabs of 5
# rows, 37 x 1000 has fewer rows than 64 slabs, 3 x 65536 is the widest row.  262221 rows of 9:
# G = 4 (fp32) and 2 (bf16), 64 slabs, more rows than the 2048 workgroups of the stream take in one trip.
CASES = [
    ("float32", (301, 1)), ("bfloat16", (1, 1)), ("float16", (1, 256)),
    ("float32", (301, 3)), ("float32", (301, 4)), ("float32", (301, 5)),
    ("float16", (301, 7)), ("float16", (301, 8)), ("float16", (301, 9)),
    ("bfloat16", (150, 15)), ("bfloat16", (150, 16)), ("bfloat16", (150, 17)),
    ("float32", (150, 7)), ("float32", (150, 8)), ("float32", (150, 9)),
    ("float32", (75, 15)), ("float32", (75, 16)), ("float32", (75, 17)),
    ("float16", (75, 31)), ("float16", (75, 32)), ("float16", (13, 3, 11)),
    ("float32", (75, 31)), ("float32", (75, 32)), ("float32", (75, 33)),
    ("bfloat16", (75, 63)), ("bfloat16", (75, 64)), ("bfloat16", (75, 65)),
    ("float32", (301, 63)), ("float32", (301, 64)), ("float32", (301, 65)),
    ("float16", (37, 127)), ("float16", (37, 128)), ("float16", (37, 129)),
    ("float32", (301, 127)), ("float32", (301, 128)), ("float32", (301, 129)),
    ("bfloat16", (301, 255)), ("bfloat16", (301, 256)), ("bfloat16", (301, 257)),
    ("float32", (19, 255)), ("float32", (19, 256)), ("float32", (19, 257)),
    ("float16", (19, 511)), ("float16", (19, 512)), ("float16", (19, 513)),
    ("float32", (37, 1000)), ("float16", (3, 65536)), ("float32", (3, 65535)),
    ("float32", (262221, 9)), ("bfloat16", (262221, 9)),
]


@pytest.mark.parametrize("dtype_name,shape", CASES)
def test_batch_norm_forward_and_gradients(dtype_name, shape):
    _check_bn(dtype_name, shape)


@pytest.mark.parametrize("dtype_name,shape", CASES)
def test_prelu_dice_forward_and_gradient(dtype_name, shape):
    _check_dice(dtype_name, shape)


def test_columns_far_from_zero_need_the_variance_around_the_mean():
    """x = 100 + 0.5 N(0, 1) in fp32: E[x^2] - E[x]^2 of the raw values loses the variance here"""
    _check_bn("float32", (390, 1000), loc=100.0, scale=0.5)
    _check_dice("float32", (390, 1000), loc=100.0, scale=0.5)


def test_running_statistics_over_two_steps_and_eval():
    import torch
    import hugectr_amd as ha
    layer = ha.BatchNormLayer(40, factor=0.25, eps=EPS).cuda()
    rm, rv = np.zeros(40), np.ones(40)
    for step in range(2):
        x, top, _ = _inputs("float32", (77 + step, 40), loc=1.0, scale=2.0)
        layer(x)
        mean, var = _bn_ref(_np64(x), 1.0, 0.0, _np64(top))[4:]
        rm, rv = 0.75 * rm + 0.25 * mean, 0.75 * rv + 0.25 * var
    assert_close(_np64(layer.running_mean), rm, *F32, "running_mean")
    assert_close(_np64(layer.running_var), rv, *F32, "running_var")
    before = layer.running_mean.clone(), layer.running_var.clone()
    with torch.no_grad():
        y = layer.eval()(x)
    assert_close(_np64(y), (_np64(x) - rm) / np.sqrt(rv + EPS), *_tol("float32", False), "eval y")
    assert torch.equal(layer.running_mean, before[0]) and torch.equal(layer.running_var, before[1])


def test_dice_guard_on_a_constant_column():
    """var = 0 and eps = 1e-9: var + eps < 1e-8, so r1 = r3 = 0, p = 0.5 in both directions"""
    got, want = _run_dice("float32", (50, 6), alpha=0.2, eps=1e-9, const_col=2)
    y, dx, x, top = (_np64(t) for t in got)
    assert_close(y, want[0], *_tol("float32", False), "y")
    assert_close(dx, want[1], *_tol("float32", True), "dx")
    assert_close(y[:, 2], 0.6 * x[:, 2], *_tol("float32", False), "y of the constant column")
    assert_close(dx[:, 2], (0.5 * (1 - 0.2) + 0.2) * top[:, 2], *_tol("float32", True), "its dx")


def test_two_runs_give_the_same_bits():
    import torch
    for run in (_run_bn, _run_dice):
        a, _ = run("float16", (2000, 72))
        b, _ = run("float16", (2000, 72))
        for u, v in zip(a, b):
            assert torch.equal(u, v)
