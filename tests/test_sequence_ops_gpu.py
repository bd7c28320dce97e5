"""matrix_multiply, reduce_mean and fused_reshape_concat (hugectr_amd/csrc/sequence_ops.hip) through
the public layers, against numpy float64 computed from the device inputs (`_np64`), so that their
rounding to the element type is not charged.  The bounds are derived, not tuned: fp32 accumulation of
`n` terms, `n 2^-23 sum|terms|` (the standard bound with a factor of two of headroom), plus one
rounding `u |exact|` on the store; `+ tiny u` is half the spacing of the type's subnormals."""
import numpy as np
import pytest

from test_mha_gpu import _np64

pytestmark = pytest.mark.gpu

U = {"float32": 2.0 ** -24, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}


def _randn(rng, shape, dtype_name, scale=1.0, loc=0.0):
    import torch
    v = loc + scale * rng.standard_normal(shape, dtype=np.float32)
    return torch.from_numpy(v.astype(np.float32)).cuda().to(getattr(torch, dtype_name))


def _within(got, exact, bound, what):
    err = np.abs(_np64(got).reshape(exact.shape) - exact)
    assert (err <= bound).all(), (f"{what}: {(err > bound).sum()} / {err.size} outside the bound, worst "
                                  f"err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")


# ---- matrix_multiply -------------------------------------------------------------------------------
# (dtype, a shape, b shape, who wants a gradient).  The bodies: m n + n k + m k <= 1024 is packed, the
# rest runs 64 x 64 tiles of 2 x 2 wavefront blocks of 32 x 32 in steps of 16, so 31 / 32 / 33 and
# 15 / 16 / 17 walk the block and step edges, 65 / 70 / 100 / 130 the tile edges.  82000 fp16 items of
# 1 x 10 x 36 are 2050 slabs of 40 for a grid of 2048; 2050 items of 19 x 18 x 19 (the smallest
# m = k, n = m - 1 shape outside the packed rule) are 2050 tiles for a grid of 2048.
MM_CASES = [
    ("float32", (3, 1, 10), (3, 10, 36), "ab"), ("float16", (3, 10, 1), (3, 1, 36), "ab"),
    ("bfloat16", (1, 1), (1, 1), "ab"),
    ("float32", (2, 31, 15), (2, 15, 33), "ab"), ("float16", (2, 32, 16), (2, 16, 32), "ab"),
    ("bfloat16", (2, 33, 17), (2, 17, 31), "ab"),
    ("float16", (2, 70, 40), (2, 40, 100), "ab"), ("bfloat16", (2, 65, 130), (2, 130, 33), "ab"),
    ("float16", (4, 3, 5), (4, 5, 7), "ab"), ("bfloat16", (4, 3, 5), (4, 5, 7), "ab"),
    ("float32", (5, 1025), (1025, 9), "ab"), ("bfloat16", (2, 3, 17, 8), (2, 3, 8, 17), "ab"),
    ("float32", (45, 64), (64, 50), "ab"), ("float16", (7, 12), (12, 5, 6), "ab"),
    ("float16", (82000, 1, 10), (82000, 10, 36), "ab"), ("float32", (2050, 19, 18), (2050, 18, 19), "ab"),
    ("bfloat16", (3, 20, 24), (3, 24, 40), "a"), ("float32", (3, 1, 10), (3, 10, 36), "b"),
]


def _run_matmul(dtype_name, sa, sb, wants):
    import hugectr_amd as ha
    rng = np.random.default_rng([len(sa), *sa, *sb])
    scale = sa[-1] ** -0.25
    a = _randn(rng, sa, dtype_name, scale).requires_grad_("a" in wants)
    b = _randn(rng, sb, dtype_name, scale).requires_grad_("b" in wants)
    c = ha.MatrixMultiplyLayer()(a, b)
    top = _randn(rng, tuple(c.shape), dtype_name)
    c.backward(top)
    return a, b, top, c


@pytest.mark.parametrize("dtype_name,sa,sb,wants", MM_CASES)
def test_matrix_multiply_forward_and_gradients(dtype_name, sa, sb, wants):
    import torch
    a, b, top, c = _run_matmul(dtype_name, sa, sb, wants)
    m, n = sa[-2:]
    A = _np64(a).reshape(-1, m, n)
    B = _np64(b).reshape(A.shape[0], n, -1)
    G = _np64(top).reshape(A.shape[0], m, -1)
    assert c.shape == ((sa[0], *sb[1:]) if len(sb) > len(sa) else (*sa[:-1], sb[-1])) and c.dtype == a.dtype
    At, Bt = A.transpose(0, 2, 1), B.transpose(0, 2, 1)
    what = f"{dtype_name} {sa} x {sb}"
    # (a product of two fp16 values can land among fp16's subnormals, where one rounding is half
    #  their spacing, 2^-25, not u |exact|: with an inner dimension of 1 nothing else is in the bound)
    tiny = float(torch.finfo(a.dtype).tiny) * U[dtype_name]
    for got, x, y, name in ((c, A, B, "c"), (a.grad, G, Bt, "da"), (b.grad, At, G, "db")):
        if name[-1] not in "c" + wants:
            assert got is None, f"{what}: {name} was not asked for"
            continue
        exact = x @ y
        bound = x.shape[2] * 2.0 ** -23 * (np.abs(x) @ np.abs(y)) + U[dtype_name] * np.abs(exact) + tiny
        assert got.shape == (a.shape if name == "da" else b.shape if name == "db" else c.shape)
        _within(got, exact, bound, f"{what} {name}")


# ---- reduce_mean -----------------------------------------------------------------------------------
# (dtype, shape, axis, loc, scale).  inner == 1: groups of 1, 4, 16, 64 lanes for len <= 8, 64, 512,
# above; inner > 1: 16-byte chunks when inner is a multiple of 4 (fp32) / 8 (16-bit), elements
# otherwise; [3, 4097, 5] and [2, 600, 8] split len over 64 and 32 row slabs; 70001 x 5 chunks are
# more than the 1024 x 256 threads of one grid.  The last case lies far from zero.
RM_CASES = [
    ("float32", (301,), 0, 0, 1), ("float16", (37, 19), 0, 0, 1), ("bfloat16", (37, 19), 1, 0, 1),
    ("float32", (5, 10, 36), 0, 0, 1), ("float16", (5, 10, 36), 0, 0, 1),
    ("float16", (5, 10, 36), 1, 0, 1), ("float32", (5, 10, 36), 1, 0, 1),
    ("bfloat16", (5, 10, 36), 2, 0, 1), ("float32", (4, 1, 6), 1, 0, 1), ("bfloat16", (300, 7), 1, 0, 1),
    ("float16", (3, 1000), 1, 0, 1), ("float32", (3, 4097, 5), 1, 0, 1), ("float16", (2, 600, 8), 1, 0, 1),
    ("bfloat16", (70001, 10, 36), 1, 0, 1), ("float32", (64, 1000), 1, 100.0, 0.5),
]


def _run_reduce_mean(dtype_name, shape, axis, loc, scale):
    import hugectr_amd as ha
    rng = np.random.default_rng([axis, *shape])
    x = _randn(rng, shape, dtype_name, scale, loc).requires_grad_(True)
    y = ha.ReduceMeanLayer(axis)(x)
    top = _randn(rng, tuple(y.shape), dtype_name)
    y.backward(top)
    return x, top, y


@pytest.mark.parametrize("dtype_name,shape,axis,loc,scale", RM_CASES)
def test_reduce_mean_forward_and_gradient(dtype_name, shape, axis, loc, scale):
    import torch
    x, top, y = _run_reduce_mean(dtype_name, shape, axis, loc, scale)
    X, u = _np64(x), U[dtype_name]
    tiny = float(torch.finfo(x.dtype).tiny) * u
    exact = X.mean(axis, keepdims=True)
    assert y.shape == exact.shape and x.grad.shape == x.shape
    what = f"{dtype_name} {shape} axis {axis}"
    _within(y, exact, shape[axis] * 2.0 ** -23 * np.abs(X).mean(axis, keepdims=True) + u * np.abs(exact)
            + tiny, what + " y")
    # one rounding of the fp32 quotient, which is itself one rounding of dy / len
    dx = np.broadcast_to(_np64(top) / shape[axis], X.shape)
    _within(x.grad, dx, (u + 2.0 ** -24) * np.abs(dx) + tiny, what + " dx")


# ---- fused_reshape_concat --------------------------------------------------------------------------
# (dtype, B, S, widths): DIN's pair; an unaligned mix (elements); one input; S = 1 (item is empty);
# eight inputs of one 16-byte chunk each; rows of 67 elements take 64 lanes, 4 rows a workgroup, so
# 9900 rows are more than the 2048 workgroups of one grid move in a trip.
FRC_CASES = [("float32", 7, 11, (18, 18)), ("float16", 5, 4, (1, 3, 8)), ("bfloat16", 3, 5, (24,)),
             ("float32", 6, 1, (4, 8)), ("float16", 3, 3, (8,) * 8), ("float16", 900, 11, (40, 27))]


def _run_frc(dtype_name, B, S, widths):
    import torch
    import hugectr_amd as ha
    rng = np.random.default_rng([B, S, *widths])
    xs = [_randn(rng, (B, S, w), dtype_name).requires_grad_(True) for w in widths]
    item, ad = ha.FusedReshapeConcatLayer()(xs)
    tops = [_randn(rng, tuple(t.shape), dtype_name) for t in (item, ad)]
    torch.autograd.backward([item, ad], tops)
    return xs, tops, item, ad


@pytest.mark.parametrize("dtype_name,B,S,widths", FRC_CASES)
def test_fused_reshape_concat_is_the_index_expression(dtype_name, B, S, widths):
    import torch
    xs, tops, item, ad = _run_frc(dtype_name, B, S, widths)
    W = sum(widths)
    X = torch.cat([x.detach() for x in xs], dim=2)
    assert item.shape == (B * (S - 1), W) and ad.shape == (B, W)
    assert torch.equal(item, X[:, :-1].reshape(-1, W)) and torch.equal(ad, X[:, -1])
    G = torch.cat([tops[0].reshape(B, S - 1, W), tops[1].reshape(B, 1, W)], dim=1)
    for x, g in zip(xs, torch.split(G, widths, dim=2)):
        assert torch.equal(x.grad, g)


def test_two_runs_give_the_same_bits():
    import torch
    runs = [(_run_matmul, ("float16", (2, 70, 40), (2, 40, 100), "ab")),
            (_run_matmul, ("float32", (300, 1, 10), (300, 10, 36), "ab")),
            (_run_reduce_mean, ("float32", (3, 4097, 5), 1, 0, 1)),
            (_run_frc, ("float16", 5, 4, (1, 3, 8)))]
    for run, args in runs:
        first, second = run(*args), run(*args)
        flat = lambda r: [t for v in r for t in (v if isinstance(v, list) else [v])]  # noqa: E731
        for u, v in zip(flat(first), flat(second)):
            assert torch.equal(u, v)
            assert not (u.is_leaf and u.requires_grad) or torch.equal(u.grad, v.grad)
