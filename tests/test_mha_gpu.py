"""Multi-head attention and the sequence mask (hugectr_amd/csrc/attention.hip) through the public
functions, against a numpy float64 restatement of the formulas (`_ref`), computed from the inputs
after rounding to the element type.  Tolerances are `_tol` of tests/test_interaction_matrix_gpu.py:
the rule for a 16-bit-MFMA, fp32-accumulate kernel judged against float64 (fp32: rtol 2e-4, atol
1e-3; 16-bit: forward (2 eps, 24 eps), backward (4 eps, 32 eps)); inputs are N(0, 1)."""
import numpy as np
import pytest

from util import assert_close

pytestmark = pytest.mark.gpu

EPS = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}


def _tol(dtype_name, backward):
    if dtype_name == "float32":
        return 2e-4, 1e-3
    eps = EPS[dtype_name]
    return (4 * eps, 32 * eps) if backward else (2 * eps, 24 * eps)


def _ref(q, k, v, mask, top, H):
    """float64: O and the gradients of q, k, v for the top gradient `top`"""
    B, m, hidden = q.shape
    d = hidden // H
    heads = lambda x: x.reshape(B, -1, H, d).transpose(0, 2, 1, 3)  # noqa: E731  [B, H, seq, d]
    merge = lambda x: x.transpose(0, 2, 1, 3).reshape(B, -1, hidden)  # noqa: E731
    T = lambda x: x.transpose(0, 1, 3, 2)  # noqa: E731
    Q, K, V, G = heads(q), heads(k), heads(v), heads(top)
    S = Q @ T(K) / np.sqrt(d)
    if mask is not None:
        S = S - (1.0 - mask) * 10000.0  # [B, 1, m, n] over the heads
    E = np.exp(S - S.max(-1, keepdims=True))
    P = E / (E.sum(-1, keepdims=True) + 1e-6)
    dP = G @ T(V)
    dS = P * (dP - (dP * P).sum(-1, keepdims=True))
    return merge(P @ V), merge(dS @ K / np.sqrt(d)), merge(T(dS) @ Q / np.sqrt(d)), merge(T(P) @ G)


def _lengths(B, top):
    """[B] lengths that walk through the maximum, a middle value and 0"""
    return np.array([(top, top // 2, 0)[b % 3] for b in range(B)], dtype=np.float32)


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# (m, n) on and around the 32-wide tiles and with m != n; d = 8 (K padded to 16), 16, 64; one and
# four heads; B H = 2400 > the grid of 2048 workgroups (the stride loop); fp32 at 128 x 128 x 64
# is the largest LDS footprint of both kernels (above 64 KB)
CASES = [
    ("float32", 3, 4, 1, 10, 8, True),
    ("float16", 3, 4, 10, 10, 8, True),
    ("bfloat16", 3, 1, 16, 16, 16, False),
    ("float32", 3, 1, 17, 33, 16, False),
    ("bfloat16", 3, 4, 17, 33, 64, True),
    ("float16", 3, 1, 128, 128, 64, False),
    ("float32", 3, 1, 128, 128, 64, True),
    ("bfloat16", 3, 4, 128, 128, 8, True),
    ("float16", 600, 4, 3, 5, 8, True),
]


@pytest.mark.parametrize("dtype_name,B,H,m,n,d,masked", CASES)
def test_forward_and_gradients(dtype_name, B, H, m, n, d, masked):
    import torch
    import hugectr_amd as ha
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng([B, H, m, n, d])
    q, k, v, top = (torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda().to(dt)
                    for s in ((B, m, H * d), (B, n, H * d), (B, n, H * d), (B, m, H * d)))
    mask = None
    if masked:
        lf, lt = _lengths(B, m), _lengths(B, n)[::-1].copy()
        mask = ha.sequence_mask(torch.from_numpy(lf).cuda().to(dt), torch.from_numpy(lt).cuda().to(dt),
                                m, n)
        want_mask = (np.arange(m)[None, :, None] < lf[:, None, None]) & \
            (np.arange(n)[None, None, :] < lt[:, None, None])
        assert np.array_equal(_np64(mask), want_mask[:, None].astype(np.float64))
    want = _ref(_np64(q), _np64(k), _np64(v), None if mask is None else _np64(mask), _np64(top), H)
    # (a fully masked row -- length 0 -- needs no special case: the -10000 is common to the row and
    #  cancels in the softmax, in float64 exactly, so the row attends as if it had no mask)

    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    out = ha.MultiHeadAttentionLayer(H)(q, k, v, mask)
    out.backward(top)
    torch.cuda.synchronize()
    what = f"{dtype_name} B={B} H={H} m={m} n={n} d={d} mask={masked}"
    assert_close(_np64(out), want[0], *_tol(dtype_name, False), what + " out")
    for got, w, name in zip((q.grad, k.grad, v.grad), want[1:], ("dq", "dk", "dv")):
        assert_close(_np64(got), w, *_tol(dtype_name, True), f"{what} {name}")


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16"])
def test_sequence_mask_is_exact(dtype_name):
    """B 37 x 7 x 13 = 3367 elements: no multiple of a 16-byte store; fractional lengths"""
    import torch
    import hugectr_amd as ha
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(3)
    lf = torch.from_numpy(rng.integers(0, 15, 37).astype(np.float32) / 2).cuda().to(dt)
    lt = torch.from_numpy(rng.integers(0, 27, 37).astype(np.float32) / 2).cuda().to(dt)
    mask = ha.SequenceMaskLayer(max_sequence_len_from=7, max_sequence_len_to=13)(lf, lt)
    want = (np.arange(7)[None, :, None] < _np64(lf)[:, None, None]) & \
        (np.arange(13)[None, None, :] < _np64(lt)[:, None, None])
    assert mask.shape == (37, 1, 7, 13) and mask.dtype == dt
    assert np.array_equal(_np64(mask)[:, 0], want.astype(np.float64))
