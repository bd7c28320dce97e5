"""The tiled attention kernels (hugectr_amd/csrc/attention_tiled.hip) through MultiHeadAttentionLayer:
every shape here lies outside m, n <= 128, d <= 64 and so takes hctr_mha_tiled_fwd / _bwd.  Forward
and the three gradients against the float64 restatement and the tolerances of tests/test_mha_gpu.py,
unchanged.  A workgroup owns Q = 128 rows, a streamed tile holds T = 64."""
import numpy as np
import pytest

from test_mha_gpu import _lengths, _np64, _ref, _tol
from util import assert_close

pytestmark = pytest.mark.gpu

# dtype, B, H, m, n, d, mask ("len": sequence_mask of lengths maximum / half / 0, so whole samples'
# rows and leading or trailing key tiles are fully masked; "rand": below), run twice
CASES = [
    ("float16", 3, 1, 127, 63, 128, "len", False),    # Q-1, T-1; in by d alone
    ("bfloat16", 3, 4, 128, 64, 72, "len", False),    # Q, T; d no multiple of 16, three column tiles
    ("float32", 3, 1, 129, 3, 8, "len", False),       # Q+1; in by m alone; k padded to 16
    ("float16", 3, 4, 1, 1025, 8, "len", False),      # in by n alone: 17 tiles, the last of one key
    ("bfloat16", 3, 1, 257, 129, 16, "len", True),    # 2Q+1, 2T+1: both beyond 128, unequal
    ("float32", 3, 4, 129, 65, 128, "len", False),    # T+1; the largest LDS footprint (fp32 planes)
    ("float32", 2, 1, 130, 131, 72, None, False),
    ("bfloat16", 2, 4, 64, 257, 128, None, False),
    ("float16", 3, 4, 130, 200, 32, "rand", False),
]


@pytest.mark.parametrize("dtype_name,B,H,m,n,d,masked,twice", CASES)
def test_forward_and_gradients(dtype_name, B, H, m, n, d, masked, twice):
    import torch
    import hugectr_amd as ha
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng([B, H, m, n, d])
    q, k, v, top = (torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda().to(dt)
                    for s in ((B, m, H * d), (B, n, H * d), (B, n, H * d), (B, m, H * d)))
    mask = None
    if masked == "len":
        lf, lt = _lengths(B, m), _lengths(B, n)[::-1].copy()
        mask = ha.sequence_mask(torch.from_numpy(lf).cuda().to(dt), torch.from_numpy(lt).cuda().to(dt),
                                m, n)
    elif masked == "rand":
        # any 0 / 1 pattern: p = 0.5, sample 1 fully masked, the key tile 64 .. 127 masked everywhere
        bits = (rng.random((B, 1, m, n)) < 0.5).astype(np.float32)
        bits[1] = 0.0
        bits[:, :, :, 64:128] = 0.0
        mask = torch.from_numpy(bits).cuda().to(dt)
    want = _ref(_np64(q), _np64(k), _np64(v), None if mask is None else _np64(mask), _np64(top), H)

    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    runs = []
    for _ in range(2 if twice else 1):
        q.grad = k.grad = v.grad = None
        out = ha.MultiHeadAttentionLayer(H)(q, k, v, mask)
        out.backward(top)
        torch.cuda.synchronize()
        runs.append([_np64(t) for t in (out, q.grad, k.grad, v.grad)])
    what = f"{dtype_name} B={B} H={H} m={m} n={n} d={d} mask={masked}"
    for got, w, name in zip(runs[0], want, ("out", "dq", "dk", "dv")):
        assert_close(got, w, *_tol(dtype_name, name != "out"), f"{what} {name}")
    for a, b in zip(runs[0], runs[-1]):  # no atomics: the same bits again
        assert np.array_equal(a, b)
