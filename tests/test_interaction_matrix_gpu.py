"""The dot interaction's kernels (hugectr_amd/csrc/interaction.hip) against a float64 restatement of
the operation, in every branch their dispatch can take and with batches larger than one grid.

  * the reference is `_ref_fwd` / `_ref_bwd` below (numpy float64), never a kernel, torch on the
    GPU or the oracle; for 16-bit types it is computed from the inputs after rounding to the type;
  * every kernel is called through the C ABI on buffers this file allocates: each output lies
    between two guard regions (at least one row each, a multiple of 16 bytes so that the inner view
    keeps the allocation's alignment) filled with a sentinel that must survive the call;
  * tolerances are the ones tests/test_dense_gpu.py applies to the same kernels (`_tol`): the cases
    here change n_emb, B, alignment and branch, not the forward dot length (W), and the backward dot
    length (n_ins) only moves from 27 to at most 41.  The pass-through columns and the pad column
    are exact.

Dispatch (interaction_fwd_impl / interaction_bwd_impl); out_len = W + n_ins (n_ins - 1) / 2 + 1:
  forward   W in {16, 32, 64, 128}, n_ins <= 32, every buffer 16-byte aligned:
            fp32 -> interaction_fwd_mfma_kernel, 16-bit -> interaction_fwd16_kernel; the output row
            leaves as 16-byte stores when out_len % 4 == 0 (fp32) / % 8 == 0 (16-bit), else by the
            scalar-store tail;  anything else -> interaction_fwd_generic_kernel<T>
  backward  W in {32, 64, 128}, n_ins <= 32, aligned, out_len % 4 == 0 (fp32) / % 8 == 0 (16-bit):
            interaction_bwd_mfma_kernel / interaction_bwd16_kernel;  anything else ->
            interaction_bwd_generic_kernel<T>
The MFMA kernels run min(B, 2048) single-wavefront workgroups, the generic ones
min(ceil(B / 4), 512) blocks of four wavefronts: only B > 2048 makes a workgroup prefetch a second
sample."""
import functools
import os

import numpy as np
import pytest

from util import assert_close

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
EPS = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}
DTYPES = ["float32", "float16", "bfloat16"]
NO_ROW = 0xFFFFFFFFFFFFFFFF
SENTINEL = -1536.0  # exact in fp16 and bf16, far outside anything the kernels compute here


def _tol(dtype_name, backward):
    """(rtol, atol) of test_interaction_fwd_bwd (fp32) and test_interaction_16bit (16-bit)"""
    if dtype_name == "float32":
        return 2e-4, 1e-3
    eps = EPS[dtype_name]
    return (4 * eps, 32 * eps) if backward else (2 * eps, 24 * eps)


# ---- the reference -------------------------------------------------------------------------------
def _ref_fwd(mlp, emb):
    X = np.concatenate([mlp[:, None, :], emb], axis=1).astype(np.float64)
    Z = X @ X.transpose(0, 2, 1)
    n, m = np.tril_indices(X.shape[1], -1)  # (1,0) (2,0) (2,1) (3,0) ..: pair n(n-1)/2 + m
    return np.concatenate([X[:, 0], Z[:, n, m], np.zeros((X.shape[0], 1))], axis=1)


def _ref_bwd(mlp, emb, top):
    X = np.concatenate([mlp[:, None, :], emb], axis=1).astype(np.float64)
    B, n_ins, W = X.shape
    n, m = np.tril_indices(n_ins, -1)
    dM = np.zeros((B, n_ins, n_ins))
    dM[:, n, m] = top[:, W:-1]
    dX = (dM + dM.transpose(0, 2, 1)) @ X
    return top[:, :W] + dX[:, 0], dX[:, 1:]


# ---- buffers -------------------------------------------------------------------------------------
class _Guarded:
    """a [shape] output inside a larger allocation of SENTINEL: `t` is the view the kernel gets
    (`off` elements past a 16-byte boundary), the rest must still hold SENTINEL afterwards"""

    def __init__(self, shape, dt, off=0):
        import torch
        n = int(np.prod(shape))
        row = int(np.prod(shape[1:]))
        pad = -(-row // 8) * 8  # >= one row, a multiple of 16 bytes for 2- and 4-byte elements
        self.buf = torch.full((pad + off + n + pad,), SENTINEL, dtype=dt, device="cuda")
        self.lo, self.hi = pad + off, pad + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        assert self.t.data_ptr() % 16 == (off * self.buf.element_size()) % 16

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        assert bool((self.buf[:self.lo] == SENTINEL).all()), f"{what}: wrote in front of its rows"
        assert bool((self.buf[self.hi:] == SENTINEL).all()), f"{what}: wrote behind its rows"


def _placed(t, off):
    """t itself (off == 0), or a contiguous copy that starts `off` elements into an allocation"""
    import torch
    if off == 0:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _np64(t):
    return t.float().cpu().numpy().astype(np.float64)


class _Case:
    """inputs of one shape on the device (already rounded to the type), the same numbers in
    float64, and the reference's forward and backward of them (computed once, never written)"""

    def __init__(self, dtype_name, mlp, emb, top):
        self.dtype_name = dtype_name
        self.mlp, self.emb, self.top = mlp, emb, top
        self.B, self.W = mlp.shape
        self.n_emb = emb.shape[1]
        n_ins = self.n_emb + 1
        self.out_len = self.W + n_ins * (n_ins - 1) // 2 + 1
        assert tuple(top.shape) == (self.B, self.out_len)
        self.mlp64, self.emb64, self.top64 = _np64(mlp), _np64(emb), _np64(top)
        self.want_out = _ref_fwd(self.mlp64, self.emb64)
        self.want_mlp_grad, self.want_emb_grad = _ref_bwd(self.mlp64, self.emb64, self.top64)

    def check_fwd(self, out, what):
        got = _np64(out)
        assert np.array_equal(got[:, :self.W], self.mlp64), f"{what}: pass-through columns"
        assert not got[:, -1].any(), f"{what}: pad column"
        assert_close(got, self.want_out, *_tol(self.dtype_name, False), what)

    def check_bwd(self, mlp_grad, emb_grad, what):
        tol = _tol(self.dtype_name, True)
        assert_close(_np64(mlp_grad), self.want_mlp_grad, *tol, what + " mlp grad")
        assert_close(_np64(emb_grad), self.want_emb_grad, *tol, what + " emb grad")


def _draw(dtype_name, B, n_emb, W, seed=0):
    """seeded standard normal mlp [B, W], emb [B, n_emb, W], top_grad [B, out_len] in the type"""
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng([B, n_emb, W, seed])
    n_ins = n_emb + 1
    shapes = [(B, W), (B, n_emb, W), (B, W + n_ins * (n_ins - 1) // 2 + 1)]
    return [torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda().to(dt)
            for s in shapes]


@functools.lru_cache(maxsize=2)
def _case(dtype_name, B, n_emb, W):
    return _Case(dtype_name, *_draw(dtype_name, B, n_emb, W))


def _abi():
    from hugectr_amd import _lib
    return _lib.lib, _lib.ptr, _lib.check, _lib.stream_ptr, \
        {"float32": _lib.F32, "float16": _lib.F16, "bfloat16": _lib.BF16}


def _forward(c, off=None):
    """hctr_interaction_fwd on the case's inputs -> the guarded output, guards checked; off names
    the one buffer (mlp / emb / out) that starts one element past a 16-byte boundary"""
    lib, ptr, check, stream_ptr, DT = _abi()
    mlp, emb = _placed(c.mlp, int(off == "mlp")), _placed(c.emb, int(off == "emb"))
    out = _Guarded((c.B, c.out_len), c.mlp.dtype, int(off == "out"))
    check(lib.hctr_interaction_fwd(c.B, c.n_emb, c.W, ptr(mlp), ptr(emb), ptr(out.t),
                                   DT[c.dtype_name], stream_ptr()))
    out.check("out")
    return out.t


def _backward(c, off=None):
    lib, ptr, check, stream_ptr, DT = _abi()
    mlp, emb = _placed(c.mlp, int(off == "mlp")), _placed(c.emb, int(off == "emb"))
    top = _placed(c.top, int(off == "top_grad"))
    mg = _Guarded((c.B, c.W), c.mlp.dtype, int(off == "mlp_grad"))
    eg = _Guarded((c.B, c.n_emb, c.W), c.mlp.dtype, int(off == "emb_grad"))
    check(lib.hctr_interaction_bwd(c.B, c.n_emb, c.W, ptr(mlp), ptr(emb), ptr(top), ptr(mg.t),
                                   ptr(eg.t), DT[c.dtype_name], stream_ptr()))
    mg.check("mlp_grad")
    eg.check("emb_grad")
    return mg.t, eg.t


def _fwd_bwd(dtype_name, B, n_emb, W):
    c = _case(dtype_name, B, n_emb, W)
    what = f"{dtype_name} B={B} n_emb={n_emb} W={W}"
    c.check_fwd(_forward(c), what + " fwd")
    c.check_bwd(*_backward(c), what + " bwd")


def test_reference_agrees_with_the_oracle(oracle):
    """the float64 reference of this file and the oracle's fp32 restatement of the reference
    layer, on one shape.  Bound: the oracle accumulates in fp32, so each of its dot products of
    length L carries at most ~L 2^-24 sum_k |a_k b_k|; L <= 32 here and sum_k |a_k b_k| of 32
    products of standard normals stays below 64, which gives 32 * 6e-8 * 64 ~ 1.2e-4 absolute"""
    rng = np.random.default_rng(5)
    B, n_emb, W = 9, 13, 32
    mlp = rng.standard_normal((B, W), dtype=np.float32)
    emb = rng.standard_normal((B, n_emb, W), dtype=np.float32)
    top = rng.standard_normal((B, W + 14 * 13 // 2 + 1), dtype=np.float32)
    assert_close(oracle.interaction_fwd(mlp, emb), _ref_fwd(mlp, emb), 0, 1.2e-4, "fwd")
    mg, eg = oracle.interaction_bwd(mlp, emb, top)
    want_mg, want_eg = _ref_bwd(mlp, emb, top.astype(np.float64))
    assert_close(mg, want_mg, 0, 1.2e-4, "mlp grad")
    assert_close(eg, want_eg, 0, 1.2e-4, "emb grad")


# ---- 1. the branch matrix ------------------------------------------------------------------------
# B = 70: more than one block, and no multiple of the generic kernels' four waves per block.
# At W in {16, 32, 64, 128} (W % 8 == 0, so out_len % 8 == (pairs + 1) % 8) and aligned buffers:
#   n_emb  pairs+1  forward                                               backward
#    1       2      fwd_mfma / fwd16, scalar-store tail (out_len % 4 = 2)  generic (out_len % 4)
#    3       7      fwd_mfma / fwd16, scalar-store tail (odd out_len)      generic
#   15     121      fwd_mfma / fwd16, scalar-store tail                    generic
#   16     137      fwd_mfma / fwd16, scalar-store tail, rows >= 16 live   generic
#   31     497      fwd_mfma / fwd16, n_ins == 32: all 496 pairs, the      generic
#                   last lane rows of the 32 x 32 tile, scalar-store tail
#   32       -      n_ins == 33: fwd_generic<T>, the first generic n       generic
# W == 16 reaches interaction_fwd_mfma_kernel<16> / interaction_fwd16_kernel<16, *> forward; there
# is no W == 16 MFMA backward.  (The 16-byte-store forward and the MFMA backward need
# out_len % 4 / % 8 == 0: those n_emb are in section 2 and 3.)
MATRIX = [(n_emb, W) for W in (16, 32, 64, 128) for n_emb in (1, 3, 15, 16, 31, 32)]
# W in {10, 24}: no MFMA width -> fwd_generic<T> and bwd_generic<T> in all three types, below
# (n_emb 3) and above (n_emb 40, n_ins 41: the longest backward dot product) the MFMA's 32 rows
MATRIX += [(n_emb, W) for W in (10, 24) for n_emb in (3, 40)]


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n_emb,W", MATRIX)
def test_branch_matrix(dtype_name, n_emb, W):
    _fwd_bwd(dtype_name, 70, n_emb, W)


# ---- 2. the MFMA backward ------------------------------------------------------------------------
@pytest.mark.parametrize("W", [32, 64, 128])
@pytest.mark.parametrize("dtype_name,n_emb", [
    ("float32", 2), ("float32", 18), ("float32", 29),  # out_len - W = 4, 172, 436: % 4 == 0
    ("float16", 5), ("float16", 10), ("float16", 21),  # out_len - W = 16, 56, 232: % 8 == 0
    ("bfloat16", 5), ("bfloat16", 10), ("bfloat16", 21)])
def test_mfma_backward_reach(dtype_name, n_emb, W):
    """interaction_bwd_mfma_kernel<W> (fp32) and interaction_bwd16_kernel<W, *, false> (16-bit),
    and the 16-byte-store forward: only n_emb with out_len % 4 == 0 (fp32) / % 8 == 0 (16-bit) get
    there.  n_emb = 29 (n_ins = 30, 435 pairs) is the largest shape the fp32 MFMA backward can
    see, 26 (section 3) the largest for the 16-bit one: 30 and 31 give out_len % 4 == 2 and 1."""
    _fwd_bwd(dtype_name, 70, n_emb, W)


# ---- 3. past one grid ----------------------------------------------------------------------------
def _default_grid_only():
    for v in ("HCTR_INTER_WAVES", "HCTR_GATHER_WAVES"):
        if os.environ.get(v):
            pytest.skip(f"{v} is set: the batch sizes of this test assume the default grid of 2048")


PAST_GRID = [("float32", 26, 128), ("float32", 2, 64), ("float32", 29, 32),  # fwd_mfma / bwd_mfma
             ("float16", 26, 128), ("float16", 5, 32),                     # fwd16 / bwd16
             ("bfloat16", 26, 128), ("bfloat16", 5, 32),
             ("float32", 3, 10), ("bfloat16", 40, 24)]                      # generic: 512 blocks
if EMU:  # (the host interpreter: the narrow shapes walk the same loops)
    PAST_GRID = [p for p in PAST_GRID if p[2] <= 32]


@pytest.mark.parametrize("B", [2049, 4133])
@pytest.mark.parametrize("dtype_name,n_emb,W", PAST_GRID)
def test_past_one_grid(dtype_name, n_emb, W, B):
    """B = 2049: one workgroup takes a second sample, every other prefetch is masked; B = 4133:
    two to three iterations with a ragged last round.  In the generic kernels (grid capped at 512
    blocks of four waves) some waves of a block idle in the last round while the others work
    across __syncthreads."""
    _default_grid_only()
    _fwd_bwd(dtype_name, B, n_emb, W)


# ---- 4. misaligned buffers -----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mlp", "emb", "out", "top_grad", "mlp_grad", "emb_grad"])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n_emb,W", [(26, 128), (5, 32)])
def test_one_misaligned_buffer_takes_the_generic_path(dtype_name, n_emb, W, which):
    """one buffer at a time starts one element past a 16-byte boundary: the MFMA kernels' 16-byte
    loads and stores cannot be used, the a16 / g16 terms of the dispatch send the call to
    interaction_{fwd,bwd}_generic_kernel<T>, and the result meets the same tolerances.  Called
    through the C ABI (the autograd wrappers' .contiguous() would not realign a contiguous view
    either)."""
    c = _case(dtype_name, 70, n_emb, W)
    what = f"{dtype_name} n_emb={n_emb} W={W} misaligned {which}"
    if which in ("mlp", "emb", "out"):
        c.check_fwd(_forward(c, which), what + " fwd")
    if which != "out":
        c.check_bwd(*_backward(c, which), what + " bwd")


# ---- 5. rows through row_of ----------------------------------------------------------------------
@pytest.mark.parametrize("scatter", [False, True])
@pytest.mark.parametrize("dtype_name,n_emb,W", [("bfloat16", 26, 128), ("float16", 10, 32)])
def test_indexed_and_scatter_against_the_reference(dtype_name, n_emb, W, scatter):
    """the entry points behind interaction_indexed: hctr_interaction_fwd_indexed and
    hctr_interaction_bwd_indexed over 97 distinct rows (heavy repeats in row_of), and
    hctr_interaction_bwd_indexed_scatter (interaction_indexed(scatter_grad=True)) where row_of is
    a permutation of the B * n_emb rows and the gradient of embedding (b, s) lands in row
    row_of[b, s]; B = 4133 (three rounds of the grid, ragged).  Against the float64 reference of
    the expanded tensor, not only against the dense kernel."""
    import torch
    _default_grid_only()
    B = 260 if EMU and W > 32 else 4133
    lib, ptr, check, stream_ptr, DT = _abi()
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng([B, n_emb, W, int(scatter)])
    R = B * n_emb if scatter else 97
    rows = torch.from_numpy(rng.standard_normal((R, W), dtype=np.float32)).cuda().to(dt)
    if scatter:
        row_np = rng.permutation(R).astype(np.int32).reshape(B, n_emb)
    else:
        row_np = rng.integers(0, R, (B, n_emb)).astype(np.int32)
    row_of = torch.from_numpy(row_np).cuda()
    mlp, _, top = _draw(dtype_name, B, n_emb, W, seed=1)
    c = _Case(dtype_name, mlp, rows[row_of.long()].contiguous(), top)

    out = _Guarded((B, c.out_len), dt)
    check(lib.hctr_interaction_fwd_indexed(B, n_emb, W, ptr(mlp), ptr(rows), ptr(row_of),
                                           ptr(out.t), DT[dtype_name], stream_ptr()))
    out.check("out")
    c.check_fwd(out.t, "indexed fwd")

    mg = _Guarded((B, W), dt)
    eg = _Guarded((B * n_emb, W), dt)
    fn = lib.hctr_interaction_bwd_indexed_scatter if scatter else lib.hctr_interaction_bwd_indexed
    check(fn(B, n_emb, W, ptr(mlp), ptr(rows), ptr(row_of), ptr(top), ptr(mg.t), ptr(eg.t),
             DT[dtype_name], stream_ptr()))
    mg.check("mlp_grad")
    eg.check("emb_grad")
    emb_grad = eg.t[row_of.long().reshape(-1)] if scatter else eg.t
    c.check_bwd(mg.t, emb_grad.view(B, n_emb, W), "indexed bwd")


# ---- 6. the gather fused into the interaction ----------------------------------------------------
def _gather_case(dtype_name, B, n_emb, W):
    """table [R][W] fp32, value_index [B * n_emb] with ~10 % missing rows (among them the whole
    first and last sample and a few whole samples in between) -> (table, value_index as int64
    bits, live mask [B, n_emb], the case of the rounded rows)"""
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng([B, n_emb, W, 6])
    R = 1000
    table = torch.from_numpy(rng.standard_normal((R, W), dtype=np.float32)).cuda()
    vi = rng.integers(0, R, (B, n_emb)).astype(np.uint64)
    vi[rng.random((B, n_emb)) < 0.08] = NO_ROW
    vi[rng.random(B) < 0.02] = NO_ROW
    vi[0] = vi[-1] = NO_ROW
    live = vi != NO_ROW
    assert 0.05 < 1.0 - live.mean() < 0.15
    vi_t = torch.from_numpy(vi.reshape(-1).view(np.int64)).cuda()
    live_t = torch.from_numpy(live).cuda()
    idx = torch.from_numpy(np.where(live, vi, 0).astype(np.int64)).cuda()
    emb = torch.where(live_t[:, :, None], table[idx], torch.zeros((), device="cuda")).to(dt)
    mlp, _, top = _draw(dtype_name, B, n_emb, W, seed=6)
    return table, vi_t, live_t, _Case(dtype_name, mlp, emb.contiguous(), top)


@pytest.mark.parametrize("store_pooled", [False, True])
@pytest.mark.parametrize("dtype_name", ["float16", "bfloat16"])
@pytest.mark.parametrize("B,n_emb,W", [(2049, 7, 16), (4133, 5, 32),
                                       (70, 26, 128) if EMU else (2049, 26, 128)])
def test_gather_forward_against_the_reference(dtype_name, B, n_emb, W, store_pooled):
    """hctr_interaction_fwd_gather (interaction_fwd16_gather_kernel<W, *, STORE>) on a torch fp32
    table and a uint64 value_index: the output against the reference of the rounded rows; the
    pooled vectors, where asked for, are the table rows rounded to the type bit for bit and exact
    +0 for a missing row.  Row numbers are prefetched two samples ahead: B = 4133 > 2 * 2048."""
    import torch
    _default_grid_only()
    lib, ptr, check, stream_ptr, DT = _abi()
    table, vi, live, c = _gather_case(dtype_name, B, n_emb, W)
    out = _Guarded((B, c.out_len), c.mlp.dtype)
    pooled = _Guarded((B, n_emb, W), c.mlp.dtype) if store_pooled else None
    check(lib.hctr_interaction_fwd_gather(B, n_emb, W, ptr(c.mlp), ptr(table), ptr(vi),
                                          ptr(pooled.t) if pooled else None, ptr(out.t),
                                          DT[dtype_name], stream_ptr()))
    out.check("out")
    c.check_fwd(out.t, "gather fwd")
    if pooled:
        pooled.check("pooled")
        assert torch.equal(pooled.t.view(torch.int16), c.emb.view(torch.int16))
        assert not bool(pooled.t.view(torch.int16)[~live].any()), "a missing row is not +0"


@pytest.mark.parametrize("B", [2049, 4133])
@pytest.mark.parametrize("dtype_name", ["float16", "bfloat16"])
@pytest.mark.parametrize("n_emb,W", [(5, 32)] if EMU else [(26, 128), (5, 32)])
def test_gather_backward_against_the_reference(dtype_name, n_emb, W, B):
    """hctr_interaction_bwd_gather (interaction_bwd16_kernel<W, *, true>): the tile is rebuilt
    from table + value_index, the row numbers one sample ahead of the rows; both gradients against
    the reference of the rounded rows (a missing row is a zero row of X: its gradient is G's row
    times the rest, not zero)"""
    _default_grid_only()
    lib, ptr, check, stream_ptr, DT = _abi()
    table, vi, live, c = _gather_case(dtype_name, B, n_emb, W)
    mg = _Guarded((B, W), c.mlp.dtype)
    eg = _Guarded((B, n_emb, W), c.mlp.dtype)
    check(lib.hctr_interaction_bwd_gather(B, n_emb, W, ptr(c.mlp), ptr(table), ptr(vi), ptr(c.top),
                                          ptr(mg.t), ptr(eg.t), DT[dtype_name], stream_ptr()))
    mg.check("mlp_grad")
    eg.check("emb_grad")
    c.check_bwd(mg.t, eg.t, "gather bwd")


# ---- 7. the host-side contract (no kernel is launched) -------------------------------------------
def test_regather_supported_is_what_bwd_gather_accepts():
    """layers.regather_supported(W, n_emb) == hctr_interaction_bwd_gather(batch = 0, ..) returns
    OK: the entry point checks n_emb, type, width and out_len before its `batch == 0` return (and
    pointers only after it)"""
    from hugectr_amd import _lib, layers
    for W in (8, 16, 32, 64, 128, 256):
        for n_emb in range(1, 34):
            rc = _lib.lib.hctr_interaction_bwd_gather(0, n_emb, W, None, None, None, None, None,
                                                      None, _lib.F16, _lib.stream_ptr())
            assert (rc == 0) == layers.regather_supported(W, n_emb), (W, n_emb, _lib.last_error())
            if rc != 0:
                assert "interaction_bwd_gather" in _lib.last_error()


def test_indexed_entry_points_refuse_what_they_cannot_run():
    """width 16 (no 16-bit MFMA backward of that width), n_emb = 32 (33 rows) and a misaligned
    buffer have no generic kernel to fall back to when the rows come through row_of: the indexed
    entry points refuse them by name -- before the `batch == 0` return, so batch = 0 asks"""
    import torch
    from hugectr_amd import _lib
    lib, ptr, s = _lib.lib, _lib.ptr, _lib.stream_ptr()
    buf = torch.zeros(64, dtype=torch.float16, device="cuda")
    ok, odd = buf[:32], buf[1:33]
    row_of = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert ok.data_ptr() % 16 == 0 and odd.data_ptr() % 16 != 0

    def fwd(n_emb, W, mlp=ok, rows=ok, out=ok):
        return lib.hctr_interaction_fwd_indexed(0, n_emb, W, ptr(mlp), ptr(rows), ptr(row_of),
                                                ptr(out), _lib.F16, s)

    def bwd(n_emb, W, mlp=ok, rows=ok, top=ok, mg=ok, eg=ok, fn=None):
        fn = fn or lib.hctr_interaction_bwd_indexed
        return fn(0, n_emb, W, ptr(mlp), ptr(rows), ptr(row_of), ptr(top), ptr(mg), ptr(eg),
                  _lib.F16, s)

    def refused(rc):
        assert rc != 0 and "indexed interaction: 16-bit rows, width 32/64/128, <= 31 embeddings" \
            in _lib.last_error(), (rc, _lib.last_error())

    assert fwd(5, 32) == 0 and bwd(5, 32) == 0  # (out_len = 48)
    assert bwd(5, 32, fn=lib.hctr_interaction_bwd_indexed_scatter) == 0
    refused(fwd(5, 16))
    refused(bwd(5, 16))
    refused(bwd(5, 16, fn=lib.hctr_interaction_bwd_indexed_scatter))
    refused(fwd(32, 32))
    refused(bwd(32, 32))
    refused(bwd(6, 32))  # out_len = 54: % 8 != 0
    for k in ("mlp", "rows", "out"):
        refused(fwd(5, 32, **{k: odd}))
    for k in ("mlp", "rows", "top", "mg", "eg"):
        refused(bwd(5, 32, **{k: odd}))
        refused(bwd(5, 32, fn=lib.hctr_interaction_bwd_indexed_scatter, **{k: odd}))
    assert lib.hctr_interaction_fwd_indexed(0, 5, 32, ptr(ok), ptr(ok), None, ptr(ok), _lib.F16,
                                            s) != 0
    assert "null pointer" in _lib.last_error()


def test_a_tile_above_160_kib_is_refused():
    """generic path, n_emb = 40, W = 256, fp32: 4 waves x 41 x 257 floats = 168,592 B forward (more
    with G backward) > 160 KiB of LDS -> "tile does not fit LDS" instead of a launch (this
    REQUIRE sits behind the `batch == 0` return: batch = 1 on real buffers)"""
    import torch
    from hugectr_amd import _lib
    lib, ptr, s = _lib.lib, _lib.ptr, _lib.stream_ptr()
    n_emb, W = 40, 256
    out_len = W + 41 * 40 // 2 + 1
    mlp = torch.zeros((1, W), device="cuda")
    emb = torch.zeros((1, n_emb, W), device="cuda")
    out = _Guarded((1, out_len), torch.float32)
    assert lib.hctr_interaction_fwd(1, n_emb, W, ptr(mlp), ptr(emb), ptr(out.t), _lib.F32, s) != 0
    assert "tile does not fit LDS" in _lib.last_error()
    mg, eg = _Guarded((1, W), torch.float32), _Guarded((1, n_emb, W), torch.float32)
    top = torch.zeros((1, out_len), device="cuda")
    assert lib.hctr_interaction_bwd(1, n_emb, W, ptr(mlp), ptr(emb), ptr(top), ptr(mg.t), ptr(eg.t),
                                    _lib.F32, s) != 0
    assert "tile does not fit LDS" in _lib.last_error()
    for g in (out, mg, eg):
        g.check("a refused call")
        assert bool((g.t == SENTINEL).all())


# ---- 8. 64 KiB < LDS <= 160 KiB ------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name,n_emb,W", [
    ("float32", 32, 128),   # 4 x 33 x 129 floats = 68,112 B forward, 85,536 B backward
    ("bfloat16", 32, 128),  # the same tile: the generic kernels stage every type as fp32
    ("float32", 40, 128)])  # 84,624 B forward, 111,520 B backward
def test_generic_tile_between_64_and_160_kib(dtype_name, n_emb, W):
    """the first shapes a model with more than 31 tables reaches: the generic kernels' dynamic LDS
    is above the 64 KiB a kernel may use without being told (the launch raises the limit with
    hipFuncSetAttribute) and within the 160 KiB the entry points promise"""
    _fwd_bwd(dtype_name, 9, n_emb, W)
