"""The dense kernels next to the GEMMs (hugectr_amd/csrc/dense_ops.hip) against a float64 restatement
of each operation, in every branch their host dispatch can take and with more rows than one grid
covers.

  * every kernel is called through the C ABI on buffers this file allocates (util.DevIn / DevOut):
    inputs must be unchanged after the call, every output lies between FRONT elements of poison and
    GUARD rows of poison that must survive it, every workspace is such an output too (NaN all over
    before the call: a finish kernel that reads a partial no producer wrote returns NaN);
  * the reference is numpy float64, or IEEE fp32 arithmetic on the CPU where the result is defined
    bit for bit; for 16-bit types it starts from the inputs after rounding to the type.  Never a
    kernel, torch on the GPU or the oracle.  Producers that need an earlier kernel's result (the
    cross backward's `outputs` / `hiddens`, the skinny backward's `y`) get the reference's, rounded;
  * the fixed-order reductions (cross v1 backward, ReLU backward, cross-v2 step, logit head, skinny
    backward, BCE) are called twice and must return the same bits.

Dispatch, as the host code decides it (a case below names the branch it is there for):

  hctr_cross_v1_fwd / _bwd   one wavefront per row, NPL columns per lane: with_npl takes
        NPL from {1, 2, 4, 8, 16, 32, 64} by ceil(w / 64) (w <= 4096).  Forward: min(ceil(B / 4),
        2048) blocks of 4 wavefronts, a second row per wavefront from B > 8192.  Backward: always
        1024 wavefronts (a second row from B > 1024, a third from B > 2048) with their dW / db
        partial rows in LDS when layers * 2 * w * 4 <= 60 KiB (layers * w <= 7680,
        cross_v1_bwd_kernel<NPL, true>, one wavefront per workgroup) and in the workspace otherwise
        (<NPL, false>, 4 wavefronts per workgroup); cross_v1_reduce_kernel adds the 1024 partial
        rows in a fixed order.
  hctr_relu_bwd_bias(_partials)   128 rows per workgroup; cw = min(n / 8, 256) column threads,
        rg = 256 / cw row groups (threads >= cw * rg idle); n / 8 > 256 walks the columns in
        several passes (the last one ragged); the COLSUM finish adds the tiles in 32 groups.
  hctr_cross_v2_bwd_step     the same thread layout on a (row tiles, column blocks) grid; rows per
        tile = 128, halved down to 16 while ceil(B / rows) * column blocks < 2048:
        at width 8   B <= 65504 -> 16,  <= 131008 -> 32,  <= 262016 -> 64,  above -> 128.
  hctr_logit_head(_partials) NSEG = {1, 2, 4, 8} by ceil(K / 256) <= 1, 2, 4, 8 with ROWS = 8, 4,
        2, 1 rows per wavefront and step; min(ceil(B / (4 ROWS)), 1024) blocks: a second sweep from
        B > 32768, 16384, 8192, 4096.  K = 1028 (ceil = 5) runs NSEG = 8 with three dead segments.
  hctr_skinny_fc_fwd         R = min(256, ceil(B / 1024) rounded up to even) rows per block.
  hctr_skinny_fc_bwd(_partials)  K < 16, N % 8 == 0, 16-byte aligned dy / y: the matrix-core form,
        min(256, ceil(B / (16 rsets))) blocks with rsets = 16 / ceil(N / 128): a second sweep from
        B > 16384 at N = 512 and B > 65536 at N <= 128.  Otherwise the vector-ALU form, min(256,
        ceil(B / 8)) blocks taking two rows per step: a second step from B > 4096.
  hctr_sgd_shadow            min(ceil(n / 4 / 256), 4096) blocks: a second pass from n > 4 * 256 *
        4096 elements.
  hctr_bce_loss              min(ceil(B / 256), 256) blocks.

Under HCTR_EMU=1 (the host interpreter of tests/emu, which steps through every thread) the cases
that exist only for a second pass over the grid are shrunk or left out; the parameter lists say
which (`_hw_only`), as tests/test_dense_ftrl_gpu.py::_sizes does."""
import functools
import os

import numpy as np
import pytest

from util import GUARD, DevIn, DevOut
from util import lib_code as _code
from util import assert_close as _within

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
FRONT = 64  # elements of poison in front of every output: a multiple of 16 bytes in every type
DT16 = ["bf16", "f16"]


def _hw_only(cases):
    """cases that are there for a second pass over the grid: left to the hardware"""
    return [] if EMU else cases


def _abi():
    from hugectr_amd import _lib
    return _lib.lib, _lib.check, _lib.stream_ptr()


def assert_close(got, want, rtol, atol, what):
    """util.assert_close on a result that holds no NaN or infinity: `|got - want| > tol` is false
    for a NaN, and NaN is what the poison of this file leaves where a kernel did not write (or
    read what no producer wrote)"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{what}: {(~np.isfinite(got)).sum()} of {got.size} not finite"
    _within(got, want, rtol, atol, what)


def _out(rows, D, dt, mis=0):
    """an output (or workspace) between poison: fp32 as NaN, 16-bit as the raw words 0xFFFF"""
    assert GUARD >= 1
    return DevOut(rows, D, dt, mis=FRONT + mis, int_bits=dt != "f32")


def _in16(words, mis=0):
    return DevIn(np.ascontiguousarray(words).view(np.int16), mis)


def _words(res):
    """the raw words of a 16-bit DevOut.result()"""
    return np.ascontiguousarray(res).view(np.uint16)


def _to16(a, dt):
    """fp32 -> the bits of the 16-bit type, round to nearest even (there is no NaN among the values
    of this file)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dt == "f16":
        with np.errstate(over="ignore", under="ignore"):
            return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _from16(words, dt):
    """the bits of the 16-bit type -> fp32 (exact)"""
    words = np.ascontiguousarray(words).view(np.uint16)
    if dt == "f16":
        return words.view(np.float16).astype(np.float32)
    return (words.astype(np.uint32) << 16).view(np.float32)


def _round16(a, dt):
    return _from16(_to16(a, dt), dt)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), f"{what}: not the same bits"


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ==================================================================================================
# 1. cross v1
# ==================================================================================================
def _cross_ref(x0, k, b, og):
    """x_{l+1} = x0 (x_l . w_l) + b_l + x_l and its backward, float64"""
    x0, k, b, og = (np.asarray(a, dtype=np.float64) for a in (x0, k, b, og))
    L, w = k.shape
    xs, hid = [x0], []
    for l in range(L):
        h = xs[-1] @ k[l]
        hid.append(h)
        xs.append(x0 * h[:, None] + b[l] + xs[-1])
    dy, dx0 = og, np.zeros_like(x0)
    dW, dB = np.zeros((L, w)), np.zeros((L, w))
    for l in range(L - 1, -1, -1):
        dx0 = dx0 + dy * hid[l][:, None]
        tv = (dy * x0).sum(1)
        dW[l] = tv @ xs[l]
        dB[l] = dy.sum(0)
        dy = dy + tv[:, None] * k[l]
    return {"hiddens": np.stack(hid), "outputs": np.stack(xs[1:]), "in_grad": dx0 + dy,
            "kernel_grads": dW, "bias_grads": dB}


# test_cross_v1_fwd_bwd's (tests/test_dense_gpu.py)
CROSS_TOL = {"hiddens": (1e-4, 1e-4), "outputs": (1e-4, 1e-4), "in_grad": (1e-4, 1e-4),
             "kernel_grads": (2e-4, 1e-4), "bias_grads": (2e-4, 1e-4)}
CROSS_FWD = ("hiddens", "outputs")
CROSS_BWD = ("in_grad", "kernel_grads", "bias_grads")


def _cross_check(got, want, names, what):
    for name in names:
        assert_close(np.asarray(got[name]).reshape(want[name].shape), want[name], *CROSS_TOL[name],
                     f"{what} {name}")


@functools.lru_cache(maxsize=1)
def _cross_case(B, w, L):
    rng = np.random.default_rng([B, w, L])
    x0 = (0.1 * np.clip(rng.standard_normal((B, w)), -0.9, 0.9)).astype(np.float32)
    k = (np.clip(rng.standard_normal((L, w)), -1, 1) * min(1.0, 8 / np.sqrt(w))).astype(np.float32)
    b = (0.01 * rng.standard_normal((L, w))).astype(np.float32)
    og = (0.1 + 0.01 * rng.standard_normal((B, w))).astype(np.float32)
    want = _cross_ref(x0, k, b, og)
    # the bound must see a lost column: the reference of the same inputs with the last column's
    # kernel weights zeroed has to fail the comparison, forward and backward (CPU only)
    k_lost = k.copy()
    k_lost[:, -1] = 0
    lost = _cross_ref(x0, k_lost, b, og)
    what = f"B={B} w={w} L={L}: a lost column"
    assert _fails(_cross_check, lost, want, CROSS_FWD, what), what + " passes the forward bound"
    assert _fails(_cross_check, lost, want, CROSS_BWD, what), what + " passes the backward bound"
    return x0, k, b, og, want


def _cross_forward(B, w, L, mis=0):
    lib, check, s = _abi()
    x0, k, b, _, want = _cross_case(B, w, L)
    what = f"cross v1 fwd B={B} w={w} L={L} mis={mis}"
    ins = [DevIn(a, mis) for a in (x0, k, b)]
    outputs, hiddens = _out(L * B, w, "f32", mis), _out(L * B, 1, "f32", mis)
    check(lib.hctr_cross_v1_fwd(B, w, L, ins[0].p, ins[1].p, ins[2].p, outputs.p, hiddens.p, s))
    got = {"outputs": outputs.result(), "hiddens": hiddens.result()}
    for a, name in zip(ins, ("x0", "kernels", "biases")):
        a.assert_unchanged(name)
    _cross_check(got, want, CROSS_FWD, what)


def _cross_backward(B, w, L, mis=0):
    lib, check, s = _abi()
    x0, k, _, og, want = _cross_case(B, w, L)
    what = f"cross v1 bwd B={B} w={w} L={L} mis={mis}"
    ins = [DevIn(a, mis) for a in (x0, k, want["outputs"].astype(np.float32),
                                   want["hiddens"].astype(np.float32), og)]
    ws_bytes = lib.hctr_cross_v1_bwd_workspace_bytes(B, w, L)
    assert ws_bytes == 1024 * L * 2 * w * 4
    runs = []
    for _ in range(2):
        ws = _out(1024 * L * 2, w, "f32", mis)
        ig, kg, bg = _out(B, w, "f32", mis), _out(L, w, "f32", mis), _out(L, w, "f32", mis)
        check(lib.hctr_cross_v1_bwd(B, w, L, *(a.p for a in ins), ig.p, kg.p, bg.p, ws.p, s))
        runs.append({"in_grad": ig.result(), "kernel_grads": kg.result(),
                     "bias_grads": bg.result()})
        ws.result()  # (the guards around the workspace)
    for a, name in zip(ins, ("x0", "kernels", "outputs", "hiddens", "out_grad")):
        a.assert_unchanged(name)
    _cross_check(runs[0], want, CROSS_BWD, what)
    for name in CROSS_BWD:
        _same_bits(runs[0][name], runs[1][name], f"{what} {name}, second call")


# widths -> NPL: 1, 63, 64 -> 1;  65, 128 -> 2;  129, 256 -> 4;  257 -> 8;  513 -> 16;
# 1025, 2048 -> 32;  2049, 4096 -> 64.  Layers 1 and 3 (2 from w = 2049 on: `outputs` stays small).
CROSS_W = [1, 63, 64, 65, 128, 129, 256, 257, 513, 1025, 2048, 2049, 4096]
# B = 3: 1021 of the backward's 1024 wavefronts own no row, their partial rows must be zeros (the
# workspace starts as NaN);  B = 1100: 76 wavefronts take a second row
CROSS = [(B, w, L) for w in CROSS_W for L in ((1, 2) if w >= 2049 else (1, 3)) for B in (3, 1100)]
# B = 2100: 52 wavefronts take a third row; one width per NPL
CROSS_3_ROWS = [(2100, w, 2 if w >= 2049 else 3) for w in (63, 65, 129, 257, 513, 1025, 2049)]
# layers * w = 7680: exactly 60 KiB, the last LDS shape;  7684, 8000, 8192: partial rows in the
# workspace (cross_v1_bwd_kernel<NPL, false>), with (B = 1100) and without a second row
CROSS_FORMS = [(B, w, L) for w, L in ((1920, 4), (1921, 4), (1000, 8), (4096, 2))
               for B in (3, 1100)]
# (all of them run under the host interpreter too: the backward's grid does not grow with B)


@pytest.mark.parametrize("B,w,L", list(dict.fromkeys(CROSS + CROSS_3_ROWS + CROSS_FORMS)))
def test_cross_v1_backward(B, w, L):
    _cross_backward(B, w, L)


# the forward at the same widths; B = 8200 > 8192 wavefronts: eight of them take a second row
@pytest.mark.parametrize("B,w,L", CROSS + _hw_only([(8200, 65, 2)]))
def test_cross_v1_forward(B, w, L):
    _cross_forward(B, w, L)


def test_cross_v1_every_tensor_one_element_into_its_allocation():
    """x0, kernels, biases, outputs, hiddens, out_grad, the gradients and the workspace all start 4
    bytes past a 16-byte boundary (NPL = 8, three layers, a second row per wavefront)"""
    _cross_forward(1100, 257, 3, mis=1)
    _cross_backward(1100, 257, 3, mis=1)


# ==================================================================================================
# 2. ReLU backward with bias, and the cross-v2 step
# ==================================================================================================
def _edge_words(dt):
    """+0, -0, the smallest positive subnormal, -1, and the smallest negative subnormal"""
    return 0x0000, 0x8000, 0x0001, (0xBC00 if dt == "f16" else 0xBF80), 0x8001


def _relu_case(rows, n, dt):
    """dy ~ N(0, 1); y = relu(N(0, 1)) with the edge values in the first and the last four columns
    of the first and the last row of every 128-row tile (dy = 1.5 there)"""
    rng = np.random.default_rng([rows, n, DT16.index(dt)])
    dy = _to16(rng.standard_normal((rows, n), dtype=np.float32), dt)
    y = _to16(np.maximum(rng.standard_normal((rows, n), dtype=np.float32), 0), dt)
    pz, nz, sub, neg, nsub = _edge_words(dt)
    at = sorted(set(range(0, rows, 128)) | set(range(127, rows, 128)) | {rows - 1})
    y[at, :4] = [pz, nz, sub, neg]
    y[at, -4:] = [sub, nsub, neg, nz]
    one_and_a_half = _to16(np.float32(1.5), dt)
    dy[at, :4] = one_and_a_half
    dy[at, -4:] = one_and_a_half
    # y > 0 on the raw words (no NaN): sign bit clear and not +0
    dz = np.where((y < 0x8000) & (y != 0), dy, np.uint16(0)).astype(np.uint16)
    assert dz[at[0], 2] == one_and_a_half and not dz[at[0], [0, 1, 3]].any()
    tiles = -(-rows // 128)
    z64 = _from16(dz, dt).astype(np.float64)
    partial = np.stack([z64[t * 128:(t + 1) * 128].sum(0) for t in range(tiles)])
    return dy, y, dz, partial, z64.sum(0)


# n: 8 -> cw 1, rg 256;  40 -> cw 5, rg 51, threads 255.. idle;  2048 -> cw 256, one pass;
# 2056 -> a second pass with ONE live column thread;  2400 -> a second pass of 44
# rows: 1 | 129: a second, one-row tile | 4225: 34 tiles > the column sum's 32 tile groups
RELU = [(rows, n) for n in (8, 40, 2048, 2056, 2400) for rows in (1, 129, 4225)]


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("rows,n", RELU)
def test_relu_bwd_bias(rows, n, dt):
    lib, check, s = _abi()
    dy_w, y_w, want_dz, want_partial, want_db = _relu_case(rows, n, dt)
    what = f"relu_bwd_bias rows={rows} n={n} {dt}"
    tiles = -(-rows // 128)
    assert lib.hctr_relu_bwd_bias_workspace_bytes(rows, n) == tiles * n * 4
    dy, y = _in16(dy_w), _in16(y_w)
    runs = []
    for entry in ("full", "full", "partials"):
        dz, db, ws = _out(rows, n, dt), _out(1, n, "f32"), _out(tiles, n, "f32")
        if entry == "full":
            check(lib.hctr_relu_bwd_bias(rows, n, dy.p, y.p, dz.p, db.p, ws.p, _code(dt), s))
        else:
            check(lib.hctr_relu_bwd_bias_partials(rows, n, dy.p, y.p, dz.p, ws.p, _code(dt), s))
        runs.append((_words(dz.result()), ws.result(), db.result()[0]))
    dy.assert_unchanged("dy")
    y.assert_unchanged("y")
    got_dz, got_partial, got_db = runs[0]
    _same_bits(got_dz, want_dz, what + " dz")
    # the bound of test_relu_bwd_bias_fused, for the column sums and for each tile's
    assert_close(got_db, want_db, 1e-5, 1e-4, what + " db")
    assert_close(got_partial, want_partial, 1e-5, 1e-4, what + " tile partials")
    _same_bits(runs[1][2], got_db, what + " db, second call")
    _same_bits(runs[1][1], got_partial, what + " tile partials, second call")
    _same_bits(runs[2][0], want_dz, what + " dz of _partials")
    _same_bits(runs[2][1], got_partial, what + " tile partials of _partials")
    assert np.isnan(runs[2][2]).all(), "hctr_relu_bwd_bias_partials has no db"


def _step_case(B, w, dt):
    """dy, x0, h, acc ~ N(0, 1) in the type; S0 = dY .* X0 and dX (+)= dY .* H in IEEE fp32: the
    product of two 16-bit values is exact in fp32, then one fp32 add and one rounding to the type
    (an FMA contracts nothing that rounds)"""
    rng = np.random.default_rng([B, w, DT16.index(dt), 2])
    dy, x0, h, acc = (_to16(rng.standard_normal((B, w), dtype=np.float32), dt) for _ in range(4))
    g, x, hf, a = (_from16(v, dt) for v in (dy, x0, h, acc))
    s0 = _to16(g * x, dt)
    gh = g * hf
    assert np.array_equal(gh.astype(np.float64), g.astype(np.float64) * hf.astype(np.float64))
    s64 = _from16(s0, dt).astype(np.float64)
    return (dy, x0, h, acc), s0, _to16(gh, dt), _to16(gh + a, dt), s64.sum(0), np.abs(s64).sum(0)


# (B, width, rows per tile): every value of cross_step_rows_per_tile; width 40: cw 5, rg 51;
# width 2056: two column blocks, the second with one live column thread
STEP = [(7, 8, 16), (40001, 8, 16), (70001, 8, 32), (131073, 8, 64), (262145, 8, 128),
        (131073, 40, 64), (300, 2056, 16)]


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("B,w,rpt", STEP)
def test_cross_v2_bwd_step(B, w, rpt, dt):
    lib, check, s = _abi()
    (dy_w, x0_w, h_w, acc_w), want_s0, want_first, want_acc, want_db, abs_db = _step_case(B, w, dt)
    what = f"cross_v2_bwd_step B={B} w={w} {dt}"
    tiles = lib.hctr_cross_v2_bwd_step_workspace_bytes(B, w) // (4 * w)
    assert tiles == -(-B // rpt), f"{what}: {tiles} tiles are not {rpt} rows per tile"
    ins = [_in16(v) for v in (dy_w, x0_w, h_w)]
    dbs = []
    for first in (1, 1, 0):
        acc, s0 = _out(B, w, dt), _out(B, w, dt)  # first: the accumulator is NaN and is not read
        if not first:
            acc.fill(acc_w.view(np.int16))
        db, ws = _out(1, w, "f32"), _out(tiles, w, "f32")
        check(lib.hctr_cross_v2_bwd_step(B, w, ins[0].p, ins[1].p, ins[2].p, acc.p, s0.p, db.p,
                                         ws.p, first, _code(dt), s))
        _same_bits(_words(s0.result()), want_s0, f"{what} first={first} s0")
        _same_bits(_words(acc.result()), want_first if first else want_acc,
                   f"{what} first={first} accumulator")
        ws.result()
        dbs.append(db.result()[0])
        # the bound of test_cross_v2_backward_step_equals_the_three_torch_passes
        assert np.abs(dbs[-1].astype(np.float64) - want_db).max() <= 1e-5 * abs_db.max() + 1e-6, \
            f"{what} first={first} db"
    for a, name in zip(ins, ("dy", "x0", "h")):
        a.assert_unchanged(name)
    _same_bits(dbs[1], dbs[0], what + " db, second call")
    _same_bits(dbs[2], dbs[0], what + " db, first = 0")


# ==================================================================================================
# 3. logit head
# ==================================================================================================
def _head_ref(x, w, b, y, scale):
    """z = x.w + b, the stable BCE and dz = (sigmoid(z) - y) scale, float64"""
    x, w, y = x.astype(np.float64), w.astype(np.float64), y.astype(np.float64)
    z = x @ w + float(b)
    e = np.exp(-np.abs(z))
    loss = (np.maximum(z, 0) - z * y + np.log1p(e)).mean()
    sig = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    dz = (sig - y) * scale
    return z, loss, dz, dz @ x, dz.sum(), dz[:, None] * w[None, :]


def _head_run(x, w, b, y, scale, dt, what):
    """hctr_logit_head with dx, again with dx = NULL, and hctr_logit_head_partials, checked against
    each other and for their guards -> (loss, dw, db, dx) of the first call"""
    lib, check, s = _abi()
    B, K = x.shape
    xi, wi, bi, yi = _in16(_to16(x, dt)), _in16(_to16(w, dt)), _in16(_to16(b, dt)), DevIn(y)
    assert lib.hctr_logit_head_workspace_bytes(K) == 1024 * (K + 2) * 4
    runs = []
    for entry in ("dx", "no dx", "partials"):
        dx, ws = _out(B, K, dt), _out(1024, K + 2, "f32")
        dw, db, loss = _out(1, K, "f32"), _out(1, 1, "f32"), _out(1, 1, "f32")
        if entry == "partials":
            check(lib.hctr_logit_head_partials(B, K, xi.p, wi.p, bi.p, yi.p, scale, dx.p, ws.p,
                                               _code(dt), s))
        else:
            check(lib.hctr_logit_head(B, K, xi.p, wi.p, bi.p, yi.p, scale,
                                      dx.p if entry == "dx" else None, dw.p, db.p, loss.p, ws.p,
                                      _code(dt), s))
        runs.append((loss.result()[0], dw.result()[0], db.result()[0], _words(dx.result()),
                     ws.result()))
    for a, name in zip((xi, wi, bi, yi), ("x", "w", "bias", "label")):
        a.assert_unchanged(name)
    for i, name in enumerate(("loss", "dw", "db")):
        _same_bits(runs[1][i], runs[0][i], f"{what} {name}, second call (dx = NULL)")
    assert (runs[1][3] == 0xFFFF).all(), what + ": dx = NULL"
    _same_bits(runs[1][4], runs[0][4], what + " block partials, second call")
    _same_bits(runs[2][3], runs[0][3], what + " dx of _partials")
    _same_bits(runs[2][4], runs[0][4], what + " block partials of _partials")
    blocks = lib.hctr_logit_head_blocks(B, K)
    assert not np.isnan(runs[0][4][:blocks]).any() and np.isnan(runs[0][4][blocks:]).all()
    return runs[0][0], runs[0][1], runs[0][2], _from16(runs[0][3], dt)


def _head_check(got, want, dt, what):
    """the bounds of test_logit_head_matches_torch"""
    loss, dw, db, dx = got
    _, want_loss, _, want_dw, want_db, want_dx = want
    assert np.isfinite(loss[0])
    assert abs(float(loss[0]) - want_loss) < 2e-6 * max(1.0, abs(want_loss)), \
        f"{what} loss {float(loss[0])!r} want {want_loss!r}"
    assert_close(dw, want_dw, 1e-4, 1e-7, what + " dw")
    assert abs(float(db[0]) - want_db) < 1e-6, f"{what} db {float(db[0])!r} want {want_db!r}"
    rtol = 2.0 ** -7 if dt == "bf16" else 2.0 ** -10  # one rounding of the 16-bit store
    atol = 1e-9 if dt == "bf16" else 6e-8             # (fp16: gradients this small are subnormal)
    assert_close(dx, want_dx, rtol, atol, what + " dx")


# (K, B, NSEG, blocks): a tail (B no multiple of 4 ROWS = 32, 16, 8, 4) at the first and the last K
# of every NSEG, and more than 1024 blocks for every NSEG
HEAD = [(4, 37, 1, 2), (256, 37, 1, 2), (260, 19, 2, 2), (512, 19, 2, 2), (516, 11, 4, 2),
        (1024, 11, 4, 2), (1028, 5, 8, 2), (2048, 5, 8, 2)]
HEAD += _hw_only([(4, 32801, 1, 1024), (260, 16401, 2, 1024), (516, 8201, 4, 1024),
                  (1028, 4101, 8, 1024)])


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("K,B,nseg,blocks", HEAD)
def test_logit_head(K, B, nseg, blocks, dt):
    lib, _, _ = _abi()
    assert lib.hctr_logit_head_blocks(B, K) == blocks
    assert min(8, 1 << (-(-K // 256) - 1).bit_length()) == nseg
    if blocks == 1024:
        assert B > 1024 * 4 * (8 // nseg), "no second sweep"
    rng = np.random.default_rng([K, B, DT16.index(dt)])
    x = _round16(rng.standard_normal((B, K), dtype=np.float32), dt)
    w = _round16(rng.standard_normal(K, dtype=np.float32) / np.sqrt(K), dt)
    b = _round16(np.float32([0.1]), dt)
    y = (rng.random(B) < 0.4).astype(np.float32)
    scale = 1.0 / B
    what = f"logit head K={K} B={B} {dt}"
    _head_check(_head_run(x, w, b, y, scale, dt, what), _head_ref(x, w, b[0], y, scale), dt, what)


@pytest.mark.parametrize("dt", DT16)
def test_logit_head_extreme_logits(dt):
    """w = 8 and x = t / 32 in all four columns: z = t + 0.1 for t = 0, +-20, +-60, +-100, +-200
    (beyond +-88.7 expf overflows or underflows in fp32), each with label 0 and label 1; the other
    rows are ordinary.  The loss stays finite and within the relative bound, |dz| <= scale"""
    B, K = 37, 4
    rng = np.random.default_rng([99, DT16.index(dt)])
    t = np.float32([0, 20, -20, 60, -60, 100, -100, 200, -200])
    x = _round16(0.1 * rng.standard_normal((B, K), dtype=np.float32), dt)
    x[:18] = np.repeat(t / 32, 2)[:, None]
    assert np.array_equal(x, _round16(x, dt))
    y = (rng.random(B) < 0.5).astype(np.float32)
    y[:18] = np.tile(np.float32([0, 1]), 9)
    w = np.full(K, 8, np.float32)
    b = _round16(np.float32([0.1]), dt)
    scale = 1.0 / B
    want = _head_ref(x, w, b[0], y, scale)
    assert np.abs(want[0][:18]).max() > 200 and np.abs(want[0][:2]).max() < 0.2
    what = f"logit head, extreme logits, {dt}"
    got = _head_run(x, w, b, y, scale, dt, what)
    _head_check(got, want, dt, what)
    # dx = round(dz w) and rounding is monotone: |dz| <= scale  =>  |dx| <= round(scale |w|)
    assert (np.abs(got[3]) <= _round16(np.float32(scale) * np.abs(w), dt)[None, :]).all(), \
        what + ": |dz| > scale"


# ==================================================================================================
# 4. skinny first layer
# ==================================================================================================
def _skinny_bounds(dz, x16):
    """test_skinny_first_layer_matches_torch's: 2e-6 (|dz|^T |x|) for dw, 2e-6 sum |dz| for db"""
    return 2e-6 * (np.abs(dz).T @ np.abs(x16)) + 1e-12, 2e-6 * np.abs(dz).sum(0) + 1e-12


# (B, K, N, R of the forward, blocks of the backward, why)
SKINNY = [(1025, 2, 8, 2, 5, "R = 2; matrix-core backward, rsets = 16, ragged last 16 rows"),
          (2049, 3, 4, 4, 256, "R = 4, odd batch; N % 8 != 0: vector-ALU backward"),
          (4099, 16, 512, 6, 256, "K = 16: vector-ALU backward, 3 rows into a second step")]
SKINNY += _hw_only([
    (16401, 13, 512, 18, 256, "matrix-core backward, rsets = 4: 17 rows into a second sweep"),
    (65537, 7, 128, 66, 256, "matrix-core backward, rsets = 16: 1 row into a second sweep"),
    (262145, 1, 4, 256, 256, "R at its cap of 256, 1025 blocks, the last one with one row")])


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("B,K,N,R,blocks,why", SKINNY)
def test_skinny_first_layer(B, K, N, R, blocks, why, dt, monkeypatch):
    lib, check, s = _abi()
    monkeypatch.delenv("HCTR_SKINNY_BWD", raising=False)
    assert min(256, (-(-B // 1024) + 1) // 2 * 2) == R, why
    what = f"skinny B={B} K={K} N={N} {dt}"
    rng = np.random.default_rng([B, K, N, DT16.index(dt)])
    x = rng.standard_normal((B, K), dtype=np.float32)
    w = _round16(rng.standard_normal((N, K), dtype=np.float32) / np.sqrt(K), dt)
    b = _round16(0.1 * rng.standard_normal(N, dtype=np.float32), dt)
    x16 = _round16(x, dt).astype(np.float64)  # (the kernels round x to the type on load)
    want_y = np.maximum(x16 @ w.astype(np.float64).T + b.astype(np.float64), 0)

    xi, wi, bi = DevIn(x), _in16(_to16(w, dt)), _in16(_to16(b, dt))
    y = _out(B, N, dt)
    check(lib.hctr_skinny_fc_fwd(B, K, N, xi.p, wi.p, bi.p, y.p, _code(dt), s))
    got_y = _words(y.result())
    # the bounds of test_skinny_first_layer_matches_torch: one rounding of the store, and the
    # rounded result itself equal to rounding the fp64 value except at rounding ties
    assert_close(_from16(got_y, dt), want_y, 2.0 ** -7 if dt == "bf16" else 2.0 ** -10, 1e-6,
                 what + " y")
    y_w = _to16(want_y.astype(np.float32), dt)
    assert (got_y != y_w).mean() < 1e-3, what + " y, rounded"

    # backward on the reference's y: dz = dy (y > 0), dw = dz^T x, db = column sums of dz
    dy_w = _to16(rng.standard_normal((B, N), dtype=np.float32) / B, dt)
    dz = np.where(_from16(y_w, dt) > 0, _from16(dy_w, dt), np.float32(0))
    dz64 = dz.astype(np.float64)
    want_dw, want_db = dz64.T @ x16, dz64.sum(0)
    bound_w, bound_b = _skinny_bounds(dz64, x16)
    if B in (16401, 65537):
        # the bound and the inputs, before the GPU is asked: a plain left-to-right fp32 sum of the
        # same terms (exact products of 16-bit values) stays inside it, the fp64 sums without the
        # last row do not
        x32 = x16.astype(np.float32)
        seq_w, seq_b = np.zeros((N, K), np.float32), np.zeros(N, np.float32)
        for r in range(B):
            seq_w += np.multiply.outer(dz[r], x32[r])
            seq_b += dz[r]
        assert (np.abs(seq_w - want_dw) <= bound_w).all() and \
            (np.abs(seq_b - want_db) <= bound_b).all(), what + ": fp32 in row order misses the bound"
        assert (np.abs(dz64[:-1].T @ x16[:-1] - want_dw) > bound_w).any() and \
            (np.abs(dz64[:-1].sum(0) - want_db) > bound_b).any(), what + ": a lost row passes"

    dyi, yi = _in16(dy_w), _in16(y_w)
    assert lib.hctr_skinny_fc_bwd_blocks(B, K, N, dyi.p, yi.p) == blocks, why
    assert lib.hctr_skinny_fc_bwd_workspace_bytes(N) == 256 * N * 17 * 4
    runs = []
    for entry in ("full", "full", "partials"):
        dw, db, ws = _out(N, K, "f32"), _out(1, N, "f32"), _out(256 * N, 17, "f32")
        if entry == "full":
            check(lib.hctr_skinny_fc_bwd(B, K, N, xi.p, dyi.p, yi.p, dw.p, db.p, ws.p, _code(dt), s))
        else:
            check(lib.hctr_skinny_fc_bwd_partials(B, K, N, xi.p, dyi.p, yi.p, ws.p, _code(dt), s))
        runs.append((dw.result(), db.result()[0], ws.result()))
    for a, name in zip((xi, wi, bi, dyi, yi), ("x", "w", "bias", "dy", "y")):
        a.assert_unchanged(name)
    got_dw, got_db, got_ws = runs[0]
    assert (np.abs(got_dw - want_dw) <= bound_w).all(), what + " dw"
    assert (np.abs(got_db - want_db) <= bound_b).all(), what + " db"
    _same_bits(runs[1][0], got_dw, what + " dw, second call")
    _same_bits(runs[1][1], got_db, what + " db, second call")
    # block partials [blocks][N][17]: K columns of dw, db in column 16 (the matrix-core form
    # leaves the columns between them as they were in LDS; nothing reads them)
    used = list(range(K)) + [16]
    assert not np.isnan(got_ws[:blocks * N, used]).any() and np.isnan(got_ws[blocks * N:]).all()
    _same_bits(runs[2][2][:, used], got_ws[:, used], what + " block partials of _partials")


# ==================================================================================================
# 5. SGD shadow and BCE
# ==================================================================================================
# n = 4: one thread;  4 * 256 * 4096 + 12: three threads take a second pass
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("n", [4] + _hw_only([4 * 256 * 4096 + 12]))
def test_sgd_shadow(n, dt):
    lib, check, s = _abi()
    rng = np.random.default_rng([n, DT16.index(dt)])
    w0 = rng.uniform(-0.1, 0.1, n).astype(np.float32)
    g0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    lr, gs = np.float32(0.0123), np.float32(0.77)  # (no powers of two: both products round)
    w, w16, g = _out(n // 4, 4, "f32").fill(w0), _out(n // 4, 4, dt), DevIn(g0)
    check(lib.hctr_sgd_shadow(n, float(lr), float(gs), w.p, g.p, w16.p, _code(dt), s))
    got = w.result().reshape(-1)
    g.assert_unchanged("g")
    step = float(lr) * float(gs) * g0.astype(np.float64)
    # one rounding of the result and two of lr * gs * g, contracted into an FMA or not
    bound = 2.0 ** -24 * np.abs(got.astype(np.float64)) + 2.0 ** -23 * np.abs(step)
    err = np.abs(got - (w0.astype(np.float64) - step))
    assert (err <= bound).all(), f"sgd_shadow n={n}: {(err > bound).sum()} masters off"
    _same_bits(_words(w16.result()).reshape(-1), _to16(got, dt), f"sgd_shadow n={n} {dt} copy")


def test_bce_loss_extreme_logits():
    """hctr_bce_loss, fp32: logits +-0, +-20, +-60, +-100, +-200 (and ordinary ones), each with
    label 0 and label 1, against float64 with the bounds of test_bce_loss_fused"""
    lib, check, s = _abi()
    t = np.float32([0.0, -0.0, 20, -20, 60, -60, 100, -100, 200, -200, 0.5, -3])
    x = np.repeat(t, 2)
    y = np.tile(np.float32([0, 1]), t.size)
    B = x.size
    scale = 0.5 / B
    z = x.astype(np.float64)
    e = np.exp(-np.abs(z))
    want_loss = (np.maximum(z, 0) - z * y + np.log1p(e)).mean()
    want_dx = (np.where(z >= 0, 1 / (1 + e), e / (1 + e)) - y) * scale
    assert lib.hctr_bce_loss_workspace_bytes() == 256 * 4
    xi, yi = DevIn(x), DevIn(y)
    runs = []
    for _ in range(2):
        dx, loss, ws = _out(B, 1, "f32"), _out(1, 1, "f32"), _out(256, 1, "f32")
        check(lib.hctr_bce_loss(B, xi.p, yi.p, scale, dx.p, loss.p, ws.p, _code("f32"), s))
        runs.append((loss.result()[0], dx.result().reshape(-1)))
        ws.result()
    xi.assert_unchanged("logit")
    yi.assert_unchanged("label")
    loss, dx = runs[0]
    assert np.isfinite(loss[0]) and abs(float(loss[0]) - want_loss) <= 1e-5 * max(1.0, want_loss)
    assert_close(dx, want_dx, 1e-6, 1e-6 / B, "bce dx")
    assert (np.abs(dx) <= np.float32(scale)).all()
    _same_bits(runs[1][0], loss, "bce loss, second call")
    _same_bits(runs[1][1], dx, "bce dx, second call")
