"""Dense Ftrl through the C ABI: hctr_ftrl_shadow (flat buffers, the twin of hctr_sgd_shadow) and
hctr_ftrl_segments (one launch over parameter tensors that do not live in one buffer).

The oracle is the formulas of ftrl_update_kernel (R/HugeCTR/src/optimizers/ftrl_optimizer.cu:28-43,
92-93) in fp64 numpy, on gradients and initial weights rounded to fp32 first.  Tolerance: rel 1e-5 /
abs 1e-6 on w, z and n -- what a float32 restatement of the same formulas keeps against the fp64
oracle on these inputs, and what the static tables' Ftrl parity uses (tests/test_ebc_gpu.py).  An
element may be left out of the w comparison only where the oracle's | |z'| - lambda1 | <=
1e-5 * (1 + |z'|) (the branch of the update is decided there by the last bit), and at most 0.1 % of
the elements of a step may be."""
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("HCTR_EMU") == "1"
LR, BETA, L1, L2, GS = 0.05, 0.9, 0.1, 0.1, 1.0
EPS = float(np.finfo(np.float32).eps)
STEPS = 3
GUARD = 64
SENTINEL = 12345.0
F16, BF16 = 1, 2
TORCH16 = {F16: torch.float16, BF16: torch.bfloat16}


def _one_pass_elems():
    """elements one pass of the flat launch's grid covers, read from the launch code"""
    src = open(os.path.join(ROOT, "hugectr_amd", "csrc", "dense_ops.hip")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
    body = src[src.index("int hctr_ftrl_shadow("):]
    cap = int(re.search(r"grid_for\(n / 4, kBlock, (\d+)\)", body).group(1))
    return 4 * cap * block


def _sizes():
    big = _one_pass_elems() + 4  # the grid-stride loop takes a second pass
    # (the host interpreter steps through every thread: the second pass is left to the hardware)
    return [4, 65540] if EMU else [4, 65540, big]


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """w0 ~ U(-0.1, 0.1), gradients 0.1 * N(0, 1) per step, the first 64 of step 1 exactly 0"""
    rng = np.random.default_rng(1234 + n % 1000)
    w0 = rng.uniform(-0.1, 0.1, n).astype(np.float32)
    g = (0.1 * rng.standard_normal((STEPS, n))).astype(np.float32)
    g[0, :min(64, n)] = 0.0
    w0.setflags(write=False)
    g.setflags(write=False)
    return w0, g


def oracle_step(w, z, n, g, lr=LR, beta=BETA, l1=L1, l2=L2, gs=GS):
    """one Ftrl step in fp64; returns (w', z', n')"""
    w, z, n, g = (np.asarray(a, np.float64) for a in (w, z, n, g))
    g = g * gs
    n1 = n + g * g
    z1 = z + g + (np.sqrt(n + EPS) - np.sqrt(n1 + EPS)) * w / lr
    sgn = np.where(np.signbit(z1), -1.0, 1.0)
    w1 = np.where(np.abs(z1) > l1, (l1 * sgn - z1) / (np.sqrt(n1 + EPS) / lr + l2 + beta / lr), 0.0)
    return w1, z1, n1


@functools.lru_cache(maxsize=None)
def _oracle(n):
    """[(w, z, n)] after each of the three steps, computed once per size"""
    w0, g = _inputs(n)
    w, z, acc = w0.astype(np.float64), np.zeros(n), np.zeros(n)
    out = []
    for s in range(STEPS):
        w, z, acc = oracle_step(w, z, acc, g[s])
        out.append((w, z, acc))
    return out


def close(got, want):
    return np.abs(got.astype(np.float64) - want) <= 1e-6 + 1e-5 * np.abs(want)


def check_step(got_w, got_z, got_n, want, what, l1=L1):
    w, z, n = want
    assert close(got_z, z).all(), f"{what}: z"
    assert close(got_n, n).all(), f"{what}: n"
    edge = np.abs(np.abs(z) - l1) <= 1e-5 * (1 + np.abs(z))
    assert edge.mean() <= 1e-3, f"{what}: {edge.mean():.2%} of the elements on the branch edge"
    assert close(got_w, w)[~edge].all(), f"{what}: w"
    return float((w == 0).mean())


def _guarded(values, dtype=torch.float32, guard=GUARD):
    """a device buffer with a sentinel-filled guard behind it: (whole, payload view)"""
    n = len(values)
    whole = torch.full((n + guard,), SENTINEL, dtype=dtype, device="cuda")
    whole[:n] = torch.tensor(np.asarray(values)).cuda().to(dtype)
    return whole, whole[:n]


def _guard_ok(whole, n):
    return bool((whole[n:] == SENTINEL).all())


def _flat_call(n, w, z, acc, g, w16, dtype, lr=LR):
    from hugectr_amd._lib import lib, ptr, stream_ptr
    return lib.hctr_ftrl_shadow(n, lr, BETA, L1, L2, GS, ptr(w), ptr(z), ptr(acc), ptr(g),
                                ptr(w16), dtype, stream_ptr())


@pytest.mark.parametrize("shadow", [0, F16, BF16], ids=["no_copy", "fp16", "bf16"])
@pytest.mark.parametrize("n", _sizes())
def test_flat_entry_follows_the_oracle(n, shadow):
    """three consecutive steps of hctr_ftrl_shadow against the fp64 oracle; the 16-bit copy is the
    round-to-nearest conversion of the fp32 result bit for bit; the zero-gradient elements of step
    1 become exactly 0 with z = n = 0; nothing behind the buffers is written"""
    from hugectr_amd._lib import check
    w0, g = _inputs(n)
    want = _oracle(n)
    ww, w = _guarded(w0)
    zw, z = _guarded(np.zeros(n, np.float32))
    nw, acc = _guarded(np.zeros(n, np.float32))
    w16w = w16 = None
    if shadow:
        w16w, w16 = _guarded(np.zeros(n, np.float32), TORCH16[shadow], 2 * GUARD)
    nz = min(64, n)
    for s in range(STEPS):
        gw, gs = _guarded(g[s])
        check(_flat_call(n, w, z, acc, gs, w16, shadow))
        torch.cuda.synchronize()
        zero = check_step(w.cpu().numpy(), z.cpu().numpy(), acc.cpu().numpy(), want[s],
                          f"n={n} step {s + 1}")
        if n > 1000:  # both branches of the update are exercised
            assert 0.1 < zero < 0.9, zero
        assert torch.equal(gw, torch.cat([torch.tensor(g[s]).cuda(),
                                          gw.new_full((GUARD,), SENTINEL)]))  # g is only read
        if shadow:
            assert torch.equal(w16, w.to(TORCH16[shadow]))
        if s == 0:
            assert (w[:nz] == 0).all() and (z[:nz] == 0).all() and (acc[:nz] == 0).all()
            assert not torch.signbit(w[:nz]).any()
            if shadow:
                assert (w16[:nz] == 0).all()
        assert _guard_ok(ww, n) and _guard_ok(zw, n) and _guard_ok(nw, n)
        if shadow:
            assert _guard_ok(w16w, n)


def _seg_layout(counts):
    offs, tot = [], 0
    for c in counts:
        offs.append(tot)
        tot += (c + 3) // 4 * 4
    return offs, tot


def test_segmented_entry_equals_the_flat_entry_bit_for_bit():
    """hctr_ftrl_segments on parameter tensors of their own (counts 1, 3, 4, 5, 1023, 4097 and one
    whose storage is not 16-byte aligned: the scalar form) against hctr_ftrl_shadow on the same
    data laid into one buffer: the same ftrl_apply, so w, z and n are equal bit for bit over three
    steps.  Guards behind every buffer and the padding between the segments keep their sentinel."""
    from hugectr_amd._lib import FTRL_SEG_BLOCK_ELEMS, check, lib, ptr, stream_ptr
    counts = [1, 3, 4, 5, 1023, 4097, 37]
    offs, tot = _seg_layout(counts)
    rng = np.random.default_rng(7)
    w0 = rng.uniform(-0.1, 0.1, tot).astype(np.float32)
    grads = (0.1 * rng.standard_normal((STEPS, tot))).astype(np.float32)
    grads[0, :2] = 0.0
    pad = np.ones(tot, bool)
    for o, c in zip(offs, counts):
        pad[o:o + c] = False
    w0[pad] = 0.0
    grads[:, pad] = 0.0
    # the flat run (padding: w = g = z = n = 0 stays 0)
    fw, fz, fn = (torch.from_numpy(a).cuda() for a in (w0, np.zeros(tot, np.float32),
                                                        np.zeros(tot, np.float32)))
    # the segmented run: every w its own tensor (the last one a 4-byte aligned view), sentinel in
    # the padding of the flat g / z / n
    segs_w = []
    for i, (o, c) in enumerate(zip(offs, counts)):
        lead = 1 if i == len(counts) - 1 else 0
        whole = torch.full((lead + c + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        whole[lead:lead + c] = torch.from_numpy(w0[o:o + c]).cuda()
        segs_w.append((whole, whole[lead:lead + c], lead))
    assert segs_w[-1][1].data_ptr() % 16 == 4 and segs_w[0][1].data_ptr() % 16 == 0
    padt = torch.from_numpy(pad).cuda()

    def flat_with_sentinel(values):
        whole, v = _guarded(values)
        v[padt] = SENTINEL
        return whole, v
    szw, sz = flat_with_sentinel(np.zeros(tot, np.float32))
    snw, sn = flat_with_sentinel(np.zeros(tot, np.float32))
    table = np.zeros((len(counts), 4), np.int64)
    block0 = 0
    for r, (o, c) in enumerate(zip(offs, counts)):
        table[r] = (segs_w[r][1].data_ptr(), o, c, block0)
        block0 += (c + FTRL_SEG_BLOCK_ELEMS - 1) // FTRL_SEG_BLOCK_ELEMS
    assert block0 == 1 + 1 + 1 + 1 + 1 + 5 + 1  # 4097 elements: more than one block
    table = torch.from_numpy(table).cuda()
    for s in range(STEPS):
        fg = torch.from_numpy(grads[s]).cuda()
        check(_flat_call(tot, fw, fz, fn, fg, None, 0))
        sgw, sg = flat_with_sentinel(grads[s])
        g_before = sgw.clone()
        check(lib.hctr_ftrl_segments(ptr(table), len(counts), block0, LR, BETA, L1, L2, GS,
                                     ptr(sz), ptr(sn), ptr(sg), stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(sgw, g_before)
        for (whole, w, lead), o, c in zip(segs_w, offs, counts):
            assert torch.equal(w, fw[o:o + c]), f"step {s + 1}: w of the segment of {c}"
            assert torch.equal(sz[o:o + c], fz[o:o + c]) and torch.equal(sn[o:o + c], fn[o:o + c])
            assert (whole[:lead] == SENTINEL).all() and (whole[lead + c:] == SENTINEL).all()
        assert (sz[padt] == SENTINEL).all() and (sn[padt] == SENTINEL).all()
        assert _guard_ok(szw, tot) and _guard_ok(snw, tot)
        assert (fw[padt] == 0).all() and (fz[padt] == 0).all() and (fn[padt] == 0).all()
    assert (fw != torch.from_numpy(w0).cuda()).any()


def test_bad_arguments_come_back_as_errors_and_touch_nothing():
    from hugectr_amd import _lib
    from hugectr_amd._lib import lib, ptr, stream_ptr
    n = 64
    w0, g0 = _inputs(65540)
    bufs = [torch.from_numpy(np.array(a[:n])).cuda()
            for a in (w0, g0[1], g0[2], g0[1])]
    w, z, acc, g = bufs
    w16 = torch.full((n,), 3.0, dtype=torch.float16, device="cuda")
    before = [b.clone() for b in bufs + [w16]]
    assert _flat_call(n - 2, w, z, acc, g, w16, F16) == -1 and "multiple of 4" in _lib.last_error()
    assert _flat_call(n, None, z, acc, g, w16, F16) == -1 and "null" in _lib.last_error()
    assert _flat_call(n, w, z, acc, g, w16, 7) == -1 and "dtype" in _lib.last_error()
    assert _flat_call(n, w, z, acc, g, w16, F16, lr=0.0) == -1 and "lr" in _lib.last_error()
    assert _flat_call(n, w[1:], z, acc, g, w16, F16) == -1 and "aligned" in _lib.last_error()
    table = torch.tensor([[w.data_ptr(), 0, n, 0]], dtype=torch.int64, device="cuda")
    assert lib.hctr_ftrl_segments(None, 1, 1, LR, BETA, L1, L2, GS, ptr(z), ptr(acc), ptr(g),
                                  stream_ptr()) == -1 and "null" in _lib.last_error()
    assert lib.hctr_ftrl_segments(ptr(table), -1, 1, LR, BETA, L1, L2, GS, ptr(z), ptr(acc),
                                  ptr(g), stream_ptr()) == -1
    assert lib.hctr_ftrl_segments(ptr(table), 1, 1, LR, BETA, -1.0, L2, GS, ptr(z), ptr(acc),
                                  ptr(g), stream_ptr()) == -1 and "lambda1" in _lib.last_error()
    torch.cuda.synchronize()
    for b, a in zip(bufs + [w16], before):
        assert torch.equal(b, a)
