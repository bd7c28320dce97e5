"""Both attention kernel families (hugectr_amd/csrc/attention.hip, attention_tiled.hip), every
template instance and mask order, against the float64 restatement `_ref` and the tolerances `_tol`
of tests/test_mha_gpu.py, unchanged; inputs are N(0, 1) as there.

  A  the tiled entries called directly: every (element type, DT) instance at m = 33, n = 70 (one
     block of 128 rows whose second wavefront has one live row, two key tiles, the second of six
     keys), and m = n = 1;
  B  masks whose valid keys come LAST, so the tiled forward's running smallest penalty drops after
     keys were already accumulated under a larger one (left-padded, staircase), and masks whose
     values are neither 0 nor 1 (graded: finite penalty differences, rows whose best key is not at
     penalty 0), through both families;
  C  the first family's tile counts the older file leaves out: m > n, three key tiles, mp = 64 and
     96, dk = 32 and 48, B H past the grid with m > n;
  D  the same device inputs through both families' entries where both have a kernel;
  E  the tiled forward without statistics, gradients wanted for some inputs only, inputs that are
     views;
  F  two runs, equal bits, one masked case per family.

Direct calls hold q, k, v, mask and the top gradient in `DevIn` (unchanged afterwards) and out,
dq, dk, dv and the statistics in `DevOut` (no poison left inside, the guard behind untouched)."""
import functools

import numpy as np
import pytest

from test_mha_gpu import _lengths, _np64, _ref, _tol
from util import DevIn, DevOut, assert_close

pytestmark = pytest.mark.gpu

SHORT = {"float32": "f32", "float16": "f16", "bfloat16": "bf16"}
TYPES = ["float32", "float16", "bfloat16"]
NAMES = ("out", "dq", "dk", "dv")


# ---- masks, built on the host (float32 arrays of values exact in the element type) ----------------
def _left_padded(B, m, n):
    """key j valid iff j >= n - len_to[b], query i valid iff i >= m - len_from[b]"""
    len_to = np.array([(n, n // 2, 1, 0)[b % 4] for b in range(B)])
    len_from = np.array([(m, 1, m // 2, 0)[b % 4] for b in range(B)])
    kv = np.arange(n)[None, :] >= n - len_to[:, None]
    qv = np.arange(m)[None, :] >= m - len_from[:, None]
    return (qv[:, :, None] & kv[:, None, :])[:, None].astype(np.float32)


def _staircase(B, m, n):
    """row i is valid from key (i n) // m on: every row changes at its own key"""
    one = np.arange(n)[None, :] >= (np.arange(m)[:, None] * n) // m
    return np.broadcast_to(one[None, None], (B, 1, m, n)).astype(np.float32).copy()


def _graded(rng, dtype_name, B, m, n):
    """fp16 / fp32: 1 - g 2^-11, g uniform in {0, 1, 2, 3} (exact in both; penalties g 4.8828125,
    exact in fp32); bf16: 1 - g / 2, g uniform in {0, 1, 2}.  Every third row has no g = 0: there g
    is raised to at least 1, 2, 3 in turn (bf16: 1, 2), so the smallest penalty of such a row is
    each of the non-zero values, the largest included (a row of one common non-zero penalty).
    Two more kinds of row, of every nine one each:
      late (i % 9 = 1): the first min(40, n // 2) keys have g >= 2, so the row's smallest penalty
        arrives after keys were taken under a larger one, by a difference (9.765625) whose
        exp() does not vanish: the tiled forward rebases what it holds and keeps it;
      deep (i % 9 = 4): mask = -256 - 2 g, exact in the three types, penalties 2 570 000 + 20 000 g,
        exact in fp32.  The row's smallest penalty r cancels in float64; a kernel that takes
        q.k / sqrt(d) - penalty without r rounds the logit to 0.25 there.  (With masks inside
        [0, 1] that rounding is at most 5e-4 of a logit, which `_tol` does not see: both families
        subtract the row's maximum before exp(), so r matters through rounding alone.)"""
    top, step = (2, 0.5) if dtype_name == "bfloat16" else (3, 2.0 ** -11)
    g = rng.integers(0, top + 1, (B, 1, m, n))
    third = np.arange(2, m, 3)
    floor = 1 + (third // 3) % top
    g[:, :, third] = np.maximum(g[:, :, third], floor[None, None, :, None])
    late, deep, head = np.arange(1, m, 9), np.arange(4, m, 9), min(40, n // 2)
    g[:, :, late, :head] = np.maximum(g[:, :, late, :head], min(2, top))
    mask = (1.0 - g * step).astype(np.float32)
    mask[:, :, deep] = (-256.0 - 2.0 * g[:, :, deep]).astype(np.float32)
    # what the mask is for: several values in a row, rows whose best key is not at penalty 0, ...
    shallow = np.delete(mask, deep, axis=2)
    assert len(np.unique(shallow)) == top + 1
    best = shallow.max(-1)
    assert (best < 1).any() and (best == 1).any() and len(np.unique(best)) == top + 1
    assert (shallow.max(-1) > shallow.min(-1)).any()
    # ... rows whose best key comes after `head` worse ones, rows far below 0 with several values
    assert len(late) and (mask[:, :, late, :head].max(-1) < mask[:, :, late, head:].max(-1)).all()
    assert len(deep) and (mask[:, :, deep].max(-1) <= -256).all()
    assert (mask[:, :, deep].max(-1) > mask[:, :, deep].min(-1)).all()
    return mask


def _assert_late_start(mask, lead):
    """the input self-check of the left-padded and staircase masks: a row whose first `lead` keys
    are all masked and that has a later valid key, and one such row whose first valid key is no
    multiple of 32 (the change falls inside a tile)"""
    valid = mask[:, 0] > 0
    first = valid.argmax(-1)
    late = valid.any(-1) & (first >= lead)
    assert late.any(), f"no row with {lead} leading masked keys and a later valid one"
    assert (late & (first % 32 != 0)).any(), "no such row that changes inside a tile"


def _mask(kind, rng, dtype_name, B, m, n, lead):
    if kind is None:
        return None
    if kind == "graded":
        return _graded(rng, dtype_name, B, m, n)
    mask = _left_padded(B, m, n) if kind == "left" else _staircase(B, m, n)
    _assert_late_start(mask, lead)
    return mask


# ---- inputs and the reference ---------------------------------------------------------------------
def _inputs(dtype_name, B, H, m, n, d, kind, lead=64):
    """host tensors of the element type (q, k, v, top, mask or None) and the float64 expectation
    from them"""
    import torch
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng([B, H, m, n, d, len(dtype_name)])
    q, k, v, top = (torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(dt)
                    for s in ((B, m, H * d), (B, n, H * d), (B, n, H * d), (B, m, H * d)))
    mask = _mask(kind, rng, dtype_name, B, m, n, lead)
    if mask is not None:
        exact = mask.astype(np.float64)
        mask = torch.from_numpy(mask).to(dt)
        assert np.array_equal(_np64(mask), exact), "a mask value is not exact in the element type"
    want = _ref(_np64(q), _np64(k), _np64(v), None if mask is None else _np64(mask), _np64(top), H)
    return (q, k, v, top, mask), want


def _check(got, want, dtype_name, what):
    for g, w, name in zip(got, want, NAMES):
        g = np.asarray(g, dtype=np.float64).reshape(w.shape)
        assert np.isfinite(g).all(), f"{what} {name}: not finite"
        assert_close(g, w, *_tol(dtype_name, name != "out"), f"{what} {name}")


def _layer(host, H, need=(True, True, True)):
    """forward and backward through MultiHeadAttentionLayer: [out, dq, dk, dv] as device tensors
    (None where no gradient was asked for)"""
    import torch
    import hugectr_amd as ha
    q, k, v, top, mask = (None if t is None else t.cuda() for t in host)
    for t, on in zip((q, k, v), need):
        t.requires_grad_(on)
    out = ha.MultiHeadAttentionLayer(H)(q, k, v, mask)
    out.backward(top)
    torch.cuda.synchronize()
    return [out.detach(), q.grad, k.grad, v.grad]


# ---- the C entries, called directly ---------------------------------------------------------------
def _dev_in(t):
    import torch
    return DevIn(t.numpy() if t.dtype == torch.float32 else t.view(torch.int16).numpy())


def _filled(o, what):
    res = o.result()  # (asserts the guard behind and the words in front)
    assert not np.isnan(res).any(), f"{what}: poison left inside the output"
    return res


def _direct(tiled, dtype_name, B, H, m, n, d, host):
    """hctr_mha[_tiled]_fwd, then _bwd, on DevIn / DevOut buffers: [out, dq, dk, dv] as fp32 rows"""
    import torch
    from hugectr_amd import _lib
    L, code, dt = _lib.lib, getattr(_lib, SHORT[dtype_name].upper()), SHORT[dtype_name]
    ins = [None if t is None else _dev_in(t) for t in host]
    q, k, v, top, mask = ins
    mp = None if mask is None else mask.p
    out, dq = DevOut(B * m, H * d, dt), DevOut(B * m, H * d, dt)
    dk, dv = DevOut(B * n, H * d, dt), DevOut(B * n, H * d, dt)
    what = f"{'tiled' if tiled else 'first'} {dtype_name} B={B} H={H} m={m} n={n} d={d}"
    if tiled:
        stats = DevOut(B * H * m, 4, "f32")
        _lib.check(L.hctr_mha_tiled_fwd(B, H, m, n, d, q.p, k.p, v.p, mp, out.p, stats.p, code,
                                        _lib.stream_ptr()))
        torch.cuda.synchronize()
        st = stats.result()
        assert np.isfinite(st[:, :3]).all(), f"{what}: statistics 0 .. 2 after the forward"
    else:
        _lib.check(L.hctr_mha_fwd(B, H, m, n, d, q.p, k.p, v.p, mp, out.p, code, _lib.stream_ptr()))
        torch.cuda.synchronize()
    o = _filled(out, what + " out").copy()
    if tiled:
        _lib.check(L.hctr_mha_tiled_bwd(B, H, m, n, d, q.p, k.p, v.p, mp, out.p, stats.p, top.p,
                                        dq.p, dk.p, dv.p, code, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert np.isfinite(_filled(stats, what + " stats")).all(), f"{what}: statistics, backward"
    else:
        _lib.check(L.hctr_mha_bwd(B, H, m, n, d, q.p, k.p, v.p, mp, top.p, dq.p, dk.p, dv.p, code,
                                  _lib.stream_ptr()))
        torch.cuda.synchronize()
    for t, name in zip(ins, ("q", "k", "v", "top", "mask")):
        if t is not None:
            t.assert_unchanged(f"{what} {name}")
    assert np.array_equal(out.result(), o), f"{what}: the backward changed the forward's output"
    return [o] + [_filled(x, f"{what} {name}") for x, name in zip((dq, dk, dv), NAMES[1:])]


# ==== A. the tiled family, every (element type, DT) =================================================
# d = 24: DT 1, ksd 2 with half a k step of padding; 40: DT 2, ksd 3; 64: DT 2 full; 88: DT 3;
# 104: DT 4, ksd 7.  With the two samples of the issue's shape the left-padded mask has keys 35 ..
# 69 valid in sample 1, so the lead that can be asked of the input is one 32-key sub-tile
@pytest.mark.parametrize("d", [24, 40, 64, 88, 104])
@pytest.mark.parametrize("dtype_name", TYPES)
def test_tiled_every_instance(dtype_name, d):
    B, H, m, n = 2, 2, 33, 70
    host, want = _inputs(dtype_name, B, H, m, n, d, "left", lead=32)
    _check(_direct(True, dtype_name, B, H, m, n, d, host), want, dtype_name,
           f"tiled direct {dtype_name} d={d}")


@pytest.mark.parametrize("dtype_name", TYPES)
def test_tiled_one_query_one_key(dtype_name):
    """the smallest shape: P = 1 / (1 + 1e-6), one live lane pair in the workgroup"""
    host, want = _inputs(dtype_name, 1, 1, 1, 1, 8, None)
    assert np.allclose(want[0], _np64(host[2]) / (1 + 1e-6), rtol=1e-12, atol=0)
    _check(_direct(True, dtype_name, 1, 1, 1, 1, 8, host), want, dtype_name,
           f"tiled direct {dtype_name} 1 x 1 x 8")


# ==== B. mask order, both families, through the layer ===============================================
# each mask meets each element type once over the three tiled shapes
TILED_SHAPES = [(130, 200, 32), (40, 129, 64), (129, 70, 128)]
TILED_MASKS = [(TILED_SHAPES[s], kind, TYPES[(s + i) % 3])
               for s in range(3) for i, kind in enumerate(("left", "staircase", "graded"))]


@pytest.mark.parametrize("shape,kind,dtype_name", TILED_MASKS)
def test_mask_order_tiled(shape, kind, dtype_name):
    m, n, d = shape
    host, want = _inputs(dtype_name, 4, 2, m, n, d, kind)
    _check([_np64(t) for t in _layer(host, 2)], want, dtype_name,
           f"tiled {dtype_name} {shape} {kind}")


# the first family holds a whole row of scores: nothing is rebased there, so the lead asked of the
# input is half the keys (n = 40 has no 64)
FIRST_MASKS = [((m, n, d), "left", t) for m, n, d in ((40, 97, 24), (97, 40, 56)) for t in TYPES] + [
    ((40, 97, 24), "staircase", "float16"), ((97, 40, 56), "staircase", "bfloat16"),
    ((40, 97, 24), "graded", "float32"), ((97, 40, 56), "graded", "float16"),
    ((40, 97, 24), "graded", "bfloat16")]


@pytest.mark.parametrize("shape,kind,dtype_name", FIRST_MASKS)
def test_mask_order_first_family(shape, kind, dtype_name):
    m, n, d = shape
    host, want = _inputs(dtype_name, 4, 2, m, n, d, kind, lead=n // 2)
    _check([_np64(t) for t in _layer(host, 2)], want, dtype_name,
           f"first {dtype_name} {shape} {kind}")


# ==== C. the first family's untouched tile counts ===================================================
# (m, n, d, masked, types): mp = 64 / 96 / 128, nt = 1 .. 4, dk = 16 / 32 / 48 / 64; every type meets
# m > n -- (33, 10), (97, 33), (127, 3), (128, 1) -- and nt = 3 -- n = 65 and 96
FIRST_TILES = [(33, 10, 24, False, ["float32"]), (64, 65, 32, True, TYPES), (65, 96, 40, False, TYPES),
               (96, 97, 48, True, ["bfloat16"]), (97, 33, 56, True, ["float16"]),
               (127, 3, 16, False, ["bfloat16"]), (128, 1, 8, True, ["float32", "float16"])]


def _len_case(dtype_name, B, H, m, n, d, masked):
    """a "len" mask of sequence_mask (valid keys first), or none, through the layer"""
    import torch
    import hugectr_amd as ha
    host, _ = _inputs(dtype_name, B, H, m, n, d, None)
    q, k, v, top, _ = host
    mask = None
    if masked:
        dt = getattr(torch, dtype_name)
        lf, lt = _lengths(B, m), _lengths(B, n)[::-1].copy()
        mask = ha.sequence_mask(torch.from_numpy(lf).cuda().to(dt), torch.from_numpy(lt).cuda().to(dt),
                                m, n).cpu()
    want = _ref(_np64(q), _np64(k), _np64(v), None if mask is None else _np64(mask), _np64(top), H)
    _check([_np64(t) for t in _layer((q, k, v, top, mask), H)], want, dtype_name,
           f"first {dtype_name} B={B} H={H} m={m} n={n} d={d} len mask={masked}")


@pytest.mark.parametrize("m,n,d,masked,dtype_name",
                         [(m, n, d, k, t) for m, n, d, k, ts in FIRST_TILES for t in ts])
def test_first_family_tile_counts(m, n, d, masked, dtype_name):
    _len_case(dtype_name, 3, 2, m, n, d, masked)


def test_first_family_grid_stride_with_more_queries_than_keys():
    """B H = 2100 heads over the 2048 workgroups of mha_grid: the second pass of the stride loop
    starts from LDS tiles the first one filled, with m > n"""
    _len_case("bfloat16", 700, 3, 5, 3, 8, True)


# ==== D. both families on the same inputs ===========================================================
@pytest.mark.parametrize("d,dtype_name", [(24, "float16"), (40, "bfloat16"), (64, "float32")])
def test_both_families_against_the_reference(d, dtype_name):
    """each judged against the reference; their roundings differ, so not against each other"""
    B, H, m, n = 4, 2, 33, 70
    host, want = _inputs(dtype_name, B, H, m, n, d, "left")
    for tiled in (False, True):
        _check(_direct(tiled, dtype_name, B, H, m, n, d, host), want, dtype_name,
               f"{'tiled' if tiled else 'first'} direct {dtype_name} d={d}")


# ==== E. no statistics, partial gradients, views ====================================================
@functools.lru_cache(maxsize=None)
def _e_case(dtype_name, m, n, d):
    return _inputs(dtype_name, 4, 2, m, n, d, "left")


@pytest.mark.parametrize("dtype_name,m,n,d", [("float16", 130, 70, 72), ("float32", 1, 200, 128)])
def test_tiled_forward_without_statistics(dtype_name, m, n, d):
    """no input needs a gradient: layers.py passes stats = nullptr; the same bits as with them"""
    import torch
    import hugectr_amd as ha
    host, want = _e_case(dtype_name, m, n, d)
    q, k, v, _, mask = (t.cuda() for t in host)
    with torch.no_grad():
        plain = ha.MultiHeadAttentionLayer(2)(q, k, v, mask)
    assert not plain.requires_grad
    with_stats = ha.MultiHeadAttentionLayer(2)(q.clone().requires_grad_(True), k, v, mask)
    assert with_stats.requires_grad
    torch.cuda.synchronize()
    assert torch.equal(plain, with_stats.detach())
    assert_close(_np64(plain), want[0], *_tol(dtype_name, False), f"{dtype_name} no-grad out")


def test_tiled_partial_gradients():
    """a gradient wanted for q alone, for k and v alone: the bits of the run that wants all three"""
    import torch
    host, want = _e_case("float16", 130, 70, 72)
    full = _layer(host, 2)
    _check([_np64(t) for t in full], want, "float16", "all three gradients")
    for need in ((True, False, False), (False, True, True)):
        got = _layer(host, 2, need)
        assert torch.equal(got[0], full[0])
        for g, f, on, name in zip(got[1:], full[1:], need, NAMES[1:]):
            assert (g is not None) == on, f"{need}: {name}"
            if on:
                assert torch.equal(g, f), f"{need}: {name} differs from the full run's"


def test_tiled_views_as_inputs():
    """q a column slice of a wider tensor, v a transpose(0, 1) view of [n, B, H d], the top
    gradient one expanded row"""
    import torch
    import hugectr_amd as ha
    (q, k, v, _, mask), _ = _e_case("float16", 130, 70, 72)
    B, m, hd = q.shape
    row = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 1, hd), dtype=np.float32))
    row = row.to(q.dtype)
    want = _ref(_np64(q), _np64(k), _np64(v), _np64(mask), _np64(row.expand(B, m, hd)), 2)
    wide = torch.zeros((B, m, hd + 16), dtype=q.dtype)
    wide[:, :, 8:8 + hd] = q
    wide = wide.cuda().requires_grad_(True)
    vt = v.transpose(0, 1).contiguous().cuda().requires_grad_(True)
    kd = k.cuda().requires_grad_(True)
    qv, vv, top = wide[:, :, 8:8 + hd], vt.transpose(0, 1), row.cuda().expand(B, m, hd)
    assert not qv.is_contiguous() and not vv.is_contiguous() and not top.is_contiguous()
    out = ha.MultiHeadAttentionLayer(2)(qv, kd, vv, mask.cuda())
    out.backward(top)
    torch.cuda.synchronize()
    side = torch.cat([wide.grad[:, :, :8], wide.grad[:, :, 8 + hd:]], -1)
    assert not bool(side.any()), "a gradient outside q's columns of the wider tensor"
    got = [out.detach(), wide.grad[:, :, 8:8 + hd], kd.grad, vt.grad.transpose(0, 1)]
    _check([_np64(t) for t in got], want, "float16", "views")


# ==== F. two runs, equal bits =======================================================================
@pytest.mark.parametrize("m,n,d,dtype_name", [(97, 40, 56, "float32"), (129, 70, 128, "bfloat16")])
def test_two_runs_equal_bits(m, n, d, dtype_name):
    host, _ = _inputs(dtype_name, 4, 2, m, n, d, "graded")
    a, b = _layer(host, 2), _layer(host, 2)
    for x, y, name in zip(a, b, NAMES):
        assert np.array_equal(_np64(x), _np64(y)), f"{dtype_name} {(m, n, d)}: {name} differs"
