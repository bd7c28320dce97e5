"""hctr_gemm_nt16 (hugectr_amd/csrc/cross_gemm.hip) called through the C ABI, every compiled variant:
the staging ring at depth 2 / 3 / 4 (HCTR_GEMM_STAGES; counted vmcnt waits, the launches above
64 KB of dynamic LDS), tile heights 64 / 128 and the 256 x 256 kernel (HCTR_GEMM_BM), both branches
of the block -> tile maps, the three epilogues, leading dimensions wider than the rows, and the
host contract.

Two checks per run:
  * fp64, element by element.  acc = A . Bt^T and S = |A| . |Bt|^T in numpy float64 from the same
    16-bit operands; eps_T = 2^-11 (fp16) / 2^-8 (bf16) is one rounding to nearest, K * 2^-24 * S the
    standard bound of a length-K fp32 accumulation:
        plain     |C - acc|       <= eps_T |acc|     + K 2^-24 S
        residual  |C - (acc + R)| <= eps_T |acc + R| + (K + 1) 2^-24 (S + |R|)
        cross, H  |H - (acc + b)| <= eps_T |acc + b| + (K + 1) 2^-24 (S + |b|)
        cross, C  |C - (XL + X0 H)| <= eps_T |XL + X0 H| + 2^-22 (|XL| + |X0 H|)   (H = the device's)
    A max-norm comparison would let a wrong small element hide behind the largest one.
  * bits.  Every variant issues the same MFMA sequence per output element (the same K order, the
    same 32 x 32 x 16 steps), so for one set of operands all of them give identical bits; each run
    is compared with torch.equal against tile height 64 at ring depth 2.  A tile multiplied before
    its DMA has landed shows here exactly; an error all variants share shows in the fp64 check.

The operands lie in buffers of 3 more rows than the matrix and `pad` more columns than a row
(lda = K + pad, ldb = K + 2 pad, ldc = N + pad).  The inputs' surplus holds NaN (reading it as data
poisons the result), C and H are pre-filled with 7.0: after a call everything outside
[0, M) x [0, N) still holds 7.0, and the inputs hold the bits they held before."""
import functools
import os
import zlib
from ctypes import c_void_p

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
SENTINEL = 7.0
EPS = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
DTYPES = ("float16", "bfloat16")
PLAIN, CROSS, RESIDUAL = 0, 1, 2
EPI_NAME = {PLAIN: "plain", CROSS: "cross", RESIDUAL: "residual"}


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16)


class _Problem:
    """one set of operands on the host and on the device, and its float64 products"""

    def __init__(self, dtype_name, M, N, K, pad):
        import torch
        from hugectr_amd import _lib
        self.dtype_name, self.M, self.N, self.K, self.pad = dtype_name, M, N, K, pad
        self.dt = getattr(torch, dtype_name)
        self.code = _lib.F16 if dtype_name == "float16" else _lib.BF16
        self.lda, self.ldb, self.ldc = K + pad, K + 2 * pad, N + pad
        g = torch.Generator()
        g.manual_seed(zlib.crc32(repr((dtype_name, M, N, K, pad)).encode()))

        def operand(rows, cols, ld):
            t = torch.full((rows + 3, ld), float("nan"))
            t[:rows, :cols] = torch.randn((rows, cols), generator=g) * 0.5
            return t

        a, bt = operand(M, K, self.lda), operand(N, K, self.ldb)
        bt[:N, 0] += torch.arange(N) * 0.01  # (asymmetric in n: a swapped fragment layout cannot pass)
        x0, xl = operand(M, N, self.ldc), operand(M, N, self.ldc)
        bias = torch.randn((N,), generator=g) * 0.5
        self.host = {k: v.to(self.dt) for k, v in dict(a=a, bt=bt, x0=x0, xl=xl, bias=bias).items()}
        self.dev = {k: v.cuda() for k, v in self.host.items()}
        self._base = {}

    @functools.cached_property
    def ref(self):
        M, N, K = self.M, self.N, self.K
        f64 = {k: v.double().numpy() for k, v in self.host.items()}
        A, B = f64["a"][:M, :K], f64["bt"][:N, :K]
        return dict(acc=A @ B.T, S=np.abs(A) @ np.abs(B).T, x0=f64["x0"][:M, :N], xl=f64["xl"][:M, :N],
                    bias=f64["bias"][None, :])

    def what(self, epi, bm, depth):
        return (f"{self.dtype_name} M={self.M} N={self.N} K={self.K} pad={self.pad} {EPI_NAME[epi]} "
                f"BM={bm} depth={depth}")


@functools.lru_cache(maxsize=6)
def _problem(dtype_name, M, N, K, pad):
    return _Problem(dtype_name, M, N, K, pad)


def _set_variant(mp, bm, depth):
    for name, val in (("HCTR_GEMM_BM", bm), ("HCTR_GEMM_STAGES", depth)):
        if val is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(val))


def _only_sentinel(t, what):
    bad = (t.float() != SENTINEL).nonzero()
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} elements outside [0, M) x [0, N) were written, the "
                               f"first at (row {int(bad[0, 0])}, col {int(bad[0, 1])})")


def _run(mp, p, epi, bm=None, depth=None):
    """one call of the kernel variant (bm, depth; None = no env): the harness checks (nothing
    outside [0, M) x [0, N) written, inputs untouched), then (C, H) [M, N] on the host"""
    import torch
    from hugectr_amd import _lib
    _set_variant(mp, bm, depth)
    what = p.what(epi, bm, depth)
    d = p.dev
    c = torch.full((p.M + 3, p.ldc), SENTINEL, dtype=p.dt, device="cuda")
    h = torch.full((p.M + 3, p.ldc), SENTINEL, dtype=p.dt, device="cuda") if epi == CROSS else None
    _lib.check(_lib.lib.hctr_gemm_nt16(
        p.M, p.N, p.K, _lib.ptr(d["a"]), p.lda, _lib.ptr(d["bt"]), p.ldb, _lib.ptr(c), p.ldc, epi,
        _lib.ptr(d["bias"]) if epi == CROSS else None, _lib.ptr(d["x0"]) if epi == CROSS else None,
        _lib.ptr(d["xl"]) if epi != PLAIN else None, _lib.ptr(h), p.code, _lib.stream_ptr()))
    torch.cuda.synchronize()
    out = []
    for name, t in (("C", c), ("H", h)):
        if t is None:
            out.append(None)
            continue
        t = t.cpu()
        out.append(t[:p.M, :p.N].clone())
        t[:p.M, :p.N] = SENTINEL
        _only_sentinel(t, f"{what}: {name}")
    for name, t in d.items():
        assert torch.equal(_bits(t.cpu()), _bits(p.host[name])), f"{what}: input {name} was changed"
    return out[0], out[1]


def _within(got, want, tol, what):
    err = np.abs(got.double().numpy() - want)
    bad = ~(err <= tol)  # (a NaN is beyond every bound)
    if bad.any():
        over = np.where(np.isnan(err), np.inf, err - tol)
        r, c = np.unravel_index(int(np.argmax(over)), over.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond the bound; worst "
                             f"|err| {err[r, c]:.4e} against {tol[r, c]:.4e} at (row {r}, col {c}), "
                             f"got {float(got[r, c])!r}, want {want[r, c]!r}")


def _check_fp64(p, epi, c, h, what):
    r, eps, u = p.ref, EPS[p.dtype_name], 2.0 ** -24
    acc, S, K = r["acc"], r["S"], p.K
    if epi == PLAIN:
        _within(c, acc, eps * np.abs(acc) + K * u * S, what + ": C")
    elif epi == RESIDUAL:
        want = acc + r["xl"]
        _within(c, want, eps * np.abs(want) + (K + 1) * u * (S + np.abs(r["xl"])), what + ": C")
    else:
        want = acc + r["bias"]
        _within(h, want, eps * np.abs(want) + (K + 1) * u * (S + np.abs(r["bias"])), what + ": H")
        # C is computed from the ROUNDED H, as the unfused passes do
        prod = r["x0"] * h.double().numpy()
        want = r["xl"] + prod
        _within(c, want, eps * np.abs(want) + 2.0 ** -22 * (np.abs(r["xl"]) + np.abs(prod)), what + ": C")


def _base(mp, p, epi):
    """tile height 64, ring depth 2 on these operands (run and compared with fp64 once)"""
    if epi not in p._base:
        c, h = _run(mp, p, epi, 64, 2)
        _check_fp64(p, epi, c, h, p.what(epi, 64, 2))
        p._base[epi] = (c, h)
    return p._base[epi]


def _same_bits(got, want, what):
    import torch
    for name, g, w in zip(("C", "H"), got, want):
        if w is None:
            assert g is None
            continue
        if not torch.equal(_bits(g), _bits(w)):
            diff = (_bits(g) != _bits(w)).nonzero()
            r, c = int(diff[0, 0]), int(diff[0, 1])
            raise AssertionError(f"{what}: {name} differs in {diff.shape[0]} of {w.numel()} elements, the first "
                                 f"at (row {r}, col {c}): {float(g[r, c])!r} against {float(w[r, c])!r}")


def _variant(mp, p, epi, bm, depth, base_too=True):
    """run a variant, compare with fp64 and with the bits of (64, 2)"""
    what = p.what(epi, bm, depth)
    base = _base(mp, p, epi) if base_too else None
    got = _run(mp, p, epi, bm, depth)
    _check_fp64(p, epi, got[0], got[1], what)
    if base is not None:
        _same_bits(got, base, what + " against BM=64 depth=2")
    return got


# ---- 1. ring depth x tile height x K x epilogue ----------------------------------------------------
def _ring_cases():
    cases, n = [], 0
    for K in (64, 128, 192, 320):  # KT = 1, 2, 3, 5: fewer tiles than buffers, a full ring, a wrapped one
        for bm, M in ((64, 70), (128, 130)):
            for depth in (2, 3, 4):
                for epi in (PLAIN, CROSS, RESIDUAL):
                    n += 1
                    for dtype_name in (DTYPES if K in (64, 320) else (DTYPES[n % 2],)):
                        cases.append(pytest.param(dtype_name, M, K, bm, depth, epi,
                                                  id=f"{dtype_name}-K{K}-bm{bm}-d{depth}-{EPI_NAME[epi]}"))
    return cases


@pytest.mark.parametrize("dtype_name,M,K,bm,depth,epi", _ring_cases())
def test_ring_depth_tile_height_k_epilogue(monkeypatch, dtype_name, M, K, bm, depth, epi):
    """every <BM, epilogue, STAGES> template at KT = 1, 2, 3 and 5, M two rows (BM 128) / six rows
    (BM 64) into a second row panel, padded leading dimensions.  The launcher builds no depth 4
    at BM = 128: asking for it gives depth 3."""
    p = _problem(dtype_name, M, 128, K, 8)
    got = _variant(monkeypatch, p, epi, bm, depth)
    if bm == 128 and depth == 4:
        _same_bits(got, _run(monkeypatch, p, epi, 128, 3), p.what(epi, bm, depth) + " against depth=3")


# ---- 2. the two production K ---------------------------------------------------------------------
@pytest.mark.parametrize("bm,depth", [(64, 2), (64, 3), (64, 4), (128, 2), (128, 3), (128, 4), (256, None)])
@pytest.mark.parametrize("K", [512, 3456])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_long_k(monkeypatch, dtype_name, K, bm, depth):
    """KT = 8 and 54: the ring wraps many times (and the 256-row kernel's two buffers alternate);
    plain and cross"""
    if EMU and K == 3456:
        pytest.skip("the host interpreter needs minutes for K = 3456")
    p = _problem(dtype_name, 300, 256, K, 0)
    for epi in (PLAIN,) if bm == 256 else (PLAIN, CROSS):
        _variant(monkeypatch, p, epi, bm, depth)


# ---- 3. block -> tile map of the 64 / 128-row kernel, XCD branch -------------------------------------
@pytest.mark.parametrize("bm,M,epis", [
    (64, 8 * 64 - 5, (PLAIN, CROSS, RESIDUAL)), (64, 16 * 64 - 1, (PLAIN,)),
    (128, 8 * 128 - 5, (PLAIN, CROSS, RESIDUAL)), (128, 16 * 128 - 1, (PLAIN,))])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_xcd_map_small_kernel(monkeypatch, dtype_name, bm, M, epis):
    """tiles_m = 8 and 16 with tiles_n = 2: block b -> panel (b / 8 / tiles_n) * 8 + b % 8.  Every
    row panel holds other random rows, so a permuted panel cannot pass; the other tile height and
    the 256-row kernel walk the same operands in other orders and must give the same bits."""
    p = _problem(dtype_name, M, 256, 64, 8)
    for epi in epis:
        got = _variant(monkeypatch, p, epi, bm, None)
        other = _run(monkeypatch, p, epi, 192 - bm, None)
        _same_bits(other, got, p.what(epi, 192 - bm, None) + f" against BM={bm}")
    big = _run(monkeypatch, p, PLAIN, 256, None)
    _same_bits(big, _base(monkeypatch, p, PLAIN), p.what(PLAIN, 256, None) + " against BM=64 depth=2")


# ---- 4. the 256 x 256 kernel -------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("M,N,K", [(2045, 512, 64), (4093, 256, 128),   # tiles_m = 8, 16: XCD branch
                                   (300, 256, 320), (513, 512, 192)])   # row-major branch
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_big_kernel(monkeypatch, dtype_name, M, N, K, pad):
    """HCTR_GEMM_BM=256: both branches of its block -> tile map; the last tile's M ends inside the
    first epilogue pass (300, and 513: one row), so the second stores nothing, or three rows before
    the end of the second (2045, 4093); KT = 1, 2, 3, 5 on the two buffers"""
    p = _problem(dtype_name, M, N, K, pad)
    _variant(monkeypatch, p, PLAIN, 256, None)


@pytest.mark.skipif(EMU, reason="2 GFLOP on the host interpreter")
def test_big_kernel_chosen_by_the_rule(monkeypatch):
    """no env: 129 x 2 tiles of 256 x 256 >= 256, so the plain product goes to the 256-row kernel
    (tiles_m = 129: row-major branch, one row in the last tile); the same bits as 128-row tiles"""
    p = _Problem("float16", 256 * 128 + 1, 512, 64, 8)
    got = _variant(monkeypatch, p, PLAIN, None, None, base_too=False)
    _same_bits(_run(monkeypatch, p, PLAIN, 128, None), got, p.what(PLAIN, 128, None) + " against no env")


# ---- 5. layers.gemm_nt16 on row-strided views ------------------------------------------------------------
@pytest.mark.parametrize("epi", [PLAIN, CROSS, RESIDUAL])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_layer_call_on_row_strided_views(dtype_name, epi):
    """gemm_nt16 forwards a.stride(0) / bt.stride(0) as lda / ldb: the result on views of wider
    buffers is the result on contiguous copies, bit for bit"""
    import torch
    from hugectr_amd.layers import gemm_nt16
    dt = getattr(torch, dtype_name)
    M, N, K = 200, 128, 192
    wide = (torch.randn((M, K + 8), device="cuda") * 0.5).to(dt)
    widew = (torch.randn((N, K + 24), device="cuda") * 0.5).to(dt)
    a, bt = wide[:, :K], widew[:, :K]
    assert not a.is_contiguous() and not bt.is_contiguous() and a.data_ptr() % 16 == 0
    bias = (torch.randn((N,), device="cuda") * 0.5).to(dt) if epi == CROSS else None
    x0 = (torch.randn((M, N), device="cuda") * 0.5).to(dt) if epi == CROSS else None
    xl = (torch.randn((M, N), device="cuda") * 0.5).to(dt) if epi != PLAIN else None
    on_views = gemm_nt16(a, bt, epi, bias, x0, xl)
    packed = gemm_nt16(a.contiguous(), bt.contiguous(), epi, bias, x0, xl)
    torch.cuda.synchronize()
    if epi != CROSS:
        on_views, packed = (on_views,), (packed,)
    for v, c in zip(on_views, packed):
        assert v.shape == (M, N) and torch.equal(_bits(v.cpu()), _bits(c.cpu()))


# ---- 6. the host contract --------------------------------------------------------------------------------
_CONTRACT = [
    ("n192", dict(n=192), "N % 128"),
    ("k96", dict(k=96), "K % 64"),
    ("lda_k_plus_4", dict(lda=68), "leading dimensions"),
    ("ldc_below_n", dict(ldc=120), "leading dimensions"),
    ("a_offset_2_bytes", dict(a_offset=2), "16-byte aligned"),
    ("cross_without_h", dict(epi=CROSS, h=False), "cross epilogue operands"),
    ("residual_without_xl", dict(epi=RESIDUAL, xl=False), "residual operand"),
    ("dtype_fp32", dict(dtype="F32"), "16-bit types only"),
    ("epilogue_3", dict(epi=3), "gemm_nt16: epilogue$"),
]


@pytest.mark.parametrize("change,message", [pytest.param(c, m, id=i) for i, c, m in _CONTRACT])
def test_host_contract_rejects(change, message):
    """what the launcher cannot run is refused with an error (never launched, never adjusted), and
    C and H keep their 7.0"""
    import torch
    from hugectr_amd import _lib
    arg = dict(m=70, n=128, k=64, lda=128, ldb=128, ldc=264, epi=CROSS, a_offset=0, h=True, xl=True,
               dtype="F16")
    arg.update(change)
    dt = torch.float16
    a = torch.ones((80, 128), dtype=dt, device="cuda")
    bt = torch.ones((256, 128), dtype=dt, device="cuda")
    x0, xl = (torch.ones((80, 264), dtype=dt, device="cuda") for _ in range(2))
    bias = torch.ones((256,), dtype=dt, device="cuda")
    c, h = (torch.full((80, 264), SENTINEL, dtype=dt, device="cuda") for _ in range(2))
    rc = _lib.lib.hctr_gemm_nt16(
        arg["m"], arg["n"], arg["k"], c_void_p(a.data_ptr() + arg["a_offset"]), arg["lda"], _lib.ptr(bt),
        arg["ldb"], _lib.ptr(c), arg["ldc"], arg["epi"], _lib.ptr(bias), _lib.ptr(x0),
        _lib.ptr(xl) if arg["xl"] else None, _lib.ptr(h) if arg["h"] else None, getattr(_lib, arg["dtype"]),
        _lib.stream_ptr())
    assert rc != 0
    with pytest.raises(_lib.HugeCTRAmdError, match=message):
        _lib.check(rc)
    torch.cuda.synchronize()
    _only_sentinel(c.cpu(), "C")
    _only_sentinel(h.cpu(), "H")


def test_host_contract_accepts_the_unchanged_call(monkeypatch):
    """(the call the rejections above are one change away from is a legal one)"""
    import torch
    from hugectr_amd import _lib
    dt = torch.float16
    a = torch.ones((80, 128), dtype=dt, device="cuda")
    bt = torch.ones((256, 128), dtype=dt, device="cuda")
    x0, xl = (torch.ones((80, 264), dtype=dt, device="cuda") for _ in range(2))
    bias = torch.ones((256,), dtype=dt, device="cuda")
    c, h = (torch.full((80, 264), SENTINEL, dtype=dt, device="cuda") for _ in range(2))
    _set_variant(monkeypatch, None, None)
    _lib.check(_lib.lib.hctr_gemm_nt16(70, 128, 64, _lib.ptr(a), 128, _lib.ptr(bt), 128, _lib.ptr(c), 264, CROSS,
                                       _lib.ptr(bias), _lib.ptr(x0), _lib.ptr(xl), _lib.ptr(h), _lib.F16,
                                       _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((h[:70, :128] == 65.0).all()) and bool((c[:70, :128] == 66.0).all())  # 64 + 1; 1 + 1 * 65
    c[:70, :128] = SENTINEL
    h[:70, :128] = SENTINEL
    _only_sentinel(c.cpu(), "C")
    _only_sentinel(h.cpu(), "H")


def test_host_contract_m_zero():
    """m = 0 is a legal empty product: OK with null pointers, nothing launched"""
    from hugectr_amd import _lib
    for epi in (PLAIN, CROSS, RESIDUAL):
        assert _lib.lib.hctr_gemm_nt16(0, 128, 64, None, 64, None, 64, None, 128, epi, None, None, None, None,
                                       _lib.F16, _lib.stream_ptr()) == 0


# ---- 7. the tile-height rule without env -----------------------------------------------------------------
@pytest.mark.parametrize("M,bm,epi", [(8192, 64, CROSS), (16384, 128, PLAIN)])
def test_tile_rule_without_env(monkeypatch, M, bm, epi):
    """N = 512: M = 8192 is 256 tiles of 128 rows (< 512: 64-row tiles, tiles_m = 128), M = 16384 is
    512 (128-row tiles, tiles_m = 128); both take the XCD branch with tiles_n = 4.  No env against
    the forced tile height."""
    p = _Problem("bfloat16" if epi == CROSS else "float16", M, 512, 64, 8)
    got = _variant(monkeypatch, p, epi, None, None, base_too=False)
    _same_bits(_run(monkeypatch, p, epi, bm, None), got, p.what(epi, bm, None) + " against no env")
