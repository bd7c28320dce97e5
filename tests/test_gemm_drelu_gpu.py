"""hctr_gemm_nt16_drelu (hugectr_amd/csrc/cross_gemm.hip) called through the C ABI: the data-gradient
GEMM with the ReLU mask of the layer below and that layer's bias partials in its epilogue, every
compiled variant -- tile heights 64 / 128 and the 256 x 256 kernel (HCTR_GEMM_BM), ring depths 2 and
3 (HCTR_GEMM_STAGES), both 16-bit types, ldc = n and n + 8.

Exact case.  A and Bt hold integers in [-2, 2], so |acc| <= 4 K and every fp32 partial sum is exact
in any order (a tile's column sum stays below 2^24); y mixes positive, negative, +0, -0, NaN and the
smallest positive subnormal.  Bit for bit:
  1. dz = hctr_relu_bwd_bias_partials applied to hctr_gemm_nt16 (plain epilogue) on the same inputs;
  2. dz = the float64 product rounded once to the 16-bit type, masked (masked lanes hold +0);
  3. the partial rows, finished through hctr_dense_grad_finish (COLSUM) and added here in tile
     order, = the float64 column sums of the stored dz.
The inputs keep their bits, the poison around dz and around the partial rows stays (util.DevOut: 64
rows behind the output; the columns n .. ldc of every row too), and a second run gives the same bits.

Real-valued case (normal inputs, K = 320): |dz - exact| <= K 2^-24 sum_k |a_k b_k| + ulp16(exact) --
the products are exact in fp32, so this is the accumulation error plus one rounding -- masked lanes
exactly 0, everything finite first (a leaked poison fails the case)."""
import functools
import math
import os

import numpy as np
import pytest

from util import DevOut

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
DTYPES = ("f16", "bf16")
MS = (1, 65, 129, 257) if EMU else (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 1025)
NS = (128, 256) if EMU else (128, 256, 384)
KS = (64, 128) if EMU else (64, 128, 320)
M_XCD_BIG = None if EMU else 8 * 256 - 7  # tiles_m = 8 of the 256 x 256 kernel: its XCD block map
MMAX = max(MS) if EMU else M_XCD_BIG
COLSUM = 1


def _tdt(dt):
    import torch
    return torch.float16 if dt == "f16" else torch.bfloat16


def _code(dt):
    from hugectr_amd import _lib
    return _lib.F16 if dt == "f16" else _lib.BF16


def _variants(N):
    """(tile height, ring depth): the 256 x 256 kernel has one ring, and needs N % 256 == 0"""
    v = [(64, 2), (64, 3), (128, 2), (128, 3)]
    return v + [(256, None)] if N % 256 == 0 else v


def _set_variant(mp, bm, depth):
    for name, val in (("HCTR_GEMM_BM", bm), ("HCTR_GEMM_STAGES", depth)):
        if val is None:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(val))


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16)


def _y_mix(gen, rows, cols, tdt):
    """positive, negative, +0, -0, NaN and the smallest positive subnormal, as bit patterns"""
    import torch
    one, neg, half = (torch.tensor([v], dtype=tdt).view(torch.int16).item() for v in (1.0, -3.0, 0.5))
    pats = torch.tensor([one, neg, 0, -32768, 0x7E00 if tdt == torch.float16 else 0x7FC0, 1, half, neg],
                        dtype=torch.int16)
    return pats[torch.randint(0, len(pats), (rows, cols), generator=gen)].view(tdt)


class _Problem:
    """operands for (dtype, N, K) at MMAX rows -- a smaller M takes the first M rows -- and what the
    unfused pair and float64 make of them"""

    def __init__(self, dt, N, K, real):
        import torch
        from hugectr_amd._lib import check, lib, ptr, stream_ptr
        self.dt, self.N, self.K, self.tdt, self.code = dt, N, K, _tdt(dt), _code(dt)
        gen = torch.Generator().manual_seed(N * 1000 + K + (7 if real else 0))
        if real:
            a = torch.randn((MMAX, K), generator=gen) * 0.5
            bt = torch.randn((N, K), generator=gen) * 0.5
            y = torch.randn((MMAX, N), generator=gen).to(self.tdt)
        else:
            a = torch.randint(-2, 3, (MMAX, K), generator=gen).float()
            bt = torch.randint(-2, 3, (N, K), generator=gen).float()
            y = _y_mix(gen, MMAX, N, self.tdt)
        bt[:, 0] += torch.arange(N) % 2  # (asymmetric in n: still an integer in [-2, 3])
        ypad = torch.full((MMAX, N + 8), float("nan"), dtype=self.tdt)  # y as dz lies: [m][ldc]
        ypad[:, :N] = y
        self.host = dict(a=a.to(self.tdt), bt=bt.to(self.tdt), y=y, ypad=ypad)
        self.dev = {k: v.cuda() for k, v in self.host.items()}
        A, B = self.host["a"].double(), self.host["bt"].double()
        self.acc = (A @ B.t()).cuda()
        self.S = (A.abs() @ B.abs().t()).cuda()
        self.keep = (self.host["y"].double() > 0).cuda()  # (a NaN compares false: masked)
        self.want = torch.where(self.keep, self.acc.to(self.tdt), torch.zeros((), dtype=self.tdt, device="cuda"))
        # the unfused pair at MMAX rows, the launcher's own choice of variant
        d = self.dev
        dy = torch.empty((MMAX, N), dtype=self.tdt, device="cuda")
        check(lib.hctr_gemm_nt16(MMAX, N, K, ptr(d["a"]), K, ptr(d["bt"]), K, ptr(dy), N, 0, None, None,
                                 None, None, self.code, stream_ptr()))
        ws = torch.empty(lib.hctr_relu_bwd_bias_workspace_bytes(MMAX, N) // 4, dtype=torch.float32,
                         device="cuda")
        self.pair = torch.empty_like(dy)
        check(lib.hctr_relu_bwd_bias_partials(MMAX, N, ptr(dy), ptr(d["y"]), ptr(self.pair), ptr(ws),
                                              self.code, stream_ptr()))
        torch.cuda.synchronize()

    def assert_inputs_unchanged(self, what):
        import torch
        for name, t in self.dev.items():
            assert torch.equal(_bits(t.cpu()), _bits(self.host[name])), f"{what}: input {name} was changed"


@functools.lru_cache(maxsize=2)
def _problem(dt, N, K, real=False):
    return _Problem(dt, N, K, real)


def _finish_colsum(partials, tiles, n):
    """the partial rows through hctr_dense_grad_finish (one COLSUM segment) -> fp32 [n]"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    g = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    w = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    w16 = torch.zeros(n + 8, dtype=torch.float16, device="cuda")
    t = np.zeros((1, 16), dtype=np.int64)
    t[0, :13] = (COLSUM, partials.data_ptr(), tiles, n, 0, 0, g.data_ptr(), w.data_ptr(), w16.data_ptr(),
                 4, 0, 0, 0)
    table = torch.from_numpy(t).cuda()
    check(lib.hctr_dense_grad_finish(ptr(table), 1, lib.hctr_dense_seg_blocks(COLSUM, n), 0, 0.0, 1.0,
                                     None, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isnan(g[:4]).all() and torch.isnan(g[4 + n:]).all()
    return g[4:4 + n]


def _run(mp, p, M, ldc, bm, depth):
    """one fused call of variant (bm, depth) on the first M rows: (dz bits [M, N] int16 on the
    device, partial rows fp32 [tiles, N] on the device, tiles); the guards and the inputs checked"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    _set_variant(mp, bm, depth)
    what = f"{p.dt} M={M} N={p.N} K={p.K} ldc={ldc} BM={bm} depth={depth}"
    tiles = lib.hctr_gemm_nt16_drelu_tiles(M, p.N)
    assert tiles == (M + bm - 1) // bm, f"{what}: {tiles} partial rows for tiles of {bm} rows"
    dz = DevOut(M, ldc, p.dt, int_bits=True)
    part = DevOut(tiles, p.N, "f32", int_bits=True)
    d = p.dev
    y = d["y"] if ldc == p.N else d["ypad"]
    assert y.shape[1] == ldc
    check(lib.hctr_gemm_nt16_drelu(M, p.N, p.K, ptr(d["a"]), p.K, ptr(d["bt"]), p.K, ptr(y), dz.p,
                                   ldc, part.p, p.code, stream_ptr()))
    torch.cuda.synchronize()
    dz.result()    # (asserts the poison around the rows)
    part.result()
    rows = dz.t[:M * ldc].view(M, ldc)
    assert bool((rows[:, p.N:] == -1).all()), f"{what}: columns past n were written"
    return rows[:, :p.N], part.t[:tiles * p.N].view(torch.float32).view(tiles, p.N), tiles, what


def _exact_case(mp, p, M, ldc, bm, depth):
    import torch
    dz, part, tiles, what = _run(mp, p, M, ldc, bm, depth)
    assert torch.equal(dz, _bits(p.pair[:M])), f"{what}: dz differs from plain GEMM + relu_bwd_bias"
    assert torch.equal(dz, _bits(p.want[:M])), f"{what}: dz differs from the float64 product, masked"
    stored = dz.contiguous().view(p.tdt).double()
    sums = stored.sum(0)
    assert bool(torch.isfinite(part).all()), f"{what}: a partial row was not written"
    finished = _finish_colsum(part, tiles, p.N)
    assert torch.equal(finished.double(), sums), f"{what}: finished column sums"
    host = np.zeros(p.N, dtype=np.float32)
    for row in part.cpu().numpy():  # (tile order)
        host = host + row
    assert np.array_equal(host.astype(np.float64), sums.cpu().numpy()), f"{what}: partial rows"
    # the rows of each tile on their own: a row counted in the wrong tile shows here
    tile_sums = torch.stack([stored[t * bm:(t + 1) * bm].sum(0) for t in range(tiles)])
    assert torch.equal(part.double(), tile_sums), f"{what}: a tile's partial row"
    if ldc != p.N:  # (once per M and variant)
        dz2, part2, _, _ = _run(mp, p, M, ldc, bm, depth)
        assert torch.equal(dz2, dz) and torch.equal(part2.view(torch.int32), part.view(torch.int32)), \
            f"{what}: a second run gave other bits"
    p.assert_inputs_unchanged(what)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dt", DTYPES)
def test_exact_every_m_tile_height_ring_depth_and_ldc(monkeypatch, dt, N, K):
    """M 1 .. 1025 around every tile edge (1024: tiles_m % 8 == 0 at BM = 128, the XCD block map;
    1025: the row-major one), N = 384 never on the 256 x 256 kernel, KT = 1, 2 and 5"""
    p = _problem(dt, N, K)
    for M in MS:
        for ldc in (N, N + 8):
            for bm, depth in _variants(N):
                _exact_case(monkeypatch, p, M, ldc, bm, depth)
    if N % 256 == 0 and M_XCD_BIG is not None:
        _exact_case(monkeypatch, p, M_XCD_BIG, N + 8, 256, None)


def _ulp16(x, dt):
    """the spacing of the 16-bit type at |x| (its subnormal spacing below the smallest normal)"""
    mant, emin = (10, -14) if dt == "f16" else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** emin)))
    return 2.0 ** (e - mant)


@pytest.mark.parametrize("bm,depth", [(64, 3), (128, 2), (256, None)])
@pytest.mark.parametrize("dt", DTYPES)
def test_real_valued_within_accumulation_error_and_one_rounding(monkeypatch, dt, bm, depth):
    import torch
    N, K, M = 256, 320, 129 if EMU else 257
    p = _problem(dt, N, K, True)
    dz, part, tiles, what = _run(monkeypatch, p, M, N + 8, bm, depth)
    got = dz.contiguous().view(p.tdt).double().cpu().numpy()
    assert np.isfinite(got).all(), f"{what}: dz is not finite"
    assert bool(torch.isfinite(part).all()), f"{what}: a partial row is not finite"
    keep = p.keep[:M].cpu().numpy()
    acc, S = p.acc[:M].cpu().numpy(), p.S[:M].cpu().numpy()
    assert (got[~keep] == 0).all(), f"{what}: a masked lane is not 0"
    err = np.abs(got - acc)[keep]
    tol = (K * 2.0 ** -24 * S + _ulp16(acc, dt))[keep]
    assert (err <= tol).all(), f"{what}: worst excess {float((err - tol).max()):.3e}"
    sums = torch.from_numpy(got).sum(0)
    finished = _finish_colsum(part, tiles, N).double().cpu()
    # fp32 sums of at most 257 stored values each <= max |dz|: M 2^-24 sum |dz| bounds any order
    bound = M * 2.0 ** -24 * torch.from_numpy(np.abs(got)).sum(0) + 1e-30
    assert bool(((finished - sums).abs() <= bound).all()), f"{what}: finished column sums"


def test_host_contract(monkeypatch):
    """what hctr_gemm_nt16 refuses is refused here, before anything is launched"""
    _set_variant(monkeypatch, None, None)
    import torch
    from hugectr_amd import _lib
    L = _lib.lib
    t = torch.zeros((64, 128), dtype=torch.float16, device="cuda")
    ws = torch.zeros(128, dtype=torch.float32, device="cuda")
    P, sp = _lib.ptr, _lib.stream_ptr()
    assert L.hctr_gemm_nt16_drelu(64, 192, 64, P(t), 64, P(t), 64, P(t), P(t), 192, P(ws), _lib.F16, sp) != 0
    assert "N % 128" in _lib.last_error()
    assert L.hctr_gemm_nt16_drelu(64, 128, 96, P(t), 96, P(t), 96, P(t), P(t), 128, P(ws), _lib.F16, sp) != 0
    assert "K % 64" in _lib.last_error()
    assert L.hctr_gemm_nt16_drelu(64, 128, 64, P(t), 64, P(t), 64, None, P(t), 128, P(ws), _lib.F16, sp) != 0
    assert L.hctr_gemm_nt16_drelu(64, 128, 64, P(t), 64, P(t), 64, P(t), P(t), 128, None, _lib.F16, sp) != 0
    assert L.hctr_gemm_nt16_drelu(64, 128, 64, P(t), 64, P(t), 64, P(t), P(t), 128, P(ws), _lib.F32, sp) != 0
    assert "16-bit types only" in _lib.last_error()
    assert L.hctr_gemm_nt16_drelu(0, 128, 64, None, 64, None, 64, None, None, 128, None, _lib.F16, sp) == 0
    assert L.hctr_gemm_nt16_drelu_tiles(0, 128) == 0 and L.hctr_gemm_nt16_drelu_tiles(64, 100) < 0
    torch.cuda.synchronize()
    assert not t.any() and not ws.any()
    # no env: 256-row tiles from 256 of them on and N >= 512, 128-row tiles from 512 of them on
    assert L.hctr_gemm_nt16_drelu_tiles(65536, 512) == math.ceil(65536 / 256)
    assert L.hctr_gemm_nt16_drelu_tiles(65536, 256) == math.ceil(65536 / 128)
    assert L.hctr_gemm_nt16_drelu_tiles(2048, 256) == math.ceil(2048 / 64)
