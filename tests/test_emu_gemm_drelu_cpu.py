"""hctr_gemm_nt16_drelu (cross_gemm.hip) stepped through on the host interpreter of tests/emu: the
dReLU epilogue of the 64 / 128-row kernel and of the 256 x 256 kernel -- the mask, rows past M, the
column sums' way through LDS, one partial row per row tile -- with integer operands in [-2, 2], for
which every sum is exact: dz and the partial rows are compared bit for bit with numpy
(tests/test_gemm_drelu_gpu.py runs the full matrix on the device)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

pytestmark = pytest.mark.skipif(not emu.available(), reason="no host clang++ / make")


@pytest.fixture(scope="module")
def elib():
    lib = emu.load_under_test()
    emu.bind(lib)
    return lib


@pytest.mark.parametrize("M,N,K,bm,stages", [(70, 128, 128, 64, 2), (130, 256, 64, 128, 3),
                                             (300, 256, 128, 256, 2)])
def test_drelu_epilogue_exact(elib, monkeypatch, M, N, K, bm, stages):
    rng = np.random.default_rng(M + N + K)
    a = rng.integers(-2, 3, (M, K)).astype(np.float16)
    bt = rng.integers(-2, 3, (N, K)).astype(np.float16)
    bt[:, 0] += (np.arange(N) % 2).astype(np.float16)  # (asymmetric in n)
    # y: positive, negative, +0, -0, NaN, the smallest positive subnormal
    pats = np.array([0x3C00, 0xC200, 0x0000, 0x8000, 0x7E00, 0x0001], dtype=np.uint16)
    y = pats[rng.integers(0, len(pats), (M, N))].view(np.float16)
    ldc = N + 8
    monkeypatch.setenv("HCTR_GEMM_BM", str(bm))
    monkeypatch.setenv("HCTR_GEMM_STAGES", str(stages))
    tiles = elib.hctr_gemm_nt16_drelu_tiles(M, N)
    assert tiles == (M + bm - 1) // bm
    ybuf = np.full((M, ldc), np.nan, np.float16)
    ybuf[:, :N] = y
    dz = np.full((M + 2, ldc), np.nan, np.float16)
    part = np.full((tiles + 2, N), np.nan, np.float32)
    emu.check(elib, elib.hctr_gemm_nt16_drelu(M, N, K, emu.ptr(a), K, emu.ptr(bt), K, emu.ptr(ybuf),
                                              emu.ptr(dz), ldc, emu.ptr(part), 1, None))
    with np.errstate(invalid="ignore"):
        keep = y.astype(np.float64) > 0
    want = np.where(keep, (a.astype(np.float64) @ bt.astype(np.float64).T).astype(np.float16),
                    np.float16(0))
    assert np.array_equal(dz[:M, :N].view(np.uint16), want.view(np.uint16))
    assert np.isnan(dz[M:]).all() and np.isnan(dz[:M, N:]).all() and np.isnan(part[tiles:]).all()
    for t in range(tiles):
        rows = want[t * bm:(t + 1) * bm].astype(np.float64).sum(0)
        assert np.array_equal(part[t].astype(np.float64), rows), f"tile {t}"
