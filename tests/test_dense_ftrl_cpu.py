"""CPU: the dense Ftrl entries (hctr_ftrl_shadow, hctr_ftrl_segments) are declared, exported and
bound, and refuse bad arguments before any HIP call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hctr_ftrl_shadow", "hctr_ftrl_segments")


def test_ftrl_entries_are_declared_exported_and_bound():
    from hugectr_amd import _lib
    src = open(os.path.join(ROOT, "include", "hugectr_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name}: not declared"
        assert hasattr(so, name), f"{name}: not exported"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name), f"{name}: not bound"
    # the header says which lines of the reference the entries stand in for
    assert "ftrl_optimizer.cu:28-43" in src
    # the block size the Python side sizes the segment table with is the header's
    assert int(re.search(r"#define HCTR_FTRL_SEG_BLOCK_ELEMS (\d+)", src).group(1)) == \
        _lib.FTRL_SEG_BLOCK_ELEMS


def test_ftrl_entries_validate_before_touching_the_device():
    """bad arguments come back as -1 with a message, without a GPU (the pointers are never read)"""
    from hugectr_amd import _lib
    L = _lib.lib
    P = ctypes.c_void_p
    a, b = P(0x1000), P(0x1004)  # 16-byte aligned / not
    hp = (0.05, 0.9, 0.1, 0.1, 1.0)
    assert L.hctr_ftrl_shadow(6, *hp, a, a, a, a, None, 0, None) == -1
    assert "multiple of 4" in _lib.last_error()
    assert L.hctr_ftrl_shadow(8, *hp, None, a, a, a, None, 0, None) == -1
    assert "null" in _lib.last_error()
    assert L.hctr_ftrl_shadow(8, *hp, a, a, None, a, None, 0, None) == -1
    assert L.hctr_ftrl_shadow(8, *hp, a, a, a, a, a, 0, None) == -1   # a copy of an unknown type
    assert "dtype" in _lib.last_error()
    assert L.hctr_ftrl_shadow(8, *hp, a, a, a, a, a, 3, None) == -1
    assert L.hctr_ftrl_shadow(8, *hp, a, b, a, a, None, 0, None) == -1
    assert "aligned" in _lib.last_error()
    assert L.hctr_ftrl_shadow(8, 0.0, 0.9, 0.1, 0.1, 1.0, a, a, a, a, None, 0, None) == -1
    assert "lr" in _lib.last_error()
    assert L.hctr_ftrl_shadow(8, 0.05, 0.9, -0.1, 0.1, 1.0, a, a, a, a, None, 0, None) == -1
    assert L.hctr_ftrl_shadow(8, 0.05, 0.9, 0.1, 0.1, float("nan"), a, a, a, a, None, 0,
                              None) == -1
    assert "grad_scale" in _lib.last_error()
    assert L.hctr_ftrl_shadow(0, *hp, None, None, None, None, None, 0, None) == 0  # nothing to do
    assert L.hctr_ftrl_segments(None, 2, 2, *hp, a, a, a, None) == -1
    assert "null" in _lib.last_error()
    assert L.hctr_ftrl_segments(a, -1, 2, *hp, a, a, a, None) == -1
    assert L.hctr_ftrl_segments(a, 2, 1 << 31, *hp, a, a, a, None) == -1
    assert "count" in _lib.last_error()
    assert L.hctr_ftrl_segments(a, 2, 2, *hp, a, None, a, None) == -1
    assert L.hctr_ftrl_segments(a, 2, 2, *hp, a, a, b, None) == -1
    assert "aligned" in _lib.last_error()
    assert L.hctr_ftrl_segments(a, 2, 2, 0.05, -1.0, 0.1, 0.1, 1.0, a, a, a, None) == -1
    assert L.hctr_ftrl_segments(a, 0, 0, *hp, None, None, None, None) == 0


def test_dense_ftrl_refuses_parameters_it_cannot_step():
    """DenseFtrl takes contiguous fp32 parameters on the GPU; anything else is an error, never a
    quiet fall-back"""
    import pytest
    import torch
    from hugectr_amd.dense import DenseFtrl
    with pytest.raises(RuntimeError, match="fp32 parameters on the GPU"):
        DenseFtrl([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
