"""CPU: the entry points of sequence_ops.hip (hctr_matmul_*, hctr_reduce_mean_*,
hctr_fused_reshape_concat_*) refuse what they cannot serve, by name and before any device call (null
pointers, no GPU), and serve zero-sized problems."""
import ctypes

import pytest

P8 = (ctypes.c_void_p * 9)(*[64] * 9)  # host table of (never touched) device pointers
W8 = (ctypes.c_int * 9)(*[4] * 9)


def _mm(batch, m, n, k, dtype=0, p=None):
    # (the backward is asked for both gradients: with neither it has nothing to do and returns 0)
    return [lambda L: L.hctr_matmul_fwd(batch, m, n, k, p, p, p, dtype, None),
            lambda L: L.hctr_matmul_bwd(batch, m, n, k, p, p, p, 64, 64, dtype, None)]


def _rm(outer, length, inner, dtype=0, p=None):
    return [lambda L: L.hctr_reduce_mean_fwd(outer, length, inner, p, p, dtype, None),
            lambda L: L.hctr_reduce_mean_bwd(outer, length, inner, p, p, dtype, None)]


def _frc(batch, slots, num, dtype=0, tab=P8, widths=W8, p=None):
    return [lambda L: L.hctr_fused_reshape_concat_fwd(batch, slots, num, tab, widths, p, p, dtype, None),
            lambda L: L.hctr_fused_reshape_concat_bwd(batch, slots, num, tab, widths, p, p, dtype, None)]


BAD = [(_mm(3, 0, 4, 4), "m 1 .. 4096"), (_mm(3, 4097, 4, 4), "m 1 .. 4096"),
       (_mm(3, 4, 0, 4), "inner dimension n"), (_mm(3, 4, 4097, 4), "inner dimension n"),
       (_mm(3, 4, 4, -1), "k 1 .. 4096"), (_mm(3, 4, 4, 4097), "k 1 .. 4096"),
       (_mm(2 ** 31, 1, 1, 1), "2^31"), (_mm(128, 4096, 4096, 1), "2^31"),
       (_mm(3, 4, 4, 4, dtype=3), "dtype"), (_mm(3, 4, 4, 4), "null pointer"),
       (_rm(3, 0, 4), "axis"), (_rm(2 ** 31, 1, 1), "outer * len * inner"),
       (_rm(2 ** 20, 2 ** 10, 2), "outer * len * inner"), (_rm(1, 2 ** 40, 2 ** 40), "outer * len * inner"),
       (_rm(3, 4, 4, dtype=-1), "dtype"), (_rm(3, 4, 4), "null pointer"),
       (_frc(3, 4, 0), "num 1 .. 8"), (_frc(3, 4, 9), "num 1 .. 8"), (_frc(3, 0, 2), "slots S >= 1"),
       (_frc(3, 4, 2, dtype=5), "dtype"), (_frc(2 ** 29, 4, 2), "rows"), (_frc(2 ** 27, 4, 2), "rows"),
       (_frc(3, 4, 2, widths=(ctypes.c_int * 2)(4, 0)), "width >= 1"),
       (_frc(3, 4, 2, tab=None), "null pointer"), (_frc(3, 4, 2, widths=None), "null pointer"),
       (_frc(3, 4, 2, tab=(ctypes.c_void_p * 2)(64, None), p=64), "null pointer"),
       (_frc(3, 4, 2), "null pointer")]


@pytest.mark.parametrize("calls,name", BAD)
def test_entry_points_validate_before_touching_the_device(calls, name):
    from hugectr_amd import _lib
    for call in calls:
        assert call(_lib.lib) == -1
        assert name in _lib.last_error()


def test_zero_sized_problems_are_served():
    from hugectr_amd import _lib
    calls = []
    for dtype in (0, 1, 2):
        calls += _mm(0, 4096, 4096, 4096, dtype) + _rm(0, 5, 7, dtype) + _rm(5, 7, 0, dtype)
        calls += _frc(0, 11, 8, dtype, tab=None, widths=None)
    assert [call(_lib.lib) for call in calls] == [0] * len(calls)
    # (a backward that is asked for neither gradient has nothing to do either)
    assert _lib.lib.hctr_matmul_bwd(3, 4, 4, 4, None, None, None, None, None, 0, None) == 0


def test_python_layers_refuse_bad_arguments_by_name():
    import torch
    import hugectr_amd as ha
    x = torch.zeros(2, 3, 4)
    for axis in (3, -1):
        with pytest.raises(ValueError, match="axis"):
            ha.reduce_mean(x, axis)
    with pytest.raises(ValueError, match="equal B and S"):
        ha.fused_reshape_concat([x, torch.zeros(2, 4, 4)])
    with pytest.raises(ValueError, match="1 .. 8 inputs"):
        ha.fused_reshape_concat([x] * 9)
    with pytest.raises(ValueError, match="matrix_multiply"):
        ha.matrix_multiply(x, torch.zeros(2, 5, 4))
    with pytest.raises(ValueError, match="matrix_multiply"):
        ha.matrix_multiply(x, torch.zeros(4, 5))
    assert all(isinstance(m, torch.nn.Module) for m in
               (ha.MatrixMultiplyLayer(), ha.ReduceMeanLayer(1), ha.FusedReshapeConcatLayer()))
