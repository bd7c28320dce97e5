"""CPU: the entry points of gru.hip (hctr_gru_fwd, hctr_gru_bwd, hctr_gru_workspace) refuse what they
cannot serve, by name and before any device call (null pointers, no GPU), and serve batch = 0; the
Python layer refuses bad arguments by name."""
import ctypes

import pytest


def _gru(batch, seq, vec, hidden, dtype=0, p=None):
    sizes = (ctypes.c_size_t * 2)()
    calls = [lambda L: L.hctr_gru_fwd(batch, seq, vec, hidden, 0, p, p, p, p, dtype, None),
             lambda L: L.hctr_gru_bwd(batch, seq, vec, hidden, 1, p, p, p, p, p, p, p, p, dtype, None)]
    if dtype in (0, 1, 2) and p is None and batch:  # (the size query knows no dtype and no tensors)
        calls.append(lambda L: L.hctr_gru_workspace(
            batch, seq, vec, hidden, ctypes.cast(sizes, ctypes.POINTER(ctypes.c_size_t)), None))
    return calls


BAD = [(_gru(3, 2, 4, 0), "hidden H 1 .. 256"), (_gru(3, 2, 4, 257), "hidden H 1 .. 256"),
       (_gru(3, 2, 0, 4), "vector size V 1 .. 1024"), (_gru(3, 2, 1025, 4), "vector size V 1 .. 1024"),
       (_gru(3, 0, 4, 4), "seq S >= 1"), (_gru(2 ** 31, 1, 1, 1), "2^31"),
       (_gru(2 ** 20, 2, 1024, 4), "2^31"), (_gru(2 ** 20, 8, 4, 256), "2^31"),
       (_gru(3, 2, 4, 4, dtype=3), "dtype"), (_gru(3, 2, 4, 4, dtype=-1), "dtype"),
       (_gru(3, 2, 4, 4), "null pointer")]


@pytest.mark.parametrize("calls,name", BAD)
def test_entry_points_validate_before_touching_the_device(calls, name):
    from hugectr_amd import _lib
    for call in calls:
        assert call(_lib.lib) == -1
        assert name in _lib.last_error()


def test_batch_zero_is_served():
    from hugectr_amd import _lib
    calls = []
    for dtype in (0, 1, 2):
        calls += _gru(0, 7, 1024, 256, dtype)
    assert [call(_lib.lib) for call in calls] == [0] * len(calls)
    reserve, scratch = ctypes.c_size_t(1), ctypes.c_size_t(1)
    assert _lib.lib.hctr_gru_workspace(0, 7, 4, 4, ctypes.byref(reserve), ctypes.byref(scratch)) == 0
    assert (reserve.value, scratch.value) == (0, 0)


def test_python_layer_refuses_bad_arguments_by_name():
    import torch
    import hugectr_amd as ha
    x = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="weight"):
        ha.gru(x, torch.zeros(3 * 5 * (4 + 5 + 1) - 1), 5)
    with pytest.raises(ValueError, match="weight"):
        ha.gru(x, torch.zeros(3 * 5 * (4 + 5 + 1), dtype=torch.float16), 5)
    with pytest.raises(ValueError, match="x of three dimensions"):
        ha.gru(x[0], torch.zeros(3 * 5 * (4 + 5 + 1)), 5)
    with pytest.raises(ValueError, match="hidden"):
        ha.gru(x, torch.zeros(0), 0)
    with pytest.raises(ValueError, match="hidden 1 .. 256"):
        ha.gru(x, torch.zeros(3 * 257 * (4 + 257 + 1)), 257)
    with pytest.raises(ValueError, match="vector size"):
        ha.gru(torch.zeros(1, 1, 1025), torch.zeros(3 * 2 * (1025 + 2 + 1)), 2)
    layer = ha.GRULayer(5, 4, batch_first=True)
    assert isinstance(layer, torch.nn.Module) and layer.weight.shape == (3 * 5 * (4 + 5 + 1),)
    assert layer.weight.abs().max().item() <= 5 ** -0.5
    with pytest.raises(ValueError, match="vector_size"):
        layer(torch.zeros(2, 3, 6))
    with pytest.raises(ValueError, match="vector_size"):
        ha.GRULayer(5, 0)
