"""CPU: hctr_mha_tiled_fwd / hctr_mha_tiled_bwd refuse what attention_tiled.hip has no kernel for, by
name and before any device call (null pointers, no GPU); hctr_mha_fwd keeps its own limits."""
import pytest

# (heads, seq_from, seq_to, size_per_head, dtype) -> what hctr_last_error() must name
BAD = [((4, 4097, 10, 8, 0), "seq_from"), ((4, 10, 4097, 8, 0), "seq_to"),
       ((4, 10, 10, 136, 1), "size_per_head"), ((4, 10, 10, 12, 2), "size_per_head"),
       ((0, 10, 10, 8, 0), "heads"), ((4, 10, 10, 8, 7), "dtype")]


@pytest.mark.parametrize("batch", [0, 3])
@pytest.mark.parametrize("shape,name", BAD)
def test_tiled_entry_points_validate_before_touching_the_device(shape, name, batch):
    from hugectr_amd import _lib
    L = _lib.lib
    heads, m, n, d, dtype = shape
    assert L.hctr_mha_tiled_fwd(batch, heads, m, n, d, None, None, None, None, None, None, dtype,
                                None) == -1
    assert name in _lib.last_error()
    assert L.hctr_mha_tiled_bwd(batch, heads, m, n, d, None, None, None, None, None, None, None,
                                None, None, None, dtype, None) == -1
    assert name in _lib.last_error()


def test_largest_shape_passes_with_an_empty_batch_and_the_first_family_keeps_its_limits():
    from hugectr_amd import _lib
    L = _lib.lib
    for dtype in (0, 1, 2):
        assert L.hctr_mha_tiled_fwd(0, 4, 4096, 4096, 128, None, None, None, None, None, None,
                                    dtype, None) == 0
        assert L.hctr_mha_tiled_bwd(0, 4, 4096, 4096, 128, None, None, None, None, None, None, None,
                                    None, None, None, dtype, None) == 0
    assert L.hctr_mha_tiled_fwd(3, 4, 10, 10, 8, None, None, None, None, None, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    assert L.hctr_mha_fwd(3, 4, 129, 10, 8, None, None, None, None, None, 0, None) == -1
    assert "seq_from" in _lib.last_error()
