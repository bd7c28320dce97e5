"""CPU: hctr_mha_fwd / hctr_mha_bwd / hctr_sequence_mask refuse what attention.hip has no kernel
for, by name and before any device call (null pointers, no GPU)."""
import pytest

# (heads, seq_from, seq_to, size_per_head, dtype) -> what hctr_last_error() must name
BAD = [((4, 129, 10, 8, 0), "seq_from"), ((4, 10, 129, 8, 0), "seq_to"),
       ((4, 10, 10, 12, 1), "size_per_head"), ((4, 10, 10, 72, 2), "size_per_head"),
       ((0, 10, 10, 8, 0), "heads"), ((4, 10, 10, 8, 7), "dtype")]


@pytest.mark.parametrize("batch", [0, 3])
@pytest.mark.parametrize("shape,name", BAD)
def test_attention_entry_points_validate_before_touching_the_device(shape, name, batch):
    from hugectr_amd import _lib
    L = _lib.lib
    heads, m, n, d, dtype = shape
    assert L.hctr_mha_fwd(batch, heads, m, n, d, None, None, None, None, None, dtype, None) == -1
    assert name in _lib.last_error()
    assert L.hctr_mha_bwd(batch, heads, m, n, d, None, None, None, None, None, None, None, None,
                          dtype, None) == -1
    assert name in _lib.last_error()


def test_sequence_mask_validates_and_good_shapes_pass_with_an_empty_batch():
    from hugectr_amd import _lib
    L = _lib.lib
    assert L.hctr_sequence_mask(3, 0, 5, None, None, None, 0, None) == -1
    assert "max_from" in _lib.last_error()
    assert L.hctr_sequence_mask(3, 4, 5, None, None, None, 9, None) == -1
    assert "dtype" in _lib.last_error()
    assert L.hctr_sequence_mask(3, 4, 5, None, None, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    assert L.hctr_mha_fwd(3, 4, 10, 10, 8, None, None, None, None, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    assert L.hctr_sequence_mask(0, 4, 5, None, None, None, 0, None) == 0
    assert L.hctr_mha_fwd(0, 4, 128, 1, 64, None, None, None, None, None, 2, None) == 0
    assert L.hctr_mha_bwd(0, 1, 1, 128, 8, None, None, None, None, None, None, None, None, 1,
                          None) == 0
