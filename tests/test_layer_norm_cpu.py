"""CPU: hctr_layer_norm_fwd / hctr_layer_norm_bwd refuse what layer_norm.hip has no kernel for, by name
and before any device call (null pointers, no GPU)."""
import pytest

# (rows, hidden, dtype, eps) -> what hctr_last_error() must name (the backward takes no eps)
BAD = [((3, 0, 0, 1e-5), "hidden"), ((3, 8193, 1, 1e-5), "hidden"), ((3, -4, 2, 1e-5), "hidden"),
       ((2 ** 31, 1, 0, 1e-5), "rows"), ((262144, 8192, 1, 1e-5), "rows"),
       ((3, 64, 7, 1e-5), "dtype"), ((3, 64, 0, 0.0), "eps"), ((0, 64, 0, -1.0), "eps")]


@pytest.mark.parametrize("args,name", BAD)
def test_entry_points_validate_before_touching_the_device(args, name):
    from hugectr_amd import _lib
    L = _lib.lib
    rows, hidden, dtype, eps = args
    assert L.hctr_layer_norm_fwd(rows, hidden, None, None, None, None, eps, None, None, dtype,
                                 None) == -1
    assert name in _lib.last_error()
    if name != "eps":
        assert L.hctr_layer_norm_bwd(rows, hidden, None, None, None, None, None, None, None, None,
                                     None, dtype, None) == -1
        assert name in _lib.last_error()


def test_no_rows_pass_at_the_widest_row_and_the_scratch_grows_with_the_rows():
    from hugectr_amd import _lib
    L = _lib.lib
    for dtype in (0, 1, 2):
        assert L.hctr_layer_norm_fwd(0, 8192, None, None, None, None, 1e-5, None, None, dtype,
                                     None) == 0
        assert L.hctr_layer_norm_bwd(0, 8192, None, None, None, None, None, None, None, None, None,
                                     dtype, None) == 0
    assert L.hctr_layer_norm_fwd(3, 64, None, None, None, None, 1e-5, None, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    sizes = [L.hctr_layer_norm_bwd_scratch_bytes(rows, 100) for rows in (0, 1, 7, 4096, 10 ** 6)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
