"""CPU: hctr_batch_norm_* / hctr_prelu_dice_* refuse what batch_norm.hip has no kernel for, by name and
before any device call (null pointers, no GPU)."""
import pytest

# (rows, n, dtype, eps, factor) -> what hctr_last_error() must name (only the BatchNorm forward takes a
# factor, the BatchNorm backward takes no eps, and eps = 0 is Dice's to accept)
BAD = [((3, 0, 0, 1e-5, 1.0), "n 1 .. 65536"), ((3, 65537, 1, 1e-5, 1.0), "n 1 .. 65536"),
       ((3, -4, 2, 1e-5, 1.0), "n 1 .. 65536"), ((2 ** 31, 1, 0, 1e-5, 1.0), "rows * n"),
       ((32768, 65536, 1, 1e-5, 1.0), "rows * n"), ((3, 64, 7, 1e-5, 1.0), "dtype"),
       ((3, 64, 0, -1.0, 1.0), "eps"), ((0, 64, 0, float("nan"), 1.0), "eps"),
       ((3, 64, 0, 1e-5, 1.5), "factor"), ((0, 64, 1, 1e-5, -0.1), "factor")]


@pytest.mark.parametrize("args,name", BAD)
def test_entry_points_validate_before_touching_the_device(args, name):
    from hugectr_amd import _lib
    L = _lib.lib
    rows, n, dtype, eps, factor = args
    calls = [lambda: L.hctr_batch_norm_fwd(rows, n, None, None, None, factor, eps, None, None, None,
                                           None, None, 1, dtype, None)]
    if name != "factor":
        calls += [lambda: L.hctr_prelu_dice_fwd(rows, n, None, 0.2, eps, None, None, None, dtype, None),
                  lambda: L.hctr_prelu_dice_bwd(rows, n, None, None, 0.2, eps, None, None, dtype, None)]
        if name != "eps":
            calls.append(lambda: L.hctr_batch_norm_bwd(rows, n, None, None, None, None, None, None,
                                                       None, None, dtype, None))
    for call in calls:
        assert call() == -1
        assert name in _lib.last_error()


def test_no_rows_pass_null_pointers_do_not_and_the_scratch_grows_with_the_rows():
    from hugectr_amd import _lib
    L = _lib.lib
    for dtype in (0, 1, 2):
        for training in (0, 1):
            assert L.hctr_batch_norm_fwd(0, 65536, None, None, None, 1.0, 1e-5, None, None, None, None,
                                         None, training, dtype, None) == 0
        assert L.hctr_batch_norm_bwd(0, 65536, None, None, None, None, None, None, None, None, dtype,
                                     None) == 0
        assert L.hctr_prelu_dice_fwd(0, 65536, None, 0.2, 0.0, None, None, None, dtype, None) == 0
        assert L.hctr_prelu_dice_bwd(0, 65536, None, None, 0.2, 0.0, None, None, dtype, None) == 0
    assert L.hctr_batch_norm_fwd(3, 64, None, None, None, 1.0, 1e-5, None, None, None, None, None, 1, 0,
                                 None) == -1
    assert "null pointer" in _lib.last_error()
    assert L.hctr_prelu_dice_bwd(3, 64, None, None, 0.2, 1e-8, None, None, 0, None) == -1
    assert "null pointer" in _lib.last_error()
    for n in (1, 100, 65536):
        sizes = [L.hctr_col_stats_scratch_bytes(rows, n) for rows in (0, 1, 7, 4096, 10 ** 6)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] >= sizes[0]
    assert L.hctr_col_stats_scratch_bytes(10 ** 6, 100) > L.hctr_col_stats_scratch_bytes(1, 100)


def test_python_layers_refuse_bad_arguments_by_name():
    import torch
    import hugectr_amd as ha
    x = torch.zeros(4, 6)
    with pytest.raises(ValueError, match="gamma"):
        ha.batch_norm(x, torch.ones(5), torch.zeros(6), torch.zeros(6), torch.ones(6), True)
    with pytest.raises(ValueError, match="fp32 / fp16 / bf16"):
        ha.prelu_dice(x.double(), 0.2, 1e-8)
    assert isinstance(ha.BatchNormLayer(6), torch.nn.Module) and ha.PReLUDiceLayer(0.2, 1e-8).alpha == 0.2
