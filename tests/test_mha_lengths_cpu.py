"""CPU: the four *_len_* attention entries (lengths in the place of the mask) are exported and bound,
and refuse what their siblings refuse, by the same names, before any device call."""
import ctypes

import pytest

from test_mha_cpu import BAD as BAD_FIRST
from test_mha_tiled_cpu import BAD as BAD_TILED

# entry -> (pointer arguments, the shapes it refuses, its largest shape)
ENTRIES = {"hctr_mha_len_fwd": (6, BAD_FIRST, (128, 128, 64)),
           "hctr_mha_len_bwd": (9, BAD_FIRST, (128, 128, 64)),
           "hctr_mha_tiled_len_fwd": (7, BAD_TILED, (4096, 4096, 128)),
           "hctr_mha_tiled_len_bwd": (11, BAD_TILED, (4096, 4096, 128))}


@pytest.mark.parametrize("entry", ENTRIES)
def test_len_entries_refuse_like_their_siblings(entry):
    from hugectr_amd import _lib
    assert entry in _lib.EXPORTED_SYMBOLS
    fn, (nptr, bad, largest) = getattr(_lib.lib, entry), ENTRIES[entry]
    for (heads, m, n, d, dtype), name in bad:
        for batch in (0, 3):
            assert fn(batch, heads, m, n, d, *[None] * nptr, dtype, None) == -1
            assert name in _lib.last_error()
    for dtype in (0, 1, 2):
        assert fn(0, 4, *largest, *[None] * nptr, dtype, None) == 0
    # every tensor given (never touched: the refusal comes first), the two lengths null
    raw = ctypes.create_string_buffer(32)
    buf = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    ptrs = [buf] * 3 + [None, None] + [buf] * (nptr - 5)
    assert fn(3, 4, 10, 10, 8, *ptrs, 0, None) == -1
    assert "null pointer" in _lib.last_error()
