"""numpy statement of the two dense-lookup routines (hctr_dist_select, hctr_indexed_row_copy):
what tests/test_sok_dense_*.py compare the kernels with.  Nothing here calls the library."""
import numpy as np


def dist_select(keys, num_splits):
    """(out_keys, order int32, splits int32): keys grouped by owner key % num_splits (numpy's
    remainder is the non-negative one), owners ascending, ascending input position inside one"""
    keys = np.asarray(keys)
    owner = keys % num_splits
    order = np.argsort(owner, kind="stable").astype(np.int32)
    splits = np.bincount(owner.astype(np.int64), minlength=num_splits).astype(np.int32)
    return keys[order], order, splits


def indexed_row_copy(src, index, index_div, n, dst, dst_pos=None, src_rows=None):
    """in place on dst: dst[dst_pos[i] or i] = src[r] if 0 <= r (< src_rows) else 0, with
    r = index[i] // index_div (floor) or i; src_rows None: the rows of src, 0: no upper bound.
    The store converts to dst's dtype (numpy rounds fp32 -> fp16 to nearest even)."""
    if src_rows is None:
        src_rows = src.shape[0]
    for i in range(n):
        r = int(index[i]) // int(index_div) if index is not None else i
        ok = r >= 0 and (src_rows == 0 or r < src_rows)
        j = int(dst_pos[i]) if dst_pos is not None else i
        dst[j] = src[r].astype(dst.dtype) if ok else 0
    return dst
