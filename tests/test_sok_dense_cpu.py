"""CPU: the surface of the SOK dense lookups (all2all_dense_embedding, group_lookup), the argument
validation of their two C-ABI entries (no device is touched), and the numpy oracle the GPU tests
use, against hand-worked cases."""
import ctypes
import inspect

import numpy as np

import dense_lookup_oracle as orc


def test_both_packages_export_the_dense_lookups():
    import sparse_operation_kit
    from hugectr_amd import sok
    for mod in (sparse_operation_kit, sok):
        a = inspect.signature(mod.all2all_dense_embedding)
        pos = [p.name for p in a.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert pos == ["param", "indices"]
        assert a.parameters["training"].kind == inspect.Parameter.KEYWORD_ONLY
        g = inspect.signature(mod.group_lookup)
        assert list(g.parameters) == ["params", "indices", "dtype", "name"]
        assert g.parameters["dtype"].default is None and g.parameters["name"].default is None
    assert sparse_operation_kit.group_lookup is sok.group_lookup


def _fails_naming(rc, word):
    from hugectr_amd import _lib
    assert rc == -1, rc
    assert word in _lib.last_error(), (word, _lib.last_error())


def test_dist_select_validates_without_a_device():
    from hugectr_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = _lib.dist_select_ws_bytes(256)
    for bad in (0, 257, -1):
        _fails_naming(L.hctr_dist_select(p, _lib.KEY_I64, 4, bad, p, p, p, p, big, None),
                      "num_splits")
    _fails_naming(L.hctr_dist_select(p, 2, 4, 2, p, p, p, p, big, None), "key_type")
    _fails_naming(L.hctr_dist_select(p, _lib.KEY_I64, 1 << 31, 2, p, p, p, p, big, None), "n must")
    _fails_naming(L.hctr_dist_select(p, _lib.KEY_I64, 4, 2, p, p, None, p, big, None), "splits")
    _fails_naming(L.hctr_dist_select(None, _lib.KEY_I64, 4, 2, p, p, p, p, big, None), "keys")
    _fails_naming(L.hctr_dist_select(p, _lib.KEY_I64, 4, 2, None, p, p, p, big, None), "out_keys")
    _fails_naming(L.hctr_dist_select(p, _lib.KEY_I64, 4, 2, p, None, p, p, big, None), "order")
    _fails_naming(L.hctr_dist_select(p, _lib.KEY_I64, 4, 2, p, p, p, None, big, None), "workspace")
    _fails_naming(L.hctr_dist_select(p, _lib.KEY_I64, 4, 2, p, p, p, p,
                                     _lib.dist_select_ws_bytes(2) - 1, None), "workspace_bytes")


def _task(_lib, **kw):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    t = _lib.RowCopyTask()
    t.src, t.src_rows, t.dim, t.index_type, t.index, t.index_div = p, 4, 4, _lib.KEY_I64, p, 1
    t.n, t.dst, t.dst_rows, t.dst_pos = 4, p, 4, None
    for k, v in kw.items():
        setattr(t, k, v)
    return t, buf


def test_indexed_row_copy_validates_without_a_device():
    from hugectr_amd import _lib
    L = _lib.lib

    def call(num=1, sd=_lib.F32, dd=_lib.F32, **kw):
        t, keep = _task(_lib, **kw)
        arr = (_lib.RowCopyTask * 1)(t)
        return L.hctr_indexed_row_copy(arr, num, sd, dd, None)

    _fails_naming(L.hctr_indexed_row_copy(None, 1, _lib.F32, _lib.F32, None), "tasks")
    _fails_naming(call(num=0), "num_tasks")
    _fails_naming(call(num=_lib.ROW_COPY_MAX_TASKS + 1), "num_tasks")
    _fails_naming(call(sd=_lib.BF16), "src_dtype")
    _fails_naming(call(dd=7), "dst_dtype")
    _fails_naming(call(dim=0), "dim")
    _fails_naming(call(index_div=0), "index_div")
    _fails_naming(call(index_type=5), "index_type")
    _fails_naming(call(src=None), "src")
    _fails_naming(call(dst=None), "dst")
    _fails_naming(call(dst_rows=3), "dst_rows")
    # nothing to copy: accepted, and still nothing of the device is touched
    assert call(n=0, src=None, dst=None, dst_rows=0) == 0


def test_the_workspace_macro_and_its_python_twin_agree():
    import os
    import re
    from hugectr_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hugectr_amd.h")).read()
    m = re.search(r"#define HCTR_DIST_SELECT_WS_BYTES\(num_splits\) (.*)", src)
    expr = m.group(1).replace("(size_t)", "")
    for n in (1, 2, 256):
        assert eval(expr, {"num_splits": n}) == _lib.dist_select_ws_bytes(n)
    m = re.search(r"#define HCTR_ROW_COPY_MAX_TASKS (\d+)", src)
    assert int(m.group(1)) == _lib.ROW_COPY_MAX_TASKS


def test_oracle_dist_select_by_hand():
    # owners (mod 3): 7->1 3->0 8->2 1->1 6->0 4->1
    k, order, splits = orc.dist_select(np.array([7, 3, 8, 1, 6, 4], dtype=np.int64), 3)
    assert k.tolist() == [3, 6, 7, 1, 4, 8]
    assert order.tolist() == [1, 4, 0, 3, 5, 2] and order.dtype == np.int32
    assert splits.tolist() == [2, 3, 1]
    k, order, splits = orc.dist_select(np.array([], dtype=np.int32), 4)
    assert k.size == 0 and order.size == 0 and splits.tolist() == [0, 0, 0, 0]


def test_oracle_indexed_row_copy_by_hand():
    src = np.arange(12, dtype=np.float32).reshape(4, 3)
    # keys 6, 1, -1, 9 with index_div 2 -> rows 3, 0, -1 (no row), 4 (out of range)
    dst = np.full((4, 3), 9, dtype=np.float32)
    orc.indexed_row_copy(src, np.array([6, 1, -1, 9]), 2, 4, dst, dst_pos=np.array([2, 0, 3, 1]))
    assert dst.tolist() == [[0, 1, 2], [0, 0, 0], [9, 10, 11], [0, 0, 0]]
    # src_rows = 0: only the sign is checked
    dst = np.zeros((2, 3), dtype=np.float16)
    orc.indexed_row_copy(src, np.array([3, -2]), 1, 2, dst, src_rows=0)
    assert dst.tolist() == [[9, 10, 11], [0, 0, 0]] and dst.dtype == np.float16
    # no index: the identity
    dst = np.zeros((3, 3), dtype=np.float32)
    orc.indexed_row_copy(src, None, 1, 3, dst)
    assert (dst == src[:3]).all()
