"""hctr_parquet_decode through the C ABI (csrc/parquet_decode.hip) on hand-built column buffers,
against the closed forms of include/hugectr_amd.h written out in numpy (tests/parquet_oracle.py).
All comparisons are exact."""
import ctypes

import numpy as np
import pytest
import torch

import parquet_oracle as po

pytestmark = pytest.mark.gpu


def _file(rng, rows):
    """columns of one 'file': 1 label (int64), 2 dense (float64, int64), param p = (int32 scalar,
    list<int64> 0..70, list<int32> 0..2), params q / r one list slot each, param s 40 scalar
    slots, param t one scalar slot.
    The lists are built as chunks of 24 rows would leave them: a batch that starts at row 40 lies
    across the boundary of the chunks [24, 48) and [48, 72)."""
    def lists(max_len, dt, hi):
        lens = rng.integers(0, max_len + 1, size=rows)
        lens[40], lens[41], lens[47], lens[48] = 0, max_len, 0, max_len
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return rng.integers(-3, hi, size=int(off[-1])).astype(dt), off
    cols = [(rng.integers(-2, 3, size=rows).astype(np.int64), None),
            (rng.random(rows) * 1e6 + 1e-7, None),
            (rng.integers(-(1 << 62), 1 << 62, size=rows).astype(np.int64) | 1, None),
            (rng.integers(-(1 << 31), 1 << 31, size=rows).astype(np.int32), None),
            lists(70, np.int64, 1 << 45), lists(2, np.int32, 1 << 31),
            lists(5, np.int64, 1 << 40), lists(1, np.int32, 1 << 20)]
    cols += [(rng.integers(0, 1 << 40, size=rows).astype(np.int64), None) for _ in range(41)]
    return cols


def _columns(cols):
    from hugectr_amd import _lib
    pt = {np.dtype(np.float32): _lib.PQ_F32, np.dtype(np.float64): _lib.PQ_F64,
          np.dtype(np.int32): _lib.PQ_I32, np.dtype(np.int64): _lib.PQ_I64}
    return [(pt[v.dtype], v.dtype.itemsize, o is not None) for v, o in cols]


PARAMS = [("p", 3), ("q", 1), ("r", 1), ("s", 40), ("t", 1)]


def _decode(cols, a, B, *, rank=0, world=1, i64=True, groups=(), mean_keys=None, rows=None):
    """stages the columns by hand, launches once, returns the plan and every output as numpy"""
    from hugectr_amd import _lib, data
    columns = _columns(cols)
    rows = len(cols[0][0]) if rows is None else rows
    addend = np.arange(1, 47, dtype=np.int64) * 1000
    pl = data.parquet_decode_plan(columns, 1, 2, PARAMS, [list(g) for g in groups], addend, B, rank,
                                  world, i64, mean_keys)
    _, lay, used = data.parquet_slot_layout(columns, len(pl["outputs"]), B, rows,
                                            [len(v) for v, _ in cols])
    buf = np.zeros(used, np.uint8)
    desc = np.zeros(len(cols), np.dtype(_lib.PQ_COLUMN_FIELDS))
    for i, ((v, o), (v_off, o_off)) in enumerate(zip(cols, lay)):
        desc[i] = (v_off, o_off, columns[i][0], columns[i][1])
        buf[v_off:v_off + v.nbytes] = v.view(np.uint8)
        if o is not None:
            buf[o_off:o_off + o.nbytes] = o.view(np.uint8)
    buf[:desc.nbytes] = desc.view(np.uint8)
    cnt = [o["const"] + sum(int(cols[c][1][a + B] - cols[c][1][a]) for c in o["cols"])
           for o in pl["outputs"]]
    tab = np.zeros(len(cnt) + 1, np.int64)
    tab[1:] = np.cumsum([(n * o["esize"] + 255) // 256 * 256 for n, o in zip(cnt, pl["outputs"])])
    blob = np.concatenate([pl["segments"].view(np.uint8).reshape(-1), pl["addend"].view(np.uint8),
                           pl["list"].view(np.uint8)])
    slot, plan, dtab = (torch.from_numpy(x).cuda() for x in (buf, blob, tab))
    arena = torch.full((int(tab[-1]) + 256,), 0xCD, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.hctr_parquet_decode(
        _lib.ptr(slot), _lib.ptr(slot), len(cols), _lib.ptr(plan), len(pl["segments"]),
        len(pl["list"]), pl["n_items"], rows, a, B, _lib.ptr(arena), _lib.ptr(dtab), len(cnt),
        _lib.stream_ptr()))
    torch.cuda.synchronize()
    raw = arena.cpu().numpy()
    # nothing is written between the outputs or behind the last one
    for k, (n, o) in enumerate(zip(cnt, pl["outputs"])):
        assert (raw[int(tab[k]) + n * o["esize"]:int(tab[k + 1])] == 0xCD).all(), k
    assert (raw[int(tab[-1]):] == 0xCD).all()

    def get(k, dt):
        return raw[int(tab[k]):int(tab[k]) + cnt[k] * pl["outputs"][k]["esize"]].view(dt).copy()
    return pl, get


@pytest.fixture(scope="module")
def cols():
    return _file(np.random.default_rng(20), 137)


@pytest.mark.parametrize("a,B", [(40, 32), (0, 1), (3, 65), (0, 137)])
def test_against_the_closed_forms(cols, a, B):
    """a = 40 starts in the middle of a chunk and crosses the boundary at row 48; B = 65 and 137
    leave partial tiles and partial lane groups; the 40-slot param takes two column passes"""
    addend = np.arange(1, 47, dtype=np.int64) * 1000
    pl, get = _decode(cols, a, B, mean_keys={"p": 36.0, "q": 2.5, "r": 0.5})
    assert [int(g) for g in pl["segments"]["group"][2:5]] == [64, 4, 1]
    lab = np.stack([cols[0][0]], 1).astype(np.float32)[a:a + B]
    assert np.array_equal(get(pl["label"][0], np.float32).reshape(B, 1).view(np.int32),
                          lab.view(np.int32))
    # float64 + int64 stack to float64: the int64 column rounds twice, as numpy's astype does
    den = np.stack([cols[1][0], cols[2][0]], 1).astype(np.float32)[a:a + B]
    assert np.array_equal(get(pl["dense"][0], np.float32).reshape(B, 2).view(np.int32),
                          den.view(np.int32))
    c = 3
    for name, S in PARAMS:
        o_ro, o_k, _ = pl["sparse"][name]
        ro, keys = po.ragged_param(cols[c:c + S], addend[c - 3:c - 3 + S], a, B)
        assert np.array_equal(get(o_k, np.int64), keys), name
        if o_ro is None:
            assert np.array_equal(ro, np.arange(B * S + 1))
        else:
            assert np.array_equal(get(o_ro, np.int64), ro), name
        c += S


def test_int64_dense_alone_rounds_once(cols):
    """two int64 dense columns stay int64 when numpy stacks them: one rounding, not two"""
    from hugectr_amd import _lib
    two = list(cols)
    v = cols[2][0].copy()
    v[:4] = [(1 << 53) + 1, (1 << 60) + (1 << 36) + 1, -(1 << 61) - (1 << 37) - 1, (1 << 24) + 1]
    two[1], two[2] = (v, None), (v[::-1].copy(), None)
    pl, get = _decode(two, 0, 64)
    assert pl["segments"][1]["out_kind"] == _lib.PQ_OUT_F32
    want = np.stack([two[1][0], two[2][0]], 1).astype(np.float32)[:64]
    assert np.array_equal(get(pl["dense"][0], np.float32).reshape(64, 2).view(np.int32),
                          want.view(np.int32))


def test_rank_slice_int32_keys_and_collections(cols):
    a, B = 40, 64
    addend = np.arange(1, 47, dtype=np.int64) * 1000
    pl, get = _decode(cols, a, B, rank=1, world=2, i64=False, groups=[["q", "r"], ["r"], ["t"]])
    lab = np.stack([cols[0][0]], 1).astype(np.float32)[a + 32:a + 64]
    assert np.array_equal(get(pl["label"][0], np.float32).reshape(32, 1), lab)
    ro, keys = po.ragged_param(cols[3:6], addend[:3], a, B)
    assert np.array_equal(get(pl["sparse"]["p"][0], np.int32), ro.astype(np.int32))
    assert np.array_equal(get(pl["sparse"]["p"][1], np.int32), keys.astype(np.int32))  # low 32 bits
    _, keys = po.ragged_param(cols[8:48], addend[5:45], a, B)
    assert np.array_equal(get(pl["sparse"]["s"][1], np.int32), keys.astype(np.int32))
    for (o_k, o_br, n), names in zip(pl["ebc"], ([6, 7], [7], [48])):
        keys, br = po.group([cols[i] for i in names], a, B)
        assert np.array_equal(get(o_k, np.int64), keys)     # raw keys, feature-major
        if o_br is None:  # a collection of scalar lookups: its bucket range is arange
            assert names == [48] and np.array_equal(br, np.arange(B + 1))
        else:
            assert np.array_equal(get(o_br, np.int64), br)


def test_more_items_than_workgroups():
    """more work items than workgroups: the grid is capped, further items are grid-strided"""
    from hugectr_amd import _lib
    B = 64 * 260 + 5
    cols = _file(np.random.default_rng(2), B)
    pl, get = _decode(cols, 0, B, mean_keys={"p": 36.0, "q": 2.5, "r": 0.5})
    assert pl["n_items"] > _lib.PQ_DECODE_MAX_BLOCKS
    lab = cols[0][0].astype(np.float32)
    assert np.array_equal(get(pl["label"][0], np.float32), lab)
    ro = np.zeros(B * 3 + 1, np.int64)
    lens = np.stack([np.ones(B, np.int64), np.diff(cols[4][1]), np.diff(cols[5][1])], 1).reshape(-1)
    np.cumsum(lens, out=ro[1:])
    assert np.array_equal(get(pl["sparse"]["p"][0], np.int64), ro)
    got = get(pl["sparse"]["s"][1], np.int64).reshape(B, 40)
    want = np.stack([c[0] for c in cols[8:48]], 1) + np.arange(6, 46, dtype=np.int64) * 1000
    assert np.array_equal(got, want)


def test_argument_checks():
    from hugectr_amd import _lib
    L = _lib.lib
    p = ctypes.c_void_p(4096)
    ok = (p, p, 3, p, 2, 4, 5, 100, 0, 32, p, p, 3, None)

    def call(**kw):
        names = ("slot", "columns", "n_columns", "plan", "n_segments", "n_list", "n_items", "rows",
                 "first_row", "batch", "out_base", "out_offsets", "n_outputs", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return L.hctr_parquet_decode(*[args[n] for n in names])

    assert call(slot=None) == -1 and "null" in _lib.last_error()
    assert call(out_offsets=None) == -1 and "null" in _lib.last_error()
    assert call(batch=0) == -1 and "batch" in _lib.last_error()
    assert call(first_row=80) == -1 and "inside the file" in _lib.last_error()
    assert call(n_columns=0) == -1 and "n_columns" in _lib.last_error()
    assert call(n_segments=0) == -1 and "n_segments" in _lib.last_error()
    assert call(n_segments=4097) == -1 and "n_segments" in _lib.last_error()
    assert call(n_list=0) == -1 and "n_list" in _lib.last_error()
    assert call(n_items=0) == -1 and "n_items" in _lib.last_error()
    assert call(n_outputs=0) == -1 and "n_outputs" in _lib.last_error()
    assert call(plan=ctypes.c_void_p(4100)) == -1 and "aligned" in _lib.last_error()
