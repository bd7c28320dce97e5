"""CPU: the host-side halves of the Parquet reader's device path (hugectr_amd/reader_parquet.py) --
the plan hctr_parquet_decode gets, the staging of a chunked file into a file slot -- as pure numpy against
pq.read_table(...).combine_chunks(); and what the reader does on every device: decode="host",
cache_batches, stats(), the schema check, close()."""
import gc
import threading

import numpy as np
import pytest
import torch

import parquet_oracle as po

B = po.B


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return po.dataset(tmp_path_factory.mktemp("pq"))


def _columns():
    from hugectr_amd import _lib
    F32, F64, I32, I64 = _lib.PQ_F32, _lib.PQ_F64, _lib.PQ_I32, _lib.PQ_I64
    return [(I64, 8, False), (F32, 4, False),                       # labels
            (F32, 4, False), (F64, 8, False), (I64, 8, False),      # dense
            (I32, 4, False), (I64, 8, True), (I32, 4, True),        # a
            (I64, 8, False), (I64, 8, False), (I64, 8, False)]      # b, c


def test_accepted_physical_types():
    import pyarrow as pa
    from hugectr_amd import _lib, data
    assert data.parquet_physical(pa.float64(), False) == (_lib.PQ_F64, 8, False)
    assert data.parquet_physical(pa.int32(), False) == (_lib.PQ_I32, 4, False)
    assert data.parquet_physical(pa.large_list(pa.int32()), True) == (_lib.PQ_I32, 4, True)
    assert data.parquet_physical(pa.list_(pa.int64()), True) == (_lib.PQ_I64, 8, True)
    for t, cat in ((pa.float32(), True), (pa.list_(pa.int64()), False), (pa.string(), True),
                   (pa.int16(), True), (pa.list_(pa.float32()), True), (pa.uint32(), True)):
        assert data.parquet_physical(t, cat) is None


def test_plan_lists_every_output_once():
    from hugectr_amd import _lib, data
    offs = np.concatenate([[0], np.cumsum(po.SIZES)[:-1]])
    lookups = [("a0", 1), ("a1", 1), ("a2", 1), ("b", 1), ("c", 2)]
    pl = data.parquet_decode_plan(_columns(), 2, 3, lookups, [["b"], ["a1", "a2"]], offs, 64, 1, 2,
                                  True, {"a1": 35.0, "a2": 1.0})
    sg = pl["segments"]
    assert sg.dtype.itemsize == 48                      # sizeof(hctr_parquet_segment)
    assert np.dtype(_lib.PQ_COLUMN_FIELDS).itemsize == 24
    kinds = sg["kind"].tolist()
    T, R, G = _lib.PQ_SEG_TILE, _lib.PQ_SEG_RAGGED, _lib.PQ_SEG_GROUP
    assert kinds == [T, T, T, R, R, T, T, G, G, G]
    # label: int64 + float32 columns stack to float64 on the host; rank 1 of 2 -> samples 32..63
    assert sg[0]["out_kind"] == _lib.PQ_OUT_F32_VIA_F64
    assert (int(sg[0]["sample0"]), int(sg[0]["sample1"]), int(sg[0]["ncols"])) == (32, 64, 2)
    assert sg[2]["out_kind"] == _lib.PQ_OUT_KEY_I64 and int(sg[2]["sample1"]) == 64
    assert int(sg[3]["group"]) == 64 and int(sg[4]["group"]) == 1
    assert int(sg[3]["n_items"]) == 16 and int(sg[4]["n_items"]) == 1
    # work items count up without gaps
    assert sg["item0"].tolist() == np.concatenate([[0], np.cumsum(sg["n_items"])[:-1]]).tolist()
    assert pl["n_items"] == int(sg["n_items"].sum())
    # addends: the slot offsets of the params' columns, 0 for label / dense / collections
    lst, add = pl["list"].tolist(), pl["addend"].tolist()
    assert lst[:5] == [0, 1, 2, 3, 4] and add[:5] == [0] * 5
    assert lst[5:11] == [5, 6, 7, 8, 9, 10] and add[5:11] == offs.tolist()
    assert lst[11:] == [8, 6, 7] and add[11:] == [0, 0, 0]
    # outputs: static ones are absent (None): one-hot row offsets, the one-hot group's range
    assert pl["sparse"]["a0"][0] is None and pl["sparse"]["a1"][0] is not None
    assert pl["ebc"][0][1] is None and pl["ebc"][1][1] is not None
    outs = pl["outputs"]
    assert outs[pl["sparse"]["a1"][1]] == {"esize": 8, "const": 0, "cols": (6,)}
    assert outs[pl["ebc"][1][0]] == {"esize": 8, "const": 0, "cols": (6, 7)}
    assert outs[pl["ebc"][1][1]]["const"] == 2 * 64 + 1
    used = sorted(int(x) for x in np.concatenate([sg["out0"], sg["out1"]]) if x != _lib.PQ_NO_OUTPUT)
    assert sorted(set(used)) == list(range(len(outs)))
    # int32 keys; pure integer dense columns need no detour through float64
    cols = _columns()
    cols[2] = cols[3] = cols[4]
    pl = data.parquet_decode_plan(cols, 2, 3, po.PARAMS, [], offs, 64, 0, 1, False)
    assert pl["segments"][1]["out_kind"] == _lib.PQ_OUT_F32
    assert pl["segments"][2]["out_kind"] == _lib.PQ_OUT_KEY_I32
    assert pl["outputs"][pl["sparse"]["a"][0]] == {"esize": 4, "const": 64 * 3 + 1, "cols": ()}
    assert pl["outputs"][pl["sparse"]["a"][1]] == {"esize": 4, "const": 64, "cols": (6, 7)}


def test_staging_of_a_chunked_file(files):
    """rebased offsets, values and descriptor table against combine_chunks()"""
    import pyarrow.parquet as pq
    from hugectr_amd import _lib, data, reader_parquet
    path = open(files).read().split()[1]
    names = po.LABELS + po.CONTS + po.CATS
    offs = np.concatenate([[0], np.cumsum(po.SIZES)[:-1]])
    pl = data.parquet_decode_plan(_columns(), 2, 3, po.PARAMS, [], offs, B, 0, 1, True)
    spec = {"names": names, "cats": tuple(po.CATS), "columns": _columns(), "batch": B,
            "outputs": pl["outputs"]}
    t = pq.read_table(path, columns=names, use_threads=False)
    assert t.column("a1").num_chunks == 5, "the fixture must arrive in several chunks"
    _, rows, nv = reader_parquet._parquet_file_info(path)
    bound = data.parquet_slot_layout(_columns(), len(pl["outputs"]), B, rows,
                                     [nv[n] for n in names])[2]
    buf = np.full(bound, 0xAB, np.uint8)
    res = data.stage_parquet_table(t, path, spec, buf)
    assert res["rows"] == 100 and res["nb"] == 3 and res["used"] <= bound
    desc = buf[:24 * len(names)].view(np.dtype(_lib.PQ_COLUMN_FIELDS))
    whole = t.combine_chunks()
    for i, n in enumerate(names):
        pt, esz, is_list = _columns()[i]
        arr = whole.column(n).chunk(0)
        assert (int(desc[i]["ptype"]), int(desc[i]["esize"])) == (pt, esz)
        assert int(desc[i]["values"]) % 8 == 0
        dt = reader_parquet._pq_numpy(pt)
        if is_list:
            o = arr.offsets.to_numpy().astype(np.int64)
            want = arr.values.to_numpy()[o[0]:o[-1]]
            got_o = buf[int(desc[i]["offsets"]):][:(rows + 1) * 8].view(np.int64)
            assert np.array_equal(got_o, o - o[0]), n
        else:
            want = arr.to_numpy()
            assert int(desc[i]["offsets"]) == _lib.PQ_NO_OFFSETS
        got = buf[int(desc[i]["values"]):][:len(want) * esz].view(dt)
        assert got.dtype == want.dtype and np.array_equal(got, want), n
    # the per-batch table: sizes from the offsets, every output on a 256-byte boundary
    tab = buf[res["tab_off"]:][:res["tab"].nbytes].view(np.int64).reshape(res["tab"].shape)
    assert np.array_equal(tab, res["tab"]) and (tab % 256 == 0).all()
    o1 = whole.column("a1").chunk(0).offsets.to_numpy().astype(np.int64)
    o2 = whole.column("a2").chunk(0).offsets.to_numpy().astype(np.int64)
    k = pl["sparse"]["a"][1]
    for b in range(3):
        n = B + (o1[(b + 1) * B] - o1[b * B]) + (o2[(b + 1) * B] - o2[b * B])
        assert res["cnt"][b, k] == n
        assert tab[b, k + 1] - tab[b, k] == (n * 8 + 255) // 256 * 256
    with pytest.raises(RuntimeError, match="file slot"):
        data.stage_parquet_table(t, path, spec, buf[:res["used"] - 64])


def _host(files, **kw):
    from hugectr_amd import data
    return data.ParquetReader(files, po.inp(), po.SIZES, B, 0, 1, torch.device("cpu"), True,
                              kw.pop("repeat", False), **kw)


def test_host_decode_cache_and_stats(files):
    r = _host(files, decode="host", cache_batches=2, repeat=True, num_workers=5, ring=3)
    plain = _host(files, repeat=True)
    want = [plain.next_batch() for _ in range(2)]
    got = [r.next_batch() for _ in range(5)]
    for i, g in enumerate(got):
        po.assert_same(g, want[i % 2])
        assert g is got[i % 2]
    st = r.stats()
    assert st == {"decode": "host", "ring": 0, "threads": 0, "batches": 5, "files": 1,
                  "wait_ms": 0.0}
    # N = 0: every batch is fresh, the epoch ends with None
    plain = _host(files)
    n = 0
    while plain.next_batch() is not None:
        n += 1
    assert n == 6 and plain.stats()["files"] == 3 and plain.stats()["batches"] == 6
    with pytest.raises(ValueError):
        _host(files, decode="gpu")
    with pytest.raises(RuntimeError, match="CUDA"):
        _host(files, decode="device")


def test_schema_check_chooses_the_host_path(files, tmp_path):
    """_check_schemas reads footers only; a string column, or files that disagree, decline"""
    import pyarrow as pa
    r = _host(files)
    assert r._check_schemas() is True
    assert r._file_rows == [100, 64, 37]
    assert r._columns == _columns()
    rng = np.random.default_rng(1)
    t = po.table(rng, 40)
    s = t.set_column(t.schema.get_field_index("b0"), "b0",
                     pa.array([str(i) for i in range(40)], type=pa.string()))
    assert _host(po.write_dataset(tmp_path / "s", [s]))._check_schemas() is False
    w = t.set_column(t.schema.get_field_index("c0"), "c0",
                     pa.array(np.arange(40, dtype=np.int32), type=pa.int32()))
    assert _host(po.write_dataset(tmp_path / "w", [w]))._check_schemas() is True
    assert _host(po.write_dataset(tmp_path / "m", [t, w]))._check_schemas() is False


def test_close_twice_and_dropped_readers_leave_no_threads(files):
    from hugectr_amd import reader_parquet, reader_prefetch
    r = _host(files)
    r.next_batch()
    r.close()
    r.close()
    with pytest.raises(RuntimeError):
        r.next_batch()
    # the staging workers hold no reference to their reader: they end with their queue
    import functools
    import queue
    tasks = queue.Queue()
    th = threading.Thread(target=reader_prefetch._worker, args=(tasks,), daemon=True,
                          name="hctr-parquet-stage-test")
    th.start()
    latch = reader_prefetch._Latch(1)
    tasks.put((functools.partial(reader_parquet._stage_file, np.zeros(16, np.uint8),
                                 "/nonexistent.parquet", {"names": []}), None, latch))
    latch.done.wait()
    assert latch.error is not None        # (handed to next_batch(), the worker lives on)
    tasks.put(None)
    th.join()
    r = _host(files)
    del r
    gc.collect()
    assert not [t for t in threading.enumerate() if t.name.startswith("hctr-parquet-stage")]


def test_make_reader_passes_workers_and_cache(files):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import data
    rp = hugectr.DataReaderParams(data_reader_type=hugectr.DataReaderType_t.Parquet, source=[files],
                                  eval_source=files, check_type=hugectr.Check_t.Non,
                                  slot_size_array=po.SIZES, num_workers=3, cache_eval_data=2)
    solver = hugectr.CreateSolver(batchsize=B, batchsize_eval=B, vvgpu=[[0]], repeat_dataset=True,
                                  i64_input_key=True)
    rd = data.make_reader(rp, po.inp(), solver, 0, 1, torch.device("cpu"))
    assert rd.train._cache_n == 0 and rd.evalr._cache_n == 2
    assert rd.train._workers == 2 and rd.evalr._workers == 2      # min(ring, num_workers, 8)
    e = [rd.evalr.next_batch() for _ in range(4)]
    assert e[2] is e[0] and e[3] is e[1] and rd.evalr.stats()["files"] == 1
