"""CPU: the Raw reader on a CPU device keeps decoding on the host (the batches computed here as
tests/test_api_cpu.py does), and the plan the device path hands to hctr_raw_decode lists the
expected segments (a host check of the plan builder; no kernel runs)."""
import numpy as np
import pytest
import torch


def _inp(hugectr, L, Dn, params):
    return hugectr.Input(label_dim=L, label_name="label", dense_dim=Dn, dense_name="dense",
                         data_reader_sparse_param_array=[
                             hugectr.DataReaderSparseParam(n, h, True, s) for n, h, s in params])


@pytest.mark.parametrize("float_ld", [True, False])
def test_cpu_device_decodes_on_the_host(tmp_path, float_ld):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import data
    rng = np.random.default_rng(1)
    n, L, Dn = 300, 1, 3
    hot, sizes = [2, 1, 3], [40, 9, 100]
    label = rng.integers(0, 2, size=(n, L))
    dense = rng.integers(0, 50, size=(n, Dn)) if not float_ld else rng.random((n, Dn))
    cats = np.concatenate([rng.integers(0, v, size=(n, h)) for v, h in zip(sizes, hot)], axis=1)
    path = str(tmp_path / "train.bin")
    data.write_raw(path, label, dense, cats, float_label_dense=float_ld)
    inp = _inp(hugectr, L, Dn, [("wide", [2, 1], 2), ("deep", 3, 1)])
    ap = hugectr.AsyncParam(num_threads=3, num_batches_per_thread=4, multi_hot_reader=False)
    r = data.RawReader(path, inp, sizes, 64, 1, 2, torch.device("cpu"), 0, float_ld, False, ap)
    r.ebc_groups = [["deep"]]
    assert r.stats() == {"decode": "host", "ring": 0, "threads": 0, "batches": 0, "wait_ms": 0.0}
    nb = 0
    while True:
        b = r.next_batch()
        if b is None:
            break
        a = nb * 64
        ro, keys = b["sparse"]["wide"]
        assert ro.tolist() == np.concatenate([[0], np.cumsum(np.tile([2, 1], 64))]).tolist()
        assert (keys.view(64, 3).numpy() == cats[a:a + 64, :3] + np.array([0, 0, 40])).all()
        ro2, keys2 = b["sparse"]["deep"]
        assert ro2.tolist() == list(range(0, 64 * 3 + 1, 3))
        assert (keys2.view(64, 3).numpy() == cats[a:a + 64, 3:] + 49).all()
        gk, gbr = b["ebc"][0]   # the collection's CSR: raw keys, bucket = lookup * batch + sample
        assert (gk.view(64, 3).numpy() == cats[a:a + 64, 3:]).all()
        assert gbr.tolist() == list(range(0, 64 * 3 + 1, 3))
        want_d = (dense[a + 32:a + 64].astype(np.float32) if float_ld else
                  np.log(dense[a + 32:a + 64].astype(np.float32) + np.float32(1.0)))
        assert (b["dense"].numpy().view(np.uint32) == want_d.view(np.uint32)).all()
        assert (b["label"].numpy() == label[a + 32:a + 64]).all()     # rank 1 of 2
        nb += 1
    assert nb == 4  # 300 // 64, tail dropped
    assert r.stats()["batches"] == 4 and r.stats()["decode"] == "host"
    r.close()
    r.close()


def test_plan_lists_the_expected_segments(tmp_path):
    import hugectr_amd.hugectr as hugectr
    from hugectr_amd import _lib, data
    L, Dn, B = 2, 3, 64
    sizes = [1 << 31, 1 << 31, 1 << 31, 5]
    params = [("wide", [2, 1], 2), ("a", 4, 1), ("b", 1, 1)]
    path = str(tmp_path / "train.bin")
    np.zeros((B, L + Dn + 8), "<u4").tofile(path)
    ap = hugectr.AsyncParam(num_threads=1, num_batches_per_thread=2, multi_hot_reader=True,
                            is_dense_float=False)
    r = data.RawReader(path, _inp(hugectr, L, Dn, params), sizes, B, 3, 4, torch.device("cpu"), 0,
                       True, False, ap, i64_key=False)
    r.ebc_groups = [["b", "a"]]
    pl = r.decode_plan()
    assert pl["width"] == 13
    assert pl["addend"].tolist() == [0] * 5 + [0, 0, 1 << 31] + [1 << 32] * 4 + [3 << 31]
    segs = [tuple(int(g[f]) for f in ("col0", "ncols", "kind", "sample0", "sample1", "dst_offset"))
            for g in pl["segments"]]
    up = lambda x: (x + 255) & ~255
    o_label = 0
    o_dense = up(16 * 2 * 4)
    o_wide = o_dense + up(16 * 3 * 4)
    o_a = o_wide + up(B * 3 * 4)
    o_b = o_a + up(B * 4 * 4)
    o_grp = o_b + up(B * 1 * 4)
    assert segs == [
        (0, 2, _lib.RAW_I2F, 48, 64, o_label),          # rank 3 of 4: samples 48..63
        (2, 3, _lib.RAW_LOG1P, 48, 64, o_dense),
        (5, 3, _lib.RAW_KEY_I32, 0, B, o_wide),
        (8, 4, _lib.RAW_KEY_I32, 0, B, o_a),
        (12, 1, _lib.RAW_KEY_I32, 0, B, o_b),
        (12, 1, _lib.RAW_RAWKEY_I64, 0, B, o_grp),      # lookup 0 of the group is input "b"
        (8, 4, _lib.RAW_RAWKEY_I64, 0, B, o_grp + B * 8),
    ]
    assert pl["label"] == (o_label, (16, 2)) and pl["dense"] == (o_dense, (16, 3))
    assert pl["sparse"] == {"wide": (o_wide, B * 3), "a": (o_a, B * 4), "b": (o_b, B)}
    assert pl["ebc"] == [(o_grp, B * 5)]
    assert pl["arena_bytes"] == o_grp + up(B * 5 * 8)
    assert pl["segments"].dtype.itemsize == 40   # sizeof(hctr_raw_segment)
    # float conventions, int64 keys, no dense features: a bit copy, 8-byte keys, no dense segment
    r2 = data.RawReader(path, _inp(hugectr, 13, 0, []), [], B, 0, 1, torch.device("cpu"), 0, True,
                        False)
    p2 = r2.decode_plan()
    assert [(int(g["col0"]), int(g["ncols"]), int(g["kind"])) for g in p2["segments"]] == \
        [(0, 13, _lib.RAW_BITS)]
    assert p2["dense"][1] == (B, 0)
