"""The asynchronous Parquet reader (hugectr_amd/data.py ParquetReader on a CUDA device): worker
threads stage whole files in pinned slots, one copy per file and one hctr_parquet_decode launch per
batch on a side stream.  The host reader (CPU device) over the same files is the oracle: every
tensor of every batch BIT FOR BIT, dtypes included."""
import numpy as np
import pytest
import torch

import parquet_oracle as po

pytestmark = pytest.mark.gpu

B = po.B
NB = sum(n // B for n in po.ROWS)   # 3 + 2 + 1 batches, three dropped tails
# the same columns with every categorical column a one-slot input, as a collection model has them
LOOKUPS = [("a0", 1), ("a1", 1), ("a2", 1), ("b", 1), ("c", 2)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return po.dataset(tmp_path_factory.mktemp("pq"))


def _readers(files, *, batch=B, rank=0, world=1, i64=True, repeat=False, params=po.PARAMS, **kw):
    from hugectr_amd import data
    return [data.ParquetReader(files, po.inp(params), po.SIZES, batch, rank, world, dev, i64, repeat,
                               **(kw if dev == "cuda" else {}))
            for dev in ("cuda", "cpu")]


def _epoch(dev, host, n):
    kept = [dev.next_batch() for _ in range(n)]   # all kept alive: nothing may be reused too early
    for got in kept:
        po.assert_same(got, host.next_batch())


def test_whole_epoch_then_none(files):
    dev, host = _readers(files)
    st = dev.stats()
    assert (st["decode"], st["ring"], st["threads"]) == ("device", 2, 2)
    _epoch(dev, host, NB)
    assert dev.next_batch() is None and dev.next_batch() is None and host.next_batch() is None
    st = dev.stats()
    assert st["batches"] == NB and st["files"] == 3 and st["wait_ms"] >= 0.0
    assert set(st) == {"decode", "ring", "threads", "batches", "files", "wait_ms"}
    dev.close()


def test_repeat_wraps(files):
    dev, host = _readers(files, repeat=True, ring=4, num_workers=3)
    assert (dev.stats()["ring"], dev.stats()["threads"]) == (4, 3)
    _epoch(dev, host, NB + 2)
    dev.close()


@pytest.mark.parametrize("rank", [0, 1])
def test_rank_slices(files, rank):
    dev, host = _readers(files, rank=rank, world=2)
    got = dev.next_batch()
    assert got["label"].shape == (B // 2, 2) and got["dense"].shape == (B // 2, 3)
    po.assert_same(got, host.next_batch())
    _epoch(dev, host, NB - 1)
    dev.close()


def test_int32_keys(files):
    dev, host = _readers(files, i64=False)
    got = dev.next_batch()
    assert got["sparse"]["a"][0].dtype == got["sparse"]["a"][1].dtype == torch.int32
    po.assert_same(got, host.next_batch())
    _epoch(dev, host, NB - 1)
    dev.close()


def test_groups_assigned_after_the_first_batch(files):
    """Model.compile names the collections after the reader exists: the plan is rebuilt and the
    batches in flight are read again"""
    dev, host = _readers(files, params=LOOKUPS)
    po.assert_same(dev.next_batch(), host.next_batch())
    for r in (dev, host):
        r.ebc_groups = [["b"], ["a1", "a2"]]
    for _ in range(NB - 1):
        got, want = dev.next_batch(), host.next_batch()
        assert len(got["ebc"]) == 2
        po.assert_same(got, want)
    assert dev.next_batch() is None and host.next_batch() is None
    dev.close()


@pytest.mark.parametrize("batch", [1, 33])
def test_partial_tiles(files, batch):
    dev, host = _readers(files, batch=batch)
    for _ in range(4):
        po.assert_same(dev.next_batch(), host.next_batch())
    dev.close()


def test_string_column_takes_the_host_path(tmp_path):
    import pyarrow as pa
    rng = np.random.default_rng(3)
    t = po.table(rng, 70)
    i = t.schema.get_field_index("b0")
    t = t.set_column(i, "b0", pa.array([str(v) for v in rng.integers(0, 1000, size=70)],
                                       type=pa.string()))
    files = po.write_dataset(tmp_path, [t])
    dev, host = _readers(str(files))
    assert dev.stats()["decode"] == "host" and dev.stats()["ring"] == 0
    for _ in range(2):
        got = dev.next_batch()
        assert got["label"].is_cuda
        po.assert_same(got, host.next_batch())
    assert dev.next_batch() is None


def test_null_is_an_error_naming_the_column(tmp_path):
    import pyarrow as pa
    rng = np.random.default_rng(4)
    t = po.table(rng, 70)
    vals = rng.integers(0, 1000, size=70).tolist()
    vals[40] = None
    t = t.set_column(t.schema.get_field_index("c1"), "c1", pa.array(vals, type=pa.int64()))
    dev, _ = _readers(str(po.write_dataset(tmp_path, [t])))
    assert dev.stats()["decode"] == "device"
    with pytest.raises(RuntimeError, match=r"part_0\.parquet.*c1"):
        dev.next_batch()
    dev.close()


def test_cache_batches(files):
    dev, host = _readers(files, repeat=True, cache_batches=2)
    want = [host.next_batch() for _ in range(2)]
    got = [dev.next_batch() for _ in range(5)]
    n_files = dev.stats()["files"]
    for i, g in enumerate(got):
        po.assert_same(g, want[i % 2])
        assert g["label"].data_ptr() == got[i % 2]["label"].data_ptr()
        assert g["sparse"]["a"][1].data_ptr() == got[i % 2]["sparse"]["a"][1].data_ptr()
    for _ in range(4):
        dev.next_batch()
    assert dev.stats()["files"] == n_files and dev.stats()["batches"] == 9
    dev.close()
