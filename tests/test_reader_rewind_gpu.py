"""What the readers' shared prefetch pipeline (hugectr_amd/reader_prefetch.py) carries alone: the
rewind when ebc_groups is assigned in mid-stream, a worker's error on its way to the caller, and the
refusal after close().  The host reader of the same format, given the same assignments at the same
points, is the oracle: every batch bit for bit, so no sample is skipped or served twice."""
import threading

import pytest
import torch

import parquet_oracle as po
import test_parquet_decode_gpu as pq_t
import test_raw_reader_async_gpu as raw_t

pytestmark = pytest.mark.gpu

RAW_NB = 7
RAW_REGROUP = [["b"], ["a"]]                    # raw_t.GROUPS is [["a", "b"]]
PQ_GROUPS = [["b"], ["a1", "a2"]]
PQ_REGROUP = [["a2", "a0"], ["a1", "b"]]        # the one-slot inputs of pq_t.LOOKUPS are a0 a1 a2 b


def _regroup_in_mid_stream(dev, host, groups, regroup, same, nb):
    for r in (dev, host):
        r.ebc_groups = groups
    early = [(dev.next_batch(), host.next_batch()) for _ in range(3)]
    for got, want in early:
        same(got, want)
    for r in (dev, host):
        r.ebc_groups = regroup
    n = 3
    while True:
        got, want = dev.next_batch(), host.next_batch()
        if want is None:
            break
        assert len(got["ebc"]) == len(regroup)
        same(got, want)
        n += 1
    assert got is None and n == nb, "every batch of the epoch once, none twice"
    torch.cuda.synchronize()
    for got, want in early:   # kept alive over the rewind: the old plan's batches are untouched
        assert len(got["ebc"]) == len(groups)
        same(got, want)
    dev.close()


# Raw: the ring is num_batches_per_thread, at least 2 and not bounded above; 8 slots hold the
# whole file, so at the regroup every batch still to come is in flight
@pytest.mark.parametrize("ring", [2, 8])
def test_raw_regroup_in_mid_stream(tmp_path, ring):
    import hugectr_amd.hugectr as hugectr
    path = raw_t._write(tmp_path / "train.bin", RAW_NB * raw_t.B + raw_t.B // 2)
    ap = hugectr.AsyncParam(num_threads=2, num_batches_per_thread=ring, multi_hot_reader=False)
    dev, host = raw_t._readers(path, ap=ap)
    assert dev.stats()["ring"] == ring
    _regroup_in_mid_stream(dev, host, raw_t.GROUPS, RAW_REGROUP, raw_t._assert_same, RAW_NB)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return po.dataset(tmp_path_factory.mktemp("pq"))


@pytest.mark.parametrize("ring", [2, 4])
def test_parquet_regroup_in_mid_stream(files, ring):
    dev, host = pq_t._readers(files, params=pq_t.LOOKUPS, ring=ring)
    assert dev.stats()["ring"] == ring
    _regroup_in_mid_stream(dev, host, PQ_GROUPS, PQ_REGROUP, po.assert_same, pq_t.NB)


def test_parquet_regroup_rebuilds_the_cache(files):
    """an eval-style reader (repeat, cache_batches=2): the regroup drops the kept batches; the
    next two are read from the first batch that was not handed out and then served for ever"""
    dev, host = pq_t._readers(files, params=pq_t.LOOKUPS, repeat=True, cache_batches=2)
    for r in (dev, host):
        r.ebc_groups = PQ_GROUPS
    want = [host.next_batch() for _ in range(2)]
    early = [dev.next_batch() for _ in range(3)]
    assert early[2] is early[0]
    for r in (dev, host):
        r.ebc_groups = PQ_REGROUP
    want2 = [host.next_batch() for _ in range(2)]   # (the host reader here keeps nothing)
    got = [dev.next_batch() for _ in range(5)]
    for i, g in enumerate(got):
        assert g is got[i % 2]
        po.assert_same(g, want2[i % 2])
    for i, g in enumerate(early):
        po.assert_same(g, want[i % 2])
    dev.close()


def test_a_workers_error_reaches_the_caller(files, tmp_path):
    import pyarrow.parquet as pq
    broken = tmp_path / "part_1.parquet"
    broken.write_bytes(b"not a parquet file " * 40)
    with pytest.raises(Exception) as want:
        pq.read_table(str(broken))
    dev, host = pq_t._readers(files)
    dev.files[1] = str(broken)                      # (the footers were read by the constructor)
    for _ in range(po.ROWS[0] // po.B):
        po.assert_same(dev.next_batch(), host.next_batch())
    with pytest.raises(type(want.value)) as got:
        dev.next_batch()
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    dev.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("hctr-parquet-stage")]


def test_next_batch_after_close_is_refused(files, tmp_path):
    path = raw_t._write(tmp_path / "train.bin", 3 * raw_t.B)
    # (the Raw reader's host path used to go on after close(): the one line of this file that
    # does not hold on the commit before the readers shared their pipeline)
    for r in (*raw_t._readers(path, repeat=True), *pq_t._readers(files, repeat=True)):
        assert r.next_batch() is not None
        r.close()
        with pytest.raises(RuntimeError, match="after close"):
            r.next_batch()
