"""numpy statement of the owner-side plan of CompressionStrategy.Unique (hctr_ebc_uniq_plan): what
tests/test_ebc_unique_gpu.py compares the kernels with.  Nothing here calls the library."""
import numpy as np


def plan(bucket_range, rows, world, buckets_per_peer):
    """routed CSR (buckets [peer][local lookup][b_local], so a peer's keys are one range) and the
    row of every key -> (urow uint64: per peer its distinct rows ascending, peers in order;
    peer_off int64 [world + 1]; ridx uint32 [keys]: index of key j's row inside its peer's list)"""
    bucket_range = np.asarray(bucket_range, np.int64)
    rows = np.asarray(rows, np.uint64)
    key_off = bucket_range[::buckets_per_peer] if buckets_per_peer else np.zeros(world + 1, np.int64)
    assert key_off.size == world + 1
    urow, peer_off = [], [0]
    ridx = np.zeros(int(key_off[-1]), np.uint32)
    for p in range(world):
        seg = rows[key_off[p]:key_off[p + 1]]
        u, inv = np.unique(seg, return_inverse=True)
        urow.append(u)
        ridx[key_off[p]:key_off[p + 1]] = inv
        peer_off.append(peer_off[-1] + u.size)
    return (np.concatenate(urow) if urow else np.zeros(0, np.uint64)), \
        np.asarray(peer_off, np.int64), ridx


def pool(rows_by_shard, count, average):
    """the receiver's arithmetic for one bucket, before the ONE rounding to the output type: per
    shard (ascending) the fp32 sum of its rows in key order -- the rows as they travelled, i.e.
    already rounded to the vector type, given here as fp32 --, the shards' partials added in shard
    order, divided by the bucket's total key count for Average"""
    acc = np.float32(0)
    for rows in rows_by_shard:
        part = np.zeros(rows.shape[1], np.float32)
        for r in rows:
            part = part + r.astype(np.float32)
        acc = acc + part
    if average and count > 0:
        acc = acc / np.float32(count)
    return np.asarray(acc, np.float32)
