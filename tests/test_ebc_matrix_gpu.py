"""Every dispatch branch of the embedding_collection operators (hugectr_amd/csrc/ebc.hip) through the
C ABI, against plain numpy written in this file: hctr_ebc_route_keys, hctr_ebc_route_whole,
hctr_ebc_routed_keys_to_indices, hctr_ebc_bucket_counts, hctr_ebc_network_forward / _backward,
hctr_ebc_scale_average, hctr_static_lookup and hctr_ebc_local_reduce.

Every call writes into a poisoned buffer (floats: NaN, integers: all ones) with GUARD rows behind
the last real row that must still hold the poison afterwards, and its inputs must come back
unchanged.  Integer outputs must be equal.  The floating outputs of the network / scale operators
are ONE fp32 sum taken in slot order, ONE fp32 division, ONE rounding to the vector type (numpy for
fp16, torch on the CPU for bf16) and must be bit-equal; the sums of the local reduce go against fp64
within the bound of any order of fp32 additions (_sum_bound).

Two properties of the network kernels that the cases state rather than discover:
  * a lookup whose block-table row is all -1 gets ZEROS from the forward, from the scalar and from
    the vec kernel alike (the backward writes nothing for it);
  * the inputs hold no negative zero: the vec kernel's plain-move branch (one live shard, divisor 1)
    keeps a zero's sign, the summing branches (0.f + x) do not.  Known, and not worth a slower move.

Grid-stride loops.  All launches use kBlock = 256 threads and at most kMaxGrid = 2048 blocks
(common.h) unless the launch names another cap: 8192 for ebc_network_vec_kernel and
ebc_scale_average_kernel, 4096 for lr_flags_kernel / lr_emit_kernel; the scan (scan.h) gives one
tile of kTile = 1024 lengths to a block, at most 2048 blocks, and its middle kernel walks the tile
sums 1024 at a time in a single block.  for_each_key_wave (block_prims.h) gives 64 buckets to a
wavefront: 2048 blocks x 4 wavefronts x 64.  The cases marked "grid" run two full passes and a
partial third:

  kernel                                     one pass covers         case that exceeds it
  ebc_count_kernel / ebc_index_kernel        2048 * 256 =   524288   test_route_keys_grid[count-index], nb = 1048613
  tile_sum_kernel / tile_downsweep_kernel    2048 * 1024 = 2097152   test_route_keys_grid[scan-tiles], nb = 4194341
  scan_tiles_u64_kernel (one trip)           1024 tiles =  1048576   test_route_keys_grid[count-index] (1025 tiles),
                                                                     [scan-tiles] (4097 tiles)
  ebc_route_whole_kernel (thread loop)       2048 * 256 =   524288   test_route_whole_grid, nb = 1048613
  ebc_route_whole_kernel (wave loop)         2048 * 4 * 64 = 524288  test_route_whole_grid, nb = 1048613
  ebc_routed_keys_to_indices_kernel          2048 * 256 =   524288   test_routed_keys_to_indices_grid, nb = 1048613
  ebc_bucket_count_kernel                    2048 * 256 =   524288   test_bucket_counts_grid, 1048613 counts
  ebc_network_vec_kernel                     8192 * 256 =  2097152   test_network_grid[vec], 4198400 16-byte units
  ebc_network_kernel                         2048 * 256 =   524288   test_network_grid[scalar], 1080000 elements
  ebc_scale_average_kernel                   8192 * 256 =  2097152   test_scale_average_grid, 4198400 elements
  static_lookup_kernel                       2048 * 256 =   524288   test_static_lookup_grid, 1048613 keys
  lr_expand_kernel (wave loop)               2048 * 4 * 64 = 524288  test_local_reduce_grid, 1048614 buckets
  lr_flags_kernel / lr_emit_kernel           4096 * 256 =  1048576   test_local_reduce_grid, 2097228 positions

Under HCTR_EMU=1 (the host interpreter of tests/emu) the grid cases are dropped; every other case
runs there, the 64-bit sort of the local reduce through the interpreter's host stand-in for the
library call."""
import ctypes
import functools
import os

import numpy as np
import pytest

from util import DevIn as _In, DevOut as _Out, assert_bits as _assert_bits, lib_code as _code

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
U = 2.0 ** -24  # unit roundoff of fp32
DTYPES = ["f32", "f16", "bf16"]
EDGES = [1, 255, 256, 257]                    # work items around one workgroup
SCAN_EDGES = EDGES + [1023, 1024, 1025, 2049]  # ... and around one / two tiles of the scan
GRID_NB = 2 * 2048 * 256 + 37                 # = 2 * 2048 * 4 * 64 + 37


def _grid(cases):
    return [] if EMU else cases


# ---- plumbing ------------------------------------------------------------------------------------
def _lib():
    from hugectr_amd import _lib
    return _lib


def _ktype(kt):
    return _lib().KEY_U32 if kt == "u32" else _lib().KEY_I64


def _knp(kt):
    return np.uint32 if kt == "u32" else np.int64


def _iout(rows, dt="i64"):
    """integer output of `rows` elements behind the all-ones poison"""
    return _Out(rows, 1, dt)


def _ires(out):
    return out.result().reshape(-1)


def _round(x, dt):
    """fp32 -> the value the vector type holds (round to nearest even), as fp32"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dt == "f32":
        return x
    if dt == "f16":
        return x.astype(np.float16).astype(np.float32)
    import torch
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def _as_type(x, dt):
    """fp32 values exact in dt -> the host array whose bytes the device reads"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dt == "f32":
        return x
    if dt == "f16":
        return x.astype(np.float16)
    return (x.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def _vals(n, dt, seed):
    """n values exact in dt, no negative zero, never written again (the small ones are shared)"""
    return (_vals_cached if n <= 1 << 20 else _vals_new)(n, dt, seed)


def _vals_new(n, dt, seed):
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32) * 3
    x = _round(x, dt) + np.float32(0)  # (-0 + +0 = +0)
    assert not np.signbit(x[x == 0]).any()
    x.setflags(write=False)
    return x


_vals_cached = functools.lru_cache(maxsize=None)(_vals_new)


def _unchanged(*pairs):
    for x, name in pairs:
        if x is not None:
            x.assert_unchanged(name)


# ---- 1. hctr_ebc_route_keys ------------------------------------------------------------------------
def _expand(starts, lens):
    """the key positions of buckets (starts, lens), in bucket order -> (position, bucket of it)"""
    which = np.repeat(np.arange(lens.size), lens)
    first = np.cumsum(lens) - lens
    return starts[which] + (np.arange(int(lens.sum())) - first[which]), which


def _route_ref(batch, world, desc, rs, keys, br):
    """output bucket ob = [peer][local lookup][b_local] holds the keys of input bucket
    [global lookup][peer * bpg + b_local] that this shard owns (key % num_shards == shard_id), each
    as row_start + key / num_shards (row_start < 0: the key itself) -> (out_range, out_indices)"""
    n_local, bpg = len(desc), batch // world
    nb = n_local * batch
    ob = np.arange(nb)
    ll = (ob // bpg) % n_local
    sb = desc[ll, 0] * batch + (ob // bpg // n_local) * bpg + ob % bpg
    br = br.astype(np.int64)
    pos, which = _expand(br[sb], br[sb + 1] - br[sb])
    k = keys[pos].astype(np.int64)
    lk = ll[which]
    ns, r0 = desc[lk, 1], rs[lk]
    keep = k % ns == desc[lk, 2]
    out_range = np.zeros(nb + 1, np.int64)
    np.cumsum(np.bincount(which[keep], minlength=nb), out=out_range[1:])
    return out_range, np.where(r0 < 0, k, r0 + k // ns)[keep]


def _route_keys_case(batch, world, desc, rs, keys_h, br_h, kt):
    L = _lib()
    desc = np.asarray(desc, np.int32).reshape(-1, 3)
    rs = np.asarray(rs, np.int64)
    n_local = len(desc)
    nb = n_local * batch
    want_range, want_idx = _route_ref(batch, world, desc, rs, keys_h, br_h) if n_local else \
        (np.zeros(1, np.int64), np.zeros(0, np.int64))
    nnz = want_idx.size
    d3, d_rs = _In(desc if n_local else np.zeros(3, np.int32)), _In(rs if n_local else [0])
    keys = _In(keys_h.astype(_knp(kt)) if keys_h.size else np.zeros(1, _knp(kt)))
    br = _In(br_h.astype(_knp(kt)))
    out_range, out_idx, d_nnz = _iout(nb + 1), _iout(nnz), _iout(1)
    import torch
    ws = torch.full((L.lib.hctr_ebc_route_workspace_bytes(batch, n_local),), -1, dtype=torch.int8,
                    device="cuda")
    L.check(L.lib.hctr_ebc_route_keys(batch, world, n_local, d3.p if n_local else None,
                                      d_rs.p if n_local else None, keys.p, br.p, _ktype(kt),
                                      out_range.p, out_idx.p, d_nnz.p, L.ptr(ws), L.stream_ptr()))
    torch.cuda.synchronize()
    assert (_ires(out_range) == want_range).all(), "out_bucket_range"
    assert _ires(d_nnz)[0] == nnz, "d_nnz"
    assert (_ires(out_idx) == want_idx).all(), "out_indices"  # (and the poison from [nnz] on)
    _unchanged((d3, "lookup_desc"), (d_rs, "row_start"), (keys, "keys"), (br, "bucket_range"))


@functools.lru_cache(maxsize=None)
def _route_input(G, batch, kt, seed=0, max_len=6, big=700):
    """G x batch ragged buckets: ~30 % empty, a run of empty ones, one bucket of `big` keys; keys up to
    the type's range (u32: the top key included)"""
    rng = np.random.default_rng(7000 + seed)
    nbk = G * batch
    lens = rng.integers(0, max_len + 1, size=nbk)
    lens[rng.random(nbk) < 0.3] = 0
    if nbk >= 40:
        lens[nbk // 3:nbk // 3 + 11] = 0
        lens[:2] = 0
        lens[nbk // 2] = big
        lens[-1] = min(5, max_len)
    br = np.zeros(nbk + 1, np.int64)
    np.cumsum(lens, out=br[1:])
    hi = 1 << 32 if kt == "u32" else 1 << 40
    keys = rng.integers(0, hi, size=int(br[-1])).astype(np.int64)
    if keys.size > 4:
        keys[:3] = [0, 1, hi - 1]
    br.setflags(write=False)
    keys.setflags(write=False)
    return br, keys


@pytest.mark.parametrize("num_shards", [1, 2, 3])
@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("kt", ["u32", "i64"])
def test_route_keys_matrix(kt, world, num_shards):
    """three local lookups out of five global ones, in an order of their own: a row-sharded static
    table, a dynamic one (row_start < 0: the key itself is kept) and a whole table; every shard_id"""
    G, batch = 5, 24
    br, keys = _route_input(G, batch, kt)
    for sid in range(num_shards):
        desc = [[4, num_shards, sid], [1, num_shards, sid], [2, 1, 0]]
        _route_keys_case(batch, world, desc, [1000, -1, 77], keys, br, kt)


@pytest.mark.parametrize("nb", SCAN_EDGES)
@pytest.mark.parametrize("kt", ["u32", "i64"])
def test_route_keys_edges(kt, nb):
    """nb = num_local_lookups * batch around one workgroup and around one and two tiles of the scan"""
    br, keys = _route_input(2, nb, kt, seed=nb, big=40)
    _route_keys_case(nb, 1, [[1, 2, 1]], [5], keys, br, kt)
    if nb % 2 == 0:  # the same buckets as two lookups on two ranks' slices
        _route_keys_case(nb, 2, [[1, 2, 0], [0, 1, 0]], [5, -1], keys, br, kt)


@pytest.mark.parametrize("kt", ["u32", "i64"])
def test_route_keys_empty(kt):
    """all buckets empty (nnz = 0, nothing stored), every bucket another shard's (the same), and
    num_local_lookups == 0 (out_bucket_range[0] == 0, d_nnz == 0)"""
    batch = 300
    _route_keys_case(batch, 2, [[1, 2, 1], [0, 1, 0]], [5, -1], np.zeros(0, np.int64),
                     np.zeros(2 * batch + 1, np.int64), kt)
    br, keys = _route_input(2, batch, kt, seed=1)
    _route_keys_case(batch, 2, [[1, 2, 1], [0, 2, 1]], [5, -1], keys - keys % 2, br, kt)
    _route_keys_case(batch, 2, np.zeros((0, 3)), [], keys, br, kt)


@pytest.mark.parametrize("which", _grid(["count-index", "scan-tiles"]))
def test_route_keys_grid(which):
    """count-index: 2 x 2048 x 256 + 37 buckets (three passes of the count / index grid, 1025 tiles);
    scan-tiles: 2 x 2048 x 1024 + 37 buckets of 0 / 1 keys (4097 tiles: the tile kernels loop)"""
    if which == "count-index":
        br, keys = _route_input(1, GRID_NB, "i64", seed=2, max_len=3)
        _route_keys_case(GRID_NB, 1, [[0, 2, 1]], [9], keys, br, "i64")
    else:
        nb = 2 * 2048 * 1024 + 37
        br, keys = _route_input(1, nb, "u32", seed=3, max_len=1, big=1)
        _route_keys_case(nb, 1, [[0, 3, 2]], [9], keys, br, "u32")


# ---- 2. hctr_ebc_route_whole -----------------------------------------------------------------------
def _route_whole_case(batch, rs, keys_h, br_h, kt, parts=1, hint=None, want_flag=None, flag=True,
                      nnz_out=True):
    """parts: the gridDim.y the hint asks for (nnz_hint = parts x buckets); want_flag: 1 = the flag
    word must stay set (non-zero), 0 = it must be cleared"""
    L = _lib()
    import torch
    rs = np.asarray(rs, np.int64)
    nl = len(rs)
    nb = nl * batch
    nnz = int(br_h[-1])
    d_rs = _In(rs if nl else [0])
    keys = _In(keys_h.astype(_knp(kt)) if keys_h.size else np.zeros(1, _knp(kt)))
    br = _In(br_h.astype(_knp(kt)))
    out_range, out_idx, d_nnz, one_hot = _iout(nb + 1), _iout(nnz), _iout(1), _iout(1, "i32")
    L.check(L.lib.hctr_ebc_route_whole(batch, nl, d_rs.p, keys.p, br.p, _ktype(kt), out_range.p,
                                       out_idx.p, d_nnz.p if nnz_out else None,
                                       one_hot.p if flag else None,
                                       parts * nb if hint is None else hint, L.stream_ptr()))
    torch.cuda.synchronize()
    r0 = rs[np.repeat(np.arange(nb), np.diff(br_h)) // batch] if nb else rs[:0]
    k = keys_h.astype(np.int64)[:nnz]
    assert (_ires(out_range) == br_h).all(), "out_bucket_range"
    assert (_ires(out_idx) == np.where(r0 < 0, k, r0 + k)).all(), "out_indices"
    assert _ires(d_nnz)[0] == (nnz if nnz_out else -1), "d_nnz"
    if want_flag is None:
        want_flag = int(nb > 0 and (br_h == np.arange(nb + 1)).all())
    word = int(_ires(one_hot)[0])
    if flag:
        # include/hugectr_amd.h: "left non-zero iff every bucket holds exactly its own key".  The
        # set flag reads 0x01010101, not 1: the call presets the word with a byte-wise memset
        assert (word != 0) == bool(want_flag) and word != -1, f"one_hot = {word:#x}"
    else:
        assert word == -1, "one_hot"
    _unchanged((d_rs, "row_start"), (keys, "keys"), (br, "bucket_range"))


@functools.lru_cache(maxsize=None)
def _whole_ragged(nb, kt):
    """lengths 0..6, a 5000-key bucket, runs of empty buckets across the 64-bucket chunk borders"""
    rng = np.random.default_rng(7100 + nb)
    lens = rng.integers(0, 7, size=nb)
    lens[rng.random(nb) < 0.3] = 0
    if nb >= 140:
        lens[58:71] = 0
        lens[120:136] = 0
        lens[100] = 5000
        lens[63 + 64] = 3
    br = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = rng.integers(0, 1 << (32 if kt == "u32" else 40), size=int(br[-1])).astype(np.int64)
    br.setflags(write=False)
    keys.setflags(write=False)
    return br, keys


def _whole_one_hot(nb, seed=0):
    keys = np.random.default_rng(7200 + seed).integers(0, 1 << 31, size=nb).astype(np.int64)
    return np.arange(nb + 1, dtype=np.int64), keys


@pytest.mark.parametrize("parts,hint_per_bucket", [(1, 0), (1, 1), (3, 3), (16, 16), (16, 40)])
@pytest.mark.parametrize("kt", ["u32", "i64"])
def test_route_whole_ragged(kt, parts, hint_per_bucket):
    """3 lookups x 67 samples (201 buckets: no multiple of 64), the middle lookup dynamic; gridDim.y
    1 (no hint, and one key per bucket), 3, 16, and a hint of 40 per bucket capped at 16"""
    batch = 67
    br, keys = _whole_ragged(3 * batch, kt)
    _route_whole_case(batch, [10, -1, 3000], keys, br, kt, hint=hint_per_bucket * 3 * batch)


@pytest.mark.parametrize("nb", EDGES + [64, 65, 201])
@pytest.mark.parametrize("kt", ["u32", "i64"])
def test_route_whole_one_hot(kt, nb):
    """an exactly one-hot batch keeps the flag set (one and three wavefronts per chunk); one-hot
    everywhere except a bucket pair of lengths (0, 2) inside a chunk -- that chunk's key count equals
    its bucket count -- or except the LAST bucket (2 keys / none: every bucket still starts at its
    own number, only the end of the range tells) clears it"""
    br, keys = _whole_one_hot(nb, nb)
    for parts in (1, 3):
        _route_whole_case(nb, [7], keys, br, kt, parts=parts, want_flag=1)
    last2 = np.concatenate([br, [nb + 1]])[np.r_[0:nb, nb + 1]]
    _route_whole_case(nb, [7], np.concatenate([keys, [5]]), last2, kt, want_flag=0)
    last0 = br.copy()
    last0[nb] = nb - 1
    _route_whole_case(nb, [7], keys, last0, kt, want_flag=0)
    if nb >= 4:
        for i in sorted({1, nb // 2, nb - 2}):
            pair = br.copy()
            pair[i + 1] = i  # bucket i empty, bucket i + 1 holds two keys
            for parts in (1, 3):
                _route_whole_case(nb, [7], keys, pair, kt, parts=parts, want_flag=0)


@pytest.mark.parametrize("kt", ["u32", "i64"])
def test_route_whole_optional_outputs(kt):
    """one_hot == nullptr, d_nnz == nullptr (both, and each alone); nb == 0 gives flag 0"""
    br, keys = _whole_ragged(201, kt)
    for flag, nnz_out in ((False, False), (True, False), (False, True)):
        _route_whole_case(67, [10, -1, 3000], keys, br, kt, parts=3, flag=flag, nnz_out=nnz_out)
    zero = np.zeros(1, np.int64)
    _route_whole_case(0, [10, -1], zero[:0], zero, kt, hint=0, want_flag=0)  # batch == 0
    _route_whole_case(16, [], zero[:0], zero, kt, hint=5, want_flag=0)      # no lookups


@pytest.mark.parametrize("kt", _grid(["u32"]))
def test_route_whole_grid(kt):
    """2 x 2048 x 4 x 64 + 37 one-hot buckets: three passes of the thread loop and of the wave loop"""
    br, keys = _whole_one_hot(GRID_NB)
    _route_whole_case(GRID_NB, [7], keys, br, kt, want_flag=1)


# ---- 3. hctr_ebc_routed_keys_to_indices ------------------------------------------------------------
def _routed_case(bpg, world, desc, rs, seed=0, max_len=5):
    """keys that arrived in the owner's bucket order [source peer][local lookup][b_local]: static
    lookups become row_start + key / num_shards in place; the keys of dynamic lookups and everything
    past out_range[nb] stay as they are"""
    L = _lib()
    import torch
    desc = np.asarray(desc, np.int32).reshape(-1, 3)
    rs = np.asarray(rs, np.int64)
    n_local = len(desc)
    nb = world * n_local * bpg
    rng = np.random.default_rng(7300 + seed)
    lens = rng.integers(0, max_len + 1, size=nb)
    lens[rng.random(nb) < 0.3] = 0
    rg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rg[-1])
    k = rng.integers(0, 1 << 40, size=nnz).astype(np.int64)
    ll = (np.repeat(np.arange(nb), lens) // bpg) % n_local
    want = np.where(rs[ll] < 0, k, rs[ll] + k // desc[ll, 1])
    d3, d_rs, d_rg = _In(desc), _In(rs), _In(rg)
    keys = _iout(nnz)
    keys.t[:nnz] = torch.from_numpy(k).to("cuda")
    L.check(L.lib.hctr_ebc_routed_keys_to_indices(bpg, world, n_local, d3.p, d_rs.p, d_rg.p, keys.p,
                                                  L.stream_ptr()))
    torch.cuda.synchronize()
    assert (_ires(keys) == want).all(), "keys_inout"
    _unchanged((d3, "lookup_desc"), (d_rs, "row_start"), (d_rg, "out_bucket_range"))


@pytest.mark.parametrize("world", [1, 4])
@pytest.mark.parametrize("bpg", EDGES + [6])
def test_routed_keys_to_indices(bpg, world):
    """static (sharded and whole) and dynamic lookups mixed; bucket counts at the edges with one
    static lookup"""
    _routed_case(bpg, world, [[4, 3, 1], [1, 2, 0], [2, 1, 0], [0, 2, 1]], [1000, -1, 77, -1], bpg)
    _routed_case(bpg, world, [[0, 3, 2]], [12], bpg + 1)


@pytest.mark.parametrize("world", _grid([1]))
def test_routed_keys_to_indices_grid(world):
    _routed_case(GRID_NB, world, [[0, 3, 2]], [12], max_len=2)


# ---- 4. hctr_ebc_bucket_counts ---------------------------------------------------------------------
def _counts_case(batch, world, num_lookup, kt, seed=0):
    L = _lib()
    import torch
    rng = np.random.default_rng(7400 + seed)
    lens = rng.integers(0, 9, size=num_lookup * batch)
    br_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    br = _In(br_h.astype(_knp(kt)))
    bpg = batch // world
    for rank in range(world):
        out = _iout(num_lookup * bpg)
        L.check(L.lib.hctr_ebc_bucket_counts(batch, world, rank, num_lookup, br.p, _ktype(kt), out.p,
                                             L.stream_ptr()))
        torch.cuda.synchronize()
        want = lens.reshape(num_lookup, world, bpg)[:, rank, :].reshape(-1)
        assert (_ires(out) == want).all(), f"counts of rank {rank} of {world}"
    br.assert_unchanged("bucket_range")


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("kt", ["u32", "i64"])
def test_bucket_counts(kt, world):
    """every rank of the world; num_lookup * bpg at the edges (one lookup) and with five lookups"""
    for n in EDGES:
        _counts_case(n * world, world, 1, kt, n)
    _counts_case(52 * world, world, 5, kt)


@pytest.mark.parametrize("kt", _grid(["i64"]))
def test_bucket_counts_grid(kt):
    _counts_case(GRID_NB, 1, 1, kt)


# ---- 5. hctr_ebc_network_forward / _backward -------------------------------------------------------
# block-table rows of a lookup, by max_shards (1 = a live slot): all live, a hole in the first slot,
# a hole in the middle, a whole row of -1, holes in front of the only live slot, one shard first
PATTERNS = {1: [(1,), (0,)],
            2: [(1, 1), (0, 1), (1, 0), (0, 0)],
            3: [(1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 1)]}
COUNTS = np.array([0, 1, 3, 7, 2])
SPARE_BLOCKS = 2  # blocks no lookup names: the backward leaves them alone


@functools.lru_cache(maxsize=None)
def _net_layout(max_shards, bpg):
    """every pattern once as a Sum and once as an Average lookup -> (blocks [L][max_shards],
    combiner [L], counts [L][bpg] cycling through 0, 1, 3, 7, 2, number of blocks)"""
    pats = [p for p in PATTERNS[max_shards] for _ in (0, 1)]
    L = len(pats)
    n_live = sum(sum(p) for p in pats)
    ids = np.random.default_rng(7500 + max_shards).permutation(n_live + SPARE_BLOCKS)
    blocks = np.full((L, max_shards), -1, np.int32)
    blocks[np.array(pats, bool)] = ids[:n_live]
    comb = (np.arange(L) % 2).astype(np.int32)
    counts = COUNTS[(np.arange(L)[:, None] // 2 + np.arange(bpg)[None, :] + max_shards) % 5]
    counts = counts.astype(np.int64)
    for a in (blocks, comb, counts):
        a.setflags(write=False)
    return blocks, comb, counts, n_live + SPARE_BLOCKS


def _divisor(comb, counts):
    return np.where((comb[:, None] == 1) & (counts > 0), counts, 1).astype(np.float32)


def _net_forward_ref(recv, blocks, comb, counts, dt):
    """recv [block][bpg][ev] -> [L][bpg][ev]: 0.f, + each live shard in slot order (fp32), / count
    (fp32, Average lookups with a count > 0 only), one rounding to the vector type"""
    acc = np.zeros((blocks.shape[0],) + recv.shape[1:], np.float32)
    for s in range(blocks.shape[1]):
        live = blocks[:, s] >= 0
        acc[live] = acc[live] + recv[blocks[live, s]]
    assert acc.dtype == np.float32
    return _round(acc / _divisor(comb, counts)[:, :, None], dt)


def _net_backward_ref(grad, blocks, comb, counts, nblocks, dt):
    """grad [L][bpg][ev] -> send [block][bpg][ev]: grad / count rounded once, to every live block of
    the lookup; NaN (the poison) in the blocks no lookup names"""
    g = _round(grad / _divisor(comb, counts)[:, :, None], dt)
    send = np.full((nblocks,) + grad.shape[1:], np.nan, np.float32)
    for s in range(blocks.shape[1]):
        live = blocks[:, s] >= 0
        send[blocks[live, s]] = g[live]
    return send


def _dense(x, batch_major):
    """[L][bpg][ev] -> the dense layout: feature-major as it is, batch-major [bpg][L][ev]"""
    return np.ascontiguousarray(x.transpose(1, 0, 2)) if batch_major else x


def _net_call(fwd, bpg, ev, layout, batch_major, src_h, dt, in_mis=0, out_mis=0):
    """one launch -> (output rows, want rows); src_h: recv [block][bpg][ev] (forward) or the
    gradient [L][bpg][ev] (backward), fp32 values exact in dt"""
    L = _lib()
    import torch
    blocks, comb, counts, nblocks = layout
    nl, ms = blocks.shape
    d_blocks, d_comb, d_counts = _In(blocks), _In(comb), _In(counts)
    if fwd:
        src = _In(_as_type(src_h, dt), mis=in_mis)
        out = _Out(nl * bpg, ev, dt, mis=out_mis)
        want = _dense(_net_forward_ref(src_h, blocks, comb, counts, dt), batch_major)
        fn = L.lib.hctr_ebc_network_forward
    else:
        src = _In(_as_type(_dense(src_h, batch_major), dt), mis=in_mis)
        out = _Out(nblocks * bpg, ev, dt, mis=out_mis)
        want = _net_backward_ref(src_h, blocks, comb, counts, nblocks, dt)
        fn = L.lib.hctr_ebc_network_backward
    L.check(fn(bpg, nl, ev, ms, d_blocks.p, d_comb.p, d_counts.p, batch_major, src.p, out.p,
               _code(dt), L.stream_ptr()))
    torch.cuda.synchronize()
    got = out.result()
    what = (f"{'forward' if fwd else 'backward'} {dt} ev={ev} bpg={bpg} max_shards={ms} "
            f"batch_major={batch_major} mis={in_mis}/{out_mis}")
    want = want.reshape(-1, ev)
    spare = np.isnan(want)  # (backward only) the blocks no lookup names: still the poison, any NaN
    assert np.isnan(got[spare]).all(), f"{what}: write into a block no lookup names"
    _assert_bits(np.where(spare, 0, got), np.where(spare, 0, want), what)
    _unchanged((d_blocks, "src_blocks"), (d_comb, "combiner"), (d_counts, "bucket_counts"),
               (src, "recv / grad"))
    return got


def _net_src(fwd, layout, bpg, ev, dt):
    blocks, _, _, nblocks = layout
    shape = (nblocks if fwd else blocks.shape[0], bpg, ev)
    return _vals(shape[0] * bpg * ev, dt, 7600 + int(fwd)).reshape(shape)


# ev per type: 16-byte rows -> ebc_network_vec_kernel, everything else -> ebc_network_kernel
NET_EV = [("f32", ev, "vec") for ev in (4, 8, 128, 200)] + \
         [("f32", ev, "scalar") for ev in (1, 6, 11)] + \
         [(dt, ev, "vec") for dt in ("f16", "bf16") for ev in (8, 128)] + \
         [(dt, ev, "scalar") for dt in ("f16", "bf16") for ev in (4, 6, 11)]


@pytest.mark.parametrize("fwd", [True, False], ids=["forward", "backward"])
@pytest.mark.parametrize("bpg", [1, 3, 64, 257])
@pytest.mark.parametrize("dt,ev,kernel", NET_EV)
def test_network_matrix(dt, ev, kernel, bpg, fwd):
    """both kernels x every type x batch_major 0 / 1 x max_shards 1 / 2 / 3 with -1 holes in the first
    slot, in the middle and in a whole row, Sum and Average lookups with counts 0, 1, 3, 7 (and 2):
    plain move, one shard with a divisor, sum over shards; the backward writes grad / count to every
    block a lookup names and leaves the poison in the others"""
    assert (ev * (4 if dt == "f32" else 2) % 16 == 0) == (kernel == "vec")
    for ms in (1, 2, 3):
        layout = _net_layout(ms, bpg)
        src = _net_src(fwd, layout, bpg, ev, dt)
        for batch_major in (0, 1):
            got = _net_call(fwd, bpg, ev, layout, batch_major, src, dt)
            if fwd:  # a whole row of -1: zeros, from either kernel
                dead = np.flatnonzero((layout[0] < 0).all(axis=1))
                rows = got.reshape((bpg, -1, ev) if batch_major else (-1, bpg, ev))
                rows = rows[:, dead] if batch_major else rows[dead]
                assert dead.size == 2 and rows.size and not rows.view(np.uint32).any()


@pytest.mark.parametrize("fwd", [True, False], ids=["forward", "backward"])
@pytest.mark.parametrize("which", ["in", "out"])
@pytest.mark.parametrize("dt,ev", [("f32", 8), ("f32", 128), ("f16", 8), ("bf16", 128)])
def test_network_misaligned(dt, ev, which, fwd):
    """a vec-eligible ev with the input / the output pointer one element off 16-byte alignment -> the
    scalar kernel: the bits of the aligned call (and of the reference)"""
    bpg = 67
    for ms in (1, 3):
        layout = _net_layout(ms, bpg)
        src = _net_src(fwd, layout, bpg, ev, dt)
        for batch_major in (0, 1):
            a = _net_call(fwd, bpg, ev, layout, batch_major, src, dt)
            b = _net_call(fwd, bpg, ev, layout, batch_major, src, dt, in_mis=int(which == "in"),
                          out_mis=int(which == "out"))
            _assert_bits(a, b, "aligned vs misaligned")


@pytest.mark.parametrize("kernel,dt,bpg,ev", _grid([("vec", "f32", 16400, 256),
                                                    ("scalar", "f32", 60000, 6)]))
def test_network_grid(kernel, dt, bpg, ev):
    """vec: 4 lookups x 16400 x 64 16-byte units > 2 x 8192 x 256; scalar: 3 lookups (of 4) x 60000 x
    6 elements > 2 x 2048 x 256; max_shards = 2 with holes, forward and backward"""
    blocks = np.array([[3, 0], [-1, 4], [1, -1], [-1, 2]], np.int32)
    comb = np.array([1, 0, 1, 1], np.int32)
    units = 4 * bpg * (ev * 4 // 16 if kernel == "vec" else ev)
    assert units > 2 * (8192 if kernel == "vec" else 2048) * 256
    counts = COUNTS[(np.arange(4)[:, None] + np.arange(bpg)[None, :]) % 5].astype(np.int64)
    layout = (blocks, comb, counts, 5)
    _net_call(True, bpg, ev, layout, 1, _net_src(True, layout, bpg, ev, dt), dt)
    _net_call(False, bpg, ev, layout, 0, _net_src(False, layout, bpg, ev, dt), dt)


# ---- 6. hctr_ebc_scale_average ---------------------------------------------------------------------
def _scale_case(fwd, bpg, nl, ev, dt, batch_major, seed=0):
    """in place on [L][bpg][ev] (or batch-major) vectors: Average lookups with more than one key are
    divided by the count, everything else keeps its bits; forward == what hctr_ebc_network_forward
    gives for the same pooled sums with one shard per lookup"""
    L = _lib()
    import torch
    comb = (np.arange(nl) % 3 != 0).astype(np.int32)  # lookups 0, 3, ... are Sum
    counts = COUNTS[(np.arange(nl)[:, None] + np.arange(bpg)[None, :]) % 5].astype(np.int64)
    x = _vals(nl * bpg * ev, dt, 7700 + seed).reshape(nl, bpg, ev)
    d_comb, d_counts = _In(comb), _In(counts)
    data = _Out(nl * bpg, ev, dt)
    n = nl * bpg * ev
    data.t[:n] = torch.from_numpy(_dense(x, batch_major).reshape(-1).copy()).to("cuda").to(
        data.t.dtype)
    L.check(L.lib.hctr_ebc_scale_average(bpg, nl, ev, d_comb.p, d_counts.p, batch_major, data.p,
                                         _code(dt), int(fwd), L.stream_ptr()))
    torch.cuda.synchronize()
    got = data.result()
    touched = (comb[:, None] == 1) & (counts > 1)
    want = np.where(touched[:, :, None], _round(x / _divisor(comb, counts)[:, :, None], dt), x)
    assert touched.any() and (counts[comb == 1] == 2).any()
    _assert_bits(got, _dense(want, batch_major).reshape(-1, ev),
                 f"scale_average fwd={fwd} {dt} ev={ev} bpg={bpg} batch_major={batch_major}")
    _unchanged((d_comb, "combiner"), (d_counts, "bucket_counts"))
    if fwd and bpg <= 4096:
        layout = (np.arange(nl, dtype=np.int32).reshape(nl, 1), comb, counts, nl)
        net = _net_call(True, bpg, ev, layout, batch_major, x, dt)
        _assert_bits(got, net, "scale_average vs network_forward with one shard per lookup")


@pytest.mark.parametrize("fwd", [True, False], ids=["forward", "backward"])
@pytest.mark.parametrize("ev", [8, 6, 128])
@pytest.mark.parametrize("dt", DTYPES)
def test_scale_average(dt, ev, fwd):
    for batch_major in (0, 1):
        for bpg in (1, 3, 257):
            _scale_case(fwd, bpg, 5, ev, dt, batch_major, seed=bpg)


@pytest.mark.parametrize("dt", _grid(["f32", "bf16"]))
def test_scale_average_grid(dt):
    """4 x 16400 x 64 = 4198400 elements > 2 x 8192 x 256"""
    _scale_case(True, 16400, 4, 64, dt, 1)


# ---- 7. hctr_static_lookup -------------------------------------------------------------------------
# the shard holds id spaces 1, 4 and 6 of the group, in one flat fp32 array, vectors of 8 / 16 / 4
SL_LOCAL = np.array([1, 4, 6], np.int32)
SL_ROWS, SL_EVS = np.array([50, 7, 300]), np.array([8, 16, 4], np.int32)
SL_START = np.concatenate([[100], 100 + np.cumsum(SL_ROWS)]).astype(np.int64)  # index numbering
SL_EV_OFF = np.concatenate([[0], np.cumsum(SL_ROWS * SL_EVS)[:-1]]).astype(np.int64)
SL_KTYPES = {"u32": (0, np.uint32), "i64": (1, np.int64), "u64": (2, np.uint64)}


def _static_case(kt, order, counts, seed=0, foreign=(), outside=0):
    """positions: counts[i] indices of id space order[i] (the call's own order; empty segments
    allowed).  foreign: id spaces of `order` the shard does not hold -> bit 1, NULL; outside: that
    many positions of held id spaces get an index below / beyond the table -> bit 2, NULL"""
    L = _lib()
    import torch
    rng = np.random.default_rng(7800 + seed)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    n = int(offs[-1])
    ids = np.repeat(np.asarray(order), counts)
    slot = np.searchsorted(SL_LOCAL, ids)
    held = (slot < SL_LOCAL.size) & (SL_LOCAL[np.minimum(slot, SL_LOCAL.size - 1)] == ids)
    assert (~held).any() == bool(foreign) and all(f not in SL_LOCAL for f in foreign)
    t = np.where(held, slot, 0)
    idx = SL_START[t] + (rng.random(n) * SL_ROWS[t]).astype(np.int64)
    if n > 8:
        idx[:2] = SL_START[t[:2]]              # the first and the last row of a table
        idx[2:4] = SL_START[t[2:4] + 1] - 1
    inside = np.ones(n, bool)
    if outside:
        bad = rng.choice(np.flatnonzero(held), size=outside, replace=False)
        idx[bad] = np.where(np.arange(outside) % 2 == 0, SL_START[t[bad] + 1], SL_START[t[bad]] - 1)
        inside[bad] = False
    table = _In(_vals(int((SL_ROWS * SL_EVS).sum()), "f32", 7801))
    ok = held & inside
    want = np.where(ok, table.t.data_ptr() + 4 * (SL_EV_OFF[t] + (idx - SL_START[t]) * SL_EVS[t]), 0)
    code, npdt = SL_KTYPES[kt]
    d_idx = _In(idx.astype(npdt))
    ins = [_In(offs), _In(np.asarray(order, np.int32)), _In(SL_LOCAL), _In(SL_START.astype(np.uint64)),
           table, _In(SL_EV_OFF.astype(np.uint64)), _In(SL_EVS)]
    ptrs, err = _iout(n), _iout(1, "i32")
    err.t[:1] = 0  # the kernel ORs its bits into the caller's word
    L.check(L.lib.hctr_static_lookup(d_idx.p, code, n, ins[0].p, offs.size, ins[1].p, ins[2].p,
                                     SL_LOCAL.size, ins[3].p, ins[4].p, ins[5].p, ins[6].p, ptrs.p,
                                     err.p, L.stream_ptr()))
    torch.cuda.synchronize()
    assert (_ires(ptrs) == want).all(), "embedding_vec"
    assert _ires(err)[0] == (1 if (~held).any() else 0) | (2 if (held & ~inside).any() else 0)
    _unchanged((d_idx, "keys"), *[(x, "table lists") for x in ins])


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("kt", ["u32", "i64", "u64"])
def test_static_lookup(kt, n):
    """tables of different vector sizes in the call's own order, an empty segment; num_keys at the
    edges (n positions in all -- a single one leaves two segments empty -- and n in one segment)"""
    _static_case(kt, [4, 1, 6], [n // 3, n - n // 3 - n // 4, n // 4], n)
    _static_case(kt, [6, 4, 1, 6], [n, 0, 20, 41], n)


@pytest.mark.parametrize("kt", ["u32", "i64", "u64"])
def test_static_lookup_errors(kt):
    """bit 1 alone (id spaces below, between and above the shard's), bit 2 alone (an index one below
    and one beyond the table), both; every other position still gets its address"""
    _static_case(kt, [0, 4, 5, 1, 9, 6], [3, 20, 33, 41, 2, 30], 1, foreign=(0, 5, 9))
    _static_case(kt, [4, 1, 6], [20, 33, 41], 2, outside=7)
    _static_case(kt, [4, 5, 6], [20, 33, 41], 3, foreign=(5,), outside=4)


@pytest.mark.parametrize("kt", _grid(["i64"]))
def test_static_lookup_grid(kt):
    _static_case(kt, [4, 1, 6], [300000, 400000, GRID_NB - 700000], 4)


# ---- 8. hctr_ebc_local_reduce ----------------------------------------------------------------------
def _sum_bound(n, sum_abs):
    """any order of n - 1 fp32 additions of addends exact in fp32: every partial sum is rounded once,
    |error| <= gamma_(n-1) sum|g|, gamma_k = k u / (1 - k u)  (Higham, Accuracy and Stability of
    Numerical Algorithms, 4.2)"""
    k = (n - 1).astype(np.float64)[:, None]
    return k * U * sum_abs / (1 - k * U)


@functools.lru_cache(maxsize=None)
def _lr_input(nnz, max_row, seed, lookups=3, per_bucket=None):
    """ragged buckets ([lookup][sample], empty ones among them) holding nnz positions; row ids out of
    [0, max_row] with both ends present: one long power-law run next to rows met only once"""
    rng = np.random.default_rng(7900 + seed)
    if per_bucket:
        samples = -(-nnz // (lookups * per_bucket))
        lens = np.full(samples * lookups, per_bucket)
        assert lens.sum() == nnz
    else:
        samples = max(2, -(-nnz // 4))
        lens = np.bincount(rng.integers(0, samples * lookups, size=nnz), minlength=samples * lookups)
    br = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pool = np.unique(np.concatenate([np.array([0, max_row], np.uint64),
                                     rng.integers(0, max_row + 1, size=400, dtype=np.uint64)]))
    pick = np.minimum(rng.pareto(0.7, size=nnz).astype(np.int64), pool.size - 1)
    rows = pool[pick]
    if nnz > 2:
        rows[nnz // 2] = max_row  # (a row of its own unless max_row is 0 or the pool is tiny)
    keys = (rng.permutation(nnz) * 3 + 1).astype(np.uint64)  # one key per POSITION
    for a in (br, rows, keys):
        a.setflags(write=False)
    return samples, lookups, br, rows, keys


def _lr_case(nnz, D, dt, max_row, want_keys, mapped, seed=0, per_bucket=None):
    L = _lib()
    import torch
    samples, lookups, br_h, rows_h, keys_h = _lr_input(nnz, max_row, seed, per_bucket=per_bucket)
    buckets = samples * lookups
    grad_h = _vals(buckets * D, dt, 7901 + D).reshape(buckets, D)
    b = np.repeat(np.arange(buckets), np.diff(br_h))
    grow = (b % samples) * lookups + b // samples if mapped else b  # gradient row of a position
    want_rows, first, inv, run = np.unique(rows_h, return_index=True, return_inverse=True,
                                           return_counts=True)
    nu = want_rows.size
    order = np.argsort(inv, kind="stable")
    starts = np.concatenate([[0], np.cumsum(run)[:-1]])
    g64 = grad_h[grow[order]].astype(np.float64)
    want = np.add.reduceat(g64, starts, axis=0)
    sum_abs = np.add.reduceat(np.abs(g64), starts, axis=0)

    upd = ctypes.c_void_p()
    L.check(L.lib.hctr_updater_create(nnz + 5, nnz + 5, D, ctypes.byref(upd)))
    try:
        if mapped:
            L.check(L.lib.hctr_updater_set_grad_map(upd, samples, lookups))
        br, rows, keys = _In(br_h), _In(rows_h), _In(keys_h)
        grad = _In(_as_type(grad_h, dt))
        urow, ukey, wg = _iout(nu), _iout(nu), _Out(nu, D, "f32")
        n_out = ctypes.c_size_t(12345)
        L.check(L.lib.hctr_ebc_local_reduce(upd, buckets, nnz, br.p, rows.p, int(max_row), keys.p,
                                            grad.p, _code(dt), ctypes.byref(n_out), urow.p,
                                            ukey.p if want_keys else None, wg.p, L.stream_ptr()))
        torch.cuda.synchronize()
        assert n_out.value == nu, "num_unique"
        assert (_ires(urow).view(np.uint64) == want_rows).all(), "unique rows (ascending)"
        got_keys = _ires(ukey).view(np.uint64)
        assert (got_keys == (keys_h[first] if want_keys else np.uint64(2 ** 64 - 1))).all(), \
            "unique keys (those of the first occurrence)"
        got = wg.result()
        err, bound = np.abs(got.astype(np.float64) - want), _sum_bound(run, sum_abs)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"local_reduce nnz={nnz} D={D} {dt} max_row={max_row:#x}: longest run {run.max()}, "
                  f"max err / bound = {np.nanmax(np.where(bound > 0, err / bound, 0.0)):.3f}")
        assert np.isfinite(got).all() and (err <= bound).all(), \
            f"local_reduce sums: {(err > bound).sum()} elements outside the bound"
        once = run == 1
        _assert_bits(got[once], grad_h[grow[order]][starts[once]], "rows met once")
        _unchanged((br, "bucket_range"), (rows, "row_ids"), (keys, "keys"), (grad, "grad"))
    finally:
        L.lib.hctr_updater_destroy(upd)
    return run


MAX_ROWS = [0, 1, 2 ** 11 - 1, 2 ** 11, 2 ** 22, 0xFFFFFFEF, 0xFFFFFFF0]


@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "grad-map"])
@pytest.mark.parametrize("want_keys", [True, False], ids=["keys", "no-keys"])
@pytest.mark.parametrize("max_row", MAX_ROWS, ids=[hex(m) for m in MAX_ROWS])
def test_local_reduce_max_row_id(max_row, want_keys, mapped):
    """end_bit from max_row_id: 1, 1, 11, 12, 23 and 32 bits through the 32-bit radix sort, 0xFFFFFFF0
    through the library's 64-bit sort; the largest row id itself is among the rows"""
    run = _lr_case(4097, 16, "f32", max_row, want_keys, mapped, seed=1)
    if max_row >= 2 ** 11:
        assert run.max() > 1000 and (run == 1).sum() > 10  # a long run next to rows met once


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [16, 128, 10])
@pytest.mark.parametrize("nnz", [1, 4095, 4096, 4097])
def test_local_reduce_matrix(nnz, D, dt):
    for want_keys, mapped in ((True, False), (False, True)):
        _lr_case(nnz, D, dt, 2 ** 22, want_keys, mapped, seed=nnz)


@pytest.mark.parametrize("dt", _grid(["f16"]))
def test_local_reduce_grid(dt):
    """3 x 349538 buckets of two positions: 1048614 buckets (lr_expand_kernel: three passes of the
    wave loop), 2097228 positions > 2 x 4096 x 256 (lr_flags_kernel / lr_emit_kernel)"""
    nnz = 2 * 3 * 349538
    assert nnz // 2 > 2 * 2048 * 4 * 64 and nnz > 2 * 4096 * 256
    _lr_case(nnz, 16, dt, 2 ** 22, True, True, seed=5, per_bucket=2)
