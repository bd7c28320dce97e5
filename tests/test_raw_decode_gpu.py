"""hctr_raw_decode through the C ABI (csrc/raw_decode.hip): one launch splits one batch of Raw
records.  The oracle is the host RawReader (CPU device) over the same file: labels, float dense
features, keys of both layouts are compared BIT FOR BIT; integer dense features are log(x + 1.f)
with the sum in fp32 and the logarithm in fp64 on the device (logf itself lands up to 2 floats off on
gfx950, profiles/raw_decode_logf.txt) and np.log in fp32 on the host, so they are held to 1 ulp (the
bound HIP documents for logf, which the reference uses) against
float32(log(float64(float32(x) + float32(1)))) and to the host's class (finite / inf / nan).
The arena is painted before the launch: every byte no output owns must keep its paint.
Runs under HCTR_EMU=1 too (the kernel's source stepped through on the host)."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MLPERF_HOT = [3, 2, 1, 2, 6, 1, 1, 1, 1, 7, 3, 8, 1, 6, 9, 5, 1, 1, 1, 12, 100, 27, 10, 3, 1, 1]
EDGE_KEYS = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
EDGE_DENSE = np.array([0, 1, (1 << 24) + 1, (1 << 31) - 1], np.uint32)
PAINT = 0xA5
GUARD = 4096


def _tile(width):
    from hugectr_amd._lib import lib
    return int(lib.hctr_raw_decode_tile(width))


def _inp(L, Dn, params):
    """params: [(name, hotness per slot: int or list, slot_num)]"""
    import hugectr_amd.hugectr as hugectr
    return hugectr.Input(label_dim=L, label_name="label", dense_dim=Dn, dense_name="dense",
                         data_reader_sparse_param_array=[
                             hugectr.DataReaderSparseParam(n, h, True, s) for n, h, s in params])


def _records(rng, n, L, Dn, nkeys, float_label, float_dense):
    """[n][width] uint32 records with the edge values sprinkled in"""
    lab = rng.integers(0, 2, size=(n, L))
    lab = lab.astype(np.float32).view(np.uint32) if float_label else lab.astype(np.uint32)
    if float_dense:
        den = rng.standard_normal((n, Dn)).astype(np.float32).view(np.uint32)
    else:
        den = rng.integers(0, 1 << 20, size=(n, Dn)).astype(np.uint32)
        flat = den.reshape(-1)
        flat[:min(flat.size, 4)] = EDGE_DENSE[:min(flat.size, 4)]
        flat[-min(flat.size, 4):] = EDGE_DENSE[:min(flat.size, 4)]
    keys = rng.integers(0, 1 << 32, size=(n, nkeys), dtype=np.uint64).astype(np.uint32)
    flat = keys.reshape(-1)
    flat[:min(flat.size, 4)] = EDGE_KEYS[:min(flat.size, 4)]
    flat[-min(flat.size, 4):] = EDGE_KEYS[:min(flat.size, 4)]
    return np.ascontiguousarray(np.concatenate([lab, den, keys], axis=1), dtype="<u4")


def _decode_and_compare(tmp_path, L, Dn, params, B, *, sizes=(), groups=(), rank=0, world=1,
                        float_ld=True, ap=None, i64=True, seed=0):
    from hugectr_amd import data
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    inp = _inp(L, Dn, params)
    # (the conventions first: they shape the file)
    if ap is not None and getattr(ap, "multi_hot_reader", True):
        float_label, float_dense = False, bool(ap.is_dense_float)
    else:
        float_label = float_dense = bool(float_ld)
    nkeys = 0
    for _, h, s in params:
        nkeys += sum(h) if isinstance(h, (list, tuple)) else h * s
    rec = _records(np.random.default_rng(seed), B, L, Dn, nkeys, float_label, float_dense)
    path = str(tmp_path / "batch.bin")
    rec.tofile(path)
    host = data.RawReader(path, inp, list(sizes), B, rank, world, torch.device("cpu"), 0, float_ld,
                          False, ap, i64)
    host.ebc_groups = [list(g) for g in groups]
    assert host.stats()["decode"] == "host"
    want = host.next_batch()
    pl = host.decode_plan()
    assert pl["width"] == rec.shape[1]

    raw = torch.from_numpy(rec.view(np.int32)).cuda()
    blob = np.concatenate([pl["segments"].view(np.uint8).reshape(-1), pl["addend"].view(np.uint8)])
    plan = torch.from_numpy(blob).cuda()
    arena = torch.full((pl["arena_bytes"] + GUARD,), PAINT, dtype=torch.uint8, device="cuda")
    check(lib.hctr_raw_decode(ptr(raw), B, rec.shape[1], ptr(plan), len(pl["segments"]),
                              ptr(arena), stream_ptr()))
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    owned = np.zeros(got.size, bool)

    def cut(off, n, dtype):
        nb = n * np.dtype(dtype).itemsize
        assert not owned[off:off + nb].any(), "two outputs share bytes of the arena"
        owned[off:off + nb] = True
        return got[off:off + nb].view(dtype)

    bpg = B // world
    lab = cut(pl["label"][0], bpg * L, np.uint32)
    assert (lab == want["label"].numpy().view(np.uint32).reshape(-1)).all(), "label"
    den = cut(pl["dense"][0], bpg * Dn, np.float32)
    wd = want["dense"].numpy().reshape(-1)
    if float_dense:
        assert (den.view(np.uint32) == wd.view(np.uint32)).all(), "float dense: bit copy"
    else:
        x = rec[rank * bpg:(rank + 1) * bpg, L:L + Dn].view(np.int32).astype(np.float32).reshape(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = np.log((x + np.float32(1.0)).astype(np.float64)).astype(np.float32)
        assert (np.isnan(den) == np.isnan(wd)).all() and (np.isinf(den) == np.isinf(wd)).all()
        fin = np.isfinite(ref)
        ulp = np.abs(den[fin].view(np.int32).astype(np.int64) - ref[fin].view(np.int32).astype(np.int64))
        print(f"integer dense: max ulp distance {int(ulp.max()) if ulp.size else 0}, "
              f"{int((ulp != 0).sum())} of {ulp.size} differ from the correctly rounded value")
        assert (ulp <= 1).all(), "integer dense: more than 1 ulp from the correctly rounded log(x + 1)"
    kdt = np.int64 if i64 else np.int32
    for name, (off, n) in pl["sparse"].items():
        ro, keys = want["sparse"][name]
        assert keys.dtype == (torch.int64 if i64 else torch.int32)
        assert (cut(off, n, kdt) == keys.numpy()).all(), f"sparse {name}"
    assert len(pl["ebc"]) == len(groups)
    for g, (off, n) in enumerate(pl["ebc"]):
        gk, gbr = want["ebc"][g]
        assert (cut(off, n, np.int64) == gk.numpy()).all(), f"collection group {g}"
    assert (got[~owned] == PAINT).all(), "a byte outside every output was written"
    return want, got, pl


W3 = (1, 1, [("s", 1, 1)])
W40 = (1, 13, [("data", 1, 26)])
W228 = (1, 13, [(f"d{i}", h, 1) for i, h in enumerate(MLPERF_HOT)])


def _batches(width):
    t = _tile(width)
    return [1, t - 1, t, t + 1, 2 * t + 2]


def test_tile_sizes():
    assert (_tile(3), _tile(40), _tile(228)) == (256, 192, 32)
    assert _tile(300) == 32 and _tile(100000) == 32  # (column passes)


@pytest.mark.parametrize("which", range(5))
def test_width_3_at_the_tile_edges(tmp_path, which):
    L, Dn, params = W3
    _decode_and_compare(tmp_path, L, Dn, params, _batches(3)[which], sizes=[1 << 20], seed=which)


@pytest.mark.parametrize("which", range(5))
def test_width_40_at_the_tile_edges(tmp_path, which):
    L, Dn, params = W40
    sizes = [1000 + 37 * i for i in range(26)]
    _decode_and_compare(tmp_path, L, Dn, params, _batches(40)[which], sizes=sizes, seed=which)


@pytest.mark.parametrize("which", range(5))
def test_width_228_mlperf_hotness_at_the_tile_edges(tmp_path, which):
    """26 multi-hot inputs, every one also a lookup of one collection: sparse AND ebc outputs"""
    import hugectr_amd.hugectr as hugectr
    L, Dn, params = W228
    assert L + Dn + sum(MLPERF_HOT) == 228
    ap = hugectr.AsyncParam(num_threads=1, num_batches_per_thread=4, multi_hot_reader=True,
                            is_dense_float=True)
    _decode_and_compare(tmp_path, L, Dn, params, _batches(228)[which],
                        groups=[[f"d{i}" for i in range(26)]], ap=ap, seed=which)


def test_tiles_outnumber_the_grid(tmp_path):
    """the smallest batch with more tiles than workgroups are ever launched (grid-stride)"""
    from hugectr_amd import _lib
    L, Dn, params = W3
    B = _lib.RAW_DECODE_MAX_BLOCKS * _tile(3) + 1
    _decode_and_compare(tmp_path, L, Dn, params, B, sizes=[77])


@pytest.mark.parametrize("i64", [True, False])
def test_key_types_and_offsets_past_2_to_32(tmp_path, i64):
    """u32 keys are zero-extended, the slot offset is a 64-bit add; int32 keys keep the low 32 bits"""
    sizes = [1 << 31, 1 << 31, 1 << 31, 5]  # offsets 0, 2^31, 2^32, 3 * 2^31
    want, got, pl = _decode_and_compare(tmp_path, 1, 2, [("k", [1, 2, 1, 3], 4)], 70, sizes=sizes,
                                        i64=i64)
    keys = want["sparse"]["k"][1].numpy().reshape(70, 7)
    if i64:
        # first record: keys 0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF in slots 0, 1, 1, 2
        assert keys[0, :4].tolist() == [0, 0x7FFFFFFF + (1 << 31), 0x80000000 + (1 << 31),
                                        0xFFFFFFFF + (1 << 32)]
        assert (keys >= 0).all() and keys.max() > (1 << 32)
    else:
        assert keys.dtype == np.int32


@pytest.mark.parametrize("conv", ["float_ld", "int_ld", "async_float_dense", "async_int_dense"])
def test_label_and_dense_conventions(tmp_path, conv):
    import hugectr_amd.hugectr as hugectr
    ap, float_ld = None, conv == "float_ld"
    if conv.startswith("async"):
        ap = hugectr.AsyncParam(num_threads=2, num_batches_per_thread=2, multi_hot_reader=True,
                                is_dense_float=conv == "async_float_dense")
    _decode_and_compare(tmp_path, 2, 5, [("a", [2, 1], 2), ("b", 3, 1)], 100, sizes=[50, 60, 70],
                        float_ld=float_ld, ap=ap)


DEEP_HOT = [1, 3, 1, 2, 1, 1, 5, 1, 1, 4, 1, 1, 2, 1, 1, 1, 7, 1, 1, 2, 1, 3, 1, 1, 1, 2]
FORMS = {
    "one_legacy_26_slots": dict(params=[("data", DEEP_HOT, 26)], sizes=list(range(10, 36))),
    "wide_and_deep": dict(params=[("wide", [2, 1], 2), ("deep", DEEP_HOT, 26)],
                          sizes=list(range(100, 128))),
    "ragged_collection": dict(params=[("a", 5, 1), ("b", 1, 1), ("c", 17, 1), ("d", 2, 1)],
                              groups=[["a", "b", "c", "d"]]),
    "legacy_and_collection": dict(params=[("legacy", [1, 4, 2], 3), ("a", 3, 1), ("b", 1, 1),
                                          ("c", 6, 1)],
                                  sizes=[9, 8, 7, 6, 5, 4], groups=[["a", "b"], ["c"]]),
    # wider than one column pass: segments cut by a pass, and one lying in the second pass only
    "column_passes": dict(params=[("x", 100, 1), ("y", [90, 60], 2), ("z", 57, 1)],
                          sizes=[3, 5, 7, 9], groups=[["z", "x"]]),
}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("i64", [True, False])
def test_legacy_and_collection_forms(tmp_path, form, i64):
    f = FORMS[form]
    L, Dn = 1, 3
    width = L + Dn + sum(sum(h) if isinstance(h, list) else h * s for _, h, s in f["params"])
    B = 2 * _tile(width) + 2
    _decode_and_compare(tmp_path, L, Dn, f["params"], B, sizes=f.get("sizes", ()),
                        groups=f.get("groups", ()), i64=i64, float_ld=False)


@pytest.mark.parametrize("world,rank", [(2, 1), (4, 3)])
@pytest.mark.parametrize("float_ld", [True, False])
def test_rank_slices(tmp_path, world, rank, float_ld):
    """label and dense: this rank's samples only (a slice that crosses tile borders); keys: all"""
    L, Dn, params = W228
    B = 2 * _tile(228) + (2 if world == 2 else 4)
    _decode_and_compare(tmp_path, L, Dn, params, B, groups=[[f"d{i}" for i in range(0, 26, 2)]],
                        rank=rank, world=world, float_ld=float_ld)


def test_arguments_are_checked_before_the_launch():
    from hugectr_amd import _lib
    L = _lib.lib
    p = ctypes.c_void_p(4096)
    assert L.hctr_raw_decode(None, 4, 3, p, 1, p, None) == -1 and "null" in _lib.last_error()
    assert L.hctr_raw_decode(p, 0, 3, p, 1, p, None) == -1 and "batch" in _lib.last_error()
    assert L.hctr_raw_decode(p, 4, 0, p, 1, p, None) == -1 and "width" in _lib.last_error()
    assert L.hctr_raw_decode(p, 4, 3, p, 0, p, None) == -1 and "n_segments" in _lib.last_error()
    assert L.hctr_raw_decode(ctypes.c_void_p(4100), 4, 3, p, 1, p, None) == -1
    assert "aligned" in _lib.last_error()
