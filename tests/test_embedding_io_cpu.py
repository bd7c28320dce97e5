"""CPU: the bytes of embedding_dump / embedding_load (hugectr_amd/embedding_io.py) against bytes
built by hand from the layout of the reference's EmbeddingParameterIO
(R/HugeCTR/embedding_storage/weight_io/parameter_IO.cpp:179-260, 551-578)."""
import os
import struct

import numpy as np
import pytest

from hugectr_amd import embedding_io as eio


def _tables(rng, key_dtype, spec=((0, 5, 4), (1, 7, 3), (2, 2, 8))):
    out = {}
    for tid, n, ev in spec:
        keys = rng.permutation(1000)[:n].astype(key_dtype)
        out[tid] = (keys, rng.standard_normal((n, ev)).astype("<f4"))
    return out


@pytest.mark.parametrize("key_dtype,code", [("<i8", 1), ("<u4", 0)])
def test_meta_data_and_heads_are_the_reference_bytes(tmp_path, key_dtype, code):
    rng = np.random.default_rng(1)
    tabs = _tables(rng, key_dtype)
    eio.write_collection(str(tmp_path), 0, tabs, key_dtype)
    d = tmp_path / "embedding_collection_0"
    want = struct.pack("<5i", 3, code, 0, 0, 8)          # head: n, key type, value type, 0, max ev
    want += struct.pack("<3i", 0, 1, 2)                  # table ids, ascending
    want += struct.pack("<3Q", 5, 7, 2)                  # key_num, at byte 32: not 8-byte aligned
    want += struct.pack("<3i", 4, 3, 8)                  # ev_size
    assert len(want) == 20 + 16 * 3
    assert (d / "meta_data").read_bytes() == want
    ksz = 8 if code else 4
    for i, (tid, (keys, w)) in enumerate(sorted(tabs.items())):
        kb = (d / f"key{i}").read_bytes()
        wb = (d / f"weight{i}").read_bytes()
        assert kb[:128] == struct.pack("<2i", 1, i) + bytes(120)
        assert wb[:128] == struct.pack("<2i", 2, i) + bytes(120)
        assert kb[128:] == keys.astype(key_dtype).tobytes() and len(kb) == 128 + ksz * keys.size
        assert wb[128:] == w.tobytes()
    assert sorted(os.listdir(d)) == sorted(["meta_data"] + [f"{s}{i}" for s in ("key", "weight")
                                                            for i in range(3)])


def test_round_trip_with_optimizer_state(tmp_path):
    rng = np.random.default_rng(2)
    tabs = {t: (k, w, [w * 2, w * 3]) for t, (k, w) in _tables(rng, "<i8").items()}
    eio.write_collection(str(tmp_path), 3, tabs, "<i8", optimizer=0)
    meta = eio.read_meta(str(tmp_path), 3)
    assert meta.table_ids == [0, 1, 2] and meta.key_dtype == np.dtype("<i8")
    for t, (k, w, st) in tabs.items():
        with eio.TableFiles(str(tmp_path), 3, t) as f:
            assert f.opt_state == (2, 0)
            assert (f.read_keys() == k).all() and (f.read_weights() == w).all()
            got = f.read_states()
            assert (got[0] == st[0]).all() and (got[1] == st[1]).all()
    head = (tmp_path / "embedding_collection_3" / "opt_state1").read_bytes()[:128]
    assert head == struct.pack("<4i", 3, 1, 2, 0) + bytes(112)


def test_subset_dumps_as_key0_key1_and_is_found_by_id(tmp_path):
    rng = np.random.default_rng(3)
    tabs = _tables(rng, "<i8", spec=((4, 6, 4), (1, 3, 4)))
    eio.write_collection(str(tmp_path), 0, tabs)
    d = tmp_path / "embedding_collection_0"
    assert sorted(os.listdir(d)) == ["key0", "key1", "meta_data", "weight0", "weight1"]
    meta = eio.read_meta(str(tmp_path), 0)
    assert meta.table_ids == [1, 4] and meta.file_index(4) == 1 and meta.file_index(1) == 0
    for t in (1, 4):
        with eio.TableFiles(str(tmp_path), 0, t) as f:
            assert (f.read_keys() == tabs[t][0]).all() and (f.read_weights() == tabs[t][1]).all()
    with pytest.raises(eio.EmbeddingIOError, match="not in this dump"):
        eio.TableFiles(str(tmp_path), 0, 0)


def test_refusals(tmp_path):
    rng = np.random.default_rng(4)
    eio.write_collection(str(tmp_path), 0, _tables(rng, "<i8"))
    d = tmp_path / "embedding_collection_0"
    good = (d / "meta_data").read_bytes()
    # a 35-byte meta_data (MetaDataValidLength, data_info.hpp:22-25)
    (d / "meta_data").write_bytes(good[:35])
    with pytest.raises(eio.EmbeddingIOError, match="too small"):
        eio.read_meta(str(tmp_path), 0)
    (d / "meta_data").write_bytes(good)
    # a key file one key short
    kb = (d / "key1").read_bytes()
    (d / "key1").write_bytes(kb[:-8])
    with pytest.raises(eio.EmbeddingIOError, match="table id 1.*key file holds 6 keys"):
        eio.TableFiles(str(tmp_path), 0, 1)
    (d / "key1").write_bytes(kb)
    eio.TableFiles(str(tmp_path), 0, 1).close()
    # a weight file for another ev_size (7 keys x 4 instead of 7 x 3)
    (d / "weight1").write_bytes(eio.file_head(eio.KIND_WEIGHT, 1) + bytes(7 * 4 * 4))
    with pytest.raises(eio.EmbeddingIOError, match="table id 1.*weight file"):
        eio.TableFiles(str(tmp_path), 0, 1)
    # a file whose head names another kind
    (d / "weight0").write_bytes(eio.file_head(eio.KIND_KEY, 0) + bytes(5 * 4 * 4))
    with pytest.raises(eio.EmbeddingIOError, match="head"):
        eio.TableFiles(str(tmp_path), 0, 0)


def test_rewriting_collection_1_leaves_collection_0_intact(tmp_path):
    rng = np.random.default_rng(5)
    eio.write_collection(str(tmp_path), 0, _tables(rng, "<i8"))
    eio.write_collection(str(tmp_path), 1, _tables(rng, "<i8"))
    d0 = tmp_path / "embedding_collection_0"
    before = {n: (d0 / n).read_bytes() for n in os.listdir(d0)}
    (tmp_path / "embedding_collection_1" / "stale").write_bytes(b"x")
    eio.write_collection(str(tmp_path), 1, _tables(rng, "<i8", spec=((0, 4, 2),)))
    assert {n: (d0 / n).read_bytes() for n in os.listdir(d0)} == before
    assert sorted(os.listdir(tmp_path / "embedding_collection_1")) == ["key0", "meta_data", "weight0"]


def test_per_rank_offsets_of_a_vocab_37_table_on_two_ranks(tmp_path):
    ev = 6
    n0 = eio.static_shard_key_count(37, 2, 0)
    n1 = eio.static_shard_key_count(37, 2, 1)
    assert (n0, n1) == (19, 18)
    assert eio.weight_offset(0, ev) == 128
    assert eio.weight_offset(n0, ev) == 128 + 19 * ev * 4   # NOT (19 * 8) * ev * 4 (:395-396)
    assert eio.key_offset(n0, "<i8") == 128 + 19 * 8 and eio.key_offset(n0, "<u4") == 128 + 19 * 4
    # two writers, rank 1 first: the file is the same as one written in one piece
    w = np.arange(37 * ev, dtype="<f4").reshape(37, ev)
    keys = np.concatenate([np.arange(0, 37, 2), np.arange(1, 37, 2)]).astype("<i8")
    meta = eio.MetaData([0], {0: 37}, {0: ev}, np.dtype("<i8"))
    eio.create_collection(str(tmp_path), 0, meta, opt_state=(1, 3))
    with eio.TableFiles(str(tmp_path), 0, 0, "r+") as f:
        for first, n in ((n0, n1), (0, n0)):
            f.write("key", first, keys[first:first + n])
            f.write("weight", first, w[keys[first:first + n]])
            f.write("opt_state", first, -w[keys[first:first + n]], 0)
    d = tmp_path / "embedding_collection_0"
    assert (d / "weight0").read_bytes()[128:] == w[keys].tobytes()
    assert (d / "key0").read_bytes()[128:] == keys.tobytes()
    assert (d / "opt_state0").read_bytes()[128:] == (-w[keys]).tobytes()
    assert eio.state_offset(1, 37, 19, ev) == 128 + (37 + 19) * ev * 4


def test_module_imports_without_torch_or_the_library():
    import subprocess
    import sys
    code = ("import sys, importlib.util as u; "
            "s = u.spec_from_file_location('eio', sys.argv[1]); m = u.module_from_spec(s); sys.modules['eio'] = m; "
            "s.loader.exec_module(m); assert 'torch' not in sys.modules; print(m.FILE_HEAD_NBYTES)")
    out = subprocess.run([sys.executable, "-c", code, eio.__file__], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "128", out.stderr
