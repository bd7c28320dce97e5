"""Records what the REFERENCE itself computes for the tests that pin this project against it, so
those tests run without the reference checkout:

* ref_murmur3.npz            -- the reference's MurmurHash3 functor (oracle/_ref/libref_hash.so,
                                compiled from its header) on the keys of
                                tests/test_hash_gpu.py::test_murmur_hash_bit_exact
* ref_sok_format.npz         -- the bytes the reference's SOK dump functions write (meta file, array
                                file heads) for the cases of tests/test_sok_format_cpu.py
* reference_script_usage.json -- the `hugectr` names, keywords and Model verbs the reference's
                                sample / test scripts use (tests/test_api_surface_cpu.py)

Needs the reference checkout and `make -C oracle ref`.  Run:  python tests/golden/make_ref_fixtures.py
(deterministic; the tests that run where the reference is mounted check the records are current)."""
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)


def murmur3():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_hash.so"))
    out = {}
    for kb in (4, 8):  # the keys test_murmur_hash_bit_exact draws
        rng = np.random.default_rng(0)
        if kb == 4:
            keys = rng.integers(0, 2**32 - 1, size=5000, dtype=np.uint64).astype(np.int64)
            k, fn = keys.astype(np.uint32), L.ref_murmur3_u32_many
        else:
            keys = rng.integers(-2**62, 2**62, size=5000, dtype=np.int64)
            k, fn = keys, L.ref_murmur3_i64_many
        h = np.empty(keys.size, np.uint32)
        fn(ctypes.c_void_p(k.ctypes.data), ctypes.c_size_t(k.size), ctypes.c_void_p(h.ctypes.data))
        out[f"keys{kb}"], out[f"hash{kb}"] = keys, h
    np.savez_compressed(os.path.join(HERE, "ref_murmur3.npz"), **out)


def sok_format():
    import test_sok_format_cpu as t
    from hugectr_amd import sok_format as fmt
    ref = t._reference_namespace()
    out = {"file_head_length": np.int64(ref["file_head_length"]),
           "meta_info_offset_opt_name_3": np.int64(
               ref["get_meta_info_offset"](ref["MetaVarType"].OptName, 3))}
    with tempfile.TemporaryDirectory() as d:
        infos = t._infos(fmt)
        for name, sub in (("meta_info", infos), ("meta_info_one", infos[:1])):
            rinfos = []
            for i in sub:
                r = ref["SOK_var_info"]()
                r.opt_name, r.key_type, r.emb_type = i.opt_name, i.key_type, i.emb_type
                r.emb_num, r.emb_length, r.emb_name = i.emb_num, i.emb_length, i.emb_name
                rinfos.append(r)
            os.makedirs(os.path.join(d, name))
            ref["save_meta_file"](os.path.join(d, name), rinfos)
            out[name] = np.fromfile(os.path.join(d, name, "meta_info"), np.uint8)
        for ftype, var, dtype in t.HEAD_CASES:
            info = ref["SOK_var_info"]()
            info.emb_name = "some/table:0"
            b = os.path.join(d, t._head_key(ftype, var, dtype))
            ref["write_file_head"](b, info, ftype, var, fmt.DTYPE_INDEX[np.dtype(dtype)])
            with open(b, "ba+") as f:  # as save_table_to_filesystem_* appends
                t._head_array(dtype).tofile(f)
            out[t._head_key(ftype, var, dtype)] = np.fromfile(b, np.uint8)
    np.savez_compressed(os.path.join(HERE, "ref_sok_format.npz"), **out)


def script_usage():
    import test_api_surface_cpu as t
    with open(t.USAGE, "w") as f:
        json.dump(t.record(), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    murmur3()
    sok_format()
    script_usage()
