"""interaction_gather(store_pooled=False): the forward does not write the pooled vectors and the
backward reads the training batch's table rows again (hctr_emb_backward_interaction).  Output and
both gradients must be those of the default form (pooled vectors written, then read back), bit for
bit, and the one-GPU DLRM training step that now uses it must train exactly as it did with the
stored vectors (tests/golden/interaction_regather_model.json, recorded with that form)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "interaction_regather_model.json")
EMU = os.environ.get("HCTR_EMU") == "1"
NO_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)


def _embedding(B, S, D, V, dt):
    import hugectr_amd as ha
    from hugectr_amd import _lib
    opt = ha.OptParams(optimizer=_lib.OPT_SGD, lr=0.1, atomic_update=False)
    emb = ha.SparseEmbeddingHash(_lib.EMB_LOCALIZED, B, B, V, D, S, S, 0, opt, out_dtype=dt)
    emb.table().normal_(0, 1)
    return emb


def _forward_backward(emb, mlp, top, between=None):
    """the default form and store_pooled=False on the indexed training batch -> (output, mlp
    gradient, embedding gradient) of each; `between` runs after both forwards"""
    import hugectr_amd as ha
    runs = []
    for store in (True, False):
        m = mlp.clone().requires_grad_()
        got = {}
        out = ha.interaction_gather(m, emb, True, on_emb_grad=lambda d, got=got: got.update(dE=d),
                                    store_pooled=store)
        runs.append((out, m, got))
    if between is not None:
        between()
    for out, _, _ in runs:
        out.backward(top)
    return [(out.detach(), m.grad, got["dE"]) for out, m, got in runs]


def _assert_bit_equal(a, b):
    import torch
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("dtype_name", ["float16", "bfloat16"])
@pytest.mark.parametrize("B,S,D", [(130, 26, 128), (65, 5, 64), (129, 21, 32)] +
                         ([] if EMU else [(65536, 26, 128), (65536 - 777, 26, 128)]))
@pytest.mark.parametrize("full", [False, True])
def test_regather_equals_stored_pooled(dtype_name, B, S, D, full):
    """forward output, mlp gradient and the embedding gradient on_emb_grad receives, bit for bit;
    full: the table has fewer rows than the batch has distinct keys, the rest resolve to no row
    (kInvalidIndex -> zeros); batch sizes that are not a multiple of the grid included"""
    import torch
    dt = getattr(torch, dtype_name)
    vps = 50
    V = S * vps // 4 if full else S * vps
    emb = _embedding(B, S, D, V, dt)
    g = torch.Generator(device="cuda").manual_seed(B + S + D)
    ro = torch.arange(B * S + 1, dtype=torch.int64, device="cuda")
    keys = (torch.randint(0, vps, (B, S), device="cuda", generator=g) +
            torch.arange(S, device="cuda") * vps).reshape(-1)
    emb.index(True, ro, keys)
    vi = emb.value_index(B * S).cpu().numpy().view(np.uint64)
    assert (vi == NO_ROW).any() == full
    n_ins = S + 1
    mlp = torch.randn(B, D, device="cuda", generator=g).to(dt)
    top = torch.randn((B, D + n_ins * (n_ins - 1) // 2 + 1), device="cuda", generator=g).to(dt)
    a, b = _forward_backward(emb, mlp, top)
    _assert_bit_equal(a, b)


def test_index_ahead_between_forward_and_backward():
    """the next batch indexed ahead (new keys inserted, hctr_emb_index_ahead) after the forward and
    before the backward, as HCTR_INDEX_AHEAD=mlp schedules it: the re-gathering backward still sees
    the current batch -- gradients bit-equal to the stored-pooled backward -- and then the update
    of the current batch runs on top of it"""
    import torch
    B, S, D, vps = 260 if EMU else 65536 - 777, 26, 128, 400
    dt = torch.float16
    emb = _embedding(B, S, D, S * vps, dt)
    g = torch.Generator(device="cuda").manual_seed(7)
    ro = torch.arange(B * S + 1, dtype=torch.int64, device="cuda")
    off = torch.arange(S, device="cuda") * vps
    cur = (torch.randint(0, vps // 2, (B, S), device="cuda", generator=g) + off).reshape(-1)
    nxt = (torch.randint(vps // 2, vps, (B, S), device="cuda", generator=g) + off).reshape(-1)
    emb.index(True, ro, cur)
    n_cur = emb.get_vocabulary_size()
    n_ins = S + 1
    mlp = torch.randn(B, D, device="cuda", generator=g).to(dt)
    top = torch.randn((B, D + n_ins * (n_ins - 1) // 2 + 1), device="cuda", generator=g).to(dt)
    a, b = _forward_backward(emb, mlp, top, between=lambda: emb.index_ahead(ro, nxt))
    torch.cuda.synchronize()
    assert emb.get_vocabulary_size() > n_cur, "the batch indexed ahead inserted no key"
    _assert_bit_equal(a, b)
    emb.backward(b[2])
    emb.update_params()
    emb.index_adopt()
    torch.cuda.synchronize()


# ---- the DLRM graph through Model.train(), against the stored-pooled form's record ---------------
def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def model_record(mode, steps=4, B=4096):
    """bench.py's DLRM (fp16, SGD, overlap on) at 1/20000 of the Criteo-1TB table, `steps` training
    steps on seeded power-law batches under HCTR_INDEX_AHEAD=mode -> losses, a digest of every
    dense parameter and a digest of the table's rows in use"""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    prev = os.environ.get("HCTR_INDEX_AHEAD")
    os.environ["HCTR_INDEX_AHEAD"] = mode
    try:
        sizes = [max(1, v // 20000) for v in bench.CRITEO_1TB]
        S = len(sizes)
        m = bench.build_dlrm(B, sizes, 128, "fp16", 1)
        gk = torch.Generator(device="cuda").manual_seed(1234)
        gd = torch.Generator(device="cuda").manual_seed(99)
        ro = torch.arange(0, B * S + 1, dtype=torch.int64, device="cuda")
        batches = []
        for _ in range(steps + 1):
            keys = bench.gen_keys(gk, B, sizes, 1.1, "cuda")
            dense = torch.rand((B, bench.DENSE_DIM), device="cuda", generator=gd)
            lab = (torch.rand((B, 1), device="cuda", generator=gd) < 0.5).float()
            batches.append({"dense": dense, "label": lab, "sparse": {"data1": (ro, keys)}})
        m.reader_override = bench._CycleReader(batches)
        m.compile()
        losses = []
        for _ in range(steps):
            assert m.train()
            losses.append(float(m.get_current_loss()).hex())
        m._drain_prefetch()
        torch.cuda.synchronize()
        emb = m._emb["sparse_embedding1"][2]
        n = emb.get_vocabulary_size()
        dense = [q.detach().float().cpu().numpy() for _, q in sorted(m._mods.named_parameters())]
        rec = {"losses": losses, "dense_sha256": _digest(dense), "rows": n,
               "table_sha256": _digest([emb.table()[:n].cpu().numpy()])}
        del m, emb
        return rec
    finally:
        if prev is None:
            os.environ.pop("HCTR_INDEX_AHEAD", None)
        else:
            os.environ["HCTR_INDEX_AHEAD"] = prev


@pytest.mark.skipif(EMU, reason="the model's GEMMs and the recorded bits are the device's")
@pytest.mark.parametrize("mode", ["0", "mlp", "tail"])
def test_model_trains_as_recorded(mode):
    """Model.train() with the re-gathering backward == the same steps with the pooled vectors
    stored (recorded): losses, dense weights and touched table rows, bit for bit -- with the index
    stage in line, under the top MLP (mlp) and behind the update (tail)"""
    with open(GOLDEN) as f:
        want = json.load(f)[mode]
    assert model_record(mode) == want


if __name__ == "__main__":
    # python tests/test_interaction_regather_gpu.py OUT.json: record the fixture on the GPU
    json.dump({mode: model_record(mode) for mode in ("0", "mlp", "tail")},
              open(sys.argv[1], "w"), indent=1)
