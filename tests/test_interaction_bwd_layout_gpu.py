"""interaction_bwd16_kernel behind its four entries (hctr_interaction_bwd, _bwd_indexed,
_bwd_indexed_scatter, _bwd_gather): the tile's LDS image, the transposed operand reads and the
packed 8-byte write-back of the accumulators move data only, so

  * both gradients are, bit for bit, what the kernel computed before that layout: sha256 digests
    recorded from the parent's library by tools/record_interaction_bwd_golden.py (cases, inputs and
    runner are imported from there) in tests/golden/interaction_bwd_layout.json.  Not under
    HCTR_EMU=1: the host interpreter's MFMA is a model, its bits are not the hardware's;
  * every output lies between two guard regions of a sentinel that must survive the call (the idea
    of _Guarded in test_interaction_matrix_gpu.py), for every case, W = 128 / n_emb = 26 at every B
    among them;
  * the same shapes meet a float64 dX = (dM + dM^T) X within the tolerances of
    test_interaction_matrix_gpu._tol for the backward, 4 eps relative and 32 eps absolute -- this
    half also runs under HCTR_EMU=1 (there only shapes up to W = 32, or B = 1: the interpreter runs
    a wide sample in about a tenth of a second) and still says something should the golden file
    ever be re-recorded."""
import json
import os
import sys

import numpy as np
import pytest

from util import assert_close

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_interaction_bwd_golden as rec  # noqa: E402

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
EPS = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}
SENTINEL = -1536.0  # exact in fp16 and bf16, far outside anything the kernels compute here

CASES = rec.cases()
if EMU:
    CASES = [c for c in CASES if c[0] <= 32 or c[3] == 1]


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)["cases"]


class _Guards:
    """alloc() for rec.run: every output inside a larger allocation of SENTINEL, at least one row
    (rounded up to 16 bytes) on either side, checked after the call"""

    def __init__(self):
        self.checked = 0

    def __call__(self, shape, dt):
        import torch
        n = int(np.prod(shape))
        pad = -(-int(np.prod(shape[1:])) // 8) * 8
        buf = torch.full((pad + n + pad,), SENTINEL, dtype=dt, device="cuda")
        t = buf[pad:pad + n].view(*shape)
        assert t.data_ptr() % 16 == 0

        def after():
            assert bool((buf[:pad] == SENTINEL).all()), f"{tuple(shape)}: wrote in front of its rows"
            assert bool((buf[pad + n:] == SENTINEL).all()), f"{tuple(shape)}: wrote behind its rows"
            self.checked += 1
        return t, after


def _reference(inp):
    """float64 (mlp_grad, emb_grad) of the case's rounded inputs"""
    W, n_emb, _, B, _ = inp.case
    f64 = lambda t: t.float().numpy().astype(np.float64)  # noqa: E731
    X = np.concatenate([f64(inp.mlp)[:, None, :], f64(inp.emb)], axis=1)
    top = f64(inp.top)
    n, m = np.tril_indices(n_emb + 1, -1)
    dM = np.zeros((B, n_emb + 1, n_emb + 1))
    dM[:, n, m] = top[:, W:-1]
    dX = (dM + dM.transpose(0, 2, 1)) @ X
    return top[:, :W] + dX[:, 0], dX[:, 1:]


@pytest.mark.parametrize("case", CASES, ids=rec.case_id)
def test_bits_guards_and_reference(case, golden):
    W, n_emb, dt_name, B, entry = case
    if os.environ.get("HCTR_INTER_WAVES"):
        pytest.skip("HCTR_INTER_WAVES is set: the batch sizes assume the default grid of 2048")
    want = golden[rec.case_id(case)]
    inp = rec.Inputs(case)
    guards = _Guards()
    got = rec.run(inp, guards)
    assert guards.checked == 2
    if got is None:
        # the entry has no kernel for this shape (out_len % 8 != 0 behind row_of / value_index)
        assert want == {"refused": True}
        return
    mlp_grad, emb_grad, emb_grad_rows = got
    what = rec.case_id(case)
    tol = (4 * EPS[dt_name], 32 * EPS[dt_name])
    want_mg, want_eg = _reference(inp)
    assert_close(mlp_grad.float().cpu().numpy(), want_mg, *tol, what + " mlp grad")
    assert_close(emb_grad_rows.float().cpu().numpy(), want_eg, *tol, what + " emb grad")
    if not EMU:
        assert want == {"mlp_grad": rec.digest(mlp_grad), "emb_grad": rec.digest(emb_grad)}, \
            what + ": not the recorded bits"


def test_the_golden_file_lists_exactly_these_cases(golden):
    assert sorted(golden) == sorted(rec.case_id(c) for c in rec.cases())
    reached = [c for c in rec.cases() if "refused" not in golden[rec.case_id(c)]]
    # the MFMA kernel is reached through every entry, at every width and B, in both types
    for e in rec.ENTRIES:
        for W in rec.WS:
            assert any(c[4] == e and c[0] == W and c[1] in (5, 10, 21, 26) for c in reached)
    pairs = {(B, e) for B in rec.BS for e in rec.ENTRIES}
    assert {(c[3], c[4]) for c in reached if c[:2] == (128, 26)} == pairs
    assert {(c[3], c[4]) for c in reached if c[:2] != (128, 26) and rec.reaches_mfma(*c[:2])} == pairs
