"""FusedMLP with the data gradient, the ReLU mask of the layer below and its bias partials in one
kernel (HCTR_DGRAD_FUSED, hugectr_amd/dense.py; hctr_gemm_nt16_drelu), and the transposed 16-bit
weights that kernel reads.

  * HCTR_DGRAD_FUSED=1: one step of a flattened module through DenseGradFinish, gradients only and
    SGD mode, equals bit for bit the same step assembled here from the C entries (as the last case
    of tests/test_dense_finish_gpu.py does for the unfused step).  dims 64-128-256-128-1 fuses the
    masks of layers 0 and 1 into the data gradients of layers 1 and 2; 13-128-256-1 has the skinny
    first layer below layer 1, which folds its own mask: nothing fuses there.
  * after sgd_step, ftrl_step, finish(sgd=True), refresh_shadow and a load of other weights (what
    Model.load_dense_weights does: masters written, then refresh_shadow) every transposed view
    holds w16.t(), bit for bit.
  * forward + backward captured in a HIP graph and replayed twice gives the eager bits.
  * HCTR_DGRAD_FUSED=0: the bits of the parent commit.  PARENT_DIGEST was printed by
    `_seeded_step_digest()` (PARENT_DIGEST_SKINNY: of dims 13-128-256-1) run on the parent commit's tree (library and hugectr_amd package of
    commit af16821, one MI355X, the same PyTorch-ROCm build as the suite's): sha256 over flat_g after a
    gradients-only step and flat_w / flat_w16 after an SGD-mode step of the seeded fp16 module below."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUM, COLSUM, HEAD, SKINNY, DIRECT = range(5)
LR, GS = 0.01, 1.0 / 1024
PARENT_DIGEST_SKINNY = "5527a8486945e05da9775d60b19afd4db515f726228c145752b197be6e71b6ed"
PARENT_DIGEST = "11df766c195bf4809db2effbc37a1ebf38bfff0b8d481eed63789ec0e093807a"


def _dt(name):
    import torch
    return (torch.bfloat16, 2) if name == "bf16" else (torch.float16, 1)


def _module(dims, tdt, seed, ftrl=False):
    import torch
    from hugectr_amd.dense import FusedMLP
    torch.manual_seed(seed)
    m = FusedMLP(dims, last_relu=False, dtype=tdt).cuda()
    m.flatten(ftrl_state=ftrl)
    return m


def _batch(B, feats, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, feats), generator=g).cuda()
    lab = (torch.rand((B, 1), generator=g) < 0.4).float().cuda()
    return x, lab


def _step(m, x, lab, gs):
    out = m.forward_bce(x, lab, gs)
    out.backward(_ones(out))
    return out


def _ones(t):
    import torch
    return torch.ones_like(t)


def _seeded_step_digest(dims=(64, 128, 256, 128, 1)):
    """sha256 over what one seeded step leaves: fp16, B = 384, the module in a DenseGradFinish --
    flat_g after finish(sgd=False), then flat_w and flat_w16 after a second step finished with
    sgd=True.  dims 13-128-256-1 takes its fp32 input through the skinny first layer"""
    import torch
    from hugectr_amd.dense import DenseGradFinish
    m = _module(list(dims), torch.float16, 11)
    fin = DenseGradFinish([m])
    x, lab = _batch(384, dims[0], 12)
    if dims[0] > 16:
        x = x.half()
    h = hashlib.sha256()
    _step(m, x, lab, 1024.0 / 384)
    fin.finish(sgd=False)
    torch.cuda.synchronize()
    h.update(m.flat_g.cpu().numpy().tobytes())
    _step(m, x, lab, 1024.0 / 384)
    fin.finish(sgd=True, lr=LR, grad_scale=GS)
    torch.cuda.synchronize()
    h.update(m.flat_w.cpu().numpy().tobytes())
    h.update(m.flat_w16.view(torch.int16).cpu().numpy().tobytes())
    return h.hexdigest()


def test_switch_off_gives_the_parent_commits_bits(monkeypatch):
    monkeypatch.setenv("HCTR_DGRAD_FUSED", "0")
    assert _seeded_step_digest() == PARENT_DIGEST


@pytest.mark.parametrize("mode", ["1", "0"])
def test_skinny_first_module_gives_the_parent_commits_bits(monkeypatch, mode):
    """nothing fuses in 13-128-256-1, whatever the switch says: the parent's bits either way"""
    monkeypatch.setenv("HCTR_DGRAD_FUSED", mode)
    assert _seeded_step_digest((13, 128, 256, 1)) == PARENT_DIGEST_SKINNY


def _colsum_into(g, off, n, partials, tiles, flat_w, flat_w16):
    """hctr_dense_grad_finish with one COLSUM segment: g[off : off + n] = the tiles added up"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    t = np.zeros((1, 16), dtype=np.int64)
    t[0, :13] = (COLSUM, partials.data_ptr(), tiles, n, 0, 0, g.data_ptr(), flat_w.data_ptr(),
                 flat_w16.data_ptr(), off, 0, int(flat_w16.dtype == torch.bfloat16), 0)
    table = torch.from_numpy(t).cuda()
    check(lib.hctr_dense_grad_finish(ptr(table), 1, lib.hctr_dense_seg_blocks(COLSUM, n), 0, 0.0, 1.0,
                                     None, stream_ptr()))
    torch.cuda.synchronize()


def _groups(B):
    g = 16
    while g > 1 and B % g:
        g //= 2
    return g


def _by_hand(m, x, lab, gs, tdt, code):
    """the step of dims 64-128-256-128-1 from the C entries: (flat_g, loss)"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    sp = stream_ptr()
    B = x.shape[0]
    w16, b16 = [t.clone() for t in m._w16], [t.clone() for t in m._b16]
    x16 = x.to(tdt)
    y0 = torch._addmm_activation(b16[0], x16, w16[0].t(), use_gelu=False)
    y1 = torch._addmm_activation(b16[1], y0, w16[1].t(), use_gelu=False)
    y2 = torch._addmm_activation(b16[2], y1, w16[2].t(), use_gelu=False)
    g = torch.zeros_like(m.flat_g)
    offw, offb = m._offs

    def view(off, n):
        return g[off:off + n]

    def wgrad(dz, xin, layer):
        o, i = dz.shape[1], xin.shape[1]
        G = _groups(B)
        p = torch.bmm(dz.view(G, B // G, o).transpose(1, 2), xin.view(G, B // G, i))
        check(lib.hctr_sum_groups(G, o * i, ptr(p), code, ptr(view(offw[layer], o * i)), sp))

    ws = torch.empty(lib.hctr_logit_head_workspace_bytes(128) // 4, dtype=torch.float32, device="cuda")
    dx2 = torch.empty_like(y2)
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    check(lib.hctr_logit_head(B, 128, ptr(y2), ptr(w16[3]), ptr(b16[3]), ptr(lab), gs, ptr(dx2),
                              ptr(view(offw[3], 128)), ptr(view(offb[3], 1)), ptr(loss), ptr(ws), code, sp))
    ws = torch.empty(lib.hctr_relu_bwd_bias_workspace_bytes(B, 128) // 4, dtype=torch.float32, device="cuda")
    dz2 = torch.empty_like(dx2)
    check(lib.hctr_relu_bwd_bias(B, 128, ptr(dx2), ptr(y2), ptr(dz2), ptr(view(offb[2], 128)), ptr(ws), code, sp))
    wgrad(dz2, y1, 2)
    # layer 2's data gradient with layer 1's mask and bias partials: N = 256, K = 128
    tiles = lib.hctr_gemm_nt16_drelu_tiles(B, 256)
    part = torch.empty(tiles * 256, dtype=torch.float32, device="cuda")
    dz1 = torch.empty_like(y1)
    wt = w16[2].t().contiguous()
    check(lib.hctr_gemm_nt16_drelu(B, 256, 128, ptr(dz2), 128, ptr(wt), 128, ptr(y1), ptr(dz1), 256, ptr(part),
                                   code, sp))
    _colsum_into(g, offb[1], 256, part, tiles, m.flat_w, m.flat_w16)
    wgrad(dz1, y0, 1)
    # layer 1's data gradient with layer 0's: N = 128, K = 256
    tiles = lib.hctr_gemm_nt16_drelu_tiles(B, 128)
    part = torch.empty(tiles * 128, dtype=torch.float32, device="cuda")
    dz0 = torch.empty_like(y0)
    wt = w16[1].t().contiguous()
    check(lib.hctr_gemm_nt16_drelu(B, 128, 256, ptr(dz1), 256, ptr(wt), 256, ptr(y0), ptr(dz0), 128, ptr(part),
                                   code, sp))
    _colsum_into(g, offb[0], 128, part, tiles, m.flat_w, m.flat_w16)
    wgrad(dz0, x16, 0)
    torch.cuda.synchronize()
    return g, loss


def _transposes_hold(m):
    import torch
    torch.cuda.synchronize()
    seen = 0
    for w, wt in zip(m._w16, m._w16t):
        if wt is not None:
            seen += 1
            assert torch.equal(wt.view(torch.int16), w.t().contiguous().view(torch.int16))
    return seen


@pytest.mark.parametrize("B", [384, 130])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fused_step_equals_the_step_from_the_c_entries(monkeypatch, dtype, B):
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    from hugectr_amd.dense import DenseGradFinish
    monkeypatch.setenv("HCTR_DGRAD_FUSED", "1")
    tdt, code = _dt(dtype)
    m = _module([64, 128, 256, 128, 1], tdt, 5)
    fin = DenseGradFinish([m])
    x, lab = _batch(B, 64, 6)
    x = x.to(tdt)
    gs = 1024.0 / B
    w_before, w16_before = m.flat_w.clone(), m.flat_w16.clone()
    assert _transposes_hold(m) == 2
    g, loss = _by_hand(m, x, lab, gs, tdt, code)
    w_ref, w16_ref = w_before.clone(), w16_before.clone()
    check(lib.hctr_sgd_shadow(w_ref.numel(), LR, GS, ptr(w_ref), ptr(g), ptr(w16_ref), code, stream_ptr()))

    out = _step(m, x, lab, gs)
    kinds = [(lw.w_seg[0] if lw.w_seg else None, lw.b_seg[0] if lw.b_seg else None) for lw in m._lw]
    assert kinds == [(SUM, COLSUM), (SUM, COLSUM), (SUM, COLSUM), (HEAD, None)]
    # layers 0 and 1 took their partial rows from the GEMM: one row per tile of the launch
    assert [m._lw[i].b_seg[2] for i in (0, 1)] == [lib.hctr_gemm_nt16_drelu_tiles(B, 128),
                                                   lib.hctr_gemm_nt16_drelu_tiles(B, 256)]
    assert all(lw.pre is None for lw in m._lw)
    fin.finish(sgd=False)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), loss)
    assert torch.equal(m.flat_g, g)
    assert torch.equal(m.flat_w, w_before)
    out = _step(m, x, lab, gs)
    fin.finish(sgd=True, lr=LR, grad_scale=GS)
    torch.cuda.synchronize()
    assert torch.equal(m.flat_w, w_ref) and torch.equal(m.flat_w16, w16_ref)
    assert not torch.equal(m.flat_w, w_before)
    assert _transposes_hold(m) == 2
    # released: every layer finishes its own gradients, the bias sums from the same partial rows
    fin.release()
    m.flat_g.zero_()
    m.flat_w.copy_(w_before)
    m.refresh_shadow()
    out = _step(m, x, lab, gs)
    torch.cuda.synchronize()
    assert torch.equal(m.flat_g, g) and torch.equal(out.detach(), loss)


@pytest.mark.parametrize("B", [384, 130])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_skinny_first_layer_keeps_its_own_mask(monkeypatch, dtype, B):
    """13-128-256-1: layer 1 could carry a mask, but the layer below is the skinny first layer, whose
    backward folds it -- the step is the unfused one, bit for bit the switch at 0"""
    import torch
    from hugectr_amd.dense import DenseGradFinish
    tdt, _ = _dt(dtype)
    x, lab = _batch(B, 13, 8)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HCTR_DGRAD_FUSED", mode)
        m = _module([13, 128, 256, 1], tdt, 7)
        fin = DenseGradFinish([m])
        assert m._skinny_first(x)
        _step(m, x, lab, 1024.0 / B)
        kinds = [(lw.w_seg[0] if lw.w_seg else None, lw.b_seg[0] if lw.b_seg else None) for lw in m._lw]
        assert kinds == [(SKINNY, None), (SUM, COLSUM), (HEAD, None)]
        fin.finish(sgd=False)
        g = m.flat_g.clone()
        _step(m, x, lab, 1024.0 / B)
        fin.finish(sgd=True, lr=LR, grad_scale=GS)
        assert _transposes_hold(m) == (1 if mode == "1" else 0)
        res[mode] = (g, m.flat_w.clone(), m.flat_w16.clone())
    for a, b in zip(res["1"], res["0"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_transposed_weights_follow_every_refresh(monkeypatch, dtype):
    import torch
    from hugectr_amd.dense import DenseGradFinish
    monkeypatch.setenv("HCTR_DGRAD_FUSED", "1")
    tdt, _ = _dt(dtype)
    m = _module([64, 128, 256, 128, 1], tdt, 21, ftrl=True)
    x, lab = _batch(130, 64, 22)
    x = x.to(tdt)

    def moved(step):
        before = m.flat_w16t.clone()
        _step(m, x, lab, 1024.0 / 130)
        step()
        assert _transposes_hold(m) == 2
        assert not torch.equal(before, m.flat_w16t)

    moved(lambda: m.sgd_step(0.05, GS))
    moved(lambda: m.ftrl_step(0.05, 0.1, 1e-6, 1e-5, GS))
    fin = DenseGradFinish([m])
    moved(lambda: fin.finish(sgd=True, lr=0.05, grad_scale=GS))
    with fin.one_transpose():  # (the model's per-module steps: one launch at the end)
        _step(m, x, lab, 1024.0 / 130)
        fin.finish(sgd=False)
        m.sgd_step(0.05, GS)
    assert _transposes_hold(m) == 2
    fin.release()
    before = m.flat_w16t.clone()
    with torch.no_grad():
        m.flat_w.mul_(1.5)
    m.refresh_shadow()
    assert _transposes_hold(m) == 2 and not torch.equal(before, m.flat_w16t)
    other = _module([64, 128, 256, 128, 1], tdt, 23)
    before = m.flat_w16t.clone()
    m.load_state_dict(other.state_dict())
    assert m.weights[1].data_ptr() == m.flat_w[m._offs[0][1]:].data_ptr()  # (still views of flat_w)
    m.refresh_shadow()
    assert _transposes_hold(m) == 2 and not torch.equal(before, m.flat_w16t)
    assert torch.equal(m.flat_w16t, other.flat_w16t)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_captured_forward_and_backward_replays_the_eager_bits(monkeypatch, dtype):
    import torch
    from hugectr_amd.dense import DenseGradFinish
    monkeypatch.setenv("HCTR_DGRAD_FUSED", "1")
    tdt, _ = _dt(dtype)
    B = 384
    m = _module([64, 128, 256, 128, 1], tdt, 31)
    fin = DenseGradFinish([m])
    x, lab = _batch(B, 64, 32)
    x = x.to(tdt)
    gs = 1024.0 / B
    _step(m, x, lab, gs)
    fin.finish(sgd=False)
    torch.cuda.synchronize()
    eager = m.flat_g.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up on the capture's side of the allocator)
        _step(m, x, lab, gs)
        fin.finish(sgd=False)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step(m, x, lab, gs)
        fin.finish(sgd=False)
    for _ in range(2):
        m.flat_g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for off, cnt in m._spans:  # (the padding between the parameters belongs to nobody)
            assert torch.equal(m.flat_g[off:off + cnt], eager[off:off + cnt])
