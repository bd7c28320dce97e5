"""hctr_dense_grad_finish: one launch finishes every partial sum of the dense backward.  The
stand-alone entries (hctr_sum_groups, the db of hctr_relu_bwd_bias, hctr_logit_head,
hctr_skinny_fc_bwd) and the finish launch run the same device bodies, so their agreeing proves no
order.  The witness of every segment kind is a float32 restatement of the documented order of
additions, computed here on the CPU from the partials read back from the workspace: the
stand-alone entry AND the finish launch must match it bit for bit (and each other, and fp64
within a tolerance); SGD mode is held against gradients-only + hctr_sgd_shadow."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SUM, COLSUM, HEAD, SKINNY, DIRECT = range(5)
LR, GS = 0.01, 1.0 / 1024   # not powers of two: the update's rounding is visible


def _np32(t):
    return t.detach().float().cpu().contiguous().numpy()


def _same_bits(t, want):
    """a float32 tensor against a float32 array, as bit patterns (-0.0 != 0.0, NaN == the same NaN)"""
    got = _np32(t).reshape(-1)
    want = np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _f32_group_sum(parts):
    """[groups][n] float32: acc = 0; for g in range(groups): acc += in[g]"""
    acc = np.zeros(parts.shape[1], dtype=np.float32)
    for g in range(parts.shape[0]):
        acc = acc + parts[g]
    return acc


def _f32_colsum(partial):
    """[tiles][n] float32: tile group tg = 0..31 adds tiles tg, tg + 32, ... in order, then the 32
    group sums are added in group order"""
    tiles, n = partial.shape
    s = np.zeros((32, n), dtype=np.float32)
    for tg in range(32):
        for t in range(tg, tiles, 32):
            s[tg] = s[tg] + partial[t]
    total = np.zeros(n, dtype=np.float32)
    for k in range(32):
        total = total + s[k]
    return total


def _f32_chunk_sum(partial):
    """[blocks][cols] float32: 16 groups of chunk = ceil(blocks / 16) consecutive blocks, each added
    in block order, then the 16 group sums in group order"""
    blocks, cols = partial.shape
    chunk = (blocks + 15) // 16
    t = np.zeros((16, cols), dtype=np.float32)
    tot = np.zeros(cols, dtype=np.float32)
    with np.errstate(all="ignore"):  # (columns no producer defines may hold anything)
        for g in range(16):
            for b in range(g * chunk, min(blocks, (g + 1) * chunk)):
                t[g] = t[g] + partial[b]
        for g in range(16):
            tot = tot + t[g]
    return tot


def _dt(name):
    import torch
    return (torch.bfloat16, 2) if name == "bf16" else (torch.float16, 1)


def _finish(segs, flats, sgd, loss=None):
    """segs: dicts(kind, src, count, n, k, dst, dst2, flat, src_bf); flats: list of (g, w, w16)"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    t = np.zeros((len(segs), 16), dtype=np.int64)
    block0 = 0
    for r, s in enumerate(segs):
        g, w, w16 = flats[s.get("flat", 0)]
        src = s.get("src")
        t[r, :13] = (s["kind"], src.data_ptr() if src is not None else 0, s.get("count", 0), s["n"],
                     s.get("k", 0), block0, g.data_ptr(), w.data_ptr(), w16.data_ptr(), s["dst"],
                     s.get("dst2", 0), int(w16.dtype == torch.bfloat16),
                     int(src is not None and src.dtype == torch.bfloat16))
        nb = lib.hctr_dense_seg_blocks(s["kind"], s["n"])
        assert nb >= 0
        block0 += nb
    table = torch.from_numpy(t).cuda()
    check(lib.hctr_dense_grad_finish(ptr(table), len(segs), block0, int(sgd), LR, GS, ptr(loss),
                                     stream_ptr()))
    torch.cuda.synchronize()


def _flat(n, tdt, seed=0):
    """(g, w, w16) of n elements: g poisoned, w random, w16 its rounding"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
    g = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    w = torch.randn(n, device="cuda", generator=gen)
    return g, w, w.to(tdt)


@pytest.mark.parametrize("groups,n", [(g, n) for n in (8, 40, 256, 1024) for g in (1, 16)] + [(3, 8)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_finish_sum_groups_segment(n, groups, dtype):
    """split-K partial products -> fp32, g = 0..G-1 in order; the segment starts 16-byte (not 32-byte)
    aligned in the flat buffer"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    tdt, code = _dt(dtype)
    gen = torch.Generator(device="cuda").manual_seed(n + groups)
    p = torch.randn((groups, n), device="cuda", generator=gen).to(tdt)
    want = torch.empty(n, dtype=torch.float32, device="cuda")
    check(lib.hctr_sum_groups(groups, n, ptr(p), code, ptr(want), stream_ptr()))
    flat = _flat(n + 8, tdt)
    _finish([dict(kind=SUM, src=p, count=groups, n=n, dst=4)], [flat], sgd=False)
    got = flat[0][4:4 + n]
    assert torch.equal(got, want)
    order = _f32_group_sum(_np32(p))
    assert _same_bits(want, order) and _same_bits(got, order)
    assert torch.isnan(flat[0][:4]).all() and torch.isnan(flat[0][4 + n:]).all()
    ref = p.double().sum(0)
    assert (got.double() - ref).norm() <= 1e-2 * ref.norm()


# rows 1, 127, 129, 4097 -> 1, 1, 2, 33 tiles of 128 rows; 8193 -> 65 tiles (not multiples of 32)
@pytest.mark.parametrize("rows", [1, 127, 129, 4097, 8193])
@pytest.mark.parametrize("n", [8, 40, 256, 1024])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_finish_colsum_segment(rows, n, dtype):
    """bias tile partials of the ReLU backward: 32 tile groups, each in order, then the groups"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    tdt, code = _dt(dtype)
    gen = torch.Generator(device="cuda").manual_seed(rows + n)
    dy = (torch.randn((rows, n), device="cuda", generator=gen) / 64).to(tdt)
    y = torch.relu(torch.randn((rows, n), device="cuda", generator=gen)).to(tdt)
    nbytes = lib.hctr_relu_bwd_bias_workspace_bytes(rows, n)
    tiles = nbytes // (4 * n)
    assert tiles == (rows + 127) // 128
    ws0 = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    ws1 = torch.empty_like(ws0)
    dz0, dz1 = torch.empty_like(dy), torch.empty_like(dy)
    want = torch.empty(n, dtype=torch.float32, device="cuda")
    check(lib.hctr_relu_bwd_bias(rows, n, ptr(dy), ptr(y), ptr(dz0), ptr(want), ptr(ws0), code,
                                 stream_ptr()))
    check(lib.hctr_relu_bwd_bias_partials(rows, n, ptr(dy), ptr(y), ptr(dz1), ptr(ws1), code,
                                          stream_ptr()))
    flat = _flat(n + 4, tdt)
    _finish([dict(kind=COLSUM, src=ws1, count=tiles, n=n, dst=4)], [flat], sgd=False)
    got = flat[0][4:4 + n]
    assert torch.equal(dz0, dz1)
    assert torch.equal(got, want)
    for ws, out in ((ws0, want), (ws1, got)):
        assert _same_bits(out, _f32_colsum(_np32(ws[:tiles * n]).reshape(tiles, n)))
    ref = (dy.double() * (y > 0)).sum(0)
    assert torch.allclose(got.double(), ref, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("B", [1, 7, 300, 5000])
@pytest.mark.parametrize("K", [4, 256, 260, 2048])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_finish_logit_head_segment(B, K, dtype):
    """block partials of the logit head: dw, db and the loss as hctr_logit_head leaves them"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    tdt, code = _dt(dtype)
    gen = torch.Generator(device="cuda").manual_seed(B + K)
    x = torch.randn((B, K), device="cuda", generator=gen).to(tdt)
    w = (torch.randn((1, K), device="cuda", generator=gen) / K ** 0.5).to(tdt)
    b = torch.tensor([0.1], device="cuda").to(tdt)
    y = (torch.rand((B, 1), device="cuda", generator=gen) < 0.4).float()
    scale = 1.0 / B
    ws = torch.empty(lib.hctr_logit_head_workspace_bytes(K) // 4, dtype=torch.float32, device="cuda")
    dx0, dx1 = torch.empty_like(x), torch.empty_like(x)
    dw = torch.empty(K, dtype=torch.float32, device="cuda")
    db = torch.empty(1, dtype=torch.float32, device="cuda")
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    check(lib.hctr_logit_head(B, K, ptr(x), ptr(w), ptr(b), ptr(y), scale, ptr(dx0), ptr(dw), ptr(db),
                              ptr(loss), ptr(ws), code, stream_ptr()))
    ws1 = torch.empty_like(ws)
    check(lib.hctr_logit_head_partials(B, K, ptr(x), ptr(w), ptr(b), ptr(y), scale, ptr(dx1),
                                       ptr(ws1), code, stream_ptr()))
    blocks = lib.hctr_logit_head_blocks(B, K)
    assert 1 <= blocks <= 1024
    flat = _flat(K + 8, tdt)
    loss1 = torch.empty_like(loss)
    _finish([dict(kind=HEAD, src=ws1, count=blocks, n=K, k=B, dst=0, dst2=K + 4)], [flat],
            sgd=False, loss=loss1)
    assert torch.equal(dx0, dx1)
    assert torch.equal(flat[0][:K], dw)
    assert torch.equal(flat[0][K + 4:K + 5], db)
    assert torch.equal(loss1, loss)
    for wsx, got_dw, got_db, got_loss in ((ws, dw, db, loss),
                                          (ws1, flat[0][:K], flat[0][K + 4:K + 5], loss1)):
        order = _f32_chunk_sum(_np32(wsx[:blocks * (K + 2)]).reshape(blocks, K + 2))
        assert _same_bits(got_dw, order[:K]) and _same_bits(got_db, order[K:K + 1])
        assert _same_bits(got_loss, order[K + 1:] / np.float32(B))
    z = x.double() @ w.double().t() + b.double()
    dz = (torch.sigmoid(z) - y.double()) * scale
    assert torch.allclose(flat[0][:K].double(), (dz.t() @ x.double())[0], rtol=1e-4, atol=1e-7)
    assert torch.allclose(flat[0][K + 4:K + 5].double(), dz.sum().reshape(1), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("B,K,N", [(1000, 13, 256), (777, 16, 128), (300, 7, 136), (3, 13, 512),
                                   (9000, 7, 508), (9300, 13, 64)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_finish_skinny_segment(B, K, N, dtype):
    """block partials of the skinny first layer's backward (matrix-core and vector forms);
    B = 9300 at N = 64 leaves 37 blocks: chunks of 3, a last chunk of 1 and three empty groups"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    tdt, code = _dt(dtype)
    gen = torch.Generator(device="cuda").manual_seed(B + K + N)
    x = torch.randn((B, K), device="cuda", generator=gen)
    y = torch.relu(torch.randn((B, N), device="cuda", generator=gen)).to(tdt)
    dy = (torch.randn((B, N), device="cuda", generator=gen) / B).to(tdt)
    nws = lib.hctr_skinny_fc_bwd_workspace_bytes(N) // 4
    ws0 = torch.empty(nws, dtype=torch.float32, device="cuda")
    ws1 = torch.empty_like(ws0)
    dw = torch.empty((N, K), dtype=torch.float32, device="cuda")
    db = torch.empty(N, dtype=torch.float32, device="cuda")
    check(lib.hctr_skinny_fc_bwd(B, K, N, ptr(x), ptr(dy), ptr(y), ptr(dw), ptr(db), ptr(ws0), code,
                                 stream_ptr()))
    check(lib.hctr_skinny_fc_bwd_partials(B, K, N, ptr(x), ptr(dy), ptr(y), ptr(ws1), code,
                                          stream_ptr()))
    blocks = lib.hctr_skinny_fc_bwd_blocks(B, K, N, ptr(dy), ptr(y))
    assert 1 <= blocks <= 256
    nw = (N * K + 3) // 4 * 4
    flat = _flat(nw + N, tdt)
    _finish([dict(kind=SKINNY, src=ws1, count=blocks, n=N, k=K, dst=0, dst2=nw)], [flat], sgd=False)
    assert torch.equal(flat[0][:N * K].view(N, K), dw)
    assert torch.equal(flat[0][nw:nw + N], db)
    # (each side from its own workspace: the columns K .. 15 of a partial row are not defined)
    for ws, got_dw, got_db in ((ws0, dw, db), (ws1, flat[0][:N * K], flat[0][nw:nw + N])):
        part = _np32(ws[:blocks * N * 17]).reshape(blocks, N * 17)
        order = _f32_chunk_sum(part).reshape(N, 17)
        assert _same_bits(got_dw, order[:, :K]) and _same_bits(got_db, order[:, 16])
    dz = dy.double() * (y > 0)
    x16 = x.to(tdt).double()
    assert torch.allclose(flat[0][nw:nw + N].double(), dz.sum(0), rtol=1e-5, atol=1e-4)
    ref = dz.t() @ x16
    assert (flat[0][:N * K].view(N, K).double() - ref).norm() <= 1e-2 * ref.norm() + 1e-12


def _mixed_table():
    """two flat buffers (bf16 and fp16 shadows) with every segment kind, and what the entry points
    of before leave for them"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    gen = torch.Generator(device="cuda").manual_seed(77)
    sp = stream_ptr()
    segs, want = [], [[], []]   # want[f]: (offset, tensor)
    sizes = [0, 0]

    def place(f, n):
        off = sizes[f]
        sizes[f] += (n + 3) // 4 * 4
        return off

    B = 300
    for f, name in enumerate(("bf16", "f16")):
        tdt, code = _dt(name)
        # split-K weight gradient 40 x 24, 4 groups, preceded by a 4-element tensor: start 16-byte
        # aligned only
        place(f, 4)
        n = 40 * 24
        p = torch.randn((4, n), device="cuda", generator=gen).to(tdt)
        o = place(f, n)
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        check(lib.hctr_sum_groups(4, n, ptr(p), code, ptr(t), sp))
        segs.append(dict(kind=SUM, src=p, count=4, n=n, dst=o, flat=f))
        want[f].append((o, t))
        # bias tile partials, 40 columns, 3 tiles
        dy = (torch.randn((B, 40), device="cuda", generator=gen) / 64).to(tdt)
        y = torch.relu(torch.randn((B, 40), device="cuda", generator=gen)).to(tdt)
        nb = lib.hctr_relu_bwd_bias_workspace_bytes(B, 40)
        ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda")
        dz = torch.empty_like(dy)
        t = torch.empty(40, dtype=torch.float32, device="cuda")
        check(lib.hctr_relu_bwd_bias(B, 40, ptr(dy), ptr(y), ptr(dz), ptr(t), ptr(ws), code, sp))
        o = place(f, 40)
        segs.append(dict(kind=COLSUM, src=ws, count=nb // 160, n=40, dst=o, flat=f))
        want[f].append((o, t))
        # a gradient that is in g already
        o = place(f, 10)
        t = torch.randn(12, device="cuda", generator=gen)
        segs.append(dict(kind=DIRECT, n=12, dst=o, flat=f, direct=t))
        want[f].append((o, t))
        # skinny first layer 13 -> 64
        x = torch.randn((B, 13), device="cuda", generator=gen)
        ys = torch.relu(torch.randn((B, 64), device="cuda", generator=gen)).to(tdt)
        dys = (torch.randn((B, 64), device="cuda", generator=gen) / B).to(tdt)
        ws = torch.empty(lib.hctr_skinny_fc_bwd_workspace_bytes(64) // 4, dtype=torch.float32,
                         device="cuda")
        dw = torch.empty(64 * 13, dtype=torch.float32, device="cuda")
        db = torch.empty(64, dtype=torch.float32, device="cuda")
        check(lib.hctr_skinny_fc_bwd(B, 13, 64, ptr(x), ptr(dys), ptr(ys), ptr(dw), ptr(db), ptr(ws),
                                     code, sp))
        ow, ob = place(f, 64 * 13), place(f, 64)
        segs.append(dict(kind=SKINNY, src=ws, n=64, k=13, dst=ow, dst2=ob, flat=f,
                         count=lib.hctr_skinny_fc_bwd_blocks(B, 13, 64, ptr(dys), ptr(ys))))
        want[f] += [(ow, dw), (ob, db)]
    # the logit head (K = 260) lands in the first buffer
    tdt, code = _dt("bf16")
    K = 260
    x = torch.randn((B, K), device="cuda", generator=gen).to(tdt)
    w = (torch.randn((1, K), device="cuda", generator=gen) / K ** 0.5).to(tdt)
    b = torch.tensor([0.1], device="cuda").to(tdt)
    lab = (torch.rand((B, 1), device="cuda", generator=gen) < 0.4).float()
    ws = torch.empty(lib.hctr_logit_head_workspace_bytes(K) // 4, dtype=torch.float32, device="cuda")
    dw = torch.empty(K, dtype=torch.float32, device="cuda")
    db = torch.empty(1, dtype=torch.float32, device="cuda")
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    check(lib.hctr_logit_head(B, K, ptr(x), ptr(w), ptr(b), ptr(lab), 1.0 / B, None, ptr(dw), ptr(db),
                              ptr(loss), ptr(ws), code, sp))
    ow, ob = place(0, K), place(0, 1)
    segs.append(dict(kind=HEAD, src=ws, count=lib.hctr_logit_head_blocks(B, K), n=K, k=B, dst=ow,
                     dst2=ob, flat=0))
    want[0] += [(ow, dw), (ob, db)]
    return segs, want, sizes, loss


def test_finish_mixed_table_gradients_and_sgd():
    """a table with every kind and both 16-bit types: gradients-only equals the old entry points;
    SGD mode equals gradients-only followed by hctr_sgd_shadow (masters and 16-bit copies)"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    segs, want, sizes, want_loss = _mixed_table()
    dts = [_dt("bf16"), _dt("f16")]
    flats = [_flat(sizes[f], dts[f][0], seed=f) for f in range(2)]
    for g, _, _ in flats:
        g.zero_()
    for s in segs:   # (the gradients written by other means)
        if s["kind"] == DIRECT:
            flats[s["flat"]][0][s["dst"]:s["dst"] + 12] = s["direct"]
    w0 = [(w.clone(), w16.clone()) for _, w, w16 in flats]
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    _finish(segs, flats, sgd=False, loss=loss)
    assert torch.equal(loss, want_loss)
    for f in range(2):
        exp = torch.zeros_like(flats[f][0])
        for o, t in want[f]:
            exp[o:o + t.numel()] = t
        assert torch.equal(flats[f][0], exp), f"flat gradient {f}"
        assert torch.equal(flats[f][1], w0[f][0]) and torch.equal(flats[f][2], w0[f][1])
    # the reference step: hctr_sgd_shadow on the finished gradients
    ref = []
    for f in range(2):
        w, w16 = w0[f][0].clone(), w0[f][1].clone()
        check(lib.hctr_sgd_shadow(w.numel(), LR, GS, ptr(w), ptr(flats[f][0]), ptr(w16), dts[f][1],
                                  stream_ptr()))
        ref.append((w, w16))
    gkeep = [g.clone() for g, _, _ in flats]
    loss2 = torch.empty_like(loss)
    _finish(segs, flats, sgd=True, loss=loss2)
    assert torch.equal(loss2, want_loss)
    for f in range(2):
        assert torch.equal(flats[f][1], ref[f][0]), f"masters {f}"
        assert torch.equal(flats[f][2], ref[f][1]), f"16-bit copy {f}"
        assert torch.equal(flats[f][0], gkeep[f])   # SGD mode leaves g alone
        assert not torch.equal(flats[f][1], w0[f][0])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_mlp_step_equals_the_step_from_the_old_entry_points(dtype):
    """FusedMLP 13 -> 64 -> 32 -> 1 with the BCE head, B = 300, one step through DenseGradFinish
    (SGD mode) against the same step assembled here from hctr_logit_head, hctr_relu_bwd_bias,
    hctr_sum_groups, hctr_skinny_fc_bwd and hctr_sgd_shadow"""
    import torch
    from hugectr_amd._lib import check, lib, ptr, stream_ptr
    from hugectr_amd.dense import DenseGradFinish, FusedMLP
    tdt, code = _dt(dtype)
    torch.manual_seed(5)
    B = 300
    m = FusedMLP([13, 64, 32, 1], last_relu=False, dtype=tdt).cuda()
    m.flatten()
    fin = DenseGradFinish([m])
    x = torch.rand((B, 13), device="cuda")
    lab = (torch.rand((B, 1), device="cuda") < 0.4).float()
    gs = 1024.0 / B
    w_before, w16_before = m.flat_w.clone(), m.flat_w16.clone()
    assert m._skinny_first(x)

    # -- the old entry points
    sp = stream_ptr()
    w16, b16 = [t.clone() for t in m._w16], [t.clone() for t in m._b16]
    y0 = torch._addmm_activation(b16[0], x.to(tdt), w16[0].t(), use_gelu=False)
    y1 = torch._addmm_activation(b16[1], y0, w16[1].t(), use_gelu=False)
    g = torch.zeros_like(m.flat_g)
    offw, offb = m._offs

    def view(off, n):
        return g[off:off + n]
    ws = torch.empty(lib.hctr_logit_head_workspace_bytes(32) // 4, dtype=torch.float32, device="cuda")
    dx1 = torch.empty_like(y1)
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    check(lib.hctr_logit_head(B, 32, ptr(y1), ptr(w16[2]), ptr(b16[2]), ptr(lab), gs, ptr(dx1),
                              ptr(view(offw[2], 32)), ptr(view(offb[2], 1)), ptr(loss), ptr(ws), code,
                              sp))
    ws = torch.empty(lib.hctr_relu_bwd_bias_workspace_bytes(B, 32) // 4, dtype=torch.float32,
                     device="cuda")
    dz1 = torch.empty_like(dx1)
    check(lib.hctr_relu_bwd_bias(B, 32, ptr(dx1), ptr(y1), ptr(dz1), ptr(view(offb[1], 32)), ptr(ws),
                                 code, sp))
    dx0 = dz1 @ w16[1]
    p = torch.bmm(dz1.view(4, B // 4, 32).transpose(1, 2), y0.view(4, B // 4, 64))  # 300 = 4 x 75
    check(lib.hctr_sum_groups(4, 32 * 64, ptr(p), code, ptr(view(offw[1], 32 * 64)), sp))
    ws = torch.empty(lib.hctr_skinny_fc_bwd_workspace_bytes(64) // 4, dtype=torch.float32,
                     device="cuda")
    check(lib.hctr_skinny_fc_bwd(B, 13, 64, ptr(x), ptr(dx0), ptr(y0), ptr(view(offw[0], 64 * 13)),
                                 ptr(view(offb[0], 64)), ptr(ws), code, sp))
    w_ref, w16_ref = w_before.clone(), w16_before.clone()
    check(lib.hctr_sgd_shadow(w_ref.numel(), LR, GS, ptr(w_ref), ptr(g), ptr(w16_ref), code, sp))

    # -- the new path: gradients only, then the step itself
    out = m.forward_bce(x, lab, gs)
    out.backward(torch.ones_like(out))
    kinds = [(lw.w_seg[0] if lw.w_seg else None, lw.b_seg[0] if lw.b_seg else None) for lw in m._lw]
    assert kinds == [(SKINNY, None), (SUM, COLSUM), (HEAD, None)]
    fin.finish(sgd=False)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), loss)
    assert torch.equal(m.flat_g, g)
    assert torch.equal(m.flat_w, w_before)
    out = m.forward_bce(x, lab, gs)
    out.backward(torch.ones_like(out))
    fin.finish(sgd=True, lr=LR, grad_scale=GS)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), loss)
    assert torch.equal(m.flat_w, w_ref)
    assert torch.equal(m.flat_w16, w16_ref)
    assert not torch.equal(m.flat_w, w_before)
    # released: the module finishes its gradients layer by layer again
    fin.release()
    m.flat_g.zero_()
    m.flat_w.copy_(w_before)
    m.flat_w16.copy_(w16_before)
    out = m.forward_bce(x, lab, gs)
    out.backward()
    assert torch.equal(m.flat_g, g) and torch.equal(out.detach(), loss)
