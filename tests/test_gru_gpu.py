"""GPU: ha.GRULayer / ha.gru (gru.hip) against the recurrence evaluated plainly on the CPU.

Two evaluations of `_reference`, from the inputs as the device holds them: `exact` in float64 with no
rounding, and the yardstick in float32 with the state rounded to T after each step for the 16-bit
types -- the contract itself.  Each of y, dx and dweight must satisfy, in the maximum norm,

    max|got - exact| <= 4 max|yardstick - exact| + 2 u_T max|exact|

(the kernels add the same fp32 terms in another order and their exp / tanh may differ from libm by a
few ulp; the last term is the one rounding of the stored result).  The test prints the ratio
max|got - exact| / max|yardstick - exact| of every tensor before it asserts."""
import pytest
import torch

import hugectr_amd as ha

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
U = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}

# (dtype, B, S, V, H, batch_first).  gru.hip's constants: a tile is 32 batch rows (fp32: 16), a K step
# 16 sum indices (fp32: 8), a wavefront's gate-column block 32 wide (fp32: 16), wavefront w owns blocks
# w, w + 4, ..; the recurrent grids stop at 512 tiles, the weight gradient's at 1024 (tile, slab) items
# with up to 2048 / tiles slabs of at least 64 rows.  The resident instance (R) serves the shapes whose
# weights [3 Hc][Vc + Hc + pad] fit 80 KB of LDS beside the tile's operands, the streamed one (S) the
# rest; `small` register arrays while V and H are at most four blocks wide.
GRU_CASES = [
    (F32, 1, 1, 1, 1, False),        # the smallest (R, as every case down to DIEN's)
    (F16, 1, 1, 1, 1, True),
    (F32, 3, 4, 5, 7, False),        # below every block; odd V: element loads
    (BF16, 3, 4, 5, 7, False),       # 16-bit rows that are not 16-byte aligned
    (F32, 15, 2, 7, 17, False),      # fp32: just under the tile and the K step, just over a block
    (F32, 16, 2, 8, 16, True),       # fp32: exactly at each; aligned rows: 16-byte loads
    (F32, 17, 3, 9, 15, False),      # fp32: just over the tile and the K step, just under a block
    (F16, 31, 2, 15, 33, False),     # 16-bit: just under tile and K step, just over a block
    (F16, 32, 2, 16, 32, False),     # 16-bit: exactly at each; 16-byte loads
    (BF16, 32, 2, 16, 32, True),
    (F16, 33, 3, 17, 31, False),     # 16-bit: just over tile and K step, just under a block
    (F32, 33, 3, 17, 31, False),     # fp32: three tiles, two blocks, three K steps
    (F32, 5, 12, 36, 36, False),     # R: DIEN
    (F32, 4, 3, 80, 16, False),      # R, five dx blocks: not small
    (F16, 5, 12, 36, 36, True),
    (BF16, 5, 12, 36, 36, False),
    (F32, 17, 2, 9, 129, False),     # S: fp32 tile, K step and ninth block just passed
    (F16, 33, 2, 17, 129, True),     # S: 16-bit tile, K step and fifth block just passed
    (F32, 70, 2, 130, 65, False),    # S: five gate blocks: a wavefront with two; dx blocks on every wavefront
    (F16, 70, 2, 130, 65, False),
    (F32, 2, 5, 20, 256, False),     # S: the widest state: four blocks a wavefront (16-bit: two)
    (F16, 2, 5, 20, 256, False),
    (F32, 3, 2, 1024, 8, False),     # S: the widest input: sixteen dx blocks a wavefront (16-bit: two passes of four)
    (BF16, 3, 2, 1024, 8, False),
    (F32, 2, 300, 8, 8, False),      # a long recurrence
    (F16, 2, 300, 8, 8, False),
    (F32, 33000, 2, 4, 4, False),    # 2063 tiles > 512; 2 tiles x 1024 slabs = 2048 items > 1024
    (F16, 33000, 2, 4, 4, True),     # 1032 tiles > 512
]


def _reference(x, w, dy, H, dtype, round_to=None):
    """x [S][B][V], w flat, dy [S][B][H] -> y, dx, dw in `dtype`; the state that enters the next step
    (and y_t) rounded to `round_to` when given, the gradient passing through the rounding"""
    S, B, V = x.shape
    x, w = x.to(dtype).requires_grad_(), w.to(dtype).requires_grad_()
    W, R, b = w[:3 * H * V].view(3, H, V), w[3 * H * V:3 * H * (V + H)].view(3, H, H), w[-3 * H:].view(3, H)
    h, ys = x.new_zeros(B, H), []
    for t in range(S):
        gx, gh = torch.einsum("bv,ghv->gbh", x[t], W), torch.einsum("bk,ghk->gbh", h, R)
        r, z = torch.sigmoid(gx[0] + gh[0] + b[0]), torch.sigmoid(gx[1] + gh[1] + b[1])
        n = torch.tanh(gx[2] + r * gh[2] + b[2])
        h = (1 - z) * n + z * h
        if round_to is not None:
            h = h + (h.detach().to(round_to).to(dtype) - h.detach())
        ys.append(h)
    y = torch.stack(ys)
    y.backward(dy.to(dtype))
    return y.detach(), x.grad, w.grad


def _run(dtype, B, S, V, H, batch_first, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (B, S, V) if batch_first else (S, B, V)
    x = (torch.rand(shape, generator=g) * 2 - 1).to(dtype)
    w = ((torch.rand(3 * H * (V + H + 1), generator=g) * 2 - 1) / max(V, H) ** 0.5).to(dtype)
    dy = (torch.rand((*shape[:2], H), generator=g) * 2 - 1).to(dtype)
    layer = ha.GRULayer(H, V, batch_first).to(device="cuda", dtype=dtype)
    with torch.no_grad():
        layer.weight.copy_(w)
    xd = x.cuda().requires_grad_()
    y = layer(xd)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return (x, w, dy), (y.detach().cpu(), xd.grad.cpu(), layer.weight.grad.cpu())


@pytest.mark.parametrize("dtype,B,S,V,H,batch_first", GRU_CASES)
def test_gru_matches_the_recurrence(dtype, B, S, V, H, batch_first):
    (x, w, dy), got = _run(dtype, B, S, V, H, batch_first)
    if batch_first:
        x, dy = x.transpose(0, 1), dy.transpose(0, 1)
        got = (got[0].transpose(0, 1), got[1].transpose(0, 1), got[2])
    exact = _reference(x, w, dy, H, torch.float64)
    yard = _reference(x, w, dy, H, torch.float32, None if dtype == F32 else dtype)
    report, ok = [], True
    for name, a, e, yd in zip(("y", "dx", "dweight"), got, exact, yard):
        err = (a.double() - e).abs().max().item()
        ref_err = (yd.double() - e).abs().max().item()
        bound = 4 * ref_err + 2 * U[dtype] * e.abs().max().item()
        report.append(f"{name}: err {err:.3e} yardstick {ref_err:.3e} ratio {err / max(ref_err, 1e-300):.2f} "
                      f"bound {bound:.3e}")
        ok = ok and err <= bound
    print(f"gru {dtype} {(B, S, V, H)}: " + "; ".join(report))
    assert ok, report


@pytest.mark.parametrize("case", [GRU_CASES[12], GRU_CASES[19]])
def test_gru_two_runs_give_the_same_bits(case):
    first, second = _run(*case)[1], _run(*case)[1]
    for a, b in zip(first, second):
        assert torch.equal(a, b)
