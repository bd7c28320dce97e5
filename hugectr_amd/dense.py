"""Dense-tower building blocks (PyTorch-ROCm / hipBLASLt GEMMs) arranged for MI355X.

The MLP GEMMs themselves stay in the vendor library (dense tower out of scope as
kernels).  What this module fixes is how they are *issued* for the DLRM shapes
(`FusedFullyConnectedLayer` / `MLPLayer` in the reference, R/HugeCTR/src/layers/mlp_layer.cu):

* weight gradients dW[out,in] = dY^T X reduce over K = batch = 65536 into a small out x in tile
  set: a single library GEMM launches 64-128 workgroups on 256 CUs.  `split_k_wgrad` reshapes the
  reduction into G batched GEMMs (torch.bmm) + a sum, i.e. split-K through the library: 2-5x faster
  on these shapes (tools/gemm_probe.py).
* bias + ReLU ride in the GEMM epilogue (`torch._addmm_activation` -> hipBLASLt RELU_BIAS).
* bf16 shadow copies of the fp32 master weights are refreshed once per optimizer step with one
  multi-tensor copy instead of one cast kernel per layer per pass.
* after `FusedMLP.flatten()` masters, gradients and 16-bit copies are three flat buffers and the
  backward's workspaces exist once per layer.  A `DenseGradFinish` over the model's flattened
  modules then turns the finishing launches of a step (a group sum per weight gradient, a column
  sum per bias gradient, the finish kernels of the logit head and the skinny first layer, one SGD
  launch per module) into ONE launch, `hctr_dense_grad_finish`: the producers leave their partial
  sums, the launch adds them in the same order as the kernels it replaces and either writes
  `flat_g` or takes the SGD step and refreshes the 16-bit copy.  A module without a
  `DenseGradFinish` finishes layer by layer as before.
* in a flattened module the data gradient of layer i + 1, the ReLU mask of layer i and layer i's
  bias partials are ONE kernel, `hctr_gemm_nt16_drelu` (the library's own MFMA GEMM with a dReLU
  epilogue), where layer i is a ReLU layer through `_LinearFn`, the type is 16-bit, in % 128 == 0
  and out % 64 == 0: layer i + 1's backward leaves dz and the partial rows with layer i's
  `_LayerWS`, layer i's backward skips `hctr_relu_bwd_bias`.  The kernel reads W^T, kept in
  `flat_w16t` and refreshed by one launch wherever `flat_w16` is.  HCTR_DGRAD_FUSED = auto (where
  it was measured faster, `_dgrad_fused_wins`) | 0 (never; read by `flatten()` too, which then keeps
  no `flat_w16t`) | 1 (wherever legal).
* `Optimizer_t.Ftrl` for the dense layers (torch has none): `FusedMLP.ftrl_step` on the flat
  buffers (`hctr_ftrl_shadow`, one launch per module, 16-bit copy included) and `DenseFtrl`, a
  torch optimizer over parameters that do not live in one buffer (`hctr_ftrl_segments`, one launch
  per step).
"""
from __future__ import annotations

import contextlib
import os

from typing import List, Sequence

import torch

from ._lib import FTRL_SEG_BLOCK_ELEMS, TRANSPOSE16_TILE, check, lib, ptr, stream_ptr

_DT16 = {torch.float16: 1, torch.bfloat16: 2}  # hctr_emb_dtype_t
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _count(rc: int) -> int:
    """a count returned by the library (negative: an error code)"""
    if rc < 0:
        check(rc)
    return rc


def _split_k_groups(B: int, o: int, i: int, groups: int) -> int:
    """groups the batch dimension is split into for dW[o, i]; 0 = one plain GEMM"""
    g = groups
    while g > 1 and B % g != 0:
        g //= 2
    # degenerate outputs (the logit layer, out = 1): the batched-GEMM path of the library
    # spends ~11 ms per call on the HOST for M = 1 (tools/gemm_probe2.py); one GEMV-like call
    # is 50-100 us
    return g if g > 1 and min(o, i) >= 8 else 0


def split_k_wgrad(dy: torch.Tensor, x: torch.Tensor, groups: int = 16,
                  out: torch.Tensor = None, part: torch.Tensor = None,
                  finish: bool = True):
    """dW = dy^T @ x with the batch (K) dimension split into `groups` batched GEMMs (fp32 result,
    written to `out` when given).  part: a preallocated 16-bit buffer of >= groups * out * in
    elements for the partial products.  finish = False: when the partial products can be left in
    `part` for `DenseGradFinish` (16-bit, out * in a multiple of 8) they are, and the number of
    groups is returned instead of dW."""
    B, o = dy.shape
    i = x.shape[1]
    g = _split_k_groups(B, o, i, groups)
    if g == 0:
        r = dy.t() @ x
        if out is not None:
            out.copy_(r)
            return out
        return r
    a, b = dy.view(g, B // g, o).transpose(1, 2), x.view(g, B // g, i)
    hip = dy.is_cuda and dy.dtype in _DT16 and (o * i) % 8 == 0
    if hip and part is not None and part.dtype == dy.dtype:
        p = torch.bmm(a, b, out=part[:g * o * i].view(g, o, i))
        if not finish:
            return g
    else:
        p = torch.bmm(a, b)
    if hip:
        if out is None:
            out = torch.empty((o, i), dtype=torch.float32, device=p.device)
        check(lib.hctr_sum_groups(g, o * i, ptr(p), _DT16[p.dtype], ptr(out), stream_ptr()))
        return out
    r = p.float().sum(0)
    if out is not None:
        out.copy_(r)
        return out
    return r


def bce_with_logits(logit: torch.Tensor, label: torch.Tensor, grad_scale: float):
    """BinaryCrossEntropyLoss forward + logit gradient in one pass (R/HugeCTR/src/loss.cu:231-262).

    Returns (mean loss [1] fp32, dlogit like `logit`) with dlogit = (sigmoid(x) - y) * grad_scale;
    feed it to `logit.backward(dlogit)`."""
    x = logit.detach().contiguous()
    y = label.contiguous()
    assert x.is_cuda and y.dtype == torch.float32 and x.numel() == y.numel()
    dlogit = torch.empty_like(x)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.hctr_bce_loss_workspace_bytes() // 4, dtype=torch.float32, device=x.device)
    check(lib.hctr_bce_loss(x.numel(), ptr(x), ptr(y), float(grad_scale), ptr(dlogit), ptr(loss),
                            ptr(ws), _DT[x.dtype], stream_ptr()))
    return loss, dlogit


# segment kinds of hctr_dense_grad_finish (include/hugectr_amd.h)
_SEG_SUM, _SEG_COLSUM, _SEG_HEAD, _SEG_SKINNY, _SEG_DIRECT = range(5)


def _dgrad_mode() -> str:
    """HCTR_DGRAD_FUSED = auto (the measured rule below) | 0 (never) | 1 (wherever the shape is legal)"""
    v = os.environ.get("HCTR_DGRAD_FUSED", "auto")
    return v if v in ("0", "1") else "auto"


def _dgrad_fused_wins(m: int, n: int, k: int) -> bool:
    """`auto`: is hctr_gemm_nt16_drelu faster than the library's data-gradient GEMM [m, k] x [k, n]
    plus hctr_relu_bwd_bias_partials?  Measured per shape, median of the fused call below the
    pair's fastest repeat (profiles/dgrad_relu_shapes.txt; DESIGN.md "Dense-tower glue")."""
    # the four (n, k) that were measured, each at m = 2048 .. 65536, all won (by 13 .. 51 us a
    # call); any other shape stays on the library until it is measured
    # (tools/microbench_dgrad_relu.py)
    return 2048 <= m <= 65536 and (n, k) in _DGRAD_MEASURED_WINS


_DGRAD_MEASURED_WINS = frozenset([(512, 256), (1024, 512), (1024, 1024), (256, 128)])


def _transpose_table(segs, device):
    """hctr_transpose16_seg table of (src, dst, rows, cols) on the device -> (table, nseg, nblocks)"""
    import numpy as np
    t = np.zeros((len(segs), 8), dtype=np.int64)
    block0, per = 0, TRANSPOSE16_TILE
    for r, (src, dst, rows, cols) in enumerate(segs):
        t[r, :5] = (src, dst, rows, cols, block0)
        block0 += ((rows + per - 1) // per) * ((cols + per - 1) // per)
    return torch.from_numpy(t).to(device), len(segs), block0


class _LayerWS:
    """Workspaces of one layer of a flattened FusedMLP (allocated once, stable addresses: nothing is
    allocated per call, a captured graph replays on them) and what the last backward left in them:
    `w_seg` / `b_seg` = (kind, tensor, count, k) as `DenseGradFinish` needs it, None = the
    gradient itself is in `flat_g`."""

    def __init__(self, mlp, idx: int, wpart: torch.Tensor):
        self.mlp, self.idx, self.wpart = mlp, idx, wpart
        self._ws = None
        self.w_seg = self.b_seg = None
        # (dz, partial rows, tiles) the layer above left with hctr_gemm_nt16_drelu: this layer's
        # masked gradient and its bias partials exist already
        self.pre = None
        self._colsum = None

    def take_pre(self, dy):
        """(partial rows, tiles) when dy IS the dz the layer above left (the same storage: a
        gradient autograd summed with another consumer's is masked here as usual), else None.
        `pre` holds dz itself, not its address: while it does, autograd cannot add another
        consumer's gradient into dz in place, nor can the allocator hand its storage to another
        tensor -- the address test relies on both.  (A backward that never reaches this layer
        leaves dz alive until the next one does.)"""
        pre, self.pre = self.pre, None
        if pre is not None and pre[0].data_ptr() == dy.data_ptr() and pre[0].shape == dy.shape:
            return pre[1], pre[2]
        return None

    def finish_colsum(self, partials: torch.Tensor, tiles: int, n: int):
        """the bias gradient from the partial rows into its place in flat_g (no DenseGradFinish):
        a one-segment table, rebuilt only when the workspace moved or the batch changed"""
        import numpy as np
        m = self.mlp
        sig = (partials.data_ptr(), tiles, n, m.flat_g.data_ptr())
        if self._colsum is None or self._colsum[0] != sig:
            t = np.zeros((1, DenseGradFinish._FIELDS), dtype=np.int64)
            t[0, :13] = (_SEG_COLSUM, sig[0], tiles, n, 0, 0, sig[3], m.flat_w.data_ptr(),
                         m.flat_w16.data_ptr(), m._offs[1][self.idx], 0,
                         int(m.dtype == torch.bfloat16), 0)
            self._colsum = (sig, torch.from_numpy(t).to(partials.device),
                            _count(lib.hctr_dense_seg_blocks(_SEG_COLSUM, n)))
        check(lib.hctr_dense_grad_finish(ptr(self._colsum[1]), 1, self._colsum[2], 0, 0.0, 1.0, None,
                                         stream_ptr()))

    @property
    def defer(self) -> bool:
        return self.mlp._finisher is not None

    def ws(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.wpart.device)
        return self._ws


class _LinearFn(torch.autograd.Function):
    """y = act(x @ W^T + b) on 16-bit shadow weights; gradients returned for the fp32 masters."""

    @staticmethod
    def forward(ctx, x, w_master, b_master, w16, b16, relu: bool, groups: int, gw=None, gb=None,
                lw=None, w16t=None, below=None):
        """gw / gb: views of the module's flat gradient buffer; when given, backward writes the
        weight / bias gradients there and returns no gradient for the masters.  lw: the layer's
        _LayerWS (flattened module).  w16t / below: W^T [in, out] and the _LayerWS of the ReLU
        layer that produced x -- backward then computes that layer's masked gradient and bias
        partials with the data gradient, in one kernel (hctr_gemm_nt16_drelu)"""
        x = x.contiguous()
        ctx.gw, ctx.gb, ctx.lw = gw, gb, lw
        ctx.w16t, ctx.below = w16t, below
        if relu:
            y = torch._addmm_activation(b16, x, w16.t(), use_gelu=False)
        else:
            y = torch.addmm(b16, x, w16.t())
        ctx.relu, ctx.groups = relu, groups
        ctx.save_for_backward(x, w16, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16, y = ctx.saved_tensors
        dy = dy.contiguous()
        n = dy.shape[1]
        lw = ctx.lw
        defer = lw is not None and lw.defer
        pre = None
        if lw is not None:
            lw.w_seg = lw.b_seg = None
            pre = lw.take_pre(dy)
        if pre is not None:  # dy is dz already, the layer above left it with the bias partials
            if defer:
                lw.b_seg = (_SEG_COLSUM, pre[0], pre[1], 0)
            else:
                lw.finish_colsum(pre[0], pre[1], n)
            db = None
        elif ctx.relu and n % 8 == 0 and dy.dtype in _DT16 and dy.is_cuda:
            # fused ReLU backward + bias gradient (HIP): one pass instead of two
            dz = torch.empty_like(dy)
            nbytes = lib.hctr_relu_bwd_bias_workspace_bytes(dy.shape[0], n)
            ws = lw.ws(nbytes) if lw is not None else \
                torch.empty(nbytes // 4, dtype=torch.float32, device=dy.device)
            if defer:  # the tile partials wait for the step's one finish launch
                check(lib.hctr_relu_bwd_bias_partials(dy.shape[0], n, ptr(dy), ptr(y), ptr(dz),
                                                      ptr(ws), _DT16[dy.dtype], stream_ptr()))
                lw.b_seg = (_SEG_COLSUM, ws, nbytes // (4 * n), 0)
                db = None
            else:
                db = ctx.gb if ctx.gb is not None else torch.empty(n, dtype=torch.float32,
                                                                 device=dy.device)
                check(lib.hctr_relu_bwd_bias(dy.shape[0], n, ptr(dy), ptr(y), ptr(dz), ptr(db),
                                             ptr(ws), _DT16[dy.dtype], stream_ptr()))
            dy = dz
        else:
            if ctx.relu:
                dy = torch.ops.aten.threshold_backward(dy, y, 0)
            db = dy.sum(0, dtype=torch.float32)
            if ctx.gb is not None:
                ctx.gb.copy_(db)
        if not ctx.needs_input_grad[0]:
            dx = None
        elif ctx.below is not None:
            # x is the ReLU output of the layer below: its dz = (x > 0) ? dy @ W : 0 and the column
            # sums of dz leave the GEMM's epilogue; that layer's backward finds them in `pre`
            rows, k = dy.shape
            dx = torch.empty_like(x)
            tiles = _count(lib.hctr_gemm_nt16_drelu_tiles(rows, x.shape[1]))
            part = ctx.below.ws(tiles * x.shape[1] * 4)
            check(lib.hctr_gemm_nt16_drelu(rows, x.shape[1], k, ptr(dy), k, ptr(ctx.w16t), k, ptr(x),
                                           ptr(dx), x.shape[1], ptr(part), _DT16[dy.dtype],
                                           stream_ptr()))
            ctx.below.pre = (dx, part, tiles)
        else:
            dx = dy @ w16
        dw = split_k_wgrad(dy, x, ctx.groups, out=ctx.gw, part=lw.wpart if lw is not None else None,
                           finish=not defer)
        if defer and isinstance(dw, int):
            lw.w_seg = (_SEG_SUM, lw.wpart, dw, 0)
        if ctx.gw is not None:  # gradients live in the flat buffer; nothing for autograd to keep
            return (dx,) + (None,) * 11
        return (dx, dw.float(), db) + (None,) * 9


class _SkinnyFirstFn(torch.autograd.Function):
    """y = relu(x @ W^T + b) for an input with a handful of features (x fp32 [B, K <= 16], no data
    gradient).  The backward (hctr_skinny_fc_bwd) reads dy and y once and leaves dw / db, no dz
    tensor in between; the forward is the library GEMM unless HCTR_SKINNY_FC_FWD=hip selects
    hctr_skinny_fc_fwd."""

    @staticmethod
    def forward(ctx, x, w_master, b_master, w16, b16, gw=None, gb=None, lw=None):
        x = x.contiguous()
        B, K = x.shape
        N = w16.shape[0]
        if os.environ.get("HCTR_SKINNY_FC_FWD", "gemm") == "hip":
            y = torch.empty((B, N), dtype=w16.dtype, device=x.device)
            check(lib.hctr_skinny_fc_fwd(B, K, N, ptr(x), ptr(w16), ptr(b16), ptr(y),
                                         _DT16[w16.dtype], stream_ptr()))
        else:  # the library GEMM is the faster forward at 13 -> 512 (30 us against 43 us)
            y = torch._addmm_activation(b16, x.to(w16.dtype), w16.t(), use_gelu=False)
        ctx.gw, ctx.gb, ctx.lw = gw, gb, lw
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        dy = dy.contiguous()
        B, K = x.shape
        N = y.shape[1]
        dev = x.device
        lw = ctx.lw
        nbytes = lib.hctr_skinny_fc_bwd_workspace_bytes(N)
        ws = lw.ws(nbytes) if lw is not None else \
            torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        if lw is not None and lw.defer:  # the block partials wait for the step's finish launch
            check(lib.hctr_skinny_fc_bwd_partials(B, K, N, ptr(x), ptr(dy), ptr(y), ptr(ws),
                                                  _DT16[y.dtype], stream_ptr()))
            blocks = _count(lib.hctr_skinny_fc_bwd_blocks(B, K, N, ptr(dy), ptr(y)))
            lw.w_seg, lw.b_seg = (_SEG_SKINNY, ws, blocks, K), None
            return None, None, None, None, None, None, None, None
        if lw is not None:
            lw.w_seg = lw.b_seg = None
        dw = ctx.gw if ctx.gw is not None else torch.empty((N, K), dtype=torch.float32, device=dev)
        db = ctx.gb if ctx.gb is not None else torch.empty(N, dtype=torch.float32, device=dev)
        check(lib.hctr_skinny_fc_bwd(B, K, N, ptr(x), ptr(dy), ptr(y), ptr(dw), ptr(db), ptr(ws),
                                     _DT16[y.dtype], stream_ptr()))
        if ctx.gw is not None:
            return None, None, None, None, None, None, None, None
        return None, dw, db, None, None, None, None, None


class _LogitHeadFn(torch.autograd.Function):
    """loss = mean BCE(x @ w^T + b, label) with the whole backward of the head computed in the same
    pass (hctr_logit_head): dx, dw, db exist when forward returns.  backward() hands dx on; it
    assumes the unit upstream gradient of `loss.backward()` -- scale through grad_scale."""

    @staticmethod
    def forward(ctx, x, w_master, b_master, w16, b16, label, grad_scale: float, gw=None, gb=None,
                lw=None):
        x = x.contiguous()
        B, K = x.shape
        dev = x.device
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nbytes = lib.hctr_logit_head_workspace_bytes(K)
        ws = lw.ws(nbytes) if lw is not None else \
            torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        label = label.contiguous()
        ctx.flat = gw is not None
        ctx.dx = dx
        if lw is not None and lw.defer:
            # dw / db / the loss are block partials until the step's finish launch, which writes
            # the loss too: it is valid on the stream after DenseGradFinish.finish()
            check(lib.hctr_logit_head_partials(B, K, ptr(x), ptr(w16), ptr(b16), ptr(label),
                                               float(grad_scale), ptr(dx), ptr(ws), _DT16[x.dtype],
                                               stream_ptr()))
            lw.w_seg = (_SEG_HEAD, ws, _count(lib.hctr_logit_head_blocks(B, K)), B)
            lw.b_seg = None
            lw.mlp._loss_out = loss
            ctx.dw = ctx.db = None
            return loss
        if lw is not None:
            lw.w_seg = lw.b_seg = None
        dw = gw if gw is not None else torch.empty((1, K), dtype=torch.float32, device=dev)
        db = gb if gb is not None else torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.hctr_logit_head(B, K, ptr(x), ptr(w16), ptr(b16), ptr(label),
                                  float(grad_scale), ptr(dx), ptr(dw), ptr(db), ptr(loss), ptr(ws),
                                  _DT16[x.dtype], stream_ptr()))
        ctx.dw, ctx.db = (None, None) if ctx.flat else (dw, db)
        return loss

    @staticmethod
    def backward(ctx, _grad_loss):
        dx, dw, db = ctx.dx, ctx.dw, ctx.db
        ctx.dx = ctx.dw = ctx.db = None
        return dx, dw, db, None, None, None, None, None, None, None


class FusedMLP(torch.nn.Module):
    """Stack of Linear(+ReLU) layers with fp32 master weights and 16-bit compute copies.

    dims = [in, h1, ..., out]; `last_relu` tells whether the final layer is activated (the DLRM
    bottom MLP is, the top MLP's logit layer is not)."""

    def __init__(self, dims: Sequence[int], last_relu: bool, dtype=torch.bfloat16,
                 wgrad_groups: int = 16):
        super().__init__()
        self.dims = list(dims)
        self.dtype = dtype
        self.wgrad_groups = wgrad_groups
        self.relu = [True] * (len(dims) - 2) + [last_relu]
        self.weights = torch.nn.ParameterList()
        self.biases = torch.nn.ParameterList()
        for i in range(len(dims) - 1):
            lin = torch.nn.Linear(dims[i], dims[i + 1])  # reference default init equivalent
            self.weights.append(torch.nn.Parameter(lin.weight.detach().clone()))
            self.biases.append(torch.nn.Parameter(lin.bias.detach().clone()))
        self._w16: List[torch.Tensor] = []
        self._b16: List[torch.Tensor] = []
        self.flat_w = self.flat_g = self.flat_w16 = None
        self.flat_w16t = None  # W^T of the layers whose data gradient may take the fused kernel
        self._w16t: List[torch.Tensor] = []
        self._t_segs = []      # (src, dst, rows, cols) per transposed layer
        self._t_table = None   # (device table, nseg, nblocks) of hctr_transpose16_segments
        self._t_hold = False
        self.flat_z = self.flat_n = None  # Ftrl state, only after flatten(ftrl_state=True)
        self._gw: List[torch.Tensor] = []
        self._gb: List[torch.Tensor] = []
        self._lw: List[_LayerWS] = []
        self._finisher = None  # a DenseGradFinish: backward leaves partial sums for its launch
        self._loss_out = None

    def flatten(self, ftrl_state: bool = False):
        """Move masters, gradients and 16-bit copies into three flat buffers (parameters become
        views).  Afterwards backward writes gradients straight into `flat_g`, `sgd_step` is one
        kernel (update + shadow refresh), and a data-parallel all-reduce runs on `flat_g` as is.
        The backward's workspaces (split-K partial products, bias tile partials) are allocated
        here, once per layer.  ftrl_state: also the Ftrl state `flat_z` / `flat_n` (fp32, zero) that
        `ftrl_step` needs; nothing is allocated for them otherwise."""
        dev = self.weights[0].device
        sizes = [p.numel() for p in list(self.weights) + list(self.biases)]
        offs, tot = [], 0
        for n in sizes:
            offs.append(tot)
            tot += (n + 3) // 4 * 4  # every view starts 16-byte aligned
        self.flat_w = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.flat_w16 = torch.zeros(tot, dtype=self.dtype, device=dev)
        if ftrl_state:
            self.flat_z = torch.zeros(tot, dtype=torch.float32, device=dev)
            self.flat_n = torch.zeros(tot, dtype=torch.float32, device=dev)
        params = list(self.weights) + list(self.biases)
        views16 = []
        self._gw, self._gb = [], []
        for p, o, n in zip(params, offs, sizes):
            v = self.flat_w[o:o + n].view_as(p)
            v.copy_(p.data)
            p.data = v
            views16.append(self.flat_w16[o:o + n].view_as(p))
        nl = len(self.weights)
        self._w16, self._b16 = views16[:nl], views16[nl:]
        gviews = [self.flat_g[o:o + n].view_as(p) for p, o, n in zip(params, offs, sizes)]
        self._gw, self._gb = gviews[:nl], gviews[nl:]
        self.flat_w16.copy_(self.flat_w)
        self._offs = (offs[:nl], offs[nl:])
        self._spans = list(zip(offs, sizes))  # (offset, count) per parameter, parameters() order
        # split-K partial products [groups][out][in] of every layer, slices 512-byte aligned
        need = [self.wgrad_groups * w.numel() if min(w.shape) >= 8 else 0 for w in self.weights]
        starts, at = [], 0
        for n in need:
            starts.append(at)
            at += (n + 255) // 256 * 256
        part = torch.empty(max(at, 1), dtype=self.dtype, device=dev)
        self._lw = [_LayerWS(self, i, part[starts[i]:starts[i] + need[i]]) for i in range(nl)]
        # W^T [in][out] of every layer whose data gradient can go through hctr_gemm_nt16_drelu (it
        # reads both operands K-contiguous), one flat buffer, every view 16-byte aligned
        fus = [i for i in range(nl) if self._dgrad_fusable(i)] if _dgrad_mode() != "0" else []
        self._w16t, self._t_segs, self._t_table, self.flat_w16t = [None] * nl, [], None, None
        if fus:
            self.flat_w16t = torch.zeros(sum(self.weights[i].numel() for i in fus), dtype=self.dtype,
                                         device=dev)
            at = 0
            for i in fus:
                o, k = self.weights[i].shape  # (out * in is a multiple of 64 * 128)
                self._w16t[i] = self.flat_w16t[at:at + o * k].view(k, o)
                self._t_segs.append((self._w16[i].data_ptr(), self._w16t[i].data_ptr(), o, k))
                at += o * k
            self._t_table = _transpose_table(self._t_segs, dev)
            self.refresh_transposed()
        return self

    def _dgrad_fusable(self, i: int) -> bool:
        """can layer i's data gradient carry the ReLU mask and the bias sums of layer i - 1?  (the
        shapes hctr_gemm_nt16_drelu takes: N = in, K = out)"""
        return (i >= 1 and self.relu[i - 1] and self.dtype in _DT16 and
                self.dims[i] % 128 == 0 and self.dims[i + 1] % 64 == 0)

    def refresh_transposed(self):
        """flat_w16t from flat_w16, one launch; called wherever flat_w16 is refreshed (inside
        DenseGradFinish.one_transpose() its one launch covers all modules instead)"""
        if self._t_table is not None and not self._t_hold:
            t, nseg, nblocks = self._t_table
            check(lib.hctr_transpose16_segments(ptr(t), nseg, nblocks, stream_ptr()))

    def sgd_step(self, lr: float, grad_scale: float = 1.0):
        """w -= lr * grad_scale * g and refresh of the 16-bit copy, one launch (after flatten())"""
        check(lib.hctr_sgd_shadow(self.flat_w.numel(), float(lr), float(grad_scale),
                                  ptr(self.flat_w), ptr(self.flat_g), ptr(self.flat_w16),
                                  _DT16[self.dtype], stream_ptr()))
        self.refresh_transposed()

    def ftrl_step(self, lr: float, beta: float, lambda1: float, lambda2: float,
                  grad_scale: float = 1.0):
        """the Ftrl step on the flat buffers and the refresh of the 16-bit copy, one launch (after
        flatten(ftrl_state=True))"""
        assert self.flat_z is not None, "ftrl_step: flatten(ftrl_state=True) first"
        check(lib.hctr_ftrl_shadow(self.flat_w.numel(), float(lr), float(beta), float(lambda1),
                                   float(lambda2), float(grad_scale), ptr(self.flat_w),
                                   ptr(self.flat_z), ptr(self.flat_n), ptr(self.flat_g),
                                   ptr(self.flat_w16), _DT16[self.dtype], stream_ptr()))
        self.refresh_transposed()

    def ftrl_state(self):
        """[(z, n)] views per parameter, in parameters() order"""
        return [(self.flat_z[o:o + c], self.flat_n[o:o + c]) for o, c in self._spans]

    def refresh_shadow(self):
        """call after every optimizer step (and once after .to(device))"""
        if self.flat_w is not None:
            self.flat_w16.copy_(self.flat_w)
            self.refresh_transposed()
            return
        if not self._w16:
            self._w16 = [w.detach().to(self.dtype) for w in self.weights]
            self._b16 = [b.detach().to(self.dtype) for b in self.biases]
        else:
            torch._foreach_copy_(self._w16 + self._b16,
                                 [w.detach() for w in self.weights] +
                                 [b.detach() for b in self.biases])

    def _skinny_first(self, x) -> bool:
        """first layer through the few-input-features kernels?  (fp32 input without a gradient)"""
        return (self.relu[0] and self.dims[0] <= 16 and self.dims[1] % 4 == 0 and
                self.dims[1] <= 512 and self.dtype in _DT16 and x.is_cuda and
                x.dtype == torch.float32 and not x.requires_grad and
                os.environ.get("HCTR_SKINNY_FC", "1") != "0")

    def _layer(self, i, x):
        gw = self._gw[i] if self._gw else None
        gb = self._gb[i] if self._gb else None
        lw = self._lw[i] if self._lw else None
        if i == 0 and self._skinny_first(x):
            return _SkinnyFirstFn.apply(x, self.weights[0], self.biases[0], self._w16[0],
                                        self._b16[0], gw, gb, lw)
        # x is the output of layer i - 1, a ReLU layer (flatten() kept W^T only then), and it came
        # straight out of _LinearFn (the skinny first layer folds its own mask): its mask and bias
        # sums ride in this layer's data-gradient GEMM (HCTR_DGRAD_FUSED)
        w16t = self._w16t[i] if lw is not None and i >= 1 and self._w16t else None
        below = None
        if w16t is not None and x.is_cuda and x.dtype == self.dtype and \
                x.grad_fn is not None and x.grad_fn.name() == "_LinearFnBackward":
            mode = _dgrad_mode()
            if mode == "1" or (mode == "auto" and
                               _dgrad_fused_wins(x.shape[0], self.dims[i], self.dims[i + 1])):
                below = self._lw[i - 1]
        if x.dtype != self.dtype:
            x = x.to(self.dtype)
        return _LinearFn.apply(x, self.weights[i], self.biases[i], self._w16[i], self._b16[i],
                               self.relu[i], self.wgrad_groups, gw, gb, lw,
                               w16t if below is not None else None, below)

    def can_fuse_bce_head(self) -> bool:
        k = self.dims[-2]
        return (self.dims[-1] == 1 and not self.relu[-1] and k % 4 == 0 and k <= 2048 and
                self.dtype in _DT16)

    def forward_bce(self, x, label, grad_scale: float):
        """the stack up to the last hidden layer, then logit layer + BinaryCrossEntropyLoss + the
        head's backward in one kernel: returns the mean loss [1]; `loss.backward()` continues
        through the hidden layers (gradients of the head are already in place)"""
        assert self.can_fuse_bce_head()
        if not self._w16:
            self.refresh_shadow()
        n = len(self.weights)
        for i in range(n - 1):
            x = self._layer(i, x)
        if x.dtype != self.dtype:
            x = x.to(self.dtype)
        return _LogitHeadFn.apply(x, self.weights[-1], self.biases[-1], self._w16[-1], self._b16[-1],
                                  label, grad_scale, self._gw[-1] if self._gw else None,
                                  self._gb[-1] if self._gb else None,
                                  self._lw[-1] if self._lw else None)

    def forward(self, x):
        if not self._w16:
            self.refresh_shadow()
        for i in range(len(self.weights)):
            x = self._layer(i, x)
        return x


class DenseGradFinish:
    """The gradient finish of a set of flattened FusedMLPs as ONE launch per step
    (hctr_dense_grad_finish).  While a module belongs to one, its backward leaves what its kernels
    produce -- split-K partial products, bias tile partials, the block partials of the logit head
    and of the skinny first layer -- where they are; `finish()` adds every one of them in the
    order of the kernel that used to, into `flat_g` (sgd = False: before an all-reduce) or through
    w -= lr * grad_scale * g into the masters and the 16-bit copies (sgd = True; `flat_g` is not
    written).  The loss of a fused BCE head is written by the same launch.

    The segment table lives on the device and is rebuilt only when the backward left something
    else than last time (another batch size, a reallocated workspace)."""

    _FIELDS = 16  # int64 per hctr_dense_seg

    def __init__(self, mlps: Sequence["FusedMLP"]):
        self.mlps = list(mlps)
        for m in self.mlps:
            assert m.flat_w is not None, "DenseGradFinish: flatten() the module first"
            m._finisher = self
        self._sig = None
        self._table = None
        self._nseg = self._nblocks = 0
        # the transposed 16-bit weights of all modules: one table, one launch
        segs = [sg for m in self.mlps for sg in m._t_segs]
        self._t_table = _transpose_table(segs, self.mlps[0].flat_w.device) if segs else None

    def refresh_transposed(self):
        """flat_w16t of every module from its flat_w16, one launch"""
        if self._t_table is not None:
            t, nseg, nblocks = self._t_table
            check(lib.hctr_transpose16_segments(ptr(t), nseg, nblocks, stream_ptr()))

    @contextlib.contextmanager
    def one_transpose(self):
        """around the per-module steps (sgd_step / ftrl_step / refresh_shadow) of one optimizer
        step: their transposes are left to ONE launch for all modules at the end"""
        for m in self.mlps:
            m._t_hold = True
        try:
            yield
        finally:
            for m in self.mlps:
                m._t_hold = False
        self.refresh_transposed()

    def release(self):
        for m in self.mlps:
            m._finisher = None

    def _segments(self):
        segs = []
        for m in self.mlps:
            base = (m.flat_g.data_ptr(), m.flat_w.data_ptr(), m.flat_w16.data_ptr(),
                    int(m.dtype == torch.bfloat16))
            offw, offb = m._offs
            for i, lw in enumerate(m._lw):
                nw, nb = m.weights[i].numel(), m.biases[i].numel()
                ws, bs = lw.w_seg, lw.b_seg
                if ws is None:
                    segs.append((_SEG_DIRECT, 0, 0, (nw + 3) // 4 * 4, 0, offw[i], 0, 0) + base)
                elif ws[0] == _SEG_SUM:
                    segs.append((_SEG_SUM, ws[1].data_ptr(), ws[2], nw, 0, offw[i], 0,
                                 int(ws[1].dtype == torch.bfloat16)) + base)
                elif ws[0] == _SEG_HEAD:   # n = K, k = batch; db at dst2
                    segs.append((_SEG_HEAD, ws[1].data_ptr(), ws[2], nw, ws[3], offw[i], offb[i],
                                 0) + base)
                else:                      # _SEG_SKINNY: n = N, k = K; db at dst2
                    segs.append((_SEG_SKINNY, ws[1].data_ptr(), ws[2], nb, ws[3], offw[i], offb[i],
                                 0) + base)
                if ws is not None and ws[0] in (_SEG_HEAD, _SEG_SKINNY):
                    continue  # (the bias gradient rides in the same segment)
                if bs is None:
                    segs.append((_SEG_DIRECT, 0, 0, (nb + 3) // 4 * 4, 0, offb[i], 0, 0) + base)
                else:
                    segs.append((_SEG_COLSUM, bs[1].data_ptr(), bs[2], nb, 0, offb[i], 0, 0) + base)
        return tuple(segs)

    def _build(self, segs):
        import numpy as np
        t = np.zeros((len(segs), self._FIELDS), dtype=np.int64)
        block0 = 0
        for r, (kind, src, count, n, k, dst, dst2, src_bf, g, w, w16, bf) in enumerate(segs):
            t[r, :13] = (kind, src, count, n, k, block0, g, w, w16, dst, dst2, bf, src_bf)
            block0 += _count(lib.hctr_dense_seg_blocks(kind, n))
        self._table = torch.from_numpy(t).to(self.mlps[0].flat_w.device)
        self._nseg, self._nblocks = len(segs), block0

    def finish(self, sgd: bool, lr: float = 0.0, grad_scale: float = 1.0):
        segs = self._segments()
        if segs != self._sig:
            self._build(segs)
            self._sig = segs
        loss = None
        for m in self.mlps:
            if m._loss_out is not None:
                loss, m._loss_out = m._loss_out, None
        check(lib.hctr_dense_grad_finish(ptr(self._table), self._nseg, self._nblocks, int(sgd),
                                         float(lr), float(grad_scale), ptr(loss), stream_ptr()))
        if sgd:  # (the 16-bit copies were refreshed)
            self.refresh_transposed()


class DenseFtrl(torch.optim.Optimizer):
    """Ftrl for dense parameters that do not live in one buffer (fp32 models, InnerProduct,
    MultiCross, WeightMultiply, FmOrder2 weights): FtrlOptimizer of the reference
    (R/HugeCTR/src/optimizers/ftrl_optimizer.cu), the whole step as ONE launch
    (`hctr_ftrl_segments`).

    The optimizer owns three flat fp32 buffers over all its parameters -- gradients `g`, and the
    state `z` / `n` (zero at the start) -- every parameter's span starting 16-byte aligned.  Each
    parameter's `.grad` is, for good, a view into `g`: autograd accumulates into an existing
    `.grad` in place, and `zero_grad` zeroes the buffer with one call whatever `set_to_none` says,
    so the gradient addresses never change and the device-resident segment table is built once
    (again only if a parameter's storage moved).  `step()` copies no table and never waits for
    the device.  A `.grad` somebody replaced or dropped is copied back into its view and
    re-attached by the next `step()` / `zero_grad()`.

    `scaler`: the loss scaler the gradients carry; the step divides by it (grad_scale = 1 / scaler),
    so the caller does not.  `lr` lives in `param_groups`.  The state dict holds `z` and `n` per
    parameter, in parameter order, and no hyper-parameters."""

    def __init__(self, params, lr: float, beta: float = 0.0, lambda1: float = 0.0,
                 lambda2: float = 0.0, scaler: float = 1.0):
        super().__init__(params, dict(lr=lr, beta=beta, lambda1=lambda1, lambda2=lambda2))
        assert len(self.param_groups) == 1, "DenseFtrl: one parameter group"
        self.scaler = float(scaler)
        self._params = list(self.param_groups[0]["params"])
        for p in self._params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("DenseFtrl: contiguous fp32 parameters on the GPU only")
        dev = self._params[0].device
        self._spans, tot = [], 0
        for p in self._params:
            self._spans.append((tot, p.numel()))
            tot += (p.numel() + 3) // 4 * 4  # every span starts 16-byte aligned
        self.flat_g = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.flat_z = torch.zeros(tot, dtype=torch.float32, device=dev)
        self.flat_n = torch.zeros(tot, dtype=torch.float32, device=dev)
        self._gviews = [self.flat_g[o:o + c].view_as(p) for p, (o, c) in zip(self._params, self._spans)]
        self._attach()
        self._sig = self._table = None
        self._nblocks = 0

    def _attach(self, keep: bool = True):
        """every parameter's .grad is its view again; keep: what a foreign .grad held goes there"""
        for p, v in zip(self._params, self._gviews):
            if p.grad is not v:
                if keep and p.grad is not None:
                    v.copy_(p.grad)
                p.grad = v

    def _build(self, sig):
        import numpy as np
        per = FTRL_SEG_BLOCK_ELEMS
        t = np.zeros((len(sig), 4), dtype=np.int64)
        block0 = 0
        for r, (w, (off, cnt)) in enumerate(zip(sig, self._spans)):
            t[r] = (w, off, cnt, block0)
            block0 += (cnt + per - 1) // per
        self._table = torch.from_numpy(t).to(self.flat_g.device)
        self._sig, self._nblocks = sig, block0

    def ftrl_state(self):
        """[(z, n)] views per parameter, in parameter order"""
        return [(self.flat_z[o:o + c], self.flat_n[o:o + c]) for o, c in self._spans]

    def zero_grad(self, set_to_none: bool = True):
        self._attach(keep=False)
        self.flat_g.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None, "DenseFtrl: no closure"
        self._attach()
        sig = tuple(p.data_ptr() for p in self._params)
        if sig != self._sig:
            self._build(sig)
        h = self.param_groups[0]
        check(lib.hctr_ftrl_segments(ptr(self._table), len(sig), self._nblocks, float(h["lr"]),
                                     float(h["beta"]), float(h["lambda1"]), float(h["lambda2"]),
                                     1.0 / self.scaler, ptr(self.flat_z), ptr(self.flat_n),
                                     ptr(self.flat_g), stream_ptr()))

    def state_dict(self):
        return ftrl_state_dict(self.ftrl_state())

    def load_state_dict(self, state_dict):
        load_ftrl_state_dict(self.ftrl_state(), state_dict)


def ftrl_state_dict(state):
    """the dense Ftrl state as a checkpoint holds it: `z` and `n` per parameter, in parameter
    order, flat fp32 on the host -- the same for `DenseFtrl` and for flattened FusedMLPs"""
    return {"optimizer": "Ftrl", "z": [z.detach().cpu().clone() for z, _ in state],
            "n": [n.detach().cpu().clone() for _, n in state]}


def load_ftrl_state_dict(state, sd):
    if sd.get("optimizer") != "Ftrl" or len(sd["z"]) != len(state) or len(sd["n"]) != len(state):
        raise ValueError("dense Ftrl state: the file does not match the model's parameters")
    for (z, n), zs, ns in zip(state, sd["z"], sd["n"]):
        if zs.numel() != z.numel() or ns.numel() != n.numel():
            raise ValueError("dense Ftrl state: the file does not match the model's parameters")
    for (z, n), zs, ns in zip(state, sd["z"], sd["n"]):
        z.copy_(zs.reshape(-1))
        n.copy_(ns.reshape(-1))
