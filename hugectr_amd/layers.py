"""torch.autograd wrappers of the dense ops on the path (HIP kernels through the C ABI).

InteractionLayer: R/HugeCTR/include/layers/interaction_layer.hpp:26-67
MultiCrossLayer:  R/HugeCTR/include/layers/multi_cross_layer.hpp:104-177
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .dense import _DT16, split_k_wgrad

_DT = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


class _InteractionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mlp, emb):
        mlp, emb = mlp.contiguous(), emb.contiguous()
        B, W = mlp.shape
        n_emb = emb.shape[1]
        n_ins = n_emb + 1
        out = torch.empty((B, W + n_ins * (n_ins - 1) // 2 + 1), dtype=mlp.dtype, device=mlp.device)
        check(lib.hctr_interaction_fwd(B, n_emb, W, ptr(mlp), ptr(emb), ptr(out), _DT[mlp.dtype],
                                       stream_ptr()))
        ctx.save_for_backward(mlp, emb)
        return out

    @staticmethod
    def backward(ctx, grad):
        mlp, emb = ctx.saved_tensors
        grad = grad.contiguous()
        B, W = mlp.shape
        n_emb = emb.shape[1]
        mlp_grad = torch.empty_like(mlp)
        emb_grad = torch.empty_like(emb)
        check(lib.hctr_interaction_bwd(B, n_emb, W, ptr(mlp), ptr(emb), ptr(grad), ptr(mlp_grad),
                                       ptr(emb_grad), _DT[mlp.dtype], stream_ptr()))
        return mlp_grad, emb_grad


class _InteractionIndexedFn(torch.autograd.Function):
    """interaction over a table of distinct rows (unique-row exchange): embedding s of sample b is
    rows[row_of[b, s]].  `on_emb_grad(dE)` receives the dense [B, n_emb, W] embedding gradient as
    soon as it exists (the exchange reduces it per row); rows itself gets no gradient here."""

    @staticmethod
    def forward(ctx, mlp, rows, row_of, on_emb_grad, scatter_grad=False):
        mlp = mlp.contiguous()
        ctx.scatter_grad = scatter_grad
        B, W = mlp.shape
        n_emb = row_of.shape[1]
        n_ins = n_emb + 1
        out = torch.empty((B, W + n_ins * (n_ins - 1) // 2 + 1), dtype=mlp.dtype, device=mlp.device)
        check(lib.hctr_interaction_fwd_indexed(B, n_emb, W, ptr(mlp), ptr(rows), ptr(row_of),
                                               ptr(out), _DT[mlp.dtype], stream_ptr()))
        ctx.save_for_backward(mlp, rows, row_of)
        ctx.on_emb_grad = on_emb_grad
        return out

    @staticmethod
    def backward(ctx, grad):
        mlp, rows, row_of = ctx.saved_tensors
        grad = grad.contiguous()
        B, W = mlp.shape
        n_emb = row_of.shape[1]
        mlp_grad = torch.empty_like(mlp)
        emb_grad = torch.empty((B, n_emb, W), dtype=mlp.dtype, device=mlp.device)
        fn = lib.hctr_interaction_bwd_indexed_scatter if ctx.scatter_grad else \
            lib.hctr_interaction_bwd_indexed
        check(fn(B, n_emb, W, ptr(mlp), ptr(rows), ptr(row_of), ptr(grad), ptr(mlp_grad),
                 ptr(emb_grad), _DT[mlp.dtype], stream_ptr()))
        if ctx.on_emb_grad is not None:
            ctx.on_emb_grad(emb_grad)
        return mlp_grad, None, None, None, None


class _InteractionGatherFn(torch.autograd.Function):
    """gather fused into the interaction (one GPU, one key per bucket): the embedding's table rows
    are read through its value_index straight into the interaction's LDS tile, the pooled vectors
    are written once for the backward.  `on_emb_grad(dE)` receives the [B, n_emb, W] gradient of
    the pooled vectors as soon as it exists (the sparse update consumes it)."""

    @staticmethod
    def forward(ctx, mlp, emb, is_train, on_emb_grad):
        mlp = mlp.contiguous()
        B, W = mlp.shape
        n_emb = emb.slot_num
        n_ins = n_emb + 1
        out = torch.empty((B, W + n_ins * (n_ins - 1) // 2 + 1), dtype=mlp.dtype, device=mlp.device)
        pooled = torch.empty((B, n_emb, W), dtype=mlp.dtype, device=mlp.device)
        check(lib.hctr_emb_forward_interaction(emb._h, 1 if is_train else 0, ptr(mlp), ptr(pooled),
                                               ptr(out), stream_ptr()))
        ctx.save_for_backward(mlp, pooled)
        ctx.on_emb_grad = on_emb_grad
        return out

    @staticmethod
    def backward(ctx, grad):
        mlp, pooled = ctx.saved_tensors
        grad = grad.contiguous()
        B, W = mlp.shape
        n_emb = pooled.shape[1]
        mlp_grad = torch.empty_like(mlp)
        emb_grad = torch.empty_like(pooled)
        check(lib.hctr_interaction_bwd(B, n_emb, W, ptr(mlp), ptr(pooled), ptr(grad), ptr(mlp_grad),
                                       ptr(emb_grad), _DT[mlp.dtype], stream_ptr()))
        if ctx.on_emb_grad is not None:
            ctx.on_emb_grad(emb_grad)
        return mlp_grad, None, None, None


class _InteractionRegatherFn(torch.autograd.Function):
    """_InteractionGatherFn without the pooled vectors: the forward does not write them, the
    backward reads the training batch's table rows again (hctr_emb_backward_interaction).  The
    rows must not change in between: the embedding's update comes after on_emb_grad."""

    @staticmethod
    def forward(ctx, mlp, emb, is_train, on_emb_grad):
        mlp = mlp.contiguous()
        B, W = mlp.shape
        n_ins = emb.slot_num + 1
        out = torch.empty((B, W + n_ins * (n_ins - 1) // 2 + 1), dtype=mlp.dtype, device=mlp.device)
        check(lib.hctr_emb_forward_interaction(emb._h, 1 if is_train else 0, ptr(mlp), None,
                                               ptr(out), stream_ptr()))
        ctx.save_for_backward(mlp)
        ctx.emb, ctx.is_train, ctx.on_emb_grad = emb, is_train, on_emb_grad
        return out

    @staticmethod
    def backward(ctx, grad):
        (mlp,) = ctx.saved_tensors
        if not ctx.is_train:
            raise RuntimeError("interaction_gather: backward of an evaluation batch")
        grad = grad.contiguous()
        B, W = mlp.shape
        mlp_grad = torch.empty_like(mlp)
        emb_grad = torch.empty((B, ctx.emb.slot_num, W), dtype=mlp.dtype, device=mlp.device)
        check(lib.hctr_emb_backward_interaction(ctx.emb._h, ptr(mlp), ptr(grad), ptr(mlp_grad),
                                                ptr(emb_grad), stream_ptr()))
        if ctx.on_emb_grad is not None:
            ctx.on_emb_grad(emb_grad)
        return mlp_grad, None, None, None


def regather_supported(width: int, n_emb: int) -> bool:
    """shapes whose backward can read the rows again (hctr_interaction_bwd_gather)"""
    n_ins = n_emb + 1
    return width in (32, 64, 128) and n_emb <= 31 and (width + n_ins * (n_ins - 1) // 2 + 1) % 8 == 0


def interaction_gather(mlp: torch.Tensor, emb, is_train: bool = True, on_emb_grad=None,
                       store_pooled: bool = True):
    """mlp [B, W] 16-bit; emb: a SparseEmbeddingHash (world 1, one key per bucket, vector size W,
    output type = mlp's) whose index stage has run (emb.index) -> interaction output; the pooled
    vectors never make a second trip through HBM.  store_pooled=False (regather_supported shapes):
    they are not written at all, the backward reads the current training batch's rows again -- no
    row of it may be updated before that backward has run."""
    assert mlp.dtype == emb.out_dtype and mlp.shape[1] == emb.embedding_vec_size
    if store_pooled:
        return _InteractionGatherFn.apply(mlp, emb, is_train, on_emb_grad)
    assert regather_supported(mlp.shape[1], emb.slot_num)
    return _InteractionRegatherFn.apply(mlp, emb, is_train, on_emb_grad)


def interaction_indexed(mlp: torch.Tensor, rows: torch.Tensor, row_of: torch.Tensor,
                        on_emb_grad=None, scatter_grad: bool = False) -> torch.Tensor:
    """mlp [B,W], rows [R,W] (same 16-bit dtype), row_of int32 [B,n_emb] -> interaction output.
    scatter_grad (row_of must be a bijection onto the B * n_emb rows, e.g. the reorder map of an
    all-to-all receive buffer): on_emb_grad receives the embedding gradient in the ROWS' layout
    (row row_of[b, s] = gradient of embedding s of sample b) instead of [B, n_emb, W]"""
    assert rows.dtype == mlp.dtype and row_of.dtype == torch.int32 and rows.is_contiguous()
    assert not scatter_grad or rows.shape[0] == row_of.numel()
    return _InteractionIndexedFn.apply(mlp, rows, row_of.contiguous(), on_emb_grad, scatter_grad)


def interaction(mlp: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
    """mlp [B,W], emb [B,n_emb,W] -> [B, W + n_ins(n_ins-1)/2 + 1] (last column zero)."""
    return _InteractionFn.apply(mlp, emb)


class InteractionLayer(torch.nn.Module):
    def forward(self, mlp, emb):
        return interaction(mlp, emb)


class _MultiHeadAttentionFn(torch.autograd.Function):
    """attention.hip's two kernel families, chosen by shape alone.  m, n <= 128 and d <= 64:
    hctr_mha_fwd / hctr_mha_bwd, one wavefront per (sample, head); the backward recomputes the
    probabilities from q, k and the mask, which are all that is saved.  Everything else up to
    4096 x 4096 x 128: hctr_mha_tiled_fwd / hctr_mha_tiled_bwd, which also keep the output and
    four fp32 statistics per (head, query row).  With the two fp32 length vectors in the place of
    the mask: the *_len_* entry of the same family, and the lengths are what is saved"""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, len_from, len_to):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, m, hidden = q.shape
        n = k.shape[1]
        if k.shape != (B, n, hidden) or v.shape != k.shape or hidden % heads != 0:
            raise ValueError(f"multi_head_attention: q {tuple(q.shape)}, k {tuple(k.shape)}, "
                             f"v {tuple(v.shape)}, {heads} heads")
        if k.dtype != q.dtype or v.dtype != q.dtype:
            raise ValueError("multi_head_attention: q, k and v of one dtype")
        if mask is not None:
            if mask.shape != (B, 1, m, n) or mask.dtype != q.dtype:
                raise ValueError(f"multi_head_attention: mask {tuple(mask.shape)} {mask.dtype}, "
                                 f"expected {(B, 1, m, n)} {q.dtype}")
            mask = mask.contiguous()
        for x in (len_from, len_to):
            if x is not None and (x.shape != (B,) or x.device != q.device):
                raise ValueError(f"multi_head_attention: lengths {tuple(x.shape)} on {x.device}, "
                                 f"expected {(B,)} on {q.device}")
        out = torch.empty_like(q)
        ctx.heads, ctx.lengths = heads, len_from is not None
        ctx.tiled = max(m, n) > 128 or hidden // heads > 64
        # the mask's place in the argument list: one pointer, or the two length vectors
        src = (ptr(len_from), ptr(len_to)) if ctx.lengths else (ptr(mask),)
        shape = (B, heads, m, n, hidden // heads, ptr(q), ptr(k), ptr(v), *src)
        if not ctx.tiled:
            fn = lib.hctr_mha_len_fwd if ctx.lengths else lib.hctr_mha_fwd
            check(fn(*shape, ptr(out), _DT[q.dtype], stream_ptr()))
            ctx.save_for_backward(q, k, v, mask, len_from, len_to)
            return out
        stats = None
        if any(ctx.needs_input_grad[:3]):
            stats = torch.empty((B, heads, m, 4), dtype=torch.float32, device=q.device)
        fn = lib.hctr_mha_tiled_len_fwd if ctx.lengths else lib.hctr_mha_tiled_fwd
        check(fn(*shape, ptr(out), ptr(stats), _DT[q.dtype], stream_ptr()))
        ctx.save_for_backward(q, k, v, mask, len_from, len_to, out, stats)
        return out

    @staticmethod
    def backward(ctx, grad):
        q, k, v, mask, len_from, len_to = ctx.saved_tensors[:6]
        grad = grad.contiguous()
        B, m, hidden = q.shape
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        src = (ptr(len_from), ptr(len_to)) if ctx.lengths else (ptr(mask),)
        shape = (B, ctx.heads, m, k.shape[1], hidden // ctx.heads, ptr(q), ptr(k), ptr(v), *src)
        grads = (ptr(grad), ptr(dq), ptr(dk), ptr(dv), _DT[q.dtype], stream_ptr())
        if ctx.tiled:
            out, stats = ctx.saved_tensors[6:]
            fn = lib.hctr_mha_tiled_len_bwd if ctx.lengths else lib.hctr_mha_tiled_bwd
            check(fn(*shape, ptr(out), ptr(stats), *grads))
        else:
            fn = lib.hctr_mha_len_bwd if ctx.lengths else lib.hctr_mha_bwd
            check(fn(*shape, *grads))
        return dq, dk, dv, None, None, None, None


def multi_head_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask, heads: int,
                         lengths=None):
    """q [B, m, H d], k, v [B, n, H d], mask None or [B, 1, m, n] in q's dtype ->
    [B, m, H d]: per head softmax(Q K^T / sqrt(d) - (1 - mask) 10000) V, the softmax's sum taken
    with + 1e-6.  The mask is read as a value, not as a flag: 1 keeps a key, 0 puts it 10000 below,
    anything between puts it (1 - mask) 10000 below; what a whole row has in common cancels, so a
    fully masked row attends as if it had no mask.  m, n <= 4096, d a
    multiple of 8 up to 128; fp32 / fp16 / bf16.  m, n <= 128 with d <= 64 run on the kernels that
    hold a whole head in one wavefront, every other shape on the tiled kernels; the shape alone
    decides.

    lengths = (len_from, len_to), two [B] tensors of fp32 / fp16 / bf16 (what sequence_mask
    accepts; widened to fp32 here, which is exact; no gradient), in the place of mask: the result
    of mask = sequence_mask(len_from, len_to, m, n) without that tensor being written or read, and
    without the work on keys past len_to.  A masked key's weight is exactly 0 where the dense mask
    gives exp(-10000 + the row's spread of scores), which is 0 in fp32 below a spread of about
    9 890 (include/hugectr_amd.h, hctr_mha_len_fwd)."""
    len_from = len_to = None
    if lengths is not None:
        if mask is not None:
            raise ValueError("multi_head_attention: mask or lengths, not both")
        if len(lengths) != 2 or any(not torch.is_tensor(x) or x.dtype not in _DT for x in lengths):
            raise ValueError("multi_head_attention: lengths = (len_from, len_to), fp32 / fp16 / bf16")
        len_from, len_to = (x.detach().float().contiguous() for x in lengths)
    return _MultiHeadAttentionFn.apply(q, k, v, mask, heads, len_from, len_to)


class MultiHeadAttentionLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/multi_head_attention_layer.hpp (3-D inputs) with the masked
    softmax folded in -- and, given lengths, the sequence mask too; no weights"""

    def __init__(self, num_attention_heads: int = 1):
        super().__init__()
        self.num_attention_heads = num_attention_heads

    def forward(self, q, k, v, mask=None, lengths=None):
        return multi_head_attention(q, k, v, mask, self.num_attention_heads, lengths)


def sequence_mask(len_from: torch.Tensor, len_to: torch.Tensor, max_from: int, max_to: int):
    """len_from, len_to [B] (fp32 / fp16 / bf16, as the reference reads them from the dense input)
    -> mask [B, 1, max_from, max_to] of that dtype: 1 where i < len_from[b] and j < len_to[b]"""
    len_from, len_to = len_from.contiguous(), len_to.contiguous()
    if len_from.dim() != 1 or len_to.shape != len_from.shape or len_to.dtype != len_from.dtype:
        raise ValueError("sequence_mask: len_from and len_to are [B] vectors of one dtype")
    B = len_from.shape[0]
    mask = torch.empty((B, 1, max_from, max_to), dtype=len_from.dtype, device=len_from.device)
    check(lib.hctr_sequence_mask(B, max_from, max_to, ptr(len_from), ptr(len_to), ptr(mask),
                                 _DT[len_from.dtype], stream_ptr()))
    return mask


class SequenceMaskLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/sequence_mask_layer.hpp; no weights"""

    def __init__(self, max_sequence_len_from: int, max_sequence_len_to: int):
        super().__init__()
        self.max_sequence_len_from = max_sequence_len_from
        self.max_sequence_len_to = max_sequence_len_to

    def forward(self, len_from, len_to):
        return sequence_mask(len_from, len_to, self.max_sequence_len_from, self.max_sequence_len_to)


class _LayerNormFn(torch.autograd.Function):
    """layer_norm.hip: hctr_layer_norm_fwd / hctr_layer_norm_bwd.  Saved for the backward: x, residual,
    gamma and two fp32 statistics per row (mean, 1 / std), which exist only when some input wants a
    gradient; the normalised rows are recomputed.  x and residual share one gradient tensor"""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, residual):
        hidden = gamma.numel()
        if x.dim() < 1 or x.shape[-1] != hidden or gamma.shape != (hidden,) or beta.shape != gamma.shape:
            raise ValueError(f"layer_norm: x {tuple(x.shape)}, gamma {tuple(gamma.shape)}, "
                             f"beta {tuple(beta.shape)}")
        if x.dtype not in _DT or gamma.dtype != torch.float32 or beta.dtype != torch.float32:
            raise ValueError("layer_norm: x of fp32 / fp16 / bf16, gamma and beta of fp32")
        if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype):
            raise ValueError(f"layer_norm: residual {tuple(residual.shape)} {residual.dtype}, "
                             f"expected {tuple(x.shape)} {x.dtype}")
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        residual = None if residual is None else residual.contiguous()
        rows = x.numel() // max(hidden, 1)
        y = torch.empty_like(x)
        stats = None
        if any(ctx.needs_input_grad):
            stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        check(lib.hctr_layer_norm_fwd(rows, hidden, ptr(x), ptr(residual), ptr(gamma), ptr(beta), eps,
                                      ptr(y), ptr(stats), _DT[x.dtype], stream_ptr()))
        ctx.save_for_backward(x, residual, gamma, stats)
        return y

    @staticmethod
    def backward(ctx, grad):
        x, residual, gamma, stats = ctx.saved_tensors
        grad = grad.contiguous()
        hidden = gamma.numel()
        rows = x.numel() // hidden
        dz, dgamma, dbeta = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        scratch = torch.empty(lib.hctr_layer_norm_bwd_scratch_bytes(rows, hidden) // 4,
                              dtype=torch.float32, device=x.device)
        check(lib.hctr_layer_norm_bwd(rows, hidden, ptr(x), ptr(residual), ptr(gamma), ptr(stats),
                                      ptr(grad), ptr(dz), ptr(dgamma), ptr(dbeta), ptr(scratch),
                                      _DT[x.dtype], stream_ptr()))
        return dz, dgamma, dbeta, None, None if residual is None else dz


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
               residual=None):
    """x [..., hidden] (fp32 / fp16 / bf16), gamma and beta [hidden] fp32, residual None or like x ->
    like x: per row of z = x (+ residual), (z - mean) / sqrt(var + eps) * gamma + beta with the biased
    variance, in fp32.  hidden 1 .. 8192, any value; x and residual receive the same gradient"""
    return _LayerNormFn.apply(x, gamma, beta, eps, residual)


class LayerNormLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/layer_norm_layer.hpp over the last dimension, with the Add that
    precedes it in a transformer block as an optional second input; fp32 gamma = 1, beta = 0"""

    def __init__(self, hidden: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.gamma = torch.nn.Parameter(torch.ones(hidden, dtype=torch.float32))
        self.beta = torch.nn.Parameter(torch.zeros(hidden, dtype=torch.float32))

    def forward(self, x, residual=None):
        return layer_norm(x, self.gamma, self.beta, self.eps, residual)


def _columns(op, x):
    """(rows, n) of the reference's rule: rows = shape[0], every other dimension is a column"""
    if x.dim() < 1 or x.dtype not in _DT:
        raise ValueError(f"{op}: x of fp32 / fp16 / bf16 with at least one dimension, got "
                         f"{tuple(x.shape)} {x.dtype}")
    n = 1
    for d in x.shape[1:]:
        n *= d
    return x.shape[0], n


def _col_scratch(rows, n, device):
    return torch.empty(lib.hctr_col_stats_scratch_bytes(rows, n) // 4, dtype=torch.float32,
                       device=device)


class _BatchNormFn(torch.autograd.Function):
    """batch_norm.hip: hctr_batch_norm_fwd / hctr_batch_norm_bwd.  Saved for the backward: x, gamma and
    the fp32 [2][n] (mean, 1 / std) of the batch, which exist only when some input wants a gradient;
    the normalised values are recomputed.  The running statistics are updated in place"""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, factor, eps):
        rows, n = _columns("batch_norm", x)
        per_col = (gamma, beta, running_mean, running_var)
        if any(t.shape != (n,) or t.dtype != torch.float32 for t in per_col):
            raise ValueError(f"batch_norm: gamma, beta, running_mean, running_var of fp32 [{n}] for x "
                             f"{tuple(x.shape)}, got {[tuple(t.shape) for t in per_col]}")
        if any(not t.is_contiguous() for t in (running_mean, running_var)):
            raise ValueError("batch_norm: running_mean and running_var contiguous (updated in place)")
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        y = torch.empty_like(x)
        save = None
        if training and any(ctx.needs_input_grad):
            save = torch.empty((2, n), dtype=torch.float32, device=x.device)
        scratch = _col_scratch(rows, n, x.device) if training else None
        check(lib.hctr_batch_norm_fwd(rows, n, ptr(x), ptr(gamma), ptr(beta), factor, eps,
                                      ptr(running_mean), ptr(running_var), ptr(y), ptr(save),
                                      ptr(scratch), int(training), _DT[x.dtype], stream_ptr()))
        ctx.save_for_backward(x, gamma, save)
        return y

    @staticmethod
    def backward(ctx, grad):
        x, gamma, save = ctx.saved_tensors
        if save is None:
            raise ValueError("batch_norm: the backward needs the batch statistics of a training forward")
        grad = grad.contiguous()
        rows, n = x.shape[0], gamma.numel()
        dx, dgamma, dbeta = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        scratch = _col_scratch(rows, n, x.device)
        check(lib.hctr_batch_norm_bwd(rows, n, ptr(x), ptr(gamma), ptr(save), ptr(grad), ptr(dx),
                                      ptr(dgamma), ptr(dbeta), ptr(scratch), _DT[x.dtype],
                                      stream_ptr()))
        return dx, dgamma, dbeta, None, None, None, None, None


def batch_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor,
               running_var: torch.Tensor, training: bool, factor: float = 1.0, eps: float = 1e-5):
    """x [rows, ...] (fp32 / fp16 / bf16), everything after the first dimension a column (n of them,
    1 .. 65536); gamma, beta, running_mean, running_var [n] fp32 -> like x.  training: the batch's
    mean and biased variance per column, (x - mean) / sqrt(var + eps) * gamma + beta, and
    running = (1 - factor) running + factor (mean, unbiased var) in place; else the running
    statistics in the same formula, one launch"""
    return _BatchNormFn.apply(x, gamma, beta, running_mean, running_var, training, factor, eps)


class BatchNormLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/batch_norm_layer.hpp; fp32 gamma = 1, beta = 0, buffers
    running_mean = 0, running_var = 1; self.training picks the path.  With the reference's default
    factor = 1 the running statistics are those of the last training batch, so the buffers' initial
    values no longer matter after one step"""

    def __init__(self, num_features: int, factor: float = 1.0, eps: float = 1e-5):
        super().__init__()
        self.factor, self.eps = factor, eps
        self.gamma = torch.nn.Parameter(torch.ones(num_features, dtype=torch.float32))
        self.beta = torch.nn.Parameter(torch.zeros(num_features, dtype=torch.float32))
        self.register_buffer("running_mean", torch.zeros(num_features, dtype=torch.float32))
        self.register_buffer("running_var", torch.ones(num_features, dtype=torch.float32))

    def forward(self, x):
        return batch_norm(x, self.gamma, self.beta, self.running_mean, self.running_var,
                          self.training, self.factor, self.eps)


class _PReLUDiceFn(torch.autograd.Function):
    """batch_norm.hip: hctr_prelu_dice_fwd / hctr_prelu_dice_bwd.  Saved for the backward: x and the
    fp32 [2][n] (mean, var) of the batch, which exist only when x wants a gradient"""

    @staticmethod
    def forward(ctx, x, alpha, eps):
        rows, n = _columns("prelu_dice", x)
        x = x.contiguous()
        y = torch.empty_like(x)
        stats = None
        if ctx.needs_input_grad[0]:
            stats = torch.empty((2, n), dtype=torch.float32, device=x.device)
        scratch = _col_scratch(rows, n, x.device)
        check(lib.hctr_prelu_dice_fwd(rows, n, ptr(x), alpha, eps, ptr(y), ptr(stats), ptr(scratch),
                                      _DT[x.dtype], stream_ptr()))
        ctx.save_for_backward(x, stats)
        ctx.alpha, ctx.eps = alpha, eps
        return y

    @staticmethod
    def backward(ctx, grad):
        x, stats = ctx.saved_tensors
        grad = grad.contiguous()
        dx = torch.empty_like(x)
        check(lib.hctr_prelu_dice_bwd(x.shape[0], stats.shape[1], ptr(x), ptr(stats), ctx.alpha,
                                      ctx.eps, ptr(grad), ptr(dx), _DT[x.dtype], stream_ptr()))
        return dx, None, None


def prelu_dice(x: torch.Tensor, alpha: float, eps: float):
    """x [rows, ...] (fp32 / fp16 / bf16) -> like x: p x + (1 - p) alpha x with
    p = sigmoid((x - mean) / sqrt(var + eps)) of the batch's mean and biased variance per column, in
    training and evaluation alike.  The gradient is the reference's: every element sees only its own
    1 / rows share of mean and variance"""
    return _PReLUDiceFn.apply(x, alpha, eps)


class PReLUDiceLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/prelu_dice_layer.hpp; no weights"""

    def __init__(self, alpha: float, eps: float):
        super().__init__()
        self.alpha, self.eps = alpha, eps

    def forward(self, x):
        return prelu_dice(x, self.alpha, self.eps)


def _matmul_shape(a, b):
    """(batch, m, n, k, output shape) of the reference's four input forms"""
    da, db = a.dim(), b.dim()
    if a.dtype not in _DT or b.dtype != a.dtype:
        raise ValueError(f"matrix_multiply: a and b of one dtype, fp32 / fp16 / bf16, got {a.dtype}, "
                         f"{b.dtype}")
    if (da, db) == (2, 3):  # [m, n] x [n, g, h] -> [m, g, h]
        ok, batch, k, out = a.shape[1] == b.shape[0], 1, b.shape[1] * b.shape[2], (a.shape[0], *b.shape[1:])
    else:
        ok = da == db and da in (2, 3, 4) and a.shape[:-2] == b.shape[:-2] and a.shape[-1] == b.shape[-2]
        batch = 1
        for d in a.shape[:-2]:
            batch *= d
        k, out = b.shape[-1], (*a.shape[:-1], b.shape[-1])
    if not ok:
        raise ValueError(f"matrix_multiply: [m, n] x [n, k] with zero, one or two equal leading "
                         f"dimensions, or [m, n] x [n, g, h]; got {tuple(a.shape)} x {tuple(b.shape)}")
    return batch, a.shape[-2], a.shape[-1], k, out


class _MatrixMultiplyFn(torch.autograd.Function):
    """sequence_ops.hip: hctr_matmul_fwd / hctr_matmul_bwd.  Saved for the backward: a and b
    themselves (no copy); an input that wants no gradient gets none computed"""

    @staticmethod
    def forward(ctx, a, b):
        batch, m, n, k, out = _matmul_shape(a, b)
        a, b = a.contiguous(), b.contiguous()
        c = torch.empty(out, dtype=a.dtype, device=a.device)
        check(lib.hctr_matmul_fwd(batch, m, n, k, ptr(a), ptr(b), ptr(c), _DT[a.dtype], stream_ptr()))
        ctx.save_for_backward(a, b)
        ctx.dims = (batch, m, n, k)
        return c

    @staticmethod
    def backward(ctx, grad):
        a, b = ctx.saved_tensors
        grad = grad.contiguous()
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        check(lib.hctr_matmul_bwd(*ctx.dims, ptr(a), ptr(b), ptr(grad), ptr(da), ptr(db),
                                  _DT[a.dtype], stream_ptr()))
        return da, db


def matrix_multiply(a: torch.Tensor, b: torch.Tensor):
    """a [..., m, n] x b [..., n, k] -> [..., m, k] per item, for 2-D x 2-D, 3-D x 3-D, 4-D x 4-D
    (equal leading sizes) and [m, n] x [n, g, h] -> [m, g, h]; fp32 / fp16 / bf16, m, n, k 1 .. 4096,
    fp32 sums rounded once.  Small items (m n + n k + m k <= 1024) run packed, the rest on MFMA tiles"""
    return _MatrixMultiplyFn.apply(a, b)


class MatrixMultiplyLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/matrix_multiply_layer.hpp; no weights"""

    def forward(self, a, b):
        return matrix_multiply(a, b)


class _ReduceMeanFn(torch.autograd.Function):
    """sequence_ops.hip: hctr_reduce_mean_fwd / hctr_reduce_mean_bwd.  Nothing is saved"""

    @staticmethod
    def forward(ctx, x, axis):
        if x.dtype not in _DT or not 1 <= x.dim() <= 3:
            raise ValueError(f"reduce_mean: x of fp32 / fp16 / bf16 with 1 to 3 dimensions, got "
                             f"{tuple(x.shape)} {x.dtype}")
        if not 0 <= axis < x.dim():
            raise ValueError(f"reduce_mean: axis 0 .. {x.dim() - 1} for x {tuple(x.shape)}, got {axis}")
        x = x.contiguous()
        outer, inner = 1, 1
        for d in x.shape[:axis]:
            outer *= d
        for d in x.shape[axis + 1:]:
            inner *= d
        ctx.dims, ctx.shape = (outer, x.shape[axis], inner), x.shape
        y = torch.empty((*x.shape[:axis], 1, *x.shape[axis + 1:]), dtype=x.dtype, device=x.device)
        check(lib.hctr_reduce_mean_fwd(*ctx.dims, ptr(x), ptr(y), _DT[x.dtype], stream_ptr()))
        return y

    @staticmethod
    def backward(ctx, grad):
        grad = grad.contiguous()
        dx = torch.empty(ctx.shape, dtype=grad.dtype, device=grad.device)
        check(lib.hctr_reduce_mean_bwd(*ctx.dims, ptr(grad), ptr(dx), _DT[grad.dtype], stream_ptr()))
        return dx, None


def reduce_mean(x: torch.Tensor, axis: int):
    """x of 1 to 3 dimensions (fp32 / fp16 / bf16) -> its mean over `axis`, which stays with size 1;
    fp32 sums in a fixed order, rounded once"""
    return _ReduceMeanFn.apply(x, axis)


class ReduceMeanLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/reduce_mean_layer.hpp; no weights"""

    def __init__(self, axis: int):
        super().__init__()
        self.axis = axis

    def forward(self, x):
        return reduce_mean(x, self.axis)


def _frc_call(entry, tensors, widths, batch, slots, item, ad, dtype):
    """the host-side arrays of device pointers and widths the entry points take by value"""
    num = len(tensors)
    ptrs = (ctypes.c_void_p * num)(*[t.data_ptr() for t in tensors])
    check(entry(batch, slots, num, ptrs, (ctypes.c_int * num)(*widths), ptr(item), ptr(ad),
                _DT[dtype], stream_ptr()))


class _FusedReshapeConcatFn(torch.autograd.Function):
    """sequence_ops.hip: hctr_fused_reshape_concat_fwd / _bwd.  Nothing is saved but the shapes"""

    @staticmethod
    def forward(ctx, *inputs):
        if not 1 <= len(inputs) <= 8:
            raise ValueError(f"fused_reshape_concat: 1 .. 8 inputs, got {len(inputs)}")
        first = inputs[0]
        for t in inputs:
            if t.dim() != 3 or t.dtype not in _DT or t.dtype != first.dtype or t.shape[:2] != first.shape[:2]:
                raise ValueError("fused_reshape_concat: inputs [B, S, w_i] of one dtype (fp32 / fp16 / "
                                 f"bf16) with equal B and S, got {[tuple(t.shape) for t in inputs]}")
        if first.shape[1] < 1 or any(t.shape[2] < 1 for t in inputs):
            raise ValueError(f"fused_reshape_concat: S >= 1 and every width >= 1, got "
                             f"{[tuple(t.shape) for t in inputs]}")
        inputs = [t.contiguous() for t in inputs]
        batch, slots = first.shape[:2]
        ctx.widths = [t.shape[2] for t in inputs]
        ctx.dims = (batch, slots)
        W = sum(ctx.widths)
        item = torch.empty((batch * (slots - 1), W), dtype=first.dtype, device=first.device)
        ad = torch.empty((batch, W), dtype=first.dtype, device=first.device)
        _frc_call(lib.hctr_fused_reshape_concat_fwd, inputs, ctx.widths, batch, slots, item, ad,
                  first.dtype)
        return item, ad

    @staticmethod
    def backward(ctx, ditem, dad):
        ditem, dad = ditem.contiguous(), dad.contiguous()
        batch, slots = ctx.dims
        grads = [torch.empty((batch, slots, w), dtype=dad.dtype, device=dad.device) for w in ctx.widths]
        _frc_call(lib.hctr_fused_reshape_concat_bwd, grads, ctx.widths, batch, slots, ditem, dad,
                  dad.dtype)
        return tuple(grads)


def fused_reshape_concat(inputs):
    """inputs: 1 .. 8 tensors [B, S, w_i] of one dtype -> (item [B (S - 1), W], ad [B, W]) with
    W = sum w_i: the inputs side by side, slots 0 .. S - 2 of every sample in item, the last in ad"""
    return _FusedReshapeConcatFn.apply(*inputs)


class FusedReshapeConcatLayer(torch.nn.Module):
    """R/HugeCTR/include/layers/fused_reshape_concat_layer.hpp; no weights"""

    def forward(self, inputs):
        return fused_reshape_concat(inputs)


def _gru_dims(x, weight, hidden, batch_first):
    """(batch, seq, vec, hidden, batch_first) of the C entry points"""
    if x.dim() != 3 or x.dtype not in _DT:
        raise ValueError(f"gru: x of three dimensions, [S, B, V] or (batch_first) [B, S, V], fp32 / "
                         f"fp16 / bf16; got {tuple(x.shape)} {x.dtype}")
    if not isinstance(hidden, int) or hidden < 1:
        raise ValueError(f"gru: hidden >= 1, got {hidden!r}")
    vec = x.shape[2]
    if hidden > 256 or not 1 <= vec <= 1024:
        raise ValueError(f"gru: hidden 1 .. 256 and x's last dimension (the vector size) 1 .. 1024, "
                         f"got hidden = {hidden}, x {tuple(x.shape)}")
    if weight.device != x.device:
        raise ValueError(f"gru: weight on x's device, got {weight.device} and {x.device}")
    if weight.dim() != 1 or weight.numel() != 3 * hidden * (vec + hidden + 1) or weight.dtype != x.dtype:
        raise ValueError(f"gru: weight is one flat vector of 3 H V + 3 H H + 3 H = "
                         f"{3 * hidden * (vec + hidden + 1)} elements of x's dtype (H = {hidden}, V = "
                         f"{vec}); got {tuple(weight.shape)} {weight.dtype}")
    batch, seq = (x.shape[0], x.shape[1]) if batch_first else (x.shape[1], x.shape[0])
    return batch, seq, vec, hidden, int(bool(batch_first))


class _GRUFn(torch.autograd.Function):
    """gru.hip: hctr_gru_fwd / hctr_gru_bwd.  Saved for the backward: x, weight, y and the fp32
    reserve [S][B][4][H] (r, z, n, Rn h), which a forward without gradient does not write"""

    @staticmethod
    def forward(ctx, x, weight, hidden, batch_first):
        dims = _gru_dims(x, weight, hidden, batch_first)
        x, weight = x.contiguous(), weight.contiguous()
        y = torch.empty((*x.shape[:2], hidden), dtype=x.dtype, device=x.device)
        train = any(ctx.needs_input_grad[:2])
        sizes = (ctypes.c_size_t(), ctypes.c_size_t())
        check(lib.hctr_gru_workspace(*dims[:4], ctypes.byref(sizes[0]), ctypes.byref(sizes[1])))
        reserve = torch.empty(sizes[0].value // 4, dtype=torch.float32, device=x.device) if train else None
        check(lib.hctr_gru_fwd(*dims, ptr(x), ptr(weight), ptr(y), ptr(reserve), _DT[x.dtype],
                               stream_ptr()))
        if train:
            ctx.save_for_backward(x, weight, y, reserve)
            ctx.dims, ctx.scratch = dims, sizes[1].value // 4
        return y

    @staticmethod
    def backward(ctx, grad):
        x, weight, y, reserve = ctx.saved_tensors
        grad = grad.contiguous()
        dx, dw = torch.empty_like(x), torch.empty_like(weight)
        scratch = torch.empty(ctx.scratch, dtype=torch.float32, device=x.device)
        check(lib.hctr_gru_bwd(*ctx.dims, ptr(x), ptr(weight), ptr(y), ptr(reserve), ptr(grad), ptr(dx),
                               ptr(dw), ptr(scratch), _DT[x.dtype], stream_ptr()))
        return dx, dw, None, None


def gru(x: torch.Tensor, weight: torch.Tensor, hidden: int, batch_first: bool = False):
    """x [S, B, V] (batch_first: [B, S, V]) -> y [S, B, H] ([B, S, H]): a one-layer GRU with initial
    state zero.  weight: flat, Wr Wz Wn [H][V], Rr Rz Rn [H][H], br bz bn [H] (z the update gate);
    n = tanh(Wn x + r o (Rn h) + bn), h_t = (1 - z) o n + z o h_{t-1}.  fp32 / fp16 / bf16, H 1 .. 256,
    V 1 .. 1024; fp32 sums and gates, the 16-bit state rounded once a step"""
    return _GRUFn.apply(x, weight, hidden, batch_first)


class GRULayer(torch.nn.Module):
    """R/HugeCTR/include/layers/gru_layer.hpp.  weight: the reference's flat layout, uniform in
    +-1 / sqrt(hidden)"""

    def __init__(self, hidden: int, vector_size: int, batch_first: bool = False):
        super().__init__()
        if not (isinstance(hidden, int) and hidden >= 1):
            raise ValueError(f"GRULayer: hidden >= 1, got {hidden!r}")
        if not (isinstance(vector_size, int) and vector_size >= 1):
            raise ValueError(f"GRULayer: vector_size >= 1, got {vector_size!r}")
        self.hidden, self.vector_size, self.batch_first = hidden, vector_size, batch_first
        bound = hidden ** -0.5
        self.weight = torch.nn.Parameter(
            torch.empty(3 * hidden * (vector_size + hidden + 1)).uniform_(-bound, bound))

    def forward(self, x):
        if x.dim() == 3 and x.shape[2] != self.vector_size:
            raise ValueError(f"GRULayer: x's last dimension is vector_size = {self.vector_size}, got "
                             f"{tuple(x.shape)}")
        return gru(x, self.weight, self.hidden, self.batch_first)


class _CrossV1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, kernels, biases):
        x0 = x0.contiguous().float()
        kernels, biases = kernels.contiguous(), biases.contiguous()
        B, w = x0.shape
        L = kernels.shape[0]
        outputs = torch.empty((L, B, w), dtype=torch.float32, device=x0.device)
        hiddens = torch.empty((L, B), dtype=torch.float32, device=x0.device)
        check(lib.hctr_cross_v1_fwd(B, w, L, ptr(x0), ptr(kernels), ptr(biases), ptr(outputs),
                                    ptr(hiddens), stream_ptr()))
        ctx.save_for_backward(x0, kernels, outputs, hiddens)
        return outputs[L - 1]

    @staticmethod
    def backward(ctx, grad):
        x0, kernels, outputs, hiddens = ctx.saved_tensors
        grad = grad.contiguous()
        B, w = x0.shape
        L = kernels.shape[0]
        in_grad = torch.empty_like(x0)
        kg = torch.empty_like(kernels)
        bg = torch.empty_like(kernels)
        ws = torch.empty(lib.hctr_cross_v1_bwd_workspace_bytes(B, w, L) // 4, dtype=torch.float32,
                         device=x0.device)
        check(lib.hctr_cross_v1_bwd(B, w, L, ptr(x0), ptr(kernels), ptr(outputs), ptr(hiddens),
                                    ptr(grad), ptr(in_grad), ptr(kg), ptr(bg), ptr(ws),
                                    stream_ptr()))
        return in_grad, kg, bg


def _mm_f32(a, b):
    """a @ b of 16-bit operands with an fp32 result (weight gradients: a sum over the whole batch
    does not fit fp16's range at loss scale 1024)"""
    if a.dtype in (torch.float16, torch.bfloat16):
        try:
            return torch.mm(a, b, out_dtype=torch.float32)
        except (TypeError, NotImplementedError, RuntimeError):  # (no out_dtype on this backend)
            return torch.mm(a.float(), b.float())
    return torch.mm(a, b)


def _own_gemm_ok(x, n, k):
    """the shapes hctr_gemm_nt16 takes (cross_gemm.hip): 16-bit operands on the device, N a
    multiple of 128, K of 64; HCTR_CROSS_GEMM=0 keeps the library GEMMs (measurements)"""
    return (x.is_cuda and x.dtype in _DT16 and n % 128 == 0 and k % 64 == 0 and
            os.environ.get("HCTR_CROSS_GEMM", "1") != "0")


def gemm_nt16(a, bt, epilogue=0, bias=None, x0=None, xl=None):
    """a [M, K] @ bt [N, K]^T on the library's own matrix-core kernel (hctr_gemm_nt16); epilogue 1
    returns (x0 * (a @ bt^T + bias) + xl, a @ bt^T + bias), epilogue 2 returns a @ bt^T + xl"""
    M, K = a.shape
    N = bt.shape[0]
    # rows may be strided (a leading dimension), elements of a row may not; the epilogue operands
    # are read as [M, N] with leading dimension N
    if a.stride(1) != 1:
        a = a.contiguous()
    if bt.stride(1) != 1:
        bt = bt.contiguous()
    assert bt.shape[1] == K and a.dtype == bt.dtype
    bias, x0, xl = (t if t is None or t.is_contiguous() else t.contiguous() for t in (bias, x0, xl))
    assert x0 is None or x0.shape == (M, N)
    assert xl is None or xl.shape == (M, N)
    c = torch.empty((M, N), dtype=a.dtype, device=a.device)
    h = torch.empty_like(c) if epilogue == 1 else None
    check(lib.hctr_gemm_nt16(M, N, K, ptr(a), a.stride(0), ptr(bt), bt.stride(0), ptr(c), N, epilogue,
                             ptr(bias) if bias is not None else None,
                             ptr(x0) if x0 is not None else None,
                             ptr(xl) if xl is not None else None,
                             ptr(h) if h is not None else None, _DT16[a.dtype], stream_ptr()))
    return (c, h) if epilogue == 1 else c


class _CrossV2Fn(torch.autograd.Function):
    """DCN-v2 cross layers, x_{l+1} = x0 * (x_l U_l V_l + b_l) + x_l, in the activations' own type
    T (fp16 / bf16 under use_mixed_precision: the GEMMs run on the matrix cores; fp32 otherwise)
    with fp32 master weights -- MultiCrossForwardFunctorv2 / MultiCrossBackwardFunctorv2
    (R/HugeCTR/src/layers/multi_cross_layer.cu:582-700,732-812): per layer two GEMMs forward (the
    bias rides in the second one's epilogue) and four backward (S1 = S0 V^T, dV = (XU)^T S0,
    dU = X^T S1, dY_{l-1} = S1 U^T + dY_l with the residual in the GEMM's epilogue); S0 = dY .* x0
    and the x0 gradient dY .* H accumulate in T as the reference's fused_mul_fma3 does.  Weight
    and bias gradients leave as fp32."""

    @staticmethod
    def forward(ctx, x0, U, V, b):
        T = x0.dtype
        L = U.shape[0]
        xs, ps, hs = [x0], [], []
        xl = x0
        w, p = U.shape[1], U.shape[2]
        # (hctr_convert_transpose16 reads U / V as fp32: 16-bit parameters -- module.half() -- take
        #  the library GEMMs; the epilogue operands are read with leading dimension N)
        own = (_own_gemm_ok(x0, p, w) and _own_gemm_ok(x0, w, p) and
               U.dtype == torch.float32 and V.dtype == torch.float32 and x0.is_contiguous())
        bt = b.to(T)
        if own:
            # the 16-bit copies of the master weights as they lie (backward) and transposed (the
            # forward's operands are read K-contiguous), one pass per tensor
            Ut, UtT = torch.empty_like(U, dtype=T), torch.empty((L, p, w), dtype=T, device=U.device)
            Vt, VtT = torch.empty_like(V, dtype=T), torch.empty((L, w, p), dtype=T, device=V.device)
            Uc, Vc = U.contiguous(), V.contiguous()
            check(lib.hctr_convert_transpose16(L, w, p, ptr(Uc), ptr(Ut), ptr(UtT), _DT16[T],
                                               stream_ptr()))
            check(lib.hctr_convert_transpose16(L, p, w, ptr(Vc), ptr(Vt), ptr(VtT), _DT16[T],
                                               stream_ptr()))
        else:
            Ut, Vt = U.to(T), V.to(T)
        for l in range(L):
            if own:
                # two launches per layer: P = X_l U; then bias + X_0 .* H + X_l in the second
                # GEMM's epilogue (the reference's fused epilogues, multi_cross_layer.cu:640-700)
                pl = gemm_nt16(xl, UtT[l])
                xl, h = gemm_nt16(pl, VtT[l], 1, bt[l], x0, xl)
            else:
                pl = xl @ Ut[l]
                h = torch.addmm(bt[l], pl, Vt[l])
                xl = torch.addcmul(xl, x0, h)
            ps.append(pl)
            hs.append(h)
            xs.append(xl)
        ctx.save_for_backward(Ut, Vt, *xs[:-1], *ps, *hs)
        ctx.L = L
        return xl

    @staticmethod
    def backward(ctx, grad):
        L = ctx.L
        sv = ctx.saved_tensors
        Ut, Vt = sv[0], sv[1]
        xs, ps, hs = sv[2:2 + L], sv[2 + L:2 + 2 * L], sv[2 + 2 * L:2 + 3 * L]
        x0 = xs[0]
        dy = grad.contiguous()
        acc = torch.empty_like(x0)
        wdt = torch.float32 if x0.dtype in (torch.float16, torch.bfloat16) else x0.dtype
        dU = torch.empty(Ut.shape, dtype=wdt, device=x0.device)
        dV = torch.empty(Vt.shape, dtype=wdt, device=x0.device)
        db = torch.empty((L, x0.shape[1]), dtype=wdt, device=x0.device)
        B, w = x0.shape
        fused = x0.is_cuda and x0.dtype in _DT16 and w % 8 == 0
        if fused:
            # S0 = dY .* X0, dX += dY .* H and db = colsum(S0) in one pass over dY (HIP), as the
            # reference's fused_mul_fma3 + the dV GEMM's bias-gradient epilogue
            s0 = torch.empty_like(x0)
            ws = torch.empty(lib.hctr_cross_v2_bwd_step_workspace_bytes(B, w) // 4,
                             dtype=torch.float32, device=x0.device)
        else:
            acc.zero_()
        for l in range(L - 1, -1, -1):
            if fused:
                check(lib.hctr_cross_v2_bwd_step(B, w, ptr(dy), ptr(x0), ptr(hs[l]), ptr(acc), ptr(s0),
                                                 ptr(db[l]), ptr(ws), 1 if l == L - 1 else 0,
                                                 _DT16[x0.dtype], stream_ptr()))
            else:
                s0 = dy * x0
                acc.addcmul_(dy, hs[l])
            own1 = _own_gemm_ok(s0, Vt.shape[1], Vt.shape[2])
            s1 = gemm_nt16(s0, Vt[l]) if own1 else s0 @ Vt[l].t()
            # weight gradients reduce over K = batch into a small tile set (512 x 3456: 27 tiles of
            # 256 x 256 on 256 CUs): split-K through batched GEMMs, as the MLP's are (dense.py)
            if x0.is_cuda and x0.dtype in (torch.float16, torch.bfloat16):
                split_k_wgrad(ps[l], s0, out=dV[l])
                split_k_wgrad(xs[l], s1, out=dU[l])
            else:
                dV[l] = _mm_f32(ps[l].t(), s0)
                dU[l] = _mm_f32(xs[l].t(), s1)
            if not fused:
                db[l] = s0.sum(0, dtype=wdt)
            if _own_gemm_ok(s1, Ut.shape[1], Ut.shape[2]):
                dy = gemm_nt16(s1, Ut[l], 2, xl=dy)  # (the residual in the GEMM's epilogue)
            else:
                dy = torch.addmm(dy, s1, Ut[l].t())
        return acc + dy, dU, dV, db


class MultiCrossLayer(torch.nn.Module):
    """DCN cross layers.  projection_dim == 0: v1 (x_{l+1} = x0 * (x_l . w_l) + b_l + x_l), all
    layers fused in one HIP launch.  projection_dim > 0: v2 (x_{l+1} = x0 * (x_l U_l V_l + b_l)
    + x_l): the GEMMs go to hipBLASLt through torch in the activations' type (16-bit inputs: on the
    matrix cores), bias and residual ride in GEMM epilogues (_CrossV2Fn)."""

    def __init__(self, width: int, num_layers: int, projection_dim: int = 0):
        super().__init__()
        self.width, self.num_layers, self.projection_dim = width, num_layers, projection_dim
        if projection_dim == 0:
            # XavierUniform-like default init (weights [1,w] per layer, bias zeros)
            bound = (6.0 / (width + 1)) ** 0.5
            self.kernels = torch.nn.Parameter(torch.empty(num_layers, width).uniform_(-bound, bound))
            self.biases = torch.nn.Parameter(torch.zeros(num_layers, width))
        else:
            bu = (6.0 / (width + projection_dim)) ** 0.5
            self.U = torch.nn.Parameter(torch.empty(num_layers, width, projection_dim).uniform_(-bu, bu))
            self.V = torch.nn.Parameter(torch.empty(num_layers, projection_dim, width).uniform_(-bu, bu))
            self.biases = torch.nn.Parameter(torch.zeros(num_layers, width))

    def forward(self, x0):
        if self.projection_dim == 0:
            return _CrossV1Fn.apply(x0, self.kernels, self.biases)
        return _CrossV2Fn.apply(x0.contiguous(), self.U, self.V, self.biases)
