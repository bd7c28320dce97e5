"""SparseOperationKit-shaped lookup surface on PyTorch.

Mirrors `sparse_operation_kit` (R/sparse_operation_kit/sparse_operation_kit/): `init`,
`Variable` (Distributed / Localized, distributed_variable.py:26-331), `DynamicVariable`
(dynamic_variable.py:34-300), `lookup_sparse` (lookup.py:425-700), the dense lookups
`all2all_dense_embedding` / `group_lookup` (lookup.py:83-139), `OptimizerWrapper`
(optimizer.py:25-250), `export` / `assign` (dynamic_variable.py:465-520).  TensorFlow's
RaggedTensor / IndexedSlices have no PyTorch equivalent, so ids are `Ragged(values, row_lengths)`
(2-D sparse COO tensors are accepted too) and the sparse gradient of a variable is kept on the
variable between `backward()` and `OptimizerWrapper.step()`.

Compute is the C ABI's: hash / index (`hctr_det_lookup_index`), gather + pooling
(`hctr_forward_pool*`), owner partition and row copies of the dense lookups (`hctr_dist_select`,
`hctr_indexed_row_copy`), per-key gradients (`hctr_expand_key_grads`), sparse update
(`hctr_updater_update` for static variables, `hctr_det_update` for dynamic ones).  Torch is used
for buffers, for the key-ownership masks of the multi-GPU route and for `torch.distributed`.

Multi-GPU (one process per GPU): the reference's schedule -- all-gather keys, every GPU pools the
rows it owns for the global batch, partial sums return to the sample's GPU (reduce-scatter), mean
is divided on the receiver.  The dense lookup sends each key to its owner and each row back to its
asker instead (two all-to-alls, lookup.py:122-139).  Distributed variables own row r on GPU r % N
at local row r // N (distributed_variable.py:231-233); dynamic variables own key k on GPU k % N; a
localized variable lives on its target GPU.
"""
from __future__ import annotations

import ctypes
import datetime as _dt
import os
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .dynamic_table import DynamicEmbeddingTable, DynamicTableOptimizer, _num_state
from .hybrid_table import (HybridTable, check_hbm_budget, check_load_factor, first_call_since,
                           hbm_slots_for)

_RANK, _WORLD = 0, 1
INVALID = -1  # 0xFFFFFFFFFFFFFFFF as int64: "row not on this GPU / unknown key"


def init(group=None):
    """sok.init(): picks rank / size up from torch.distributed (horovod in the reference)"""
    global _RANK, _WORLD
    if dist.is_available() and dist.is_initialized():
        _RANK, _WORLD = dist.get_rank(group), dist.get_world_size(group)
    else:
        _RANK, _WORLD = 0, 1


def rank() -> int:
    return _RANK


def num_gpus() -> int:
    return _WORLD


class Ragged:
    """values[nnz] (int64 keys or float weights) + row_lengths[batch] -- tf.RaggedTensor's two
    components as lookup.py:446-460 reads them"""

    def __init__(self, values: torch.Tensor, row_lengths: torch.Tensor):
        self.values = values.contiguous()
        self.row_lengths = row_lengths.to(torch.int64).contiguous()
        assert int(self.row_lengths.sum()) == self.values.numel()

    @staticmethod
    def from_sparse(sp: torch.Tensor) -> "Ragged":
        sp = sp.coalesce()
        rows = sp.indices()[0]
        lens = torch.bincount(rows, minlength=sp.shape[0])
        return Ragged(sp.values(), lens)

    @property
    def batch(self) -> int:
        return self.row_lengths.numel()


def _as_ragged(x) -> Ragged:
    if isinstance(x, Ragged):
        return x
    if isinstance(x, torch.Tensor) and x.is_sparse:
        return Ragged.from_sparse(x)
    if isinstance(x, (tuple, list)) and len(x) == 2:
        return Ragged(x[0], x[1])
    raise TypeError("sp_ids / sp_weights must be sok.Ragged, a 2-D sparse COO tensor or "
                    "(values, row_lengths)")


def _offsets(lens: torch.Tensor) -> torch.Tensor:
    ro = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=lens.device)
    torch.cumsum(lens, 0, out=ro[1:])
    return ro


# ---- variables ----------------------------------------------------------------------------------
class _VariableBase:
    """what lookup_sparse needs of a variable: dimension, target_gpu, key -> local row"""
    dimension: int
    target_gpu: int  # -1: distributed over all GPUs

    _count = 0

    def __init__(self, name: Optional[str] = None):
        _VariableBase._count += 1
        self.name = name or f"sok_variable_{_VariableBase._count}"
        # autograd handle: lookups take it as an input so that backward reaches the variable
        self._token = torch.zeros(1, device="cuda", requires_grad=True)
        self._pending: List[tuple] = []  # (row_offset, rows/keys, bucket grads | None, key grads | None)

    def _owned(self, keys: torch.Tensor) -> torch.Tensor:
        if self.target_gpu >= 0:
            full = self.target_gpu == _RANK
            return torch.full_like(keys, full, dtype=torch.bool)
        if _WORLD == 1:
            return torch.ones_like(keys, dtype=torch.bool)
        return (keys % _WORLD) == _RANK


class DistributedVariable(_VariableBase):
    """rows sharded round-robin: global row r -> GPU r % N, local row r // N"""

    def __init__(self, initial_value: torch.Tensor, target_gpu: int = -1,
                 name: Optional[str] = None):
        super().__init__(name)
        v = torch.as_tensor(initial_value, dtype=torch.float32)
        assert v.dim() == 2
        self.global_shape = tuple(v.shape)
        self.dimension = v.shape[1]
        self.target_gpu = target_gpu
        if target_gpu >= 0:
            local = v if target_gpu == _RANK else v[:0]
        elif _WORLD > 1:
            local = v[_RANK::_WORLD]
        else:
            local = v
        self.weight = local.contiguous().cuda()
        self._updater = None
        self._states: List[torch.Tensor] = []

    def key_map(self, keys: torch.Tensor) -> torch.Tensor:
        if self.target_gpu >= 0 or _WORLD == 1:
            return keys
        return torch.div(keys, _WORLD, rounding_mode="floor")

    def _rows(self, keys: torch.Tensor, train: bool) -> torch.Tensor:
        return self.key_map(keys)

    def _table(self):
        return self.weight

    def numpy(self):
        return self.weight.detach().cpu().numpy()


class LocalizedVariable(DistributedVariable):
    pass


def Variable(initial_value, mode: Optional[str] = None, name: Optional[str] = None, **_kw):
    """sok.Variable: mode None / "distributed" -> DistributedVariable, "localized:<gpu>" ->
    LocalizedVariable on that GPU (distributed_variable.py:26-125)"""
    if mode is None or mode == "distributed":
        return DistributedVariable(initial_value, name=name)
    if mode.startswith("localized"):
        gpu = int(mode.split(":")[1]) if ":" in mode else 0
        return LocalizedVariable(initial_value, target_gpu=gpu, name=name)
    raise ValueError(f"unknown mode {mode!r}")


class DynamicVariable(_VariableBase):
    """key -> vector map; keys live on GPU key % N.

    var_type None / "hbm" (the default here; the reference defaults to "hybrid"): the dynamic
    table, which grows on demand and keeps every key it has seen.
    var_type="hybrid": a table of fixed capacity that evicts its least recently used entries
    (hybrid_table.py, hctr_lru_*).  Keyword options: max_capacity (required; rounded up to whole
    buckets), max_bucket_size=128, evict_strategy="kLru" (the only strategy), filter_ratio=1.0 (the
    admission probability of lookup_sparse(..., use_low_frequency_filter=True)).  init_capacity
    (default: max_capacity) is where the table starts: an inserting call doubles it, up to
    max_capacity, while the occupied slots plus the call's new keys exceed max_load_factor (0.5, in
    (0, 1]) times the slots, and only a table at max_capacity evicts; max_capacity must be
    init_capacity times a power of two, in whole buckets.  max_hbm_for_vectors=G
    (GiB, int or float, >= 0): the rows of H = min(C, floor(G * 2^30 / (dimension * 4) / S) * S)
    slots, and their optimizer states, stay in HBM and the others live in pinned host memory
    (DESIGN.md "Hybrid table"); without it everything is in HBM (the reference defaults to 16).
    The reference's other options are kept in config_dict.  Evicted pairs go
    back to the caller (sparse_read_and_evict), not to host memory."""

    def __init__(self, dimension: int, initializer: Union[str, float, None] = None,
                 key_type=torch.int64, init_capacity: Optional[int] = None,
                 mode: Optional[str] = None,
                 seed: int = 0, name: Optional[str] = None, *, var_type: Optional[str] = None,
                 **kwargs):
        if var_type not in (None, "hbm", "hybrid"):
            raise ValueError(f'var_type must be "hbm" or "hybrid", not {var_type!r}')
        if var_type != "hybrid" and kwargs:
            raise TypeError(f"unexpected keyword arguments {sorted(kwargs)} (they belong to "
                            'var_type="hybrid")')
        ratio = kwargs.get("filter_ratio", 1.0)
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or \
                not 0.0 <= float(ratio) <= 1.0:
            raise ValueError(f"filter_ratio must be a float in [0, 1], not {ratio!r}")
        self.filter_ratio = float(ratio)
        if var_type == "hybrid" and "max_hbm_for_vectors" in kwargs:
            check_hbm_budget(kwargs["max_hbm_for_vectors"])
        load = check_load_factor(kwargs.get("max_load_factor", 0.5))
        cap = kwargs.get("max_capacity")
        if var_type == "hybrid" and cap is not None and init_capacity is not None and \
                int(init_capacity) > int(cap):
            raise ValueError(f"init_capacity {init_capacity} is above max_capacity {cap}")
        super().__init__(name)
        self.dimension = int(dimension)
        self.key_type = key_type
        self.target_gpu = -1
        if mode is not None and mode.startswith("localized"):
            self.target_gpu = int(mode.split(":")[1]) if ":" in mode else 0
        self.initializer_str = "" if initializer is None else str(initializer)
        self._var_type = var_type or "hbm"
        self.config_dict = dict(kwargs, var_type=self._var_type,
                                init_capacity=1 << 20 if init_capacity is None else init_capacity)
        self._det: Optional[DynamicEmbeddingTable] = None
        self._lru: Optional[HybridTable] = None
        if self._var_type == "hybrid":
            if kwargs.get("max_capacity") is None:
                raise ValueError('var_type="hybrid" needs max_capacity')
            strategy = kwargs.get("evict_strategy", "kLru")
            if strategy != "kLru":
                raise ValueError(f"evict_strategy {strategy!r} is not supported: only \"kLru\"")
            # the initial value is a function of (seed, key, element): the same on every rank
            bucket = int(kwargs.get("max_bucket_size", 128))
            hbm = None
            if kwargs.get("max_hbm_for_vectors") is not None:
                # every rank tiers its own shard of max_capacity slots with the same budget
                hbm = hbm_slots_for(kwargs["max_hbm_for_vectors"], self.dimension,
                                    int(kwargs["max_capacity"]), bucket)
            self._lru = HybridTable(int(cap), self.dimension, self.initializer_str, bucket, key_type,
                                    seed=seed, hbm_slots=hbm, init_capacity=init_capacity,
                                    max_load_factor=float(load))
        else:
            self._det = DynamicEmbeddingTable([self.dimension], self.initializer_str,
                                              1 << 20 if init_capacity is None else init_capacity,
                                              key_type, seed=seed + 1000003 * _RANK)
        self._opt: Optional[DynamicTableOptimizer] = None
        # (hctr_updater handle, capacity[, row bound: hybrid]) of the gradient reduce
        self._updater = None

    @property
    def backend_type(self) -> str:
        return self._var_type

    @property
    def size(self) -> int:
        return self._lru.size() if self._lru is not None else self._det.size()

    def _rows(self, keys: torch.Tensor, train: bool, admit: Optional[float] = None) -> torch.Tensor:
        if self._lru is not None:
            return self._lru.lookup_index(keys, insert=train, admit=admit if train else None)
        idx = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
        check(lib.hctr_det_lookup_index(self._det._h, 0, ptr(keys), keys.numel(), 1 if train else 0,
                                        ptr(idx), stream_ptr()))
        return idx

    @property
    def tiered(self) -> bool:
        """a hybrid variable whose slots are partly in host memory"""
        return self._lru is not None and self._lru.tiered

    def _table(self) -> torch.Tensor:
        if self._lru is not None:
            # the slots in HBM and the per-call rows the last lookup handed out
            p, _ = self._lru.rows_ptr()
            return _view_f32(p, (self._lru.placement()[1], self.dimension))
        p, cap = ctypes.c_void_p(), ctypes.c_size_t()
        check(lib.hctr_det_rows(self._det._h, 0, ctypes.byref(p), ctypes.byref(cap)))
        return _view_f32(p.value, (cap.value, self.dimension))

    def _hybrid_scatter(self, indices, values, add: bool):
        """stored keys only, as the dynamic table's scatter does"""
        idx = self._lru.find(indices.reshape(-1))
        live = idx >= 0
        # slot-addressed (the table knows where a slot's bytes live): distinct slots, the values
        # summed per slot for an add as index_add_ does
        v = values.reshape(-1, self.dimension).float()[live]
        slots, inv = torch.unique(idx[live], return_inverse=True)
        if add:
            u = torch.zeros((slots.numel(), self.dimension), dtype=torch.float32,
                            device=v.device).index_add_(0, inv, v)
        else:
            u = torch.empty((slots.numel(), self.dimension), dtype=torch.float32,
                            device=v.device)
            u[inv] = v
        self._lru.scatter_slots(0, slots, u, add=add)

    # dynamic_variable.py:294-340
    def sparse_read(self, indices: torch.Tensor) -> torch.Tensor:
        if self._lru is not None:
            rows = self._lru.lookup_index(indices.reshape(-1).contiguous(), insert=False)
            return _gather(self._table(), rows, self.dimension)  # (the store may have moved)
        return self._det.lookup(indices.contiguous()).view(-1, self.dimension)

    def scatter_add(self, indices, values):
        if self._lru is not None:
            return self._hybrid_scatter(indices, values, True)
        self._det.scatter_add(indices.contiguous(), values)

    def scatter_sub(self, indices, values):
        if self._lru is not None:
            return self._hybrid_scatter(indices, -values, True)
        self._det.scatter_add(indices.contiguous(), -values)

    def scatter_update(self, indices, values):
        if self._lru is not None:
            return self._hybrid_scatter(indices, values, False)
        self._det.scatter_update(indices.contiguous(), values)


def _view_f32(addr: int, shape) -> torch.Tensor:
    """torch view of library-owned device memory (no copy)"""
    n = 1
    for s in shape:
        n *= s

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (addr, False),
                                  "version": 2}
    return torch.as_tensor(h, device="cuda").view(*shape)


def _gather(table: torch.Tensor, rows: torch.Tensor, D: int) -> torch.Tensor:
    """out[i] = table[rows[i]]: the path's pooling with one key per bucket"""
    ro = torch.arange(rows.numel() + 1, dtype=torch.int64, device=rows.device)
    return _pool(table, ro, rows, None, 0, D)


def export(var: DynamicVariable):
    """(indices, values) of a DynamicVariable (dynamic_variable.py:465-492); a hybrid variable
    lists its occupied slots in slot order"""
    if var._lru is not None:
        return var._lru.export()
    return var._det.export(0)


def assign(var: DynamicVariable, indices: torch.Tensor, values: torch.Tensor):
    """insert-or-overwrite (dynamic_variable.py:494-520).  On a hybrid variable the insert may
    evict other keys, and a key the table rejects is not stored."""
    if var._lru is not None:
        keys = indices.reshape(-1).contiguous()
        var._lru.lookup_index(keys, insert=True)
        # the rows handed out may be per-call copies: write the stored keys' slots
        slots = var._lru.find(keys)
        live = slots >= 0
        var._lru.scatter_slots(0, slots[live], values.reshape(-1, var.dimension).float()[live])
        return
    var._det.lookup(indices.contiguous())       # inserts what is missing
    var._det.scatter_update(indices.contiguous(), values)


class _ReadEvictFn(torch.autograd.Function):
    """values of sparse_read_and_evict; backward leaves the keys' gradients for OptimizerWrapper"""

    @staticmethod
    def forward(ctx, token, var, keys, rows):
        ctx.var, ctx.keys, ctx.rows = var, keys, rows
        return _gather(var._table(), rows, var.dimension)

    @staticmethod
    def backward(ctx, g):
        n = ctx.keys.numel()
        ro = torch.arange(n + 1, dtype=torch.int64, device=g.device)
        ctx.var._pending.append((ro, ctx.rows, ctx.keys, None, g.contiguous().float(), 0))
        return torch.zeros(1, device=g.device), None, None, None


def sparse_read_and_evict(var: DynamicVariable, indices: torch.Tensor):
    """(values [n, dimension], evict_keys, evict_values) -- lookup.py:75-80.  An inserting lookup
    on this GPU's table (as the reference's op); the pairs it evicted come back to the caller, in
    bucket order.  values carries autograd: OptimizerWrapper.step updates those keys.  Hybrid
    variables only."""
    if not isinstance(var, DynamicVariable) or var.backend_type != "hybrid":
        raise TypeError("sparse_read_and_evict only supports DynamicVariable with "
                        'var_type="hybrid"')
    keys = indices.reshape(-1).to(var.key_type).contiguous()
    rows, ek, ev = var._lru.lookup_index(keys, insert=True, evict=True)
    values = _ReadEvictFn.apply(var._token, var, keys, rows)
    return values, ek, ev


# ---- collectives (NCCL = RCCL on the GPU boxes; gloo stages through the host, used by tests) ------
def _backend_is_gloo() -> bool:
    return dist.get_backend() == "gloo"


def _all_gather_cat(t: torch.Tensor) -> torch.Tensor:
    """concatenate every rank's 1-D tensor (sizes may differ)"""
    n = torch.tensor([t.numel()], dtype=torch.int64, device=t.device)
    sizes = [torch.zeros_like(n) for _ in range(_WORLD)]
    if _backend_is_gloo():
        sizes = [s.cpu() for s in sizes]
        dist.all_gather(sizes, n.cpu())
    else:
        dist.all_gather(sizes, n)
    sizes = [int(s) for s in sizes]
    m = max(sizes)
    pad = torch.zeros(m, dtype=t.dtype, device=t.device)
    pad[:t.numel()] = t
    if _backend_is_gloo():
        outs = [torch.zeros(m, dtype=t.dtype) for _ in range(_WORLD)]
        dist.all_gather(outs, pad.cpu())
        outs = [o.to(t.device) for o in outs]
    else:
        outs = [torch.zeros_like(pad) for _ in range(_WORLD)]
        dist.all_gather(outs, pad)
    return torch.cat([o[:s] for o, s in zip(outs, sizes)])


def _reduce_scatter_rows(x: torch.Tensor, local_rows: int) -> torch.Tensor:
    """x [N * local_rows, D] partial sums -> my [local_rows, D] slice of the total"""
    if _backend_is_gloo():
        c = x.cpu()
        dist.all_reduce(c)
        return c[_RANK * local_rows:(_RANK + 1) * local_rows].to(x.device)
    out = torch.empty((local_rows, x.shape[1]), dtype=x.dtype, device=x.device)
    dist.reduce_scatter_tensor(out, x.contiguous())
    return out


def _all_gather_rows(x: torch.Tensor) -> torch.Tensor:
    if _backend_is_gloo():
        outs = [torch.zeros(x.shape, dtype=x.dtype) for _ in range(_WORLD)]
        dist.all_gather(outs, x.cpu())
        return torch.cat(outs).to(x.device)
    out = torch.empty((x.shape[0] * _WORLD, x.shape[1]), dtype=x.dtype, device=x.device)
    dist.all_gather_into_tensor(out, x.contiguous())
    return out


# ---- lookup -------------------------------------------------------------------------------------
def _pool(table: torch.Tensor, ro: torch.Tensor, rows: torch.Tensor, weights, combiner: int, D):
    buckets = ro.numel() - 1
    if rows.numel() == 0:  # nothing of this batch lives here: all pooled vectors are zero
        return torch.zeros((buckets, D), dtype=torch.float32, device=ro.device)
    out = torch.empty((buckets, D), dtype=torch.float32, device=ro.device)
    if weights is None:
        multi = rows.numel() > buckets + buckets // 2
        fn = lib.hctr_forward_pool_multihot if multi else lib.hctr_forward_pool
        check(fn(buckets, D, combiner, ptr(ro), _lib.KEY_I64, ptr(rows), ptr(table), ptr(out),
                 _lib.F32, stream_ptr()))
    else:
        check(lib.hctr_forward_pool_weighted(buckets, D, combiner, ptr(ro), ptr(rows), ptr(weights),
                                             ptr(table), ptr(out), stream_ptr()))
    return out


class _LookupFn(torch.autograd.Function):
    """one (variable, ids[, weights]) lookup; the token input routes backward to the variable"""

    @staticmethod
    def forward(ctx, token, var, ids: Ragged, w: Optional[Ragged], combiner: int, train: bool,
                filt: bool = False):
        D = var.dimension
        filt = filt and train
        lens, keys = ids.row_lengths, ids.values
        weights = w.values.float().contiguous() if w is not None else None
        b_local = lens.numel()
        if _WORLD > 1:
            # all-gather keys / lengths / weights: the global batch in rank order (lookup.py:484-496)
            keys = _all_gather_cat(keys)
            lens = _all_gather_cat(lens)
            if weights is not None:
                weights = _all_gather_cat(weights)
            own = var._owned(keys)
            # this GPU pools only the rows it owns: filtered CSR over the global batch
            seg = torch.repeat_interleave(torch.arange(lens.numel(), device=lens.device), lens)
            lens_own = torch.bincount(seg[own], minlength=lens.numel())
            keys_own = keys[own].contiguous()
            w_own = weights[own].contiguous() if weights is not None else None
        else:
            lens_own, keys_own, w_own = lens, keys, weights
        ro = _offsets(lens_own)
        if filt:
            # keys the low-frequency filter refused leave their samples before pooling
            rows = var._rows(keys_own, True, admit=var.filter_ratio)
            ro, rows, keys_own, w_own = var._lru.compact(ro, rows, keys_own, w_own)
        else:
            rows = var._rows(keys_own, train)
        table = var._table()
        # the receiver divides for mean (after all shards are added), so shards always sum
        part = _pool(table, ro, rows, w_own, combiner if _WORLD == 1 else 0, D)
        den = None
        if _WORLD > 1 and filt and combiner == 1:
            # mean over the admitted keys: their count (weight sum) per sample, added over owners
            # beside the pooled partials
            nb = ro.numel() - 1
            if w_own is not None:
                seg = torch.repeat_interleave(torch.arange(nb, device=ro.device), ro.diff())
                den_own = torch.zeros(nb, device=ro.device).index_add_(0, seg, w_own)
            else:
                den_own = ro.diff().float()
            both = _reduce_scatter_rows(torch.cat([part, den_own.unsqueeze(1)], 1), b_local)
            out, den = both[:, :D], both[:, D].contiguous()
            out = out / den.clamp_min(1e-30).unsqueeze(1) * (den > 0).unsqueeze(1)
        elif _WORLD > 1:
            out = _reduce_scatter_rows(part, b_local)
            if combiner == 1:
                if w is not None:
                    seg_l = torch.repeat_interleave(
                        torch.arange(b_local, device=out.device), ids.row_lengths)
                    den = torch.zeros(b_local, device=out.device).index_add_(
                        0, seg_l, w.values.float())
                else:
                    den = ids.row_lengths.float()
                out = out / den.clamp_min(1e-30).unsqueeze(1) * (den > 0).unsqueeze(1)
        else:
            out = part
        ctx.var, ctx.combiner, ctx.train = var, combiner, train
        ctx.ro, ctx.rows, ctx.keys, ctx.w = ro, rows, keys_own, w_own
        ctx.local = (ids.row_lengths, w.values.float() if w is not None else None, b_local)
        ctx.den = den
        return out

    @staticmethod
    def backward(ctx, g):
        var, combiner = ctx.var, ctx.combiner
        g = g.contiguous().float()
        if _WORLD > 1:
            lens_l, w_l, b_local = ctx.local
            if combiner == 1:  # mean was divided on the receiver: its gradient scales here
                if ctx.den is not None:
                    den = ctx.den
                elif w_l is not None:
                    seg_l = torch.repeat_interleave(torch.arange(b_local, device=g.device), lens_l)
                    den = torch.zeros(b_local, device=g.device).index_add_(0, seg_l, w_l)
                else:
                    den = lens_l.float()
                g = g / den.clamp_min(1e-30).unsqueeze(1) * (den > 0).unsqueeze(1)
            g = _all_gather_rows(g)  # every owner sees the whole global batch's gradients
            comb_local = 0
        else:
            comb_local = combiner
        var._pending.append((ctx.ro, ctx.rows, ctx.keys, ctx.w, g, comb_local))
        return torch.zeros(1, device=g.device), None, None, None, None, None, None


def lookup_sparse(params, sp_ids, sp_weights=None, combiners=None, training: bool = True,
                  use_low_frequency_filter: bool = False):
    """sok.lookup_sparse(params, sp_ids, sp_weights=None, combiners=None): fused lookup of several
    variables; returns one [batch, dimension] tensor per variable (a list iff sp_ids is one).
    use_low_frequency_filter=True (hybrid DynamicVariables only; lookup.py:543,566): in a training
    lookup a key the table does not hold enters it with probability filter_ratio (a function of
    (seed, key, call), DESIGN.md "Hybrid table"); a key that does not is left out of its sample's
    pooling and gets no gradient."""
    is_list = isinstance(sp_ids, (list, tuple)) and not (
        len(sp_ids) == 2 and isinstance(sp_ids[0], torch.Tensor) and not sp_ids[0].is_sparse
        and sp_ids[0].dim() == 1 and isinstance(params, _VariableBase))
    params = list(params) if isinstance(params, (list, tuple)) else [params]
    sp_ids = list(sp_ids) if is_list else [sp_ids]
    if combiners is None:
        combiners = ["mean"] * len(params)  # lookup.py:620-623
    combiners = list(combiners) if isinstance(combiners, (list, tuple)) else [combiners]
    if sp_weights is None:
        sp_weights = [None] * len(params)
    elif not isinstance(sp_weights, (list, tuple)) or not is_list:
        sp_weights = [sp_weights]
    if not (len(params) == len(sp_ids) == len(combiners) == len(sp_weights)):
        raise RuntimeError("params, sp_ids, sp_weights and combiners must have the same length")
    for p in params[1:]:
        if type(p) is not type(params[0]) and not (
                isinstance(p, DistributedVariable) and isinstance(params[0], DistributedVariable)):
            raise RuntimeError("Distributed/Localized/Dynamic Variable cannot be used in the same "
                               "lookup currently")  # lookup.py:436-440
    if use_low_frequency_filter:
        for p in params:
            if not isinstance(p, DynamicVariable) or p.backend_type != "hybrid":
                raise TypeError("use_low_frequency_filter only supports DynamicVariable with "
                                'var_type="hybrid"')
    outs = []
    for var, ids, w, c in zip(params, sp_ids, sp_weights, combiners):
        if c not in ("sum", "mean"):
            raise ValueError('combiner must be "sum" or "mean"')
        ids = _as_ragged(ids)
        w = _as_ragged(w) if w is not None else None
        if w is not None and not torch.equal(w.row_lengths, ids.row_lengths):
            raise RuntimeError("sp_id and sp_weight should be have same shape.")
        outs.append(_LookupFn.apply(var._token, var, ids, w, 1 if c == "mean" else 0, training,
                                    bool(use_low_frequency_filter)))
    return outs if is_list else outs[0]


# ---- dense lookups (lookup.py:83-139) -----------------------------------------------------------
def _row_copy(tasks, src_dtype=_lib.F32, dst_dtype=_lib.F32):
    """hctr_indexed_row_copy over (src, src_rows, dim, index, index_div, n, dst, dst_pos) tuples:
    one launch per HCTR_ROW_COPY_MAX_TASKS tasks.  index is int32 (read as U32: keys and rows are
    non-negative) / int64 or None, dst_pos int32 or None."""
    for a in range(0, len(tasks), _lib.ROW_COPY_MAX_TASKS):
        part = tasks[a:a + _lib.ROW_COPY_MAX_TASKS]
        arr = (_lib.RowCopyTask * len(part))()
        for t, (src, src_rows, dim, index, div, n, dst, dst_pos) in zip(arr, part):
            t.src, t.src_rows, t.dim = src.data_ptr(), src_rows, dim
            if index is not None:
                t.index = index.data_ptr()
                t.index_type = _lib.KEY_I64 if index.dtype == torch.int64 else _lib.KEY_U32
            t.index_div, t.n = div, n
            t.dst, t.dst_rows = dst.data_ptr(), dst.numel() // dim
            if dst_pos is not None:
                t.dst_pos = dst_pos.data_ptr()
        check(lib.hctr_indexed_row_copy(arr, len(part), src_dtype, dst_dtype, stream_ptr()))


def _dist_select(keys: torch.Tensor, n_splits: int):
    """(keys grouped by key % n_splits, order, splits) -- hctr_dist_select; stable inside a group"""
    n = keys.numel()
    out = torch.empty_like(keys)
    order = torch.empty(n, dtype=torch.int32, device=keys.device)
    splits = torch.empty(n_splits, dtype=torch.int32, device=keys.device)
    nbytes = _lib.dist_select_ws_bytes(n_splits)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=keys.device)
    kt = _lib.KEY_I64 if keys.dtype == torch.int64 else _lib.KEY_U32
    check(lib.hctr_dist_select(ptr(keys), kt, n, n_splits, ptr(out), ptr(order), ptr(splits),
                               ptr(ws), nbytes, stream_ptr()))
    return out, order, splits


def _check_indices(indices):
    if not isinstance(indices, torch.Tensor) or indices.dtype not in (torch.int32, torch.int64) \
            or not indices.is_cuda:
        raise TypeError("indices must be an int32 or int64 CUDA tensor")


def _static_rows(var: DistributedVariable, keys: torch.Tensor) -> torch.Tensor:
    """local rows (int64) of a static variable for the sparse update; a key without a row here
    carries INVALID, which the update drops as the lookup read it as zero"""
    rows = var.key_map(keys.to(torch.int64))
    ok = (keys >= 0) & (rows < var.weight.shape[0])
    return torch.where(ok, rows, torch.full_like(rows, INVALID))


def _local_rows_into(var, keys: torch.Tensor, train: bool, dst: torch.Tensor, dst_pos=None):
    """dst[dst_pos[i] or i] = the variable's vector of keys[i] (keys this rank owns); returns the
    rows a DynamicVariable handed out (None for a static variable)"""
    n, D = keys.numel(), var.dimension
    if isinstance(var, DynamicVariable):
        rows = var._rows(keys, train)
        if not train and var._lru is not None:
            # a hybrid table gives a read-only miss a per-call row holding the initializer's
            # value; here an evaluation lookup reads an unknown key as zero, whatever the backend
            rows = torch.where(var._lru.find(keys) < 0, torch.full_like(rows, INVALID), rows)
        table = var._table()
        # (rows are per-call rows behind the slots for a tiered variable: no upper bound)
        task = (table, 0, D, rows, 1, n, dst, dst_pos)
    else:
        rows = None
        table = var.weight
        div = _WORLD if var.target_gpu < 0 else 1
        task = (table, table.shape[0], D, keys, div, n, dst, dst_pos)
    if n and table.numel() == 0:
        dst.zero_()  # nothing is stored here: every key reads as zero
    elif n:
        _row_copy([task])
    return rows


class _DenseFn(torch.autograd.Function):
    """all2all_dense_embedding of one variable; the token input routes backward to the variable"""

    @staticmethod
    def forward(ctx, token, var, keys, train: bool):
        n, D = keys.numel(), var.dimension
        out = torch.empty((n, D), dtype=torch.float32, device=keys.device)
        if _WORLD == 1:
            rows = _local_rows_into(var, keys, train, out)
            ctx.route = None
            ctx.var, ctx.keys, ctx.rows = var, keys, rows
            return out
        from .parallel import all_to_all_single
        # keys grouped by owner (dist_select), counts then keys to the owners (lookup.py:125-129)
        sel, order, splits = _dist_select(keys, _WORLD)
        send = splits.cpu().to(torch.int64)
        recv = torch.empty(_WORLD, dtype=torch.int64)
        if _backend_is_gloo():
            dist.all_to_all_single(recv, send)
        else:
            r = torch.empty(_WORLD, dtype=torch.int64, device=keys.device)
            dist.all_to_all_single(r, send.to(keys.device))
            recv = r.cpu()
        send, recv = send.tolist(), recv.tolist()
        m = sum(recv)
        mine = torch.empty(m, dtype=keys.dtype, device=keys.device)
        all_to_all_single(mine, sel, recv, send)
        # the owners' rows (lookup.py:131-134), back to the askers, into input order (:136-138)
        vecs = torch.empty((m, D), dtype=torch.float32, device=keys.device)
        rows = _local_rows_into(var, mine, train, vecs)
        got = torch.empty((n, D), dtype=torch.float32, device=keys.device)
        all_to_all_single(got, vecs, send, recv)
        if n:
            _row_copy([(got, n, D, None, 1, n, out, order)])
        ctx.route = (order, send, recv)
        ctx.var, ctx.keys, ctx.rows = var, mine, rows
        return out

    @staticmethod
    def backward(ctx, g):
        var, keys, rows = ctx.var, ctx.keys, ctx.rows
        g = g.contiguous().float()
        if ctx.route is not None:
            from .parallel import all_to_all_single
            order, send, recv = ctx.route
            n, D = order.numel(), var.dimension
            sel = torch.empty((n, D), dtype=torch.float32, device=g.device)
            if n:  # gradient rows in the order the keys were sent (gatherEx)
                _row_copy([(g, n, D, order, 1, n, sel, None)])
            g = torch.empty((keys.numel(), D), dtype=torch.float32, device=g.device)
            all_to_all_single(g, sel, recv, send)
        if rows is None:
            rows = _static_rows(var, keys)
        ro = torch.arange(keys.numel() + 1, dtype=torch.int64, device=g.device)
        var._pending.append((ro, rows, keys, None, g, 0))
        return torch.zeros(1, device=g.device), None, None, None


def all2all_dense_embedding(param, indices, *, training: bool = True):
    """sok.all2all_dense_embedding(param, indices) (lookup.py:122-139): a dense lookup -- one key
    per position, no pooling -- returning fp32 indices.shape + (dimension,).  param: a distributed
    sok.Variable or a DynamicVariable (keys live on GPU key % N).  With several GPUs every key goes
    to its owner and every vector back to its asker (two all-to-alls; B_local * D floats per rank
    and direction, where lookup_sparse's all-gather / reduce-scatter moves B_global * D).  A
    training lookup inserts unknown keys into a DynamicVariable, an evaluation lookup reads them
    as zero.  OptimizerWrapper.step applies the gradients."""
    if isinstance(param, LocalizedVariable) or not isinstance(
            param, (DistributedVariable, DynamicVariable)) or param.target_gpu >= 0:
        raise TypeError("all2all_dense_embedding takes a distributed sok.Variable or a "
                        "sok.DynamicVariable (keys are sharded by key % num_gpus)")
    _check_indices(indices)
    keys = indices.reshape(-1).contiguous()
    if isinstance(param, DynamicVariable):
        keys = keys.to(param.key_type)
    out = _DenseFn.apply(param._token, param, keys, bool(training))
    return out.view(*indices.shape, param.dimension)


class _GroupFn(torch.autograd.Function):
    """group_lookup: every table through one hctr_indexed_row_copy call"""

    @staticmethod
    def forward(ctx, params, indices, out_dtype, *handles):
        outs, tasks = [], []
        for p, idx in zip(params, indices):
            w = p.weight if isinstance(p, _VariableBase) else p.detach()
            rows, D = w.shape
            out = torch.empty((idx.numel(), D), dtype=out_dtype, device=idx.device)
            if idx.numel() and rows == 0:
                out.zero_()
            elif idx.numel():
                tasks.append((w, rows, D, idx, 1, idx.numel(), out, None))
            outs.append(out)
        if tasks:
            _row_copy(tasks, _lib.F32, _lib.F16 if out_dtype == torch.float16 else _lib.F32)
        ctx.params, ctx.indices = params, indices
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        grads = []
        for p, idx, g in zip(ctx.params, ctx.indices, gs):
            if g is None:
                grads.append(None)
                continue
            g = g.contiguous().float()
            if isinstance(p, _VariableBase):
                ro = torch.arange(idx.numel() + 1, dtype=torch.int64, device=g.device)
                p._pending.append((ro, _static_rows(p, idx), idx, None, g, 0))
                grads.append(torch.zeros(1, device=g.device))
            elif p.requires_grad:
                # sparse COO, uncoalesced, as nn.Embedding(sparse=True) gives; a row out of range
                # was read as zero and gets a zero gradient on row 0
                i64 = idx.to(torch.int64)
                ok = (i64 >= 0) & (i64 < p.shape[0])
                grads.append(torch.sparse_coo_tensor(
                    torch.where(ok, i64, torch.zeros_like(i64)).unsqueeze(0),
                    g * ok.unsqueeze(1), size=tuple(p.shape)))
            else:
                grads.append(None)
        return (None, None, None, *grads)


def group_lookup(params, indices, dtype=None, name=None):
    """sok.group_lookup(params, indices, dtype=None, name=None) (lookup.py:83-96): the fused
    tf.nn.embedding_lookup of several tables on one GPU -- one kernel launch for all of them.
    params / indices: one item or equally long lists; a param is a static sok.Variable wholly held
    by this GPU or a 2-D float32 CUDA tensor / nn.Parameter.  dtype: torch.float32 (default) or
    torch.float16.  Always returns a list of indices.shape + (dimension,) tensors.  Gradients: a
    sok.Variable's wait for OptimizerWrapper.step, a plain tensor's is a sparse COO tensor."""
    params = list(params) if isinstance(params, (list, tuple)) else [params]
    indices = list(indices) if isinstance(indices, (list, tuple)) else [indices]
    if len(params) != len(indices):
        raise RuntimeError("params and indices must have the same length")
    if dtype is None:
        dtype = torch.float32
    if dtype not in (torch.float32, torch.float16):
        raise TypeError("dtype must be torch.float32 or torch.float16")
    for p in params:
        if isinstance(p, DistributedVariable):
            if (p.target_gpu < 0 and _WORLD > 1) or (p.target_gpu >= 0 and p.target_gpu != _RANK):
                raise TypeError("group_lookup is a single-GPU lookup: the variable must be held "
                                "wholly by this GPU (all2all_dense_embedding looks up a "
                                "distributed one)")
        elif not (isinstance(p, torch.Tensor) and p.dim() == 2 and p.dtype == torch.float32
                  and p.is_cuda and p.is_contiguous()):
            raise TypeError("params must be static sok.Variables or contiguous 2-D float32 CUDA "
                            "tensors")
    flat = []
    for idx in indices:
        _check_indices(idx)
        flat.append(idx.reshape(-1).contiguous())
    handles = [p._token if isinstance(p, _VariableBase) else p for p in params]
    outs = _GroupFn.apply(params, flat, dtype, *handles)
    dims = [p.dimension if isinstance(p, _VariableBase) else p.shape[1] for p in params]
    return [o.view(*idx.shape, d) for o, idx, d in zip(outs, indices, dims)]


# ---- optimizer ----------------------------------------------------------------------------------
class OptimizerWrapper:
    """sok.OptimizerWrapper: applies the sparse gradients `lookup_sparse` left on its variables.
    optimizer: "sgd" | "adagrad" | "adam" | "momentum" | "nesterov" (static and dynamic
    variables) | "rmsprop" | "ftrl" (dynamic variables only, as in the reference's tables)."""

    _CODES = {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "adam": _lib.OPT_ADAM,
              "momentum": _lib.OPT_MOMENTUM_SGD, "nesterov": _lib.OPT_NESTEROV,
              "rmsprop": _lib.OPT_RMSPROP, "ftrl": _lib.OPT_FTRL}

    def __init__(self, optimizer: str = "sgd", lr: float = 0.01, beta1=0.9, beta2=0.999,
                 epsilon=1e-7, momentum=0.9, rmsprop_beta=0.9, ftrl_lambda1=0.0, ftrl_lambda2=0.0,
                 ftrl_beta=0.0, scaler: float = 1.0):
        self.name = optimizer.lower()
        self.code = self._CODES[self.name]
        self.hp = dict(lr=lr, beta1=beta1, beta2=beta2, epsilon=epsilon, momentum=momentum,
                       rmsprop_beta=rmsprop_beta, ftrl_lambda1=ftrl_lambda1,
                       ftrl_lambda2=ftrl_lambda2, ftrl_beta=ftrl_beta, scaler=scaler)
        self.times = 0

    def set_learning_rate(self, lr: float):
        self.hp["lr"] = lr

    def step(self, variables: Sequence[_VariableBase]):
        """apply_gradients over the variables touched since the last step"""
        self.times += 1
        for var in variables:
            pend, var._pending = var._pending, []
            if not pend:
                continue
            if isinstance(var, DynamicVariable):
                # one optimizer step per variable per call, however many lookups used it
                ks, gs = [], []
                for ro, rows, keys, w, g, comb in pend:
                    if keys.numel() == 0:
                        continue
                    kg = torch.empty((keys.numel(), var.dimension), dtype=torch.float32,
                                     device=g.device)
                    check(lib.hctr_expand_key_grads(ro.numel() - 1, var.dimension, comb, ptr(ro),
                                                    ptr(w), ptr(g), ptr(kg), stream_ptr()))
                    ks.append(keys)
                    gs.append(kg)
                if ks and var._lru is not None:
                    self._step_hybrid(var, torch.cat(ks), torch.cat(gs))
                elif ks:
                    self._step_dynamic(var, torch.cat(ks), torch.cat(gs))
            else:
                for ro, rows, keys, w, g, comb in pend:
                    self._step_static(var, ro, rows, w, g, comb)

    def _ensure_dynamic(self, var: "DynamicVariable"):
        """the variable's fused optimizer (and its state table) for this wrapper's optimizer"""
        if var._opt is None or var._opt.p.optimizer != self.code:
            hp = self.hp
            var._opt = DynamicTableOptimizer(
                var._det, self.code, hp["lr"], hp["beta1"], hp["beta2"], hp["epsilon"],
                hp["momentum"], hp["rmsprop_beta"], hp["ftrl_lambda1"], hp["ftrl_lambda2"],
                hp["ftrl_beta"], hp["scaler"])

    # static variable: the path's sort + segmented reduce + optimizer on the local shard
    def _step_static(self, var: DistributedVariable, ro, rows, w, g, comb):
        if self.name in ("rmsprop", "ftrl"):
            raise RuntimeError(f"{self.name} is only available for DynamicVariable")
        D = var.dimension
        nnz = rows.numel()
        if nnz == 0:
            return
        if w is not None or comb == 1:
            kg = torch.empty((nnz, D), dtype=torch.float32, device=g.device)
            check(lib.hctr_expand_key_grads(ro.numel() - 1, D, comb, ptr(ro), ptr(w), ptr(g),
                                            ptr(kg), stream_ptr()))
            g, ro = kg, torch.arange(nnz + 1, dtype=torch.int64, device=g.device)
        rows_n = max(var.weight.shape[0], 1)
        if var._updater is None or var._updater[1] < nnz:
            if var._updater is not None:
                lib.hctr_updater_destroy(var._updater[0])
            h = ctypes.c_void_p()
            cap = max(2 * nnz, 1024)
            check(lib.hctr_updater_create(cap, rows_n, D, ctypes.byref(h)))
            var._updater = (h, cap)
        ns = _num_state(self.code)
        while len(var._states) < ns:
            var._states.append(torch.zeros_like(var.weight))
        hp = self.hp
        check(lib.hctr_updater_update(
            var._updater[0], ro.numel() - 1, nnz, ptr(ro), ptr(rows), ptr(g), _lib.F32, self.code,
            _lib.UPDATE_LOCAL, hp["lr"], hp["beta1"], hp["beta2"], hp["epsilon"], hp["momentum"],
            hp["scaler"], self.times, ptr(var.weight),
            ptr(var._states[0]) if ns >= 1 else None, ptr(var._states[1]) if ns >= 2 else None,
            stream_ptr()))

    # hybrid variable: the keys are found again (find only) -- one evicted since its lookup has no
    # row any more and its gradient is dropped (kInvalidIndex), never applied to the slot's new
    # owner -- then the static path's sort + segmented reduce + optimizer on the slot rows
    def _step_hybrid(self, var: DynamicVariable, keys, kg):
        if self.name in ("rmsprop", "ftrl"):
            raise RuntimeError(f"{self.name} is not available for a hybrid DynamicVariable")
        D = var.dimension
        n = keys.numel()
        slots = var._lru.find(keys)
        # (the row bound follows a table that is still growing)
        ucap = max(2 * n, 1024) if var._updater is None or var._updater[1] < n else var._updater[1]
        bound = var._lru.update_rows(ucap)
        if var._updater is None or var._updater[1] < ucap or var._updater[2] < bound:
            if var._updater is not None:
                lib.hctr_updater_destroy(var._updater[0])
            h = ctypes.c_void_p()
            check(lib.hctr_updater_create(ucap, bound, D, ctypes.byref(h)))
            var._updater = (h, ucap, bound)
        for i in range(_num_state(self.code)):
            var._lru.state_ptr(i)
        ro = torch.arange(n + 1, dtype=torch.int64, device=kg.device)
        # (host slots, if any, are staged into HBM rows, updated there and written back)
        var._lru.apply_update(var._updater[0], ro, slots, kg, self.code, self.hp, self.times)

    # dynamic variable: per-key gradients -> unique keys + sums (the reference's OptimizerWrapper
    # does this with tf.unique / unsorted_segment_sum, optimizer.py:170-230) -> fused HIP step
    def _step_dynamic(self, var: DynamicVariable, keys, kg):
        D = var.dimension
        n = keys.numel()
        keys = keys.contiguous()
        # unique keys + per-key gradient sums in ascending position order (deterministic): the
        # path's local reduce, sorted by the keys' row numbers in the table
        _, rows, base = var._det.lookup_rows(keys, insert=False, want_ptrs=False)
        if var._updater is None or var._updater[1] < n:
            if var._updater is not None:
                lib.hctr_updater_destroy(var._updater[0])
            h = ctypes.c_void_p()
            cap = max(2 * n, 1024)
            check(lib.hctr_updater_create(cap, cap, D, ctypes.byref(h)))
            var._updater = (h, cap)
        ro = torch.arange(n + 1, dtype=torch.int64, device=kg.device)
        urow = torch.empty(n, dtype=torch.int64, device=kg.device)
        ukey = torch.empty(n, dtype=torch.int64, device=kg.device)
        wg = torch.empty((n, D), dtype=torch.float32, device=kg.device)
        nu = ctypes.c_size_t()
        k64 = keys if keys.dtype == torch.int64 else keys.to(torch.int64)
        kg = kg.contiguous()
        check(lib.hctr_ebc_local_reduce(var._updater[0], n, n, ptr(ro), ptr(rows), base[-1],
                                        ptr(k64), ptr(kg), _lib.F32, ctypes.byref(nu),
                                        ptr(urow), ptr(ukey), ptr(wg), stream_ptr()))
        uniq = ukey[:nu.value].to(keys.dtype)
        sums = wg[:nu.value]
        self._ensure_dynamic(var)
        var._opt.set_learning_rate(self.hp["lr"])
        ev = torch.arange(0, (uniq.numel() + 1) * D, D, dtype=torch.int32, device=kg.device)
        var._opt.update(uniq.contiguous(), ev, sums.view(-1))


# ---- dump / load (R/sparse_operation_kit/sparse_operation_kit/dump_load.py; byte layout in
#      sok_format.py): per variable `<name>-key`, `<name>-weight` and, when the optimizer holds
#      state for it, `<name>-<Optimizer>-<slot>`; plus one `meta_info`.  GPU 0 writes. -------------
from . import sok_format as _fmt  # noqa: E402

# slot names follow the TF optimizers the reference wraps (optimizer.get_slot_names())
_SLOTS = {"sgd": [], "adam": ["m", "v"], "adagrad": ["accumulator"], "momentum": ["momentum"],
          "nesterov": ["momentum"], "rmsprop": ["rms"], "ftrl": ["accumulator", "linear"]}
# get_sok_optimizer_name (dump_load.py:126-143) looks for one of these in the class name
_OPT_FILE_NAME = {"sgd": "SGD", "adam": "Adam", "adagrad": "Adagrad", "ftrl": "Ftrl",
                  "momentum": "SGD", "nesterov": "SGD", "rmsprop": "RMSprop"}


def filter_variables(variables):
    """(sok variables, the others) -- sok.filter_variables (sparse_operation_kit/__init__.py)"""
    a = [v for v in variables if isinstance(v, _VariableBase)]
    return a, [v for v in variables if not isinstance(v, _VariableBase)]


def _gather_rounds(keys: torch.Tensor, mats: List[torch.Tensor], shared: bool):
    """the reference's write order (save_table_to_filesystem_*): rows go out in rounds of at most
    64 MiB; with several GPUs a round holds that slice of every rank, rank after rank"""
    n = keys.numel()
    if not shared or _WORLD == 1:
        return keys, mats
    D = mats[0].shape[1] if mats else 1
    total = torch.tensor([n], dtype=torch.int64, device=keys.device)
    sizes = _all_gather_cat(total)
    rounds, per = _fmt.rows_per_round(int(sizes.max()), D, 4)
    ks, ms = [], [[] for _ in mats]
    for r in range(rounds):
        a, b = min(r * per, n), min((r + 1) * per, n)
        ks.append(_all_gather_cat(keys[a:b]))
        for j, m in enumerate(mats):
            ms[j].append(_all_gather_cat(m[a:b].reshape(-1)).view(-1, m.shape[1]))
    return torch.cat(ks), [torch.cat(x) for x in ms]


def _var_arrays(var, optimizer):
    """(keys int64 [n], weight [n, D], [state matrices in slot order]) of this rank"""
    D = var.dimension
    slots = _SLOTS[optimizer.name] if optimizer is not None else []
    if isinstance(var, DynamicVariable) and var._lru is not None:
        k, w, sl, _ = var._lru.export(with_slots=True)
        order = torch.argsort(k)
        k, w, sl = k[order].to(torch.int64), w[order], sl[order]
        states = []
        for j in range(len(slots)):
            var._lru.state_ptr(j)  # (allocated, zeroed, if the optimizer has not stepped yet)
            states.append(var._lru.gather_slots(1 + j, sl))
        return k, w, states
    if isinstance(var, DynamicVariable):
        k, w = var._det.export(0)
        order = torch.argsort(k)
        k, w = k[order].to(torch.int64), w[order]
        states = []
        if slots and var._opt is not None and var._opt.states is not None:
            sk, sv = var._opt.states.export(0)
            sv = sv[torch.argsort(sk)]
            if sv.shape[0] == k.numel():
                states = [sv[:, j * D:(j + 1) * D].contiguous() for j in range(len(slots))]
        return k, w, states
    n = var.weight.shape[0]
    if var.target_gpu >= 0:
        k = torch.arange(n, dtype=torch.int64, device=var.weight.device)
    else:
        k = torch.arange(n, dtype=torch.int64, device=var.weight.device) * _WORLD + _RANK
    states = [t for t in var._states[:len(slots)]] if len(var._states) >= len(slots) else []
    return k, var.weight, states


def dump(path: str, dump_vars, optimizer: Optional["OptimizerWrapper"] = None):
    """sok.dump(path, sok_vars, optimizer): the reference's directory layout and byte format"""
    if not isinstance(dump_vars, (list, tuple)):
        dump_vars = [dump_vars]
    os.makedirs(path, exist_ok=True)
    infos = []
    opt_name = _OPT_FILE_NAME[optimizer.name] if optimizer is not None else ""
    slots = _SLOTS[optimizer.name] if optimizer is not None else []
    for var in dump_vars:
        k, w, states = _var_arrays(var, optimizer)
        shared = var.target_gpu < 0
        writer = 0 if shared else var.target_gpu
        if shared:
            k, mats = _gather_rounds(k, [w] + states, True)
            w, states = mats[0], mats[1:]
        if isinstance(var, DynamicVariable) and _RANK == writer and k.numel() == 0:
            raise Exception(f"dynamic table don't have value in it , table_name: {var.name}")
        if _RANK == writer:
            fname = os.path.join(path, _fmt.file_table_name(var.name))
            kn = k.cpu().numpy().astype(np.int64 if shared or isinstance(var, DynamicVariable)
                                        else np.uint64)
            _fmt.write_array_file(fname + "-key", var.name, _fmt.FILE_KEY, "", kn)
            _fmt.write_array_file(fname + "-weight", var.name, _fmt.FILE_EMB, "",
                                  w.detach().cpu().numpy().astype(np.float32))
            for slot, st in zip(slots, states):
                _fmt.write_array_file(f"{fname}-{opt_name}-{slot}", var.name, _fmt.FILE_OPT_STATE,
                                      slot, st.detach().cpu().numpy().astype(np.float32))
        infos.append(_fmt.VarInfo(var.name, opt_name, _fmt.DTYPE_INDEX[np.dtype(np.int64)],
                                  _fmt.DTYPE_INDEX[np.dtype(np.float32)], int(k.numel()),
                                  var.dimension))
    if _RANK == 0:
        _fmt.save_meta_file(path, infos)
    if _WORLD > 1:
        dist.barrier()


def load(path: str, load_vars, optimizer: Optional["OptimizerWrapper"] = None):
    """sok.load(path, sok_vars, optimizer): every rank reads the files and keeps its own keys"""
    if not isinstance(load_vars, (list, tuple)):
        load_vars = [load_vars]
    meta = _fmt.load_meta_file(path)
    opt_name = _OPT_FILE_NAME[optimizer.name] if optimizer is not None else ""
    slots = _SLOTS[optimizer.name] if optimizer is not None else []
    for var in load_vars:
        if var.name not in meta:
            raise Exception(f"table {var.name} is not in the meta_info of {path}")
        fname = os.path.join(path, _fmt.file_table_name(var.name))
        state_paths = [f"{fname}-{opt_name}-{slot}" for slot in slots]
        state_paths = [p for p in state_paths if os.path.exists(p)] if slots else []
        ok, msg, n, ev = _fmt.check_weight_files(fname + "-key", fname + "-weight", state_paths)
        if not ok:
            raise Exception(msg)
        if ev != var.dimension:
            raise Exception(f"{var.name}: file vectors have {ev} elements, the variable {var.dimension}")
        keys = _fmt.read_array_file(fname + "-key").astype(np.int64)
        w = _fmt.read_array_file(fname + "-weight").reshape(n, ev).astype(np.float32)
        states = [_fmt.read_array_file(p).reshape(n, ev).astype(np.float32) for p in state_paths]
        if var.target_gpu >= 0:
            mine = np.full(n, _RANK == var.target_gpu)
        else:
            mine = keys % _WORLD == _RANK
        keys, w, states = keys[mine], w[mine], [x[mine] for x in states]
        dev = torch.device("cuda", torch.cuda.current_device())
        kt = torch.from_numpy(keys).to(dev)
        wt = torch.from_numpy(w).to(dev)
        if isinstance(var, DynamicVariable) and var._lru is not None:
            if kt.numel():
                assign(var, kt.to(var.key_type), wt)
            if states and len(states) == len(slots) and kt.numel():
                idx = var._lru.find(kt.to(var.key_type))
                live = idx >= 0
                for j, x in enumerate(states):
                    var._lru.state_ptr(j)
                    var._lru.scatter_slots(1 + j, idx[live], torch.from_numpy(x).to(dev)[live])
        elif isinstance(var, DynamicVariable):
            if kt.numel():
                assign(var, kt.to(var.key_type), wt)
            if states and len(states) == len(slots) and kt.numel():
                optimizer._ensure_dynamic(var)
                st = var._opt.states
                sk = kt.to(var.key_type)
                st.lookup(sk)
                st.scatter_update(sk, torch.from_numpy(np.concatenate(states, axis=1)).to(dev))
        else:
            rows = var.key_map(kt)
            if rows.numel() and int(rows.max()) >= var.weight.shape[0]:
                raise Exception(f"{var.name}: the file holds more rows than the variable")
            var.weight[rows] = wt
            if states and len(states) == len(slots):
                while len(var._states) < len(slots):
                    var._states.append(torch.zeros_like(var.weight))
                for j, x in enumerate(states):
                    var._states[j][rows] = torch.from_numpy(x).to(dev)
    if _WORLD > 1:
        dist.barrier()


def _threshold_ns(threshold) -> int:
    """a time threshold in nanoseconds since the epoch, converted as dump_load.py does"""
    return int(_dt.datetime.timestamp(threshold) * 1e9)


def incremental_model_dump(sok_vars, time_threshold, sess=None):
    """sok.incremental_model_dump(sok_vars, time_threshold, sess=None) -> (keys_list, values_list)
    (dump_load.py:1343-1500): per variable, the keys and rows of the slots touched by an inserting
    call issued at or after time_threshold (a datetime, or a list of 1 or len(sok_vars) of them).
    Every rank exports its shard; the results are all-gathered in rank order.  Hybrid
    DynamicVariables only; sess is accepted for the signature's sake and must be None."""
    if not isinstance(sok_vars, (list, tuple)):
        sok_vars = [sok_vars]
    thresholds = list(time_threshold) if isinstance(time_threshold, (list, tuple)) \
        else [time_threshold]
    if not (len(thresholds) == 1 or len(thresholds) == len(sok_vars)):
        raise Exception("length of time_threshold should be 1 or same length with sok_vars, if "
                        "length equals 1 , every sok_var will use same time_threshold!")
    if sess is not None:
        raise Exception("sess is a TensorFlow 1.15 session: it must be None here")
    for i, v in enumerate(sok_vars):
        if not isinstance(v, DynamicVariable):
            raise Exception("Now only support sok.DynamicVariable with HKV backend, but the "
                            f"{i}-th sok variable in the input sok_vars is not a "
                            "sok.DynamicVariable!")
        if v.backend_type != "hybrid":
            raise Exception("Now only support sok.DynamicVariable with HKV backend, but the "
                            f"{i}-th sok variable in the input sok_vars is not hkv backend!")
    if len(thresholds) == 1:
        thresholds = thresholds * len(sok_vars)
    keys_list, values_list = [], []
    for var, th in zip(sok_vars, thresholds):
        t0 = first_call_since(var._lru.call_ns, _threshold_ns(th))
        if t0 is None:
            k = torch.empty(0, dtype=var.key_type, device="cuda")
            w = torch.empty((0, var.dimension), dtype=torch.float32, device="cuda")
        else:
            k, w, _, _ = var._lru.export_if(t0)
        if _WORLD > 1:
            k = _all_gather_cat(k)
            w = _all_gather_cat(w.reshape(-1)).view(-1, var.dimension)
        keys_list.append(k.cpu().numpy())
        values_list.append(w.cpu().numpy())
    return keys_list, values_list
