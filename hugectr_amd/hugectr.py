"""`hugectr`-shaped Python surface (solver + layer API) over the MI355X-native hot path.

Mirrors the reference's pybind module (R/HugeCTR/src/pybind/module_main.cpp:36-48): CreateSolver
(kwargs/defaults of R/HugeCTR/include/pybind/solver_wrapper.hpp:127-150), DataReaderParams,
CreateOptimizer (optimizer_wrapper.hpp:35-40), Input / DataReaderSparseParam / SparseEmbedding /
DenseLayer (model_wrapper.hpp:56-121) and Model.add/compile/summary/fit/eval/... (:123-227), so
that scripts written as `samples/dcn/*.py`, `samples/deepfm/*.py`, `samples/wdl/*.py`, DLRM-style
(Interaction) models run with `import hugectr_amd.hugectr as hugectr`.

The sparse embeddings, Interaction and MultiCross run on the HIP kernels behind the C ABI; the
remaining dense layers are thin PyTorch-ROCm modules (out of scope as kernels).
One process drives one GPU: `vvgpu` must list as many GPUs as there are torch.distributed ranks
(a plain single-process run uses vvgpu=[[0]]).
"""
from __future__ import annotations

import enum
import json
import os
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .dense import (DenseFtrl, DenseGradFinish, FusedMLP, bce_with_logits, ftrl_state_dict,
                    load_ftrl_state_dict)
from .embedding import OptParams, SparseEmbeddingHash, backward_reorder, forward_reorder
from .embedding_collection import (DataParallelCollection, EmbeddingCollection,  # noqa: F401
                                   EmbeddingCollectionConfig, EmbeddingTableConfig,
                                   check_init_param, check_table_optimizer,
                                   group_lookups_by_optimizer, resolve_table_optimizer, table_kind)
from .metrics import EvalMetrics
from .layers import (MultiCrossLayer, interaction, interaction_gather, interaction_indexed,
                     regather_supported)
from .parallel import DistributedExchange, LocalizedExchange, reorder_row_map
from .parallel import all_reduce as _all_reduce
from . import data as _data


# ---- enums (values follow R/HugeCTR/include/common.hpp:67-157) ------------------------------------
class Check_t(enum.Enum):
    Sum = 0
    Non = 1
    Unknown = 2


class DataReaderType_t(enum.Enum):
    Norm = 0
    Raw = 1
    Parquet = 2
    RawAsync = 3


class LrPolicy_t(enum.Enum):
    fixed = 0


class Optimizer_t(enum.IntEnum):
    Ftrl = 0
    Adam = 1
    RMSProp = 2
    AdaGrad = 3
    Nesterov = 4
    MomentumSGD = 5
    SGD = 6


class Update_t(enum.IntEnum):
    Local = 0
    Global = 1
    LazyGlobal = 2


class Embedding_t(enum.IntEnum):
    DistributedSlotSparseEmbeddingHash = 0
    LocalizedSlotSparseEmbeddingHash = 1


class Activation_t(enum.Enum):
    Relu = 0
    Non = 1
    Unspecified = 2


class Initializer_t(enum.Enum):
    Default = 0
    Uniform = 1
    XavierNorm = 2
    XavierUniform = 3
    Sinusoidal = 4
    Zero = 5


class Distribution_t(enum.Enum):
    Uniform = 0
    PowerLaw = 1


class PowerLaw_t(enum.Enum):
    Long = 0
    Medium = 1
    Short = 2
    Specific = 3


class MetricsType(enum.Enum):
    AUC = 0
    AverageLoss = 1
    HitRate = 2
    NDCG = 3
    SMAPE = 4


Layer_t = enum.Enum("Layer_t", [
    "BatchNorm", "LayerNorm", "BinaryCrossEntropyLoss", "Reshape", "Select", "Concat",
    "CrossEntropyLoss", "Dropout", "ELU", "InnerProduct", "MLP", "Interaction",
    "MultiCrossEntropyLoss", "ReLU", "ReLUHalf", "GRU", "MatrixMultiply", "MultiHeadAttention",
    "Scale", "FusedReshapeConcat", "FusedReshapeConcatGeneral", "Softmax", "PReLU_Dice",
    "ReduceMean", "Sub", "Gather", "Sigmoid", "Slice", "WeightMultiply", "FmOrder2", "Add",
    "ReduceSum", "MultiCross", "Cast", "ElementwiseMultiply", "SequenceMask", "Unknown"])


# ---- plain parameter holders -------------------------------------------------------------------
@dataclass
class Solver:
    model_name: str = ""
    seed: int = 0
    lr_policy: LrPolicy_t = LrPolicy_t.fixed
    lr: float = 0.001
    warmup_steps: int = 1
    decay_start: int = 0
    decay_steps: int = 1
    decay_power: float = 2.0
    end_lr: float = 0.0
    max_eval_batches: int = 100
    batchsize_eval: int = 2048
    batchsize: int = 2048
    vvgpu: List[List[int]] = field(default_factory=lambda: [[0]])
    repeat_dataset: bool = True
    use_mixed_precision: bool = False
    enable_tf32_compute: bool = False
    scaler: float = 1.0
    metrics_spec: Dict = field(default_factory=lambda: {MetricsType.AUC: 1.0})
    i64_input_key: bool = False
    use_algorithm_search: bool = True
    use_cuda_graph: bool = True
    gen_loss_summary: bool = True
    train_intra_iteration_overlap: bool = False
    train_inter_iteration_overlap: bool = False
    eval_intra_iteration_overlap: bool = False
    eval_inter_iteration_overlap: bool = False
    device_layout: str = "LOCAL_FIRST"
    use_embedding_collection: bool = False
    all_reduce_algo: str = "NCCL"
    grouped_all_reduce: bool = False
    num_iterations_statistics: int = 20
    perf_logging: bool = False
    drop_incomplete_batch: bool = True
    kafka_brockers: str = ""
    training_callbacks: list = field(default_factory=list)


def CreateSolver(**kw) -> Solver:
    s = Solver()
    for k, v in kw.items():
        if not hasattr(s, k):
            raise RuntimeError(f"CreateSolver: unknown argument '{k}'")
        setattr(s, k, v)
    if s.use_mixed_precision and s.scaler not in (128.0, 256.0, 512.0, 1024.0):
        # solver_wrapper / parser check: mixed precision requires one of these loss scalers
        raise RuntimeError("use_mixed_precision requires scaler in {128, 256, 512, 1024}")
    _launch_one_process_per_gpu(sum(len(v) for v in s.vvgpu))
    return s


def _launch_one_process_per_gpu(n_gpus: int):
    """`python train.py` with vvgpu = [[0 .. N-1]]: the reference drives its N GPUs from one process
    (one OpenMP thread per GPU, R/HugeCTR/src/pybind/model.cpp:1100).  Here one PROCESS drives one
    GPU, so a script that asks for N > 1 GPUs and was not started by torch.distributed.run is
    started again as N ranks (RCCL rendezvous on 127.0.0.1) and this process only waits for them.
    Happens in CreateSolver, the first hugectr call of the reference's scripts, so that little of
    the script runs twice."""
    import sys
    if n_gpus <= 1 or "WORLD_SIZE" in os.environ or dist.is_initialized():
        return
    script = sys.argv[0] if sys.argv else ""
    main_file = getattr(sys.modules.get("__main__"), "__file__", None)
    # only a script started as `python train.py` is started again: not a test runner, a notebook
    # kernel or `python -m something` whose argv[0] happens to be a file
    direct = bool(main_file) and os.path.isfile(script) and \
        os.path.abspath(main_file) == os.path.abspath(script) and "pytest" not in sys.modules and \
        os.environ.get("HCTR_NO_RELAUNCH") != "1"
    if not direct:
        return  # (Model() reports the mismatch between vvgpu and the running ranks)
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           script] + list(sys.argv[1:])
    print(f"[HCTR][INFO] vvgpu lists {n_gpus} GPUs: starting one process per GPU: {' '.join(cmd)}",
          flush=True)
    raise SystemExit(subprocess.call(cmd))


def _use_gemm_selection(solver) -> str:
    """solver.use_algorithm_search (the reference searches cublasGemmEx algorithms when the layers
    are built, solver_wrapper.hpp:139): here the dense GEMMs of torch / hipBLASLt take the
    solutions recorded in hugectr_amd/tuning/tunableop_gfx950.csv through PyTorch TunableOp --
    read only, nothing is tuned at run time.  HCTR_TUNABLEOP=off keeps the library heuristics."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning",
                        "tunableop_gfx950.csv")
    if not solver.use_algorithm_search or os.environ.get("HCTR_TUNABLEOP", "file") == "off" or \
            not os.path.exists(path):
        return "off"
    try:
        import torch.cuda.tunable as tunable
        if not tunable.is_enabled():
            tunable.enable(True)
            tunable.tuning_enable(False)
            tunable.read_file(path)
            # the recorded selections are read, never rewritten: whatever TunableOp writes when
            # the process ends goes to a scratch file
            import tempfile
            tunable.set_filename(os.path.join(tempfile.gettempdir(),
                                              f"hctr_tunableop_{os.getpid()}.csv"))
        return "file"
    except Exception:  # an optimisation only
        return "off"


def _join_process_group():
    """a rank started by torch.distributed.run (by hand or by _launch_one_process_per_gpu) joins
    the job: RCCL ("nccl") unless HCTR_DIST_BACKEND says otherwise (the CPU / one-GPU tests use
    gloo)"""
    if dist.is_initialized() or int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("HCTR_DIST_BACKEND", "nccl")
    if backend == "nccl":
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)


class Alignment_t(enum.Enum):
    Auto = 0
    Non = 1


@dataclass
class AsyncParam:  # R/HugeCTR/include/pybind/common_wrapper.hpp:144-151 (same names and defaults)
    num_threads: int
    num_batches_per_thread: int
    max_num_requests_per_thread: int = 0
    io_depth: int = 0
    io_alignment: int = 0
    shuffle: bool = False
    aligned_type: Alignment_t = Alignment_t.Non
    multi_hot_reader: bool = True
    is_dense_float: bool = True


@dataclass
class DataReaderParams:
    data_reader_type: DataReaderType_t
    source: Sequence[str]
    eval_source: str = ""
    check_type: Check_t = Check_t.Non
    cache_eval_data: int = 0
    num_samples: int = 0
    eval_num_samples: int = 0
    float_label_dense: bool = False
    num_workers: int = 12
    slot_size_array: Sequence[int] = field(default_factory=list)
    async_param: object = None

    def __post_init__(self):
        if isinstance(self.source, str):
            self.source = [self.source]


@dataclass
class OptParamsPy:
    optimizer_type: Optimizer_t = Optimizer_t.Adam
    update_type: Update_t = Update_t.Global
    beta: float = 0.0
    lambda1: float = 0.0
    lambda2: float = 0.0
    beta1: float = 0.9
    beta2: float = 0.999
    epsilon: float = 1e-7
    initial_accu_value: float = 0.0
    momentum_factor: float = 0.0
    atomic_update: bool = True
    initialized: bool = True


def CreateOptimizer(optimizer_type=Optimizer_t.Adam, update_type=Update_t.Global, beta=0.0,
                    lambda1=0.0, lambda2=0.0, beta1=0.9, beta2=0.999, epsilon=1e-7,
                    initial_accu_value=0.0, momentum_factor=0.0, atomic_update=True) -> OptParamsPy:
    return OptParamsPy(optimizer_type, update_type, beta, lambda1, lambda2, beta1, beta2, epsilon,
                       initial_accu_value, momentum_factor, atomic_update)


class InitParams:
    """EmbeddingTableConfig(init_param=...): how a static embedding_collection table is first
    filled.  The reference's module has the argument but no constructor for it; this holder has
    the arguments and checks of embedding::InitParams
    (R/HugeCTR/embedding_storage/common.hpp:54-73).  Default: U(+-sqrt(1/vocabulary));
    Uniform: U(-up_bound, up_bound); Sinusoidal: the position table of max_sequence_len rows
    (embedding_collection.sinusoidal_table), max_sequence_len * ev_size being the table's size."""

    def __init__(self, ev_size, initializer_type=Initializer_t.Default, up_bound=-1,
                 max_sequence_len=-1):
        if not isinstance(initializer_type, Initializer_t):
            raise RuntimeError(f"InitParams: initializer_type must be an Initializer_t, not "
                               f"{initializer_type!r}")
        self.ev_size, self.initializer_type = int(ev_size), initializer_type
        self.up_bound, self.max_sequence_len = 0.0, 0
        if initializer_type == Initializer_t.Uniform:
            if not up_bound > 0:
                raise RuntimeError("InitParams: initialize type uniform should specify up_bound")
            self.up_bound = float(up_bound)
        if initializer_type == Initializer_t.Sinusoidal:
            if not max_sequence_len > 0:
                raise RuntimeError("InitParams: initialize type sinusoidal should specify "
                                   "max_sequence_len")
            self.max_sequence_len = int(max_sequence_len)

    def __repr__(self):
        return (f"InitParams(ev_size={self.ev_size}, initializer_type={self.initializer_type}, "
                f"up_bound={self.up_bound}, max_sequence_len={self.max_sequence_len})")


def check_embedding_collection_config(cfg: EmbeddingCollectionConfig, model_opt, world: int = 1):
    """what Model.compile checks of a config's per-table options before any device call: every
    table's resolved optimizer (its opt_params, else the model's) is one its kind of table runs,
    and its init_param is one its storage honours.  Raises RuntimeError naming the table."""
    from types import SimpleNamespace
    for sub, _ in Model._split_by_ev_size(SimpleNamespace(world=world, opt=model_opt), cfg):
        kinds = {table_kind(t) for t, _, _, _ in sub.lookups}
        # (a static table beside a dynamic one is held by the dynamic table, all seven optimizers)
        kind = "dp" if sub.shard_strategy == "dp" else "hybrid" if "hybrid" in kinds else \
            "dynamic" if "dynamic" in kinds else "static"
        tables = []
        for t, _, _, _ in sub.lookups:
            if t not in tables:
                tables.append(t)
        for t in tables:
            check_table_optimizer(t, kind, *resolve_table_optimizer(t, model_opt))
            check_init_param(t, "static" if kind == "dp" else kind)


@dataclass
class DataReaderSparseParam:
    top_name: str
    nnz_per_slot: object  # int or list of int
    is_fixed_length: bool
    slot_num: int

    def max_nnz(self) -> int:
        if isinstance(self.nnz_per_slot, (list, tuple)):
            return int(max(self.nnz_per_slot))
        return int(self.nnz_per_slot)

    def max_feature_num(self) -> int:
        if isinstance(self.nnz_per_slot, (list, tuple)):
            return int(sum(self.nnz_per_slot))
        return int(self.nnz_per_slot) * self.slot_num


class Input:
    def __init__(self, label_dim=None, label_name=None, dense_dim=0, dense_name="dense",
                 data_reader_sparse_param_array=(), label_dims=None, label_names=None,
                 label_weights=None):
        if label_dims is not None:
            self.label_dims, self.label_names = list(label_dims), list(label_names)
        else:
            self.label_dims, self.label_names = [int(label_dim)], [label_name]
        self.label_dim = sum(self.label_dims)
        self.label_name = self.label_names[0]
        self.dense_dim, self.dense_name = int(dense_dim), dense_name
        self.sparse_params: List[DataReaderSparseParam] = list(data_reader_sparse_param_array)
        # label_weights_ of the reference (model_compile.cpp:748-765): the tasks' default weights
        if label_weights is not None and len(list(label_weights)) != len(self.label_names):
            raise RuntimeError("Input: label_weights and label_names differ in length")
        self.label_weights = [float(w) for w in label_weights] if label_weights is not None \
            else [1.0] * len(self.label_names)


class LearningRateScheduler:
    """R/HugeCTR/include/learning_rate_scheduler.hpp:20-90: linear warm-up over warmup_steps, then
    the base rate, then (decay_start > 0) polynomial decay over decay_steps down to end_lr"""

    def __init__(self, base_lr: float, warmup_steps: int = 1, decay_start: int = 0,
                 decay_steps: int = 1, decay_power: float = 2.0, end_lr: float = 0.0):
        if base_lr < 0 or warmup_steps < 0 or decay_steps < 0 or decay_power < 1.0 or end_lr < 0:
            raise RuntimeError("base_lr < 0 || warmup_steps < 0 || decay_steps < 0 || "
                               "decay_power < 1.0 || end_lr < 0.f")
        self.base_lr, self.warmup_steps, self.decay_start = base_lr, warmup_steps, decay_start
        self.decay_steps, self.decay_power, self.end_lr = decay_steps, decay_power, end_lr
        self.step, self.current_lr = 0, 0.0

    def get_next(self) -> float:
        self.step += 1
        st = self.step
        if st <= self.warmup_steps:
            self.current_lr = st * self.base_lr / self.warmup_steps
        elif self.decay_start != 0:
            if st <= self.decay_start:
                self.current_lr = self.base_lr
            elif st <= self.decay_start + self.decay_steps:
                f = ((self.decay_start + self.decay_steps - st) / float(self.decay_steps)) ** self.decay_power
                self.current_lr = max(self.base_lr * f, self.end_lr)
            else:
                self.current_lr = self.end_lr
        else:
            self.current_lr = self.base_lr
        return self.current_lr

    def get_lr(self) -> float:
        return self.current_lr

    def get_step(self) -> int:
        return self.step


class AllReduceAlgo(enum.Enum):  # R/HugeCTR/include/pybind/common_wrapper.hpp:199-201
    OneShot = 0
    NCCL = 1


class TrainingCallback:
    """R/HugeCTR/include/training_callback.hpp:20-26; pass instances in
    CreateSolver(training_callbacks=[...]).  on_eval_end returning True stops fit() early."""

    def on_training_start(self):
        pass

    def on_training_end(self, current_iter: int):
        pass

    def on_eval_start(self, current_iter: int) -> bool:
        return False

    def on_eval_end(self, current_iter: int, eval_results: Dict[str, float]) -> bool:
        return False


class CommunicationStrategy(enum.Enum):  # R/HugeCTR/include/embedding/common.hpp
    Uniform = 0
    Hierarchical = 1


class CompressionStrategy(enum.Enum):  # embedding_collection_wrapper.hpp:40-43
    Reduction = 0  # pool on the owner, ship pooled vectors (SparseModelParallel)
    Unique = 1     # ship each distinct row once, pool on the receiver (DenseModelParallel*)


@dataclass
class DenseLayerComputeConfig:  # scheduling hints of the reference's MLP layer; accepted, unused
    async_wgrad: bool = False
    fuse_wb: bool = False


class SparseEmbedding:
    def __init__(self, embedding_type, embedding_vec_size, combiner, sparse_embedding_name,
                 bottom_name, workspace_size_per_gpu_in_mb=0, slot_size_array=(), optimizer=None):
        self.embedding_type = Embedding_t(embedding_type)
        self.workspace_size_per_gpu_in_mb = int(workspace_size_per_gpu_in_mb)
        self.embedding_vec_size = int(embedding_vec_size)
        if combiner not in ("sum", "mean"):
            raise RuntimeError("combiner must be 'sum' or 'mean'")
        self.combiner = 0 if combiner == "sum" else 1
        self.sparse_embedding_name = sparse_embedding_name
        self.bottom_name = bottom_name
        self.slot_size_array = list(slot_size_array)
        self.optimizer = optimizer


class DenseLayer:
    def __init__(self, layer_type, bottom_names, top_names, **kw):
        self.layer_type = layer_type
        self.bottom_names, self.top_names = list(bottom_names), list(top_names)
        d = dict(factor=1.0, eps=1e-5, dropout_rate=0.5, elu_alpha=1.0, num_output=1, num_layers=0,
                 leading_dim=0, time_step=0, selected=False, selected_slots=[], ranges=[],
                 indices=[], weight_dims=[], projection_dim=0, out_dim=0, axis=1,
                 target_weight_vec=[], use_regularizer=False, act_type=Activation_t.Relu,
                 num_outputs=[], use_bias=True, activations=[], biases=[], shape=[], dim=0,
                 index=[], pos_type=None, compute_config=None, weight_init_type=None,
                 bias_init_type=None, gamma_init_type=None, beta_init_type=None,
                 regularizer_type=None, batchsize=1, SeqLength=1, vector_size=1,
                 max_sequence_len_from=1, max_sequence_len_to=1, num_attention_heads=1,
                 transpose_b=False)
        d["lambda"] = 0
        for k, v in kw.items():
            if k not in d:
                raise RuntimeError(f"DenseLayer: unknown argument '{k}'")
            d[k] = v
        self.__dict__.update(d)


def _max_vocab_from_workspace(ws_mb: int, opt: OptParamsPy, vec: int) -> int:
    """max_vocabulary_size_per_gpu = ws_MB * 2^20 / ((1 + #opt_states) * 4 * D)
    (R/HugeCTR/src/pybind/model.cpp:186-196)"""
    states = {Optimizer_t.Adam: 2, Optimizer_t.AdaGrad: 1, Optimizer_t.MomentumSGD: 1,
              Optimizer_t.Nesterov: 1, Optimizer_t.SGD: 0, Optimizer_t.Ftrl: 2,
              Optimizer_t.RMSProp: 1}[Optimizer_t(opt.optimizer_type)]
    if Optimizer_t(opt.optimizer_type) == Optimizer_t.Adam and \
            Update_t(opt.update_type) == Update_t.LazyGlobal:
        states += 1  # the per-element prev_time copy (model.cpp:189-192)
    return (ws_mb * 1024 * 1024) // ((1 + states) * 4 * vec)


class _FmOrder2(torch.nn.Module):
    def __init__(self, out_dim):
        super().__init__()
        self.out_dim = out_dim

    def forward(self, x):  # [B, slots*out_dim] -> 0.5 * ((sum v)^2 - sum v^2)
        v = x.view(x.shape[0], -1, self.out_dim)
        return 0.5 * (v.sum(1) ** 2 - (v ** 2).sum(1))


class _ScaleFn(torch.autograd.Function):
    """Layer_t.Scale (R/HugeCTR/src/layers/scale_layer.cu:30-66): fprop repeats -- axis 0: every
    element `factor` times in place ([B, n] -> [B, n * factor], out[j * factor + i] = in[j]);
    axis 1: the row `factor` times side by side.  bprop is the reference's downscale_kernel: it
    takes the gradient of the FIRST copy only (it does not sum over the copies)."""

    @staticmethod
    def forward(ctx, x, axis, factor):
        ctx.axis, ctx.factor, ctx.n = axis, factor, x.shape[1]
        if axis == 0:
            return x.repeat_interleave(factor, dim=1)
        return x.repeat(1, factor)

    @staticmethod
    def backward(ctx, g):
        if ctx.axis == 0:
            return g[:, ::ctx.factor].contiguous(), None, None
        return g[:, :ctx.n].contiguous(), None, None


class _WeightMultiply(torch.nn.Module):
    def __init__(self, slots, vec):
        super().__init__()
        self.w = torch.nn.Parameter(torch.empty(slots, vec).uniform_(-0.05, 0.05))

    def forward(self, x):  # [B, slots] -> [B, slots*vec]
        return (x.unsqueeze(2) * self.w.unsqueeze(0)).reshape(x.shape[0], -1)


class _Pending:
    """an embedding output that is still in flight (all-to-all issued, not waited for): resolved
    by the first dense layer that names it, so every layer in front of that one -- the bottom
    MLP of a DLRM -- is enqueued under the exchange (the reference's intra-iteration overlap:
    bottom_network_fprop does not wait for the embedding's network forward,
    R/HugeCTR/src/pybind/model_pipeline.cpp:299-346)"""

    def __init__(self, resolve):
        self.resolve = resolve


class _IndexedEmb:
    """embedding output of the unique-row exchange kept as (distinct rows, (sample, slot) -> row):
    the Interaction layer reads the rows through the table, the [B, S, D] tensor is never written"""

    def __init__(self, rows, row_of, on_grad, scatter=False):
        # scatter: row_of is a bijection (the reorder map of an all-to-all receive buffer) and
        # on_grad takes the gradient in the rows' layout
        self.rows, self.row_of, self.on_grad, self.scatter = rows, row_of, on_grad, scatter


class _GatherEmb:
    """embedding output that is not materialised before the Interaction layer: on one GPU with one
    key per bucket the interaction kernel reads the table rows through the index stage's result
    itself (hctr_emb_forward_interaction); the pooled vectors are written once for the backward,
    or, where the shape allows (regather_supported), not at all: the backward reads the rows again"""

    def __init__(self, emb, train, on_grad, after_forward=None):
        self.emb, self.train, self.on_grad = emb, train, on_grad
        self.after_forward = after_forward  # called once the interaction's forward is enqueued


class _Tensors(dict):
    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        if isinstance(v, _Pending):
            v = v.resolve()
            dict.__setitem__(self, k, v)
        return v


class Model:
    """hugectr.Model for one rank.  Supported graph: Input -> SparseEmbedding* -> DenseLayer* with
    one BinaryCrossEntropyLoss."""

    def __init__(self, solver: Solver, reader_params: DataReaderParams, opt: OptParamsPy):
        if not torch.cuda.is_available():
            raise RuntimeError("hugectr_amd needs a HIP device (MI355X); there is no CPU fallback")
        self.solver, self.reader_params, self.opt = solver, reader_params, opt
        _join_process_group()
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        n_gpus = sum(len(v) for v in solver.vvgpu)
        if n_gpus != self.world:
            raise RuntimeError(f"vvgpu lists {n_gpus} GPUs but {self.world} rank(s) are running: "
                               "launch one process per GPU (torch.distributed.run)")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if os.environ.get("HCTR_RANKS_ON_ONE_GPU") == "1":  # functional tests on a 1-GPU box
            local = 0
        self.device = torch.device("cuda", local)
        torch.cuda.set_device(self.device)
        torch.manual_seed(solver.seed + 1)
        self.input: Optional[Input] = None
        self.embeddings: List[SparseEmbedding] = []
        self.ebc_configs: List[EmbeddingCollectionConfig] = []
        self.layers: List[DenseLayer] = []
        self._compiled = False
        self._loss = float("nan")
        self._lr = solver.lr
        self._iter = 0

    # -- graph construction ------------------------------------------------------------------------
    def add(self, item):
        if isinstance(item, Input):
            self.input = item
        elif isinstance(item, SparseEmbedding):
            self.embeddings.append(item)
        elif isinstance(item, EmbeddingCollectionConfig):
            self.ebc_configs.append(item)  # use_embedding_collection path (model.cpp add(ebc))
        elif isinstance(item, DenseLayer):
            self.layers.append(item)
        else:
            raise RuntimeError(f"Model.add: unsupported item {type(item)}")

    def _emb_opt(self, se: SparseEmbedding) -> OptParams:
        o = se.optimizer if (se.optimizer is not None and se.optimizer.initialized) else self.opt
        return OptParams(optimizer=int(o.optimizer_type), update_type=int(o.update_type),
                         lr=self._lr, beta1=o.beta1, beta2=o.beta2, epsilon=o.epsilon,
                         initial_accu_value=o.initial_accu_value,
                         momentum_factor=o.momentum_factor,
                         # CreateOptimizer's default atomic_update=True (optimizer_wrapper.hpp:40)
                         # is read as PERMISSION for an order-nondeterministic update, not as a
                         # demand for fp32 atomics: the sorted, segmented update is 5x faster under
                         # power-law duplicates and deterministic.  HCTR_SGD_ATOMIC=1
                         # selects the reference's literal opt_sgd_atomic_kernel form.
                         atomic_update=bool(o.atomic_update) and
                         os.environ.get("HCTR_SGD_ATOMIC") == "1",
                         scaler=self.solver.scaler)

    def compile(self, loss_names=None, loss_weights=None):
        """loss_names / loss_weights: the multi-task form (model_wrapper.hpp compile overload);
        one BinaryCrossEntropyLoss is what this surface trains, so they must name that loss"""
        assert self.input is not None, "Model.add(Input(...)) first"
        for cfg in self.ebc_configs:  # per-table opt_params / init_param: before any device call
            check_embedding_collection_config(cfg, self.opt, self.world)
        # multi-task models (R/samples/mmoe): one BinaryCrossEntropyLoss per label, the training
        # loss is their weighted sum (Model::compile(loss_names, loss_weights), model.cpp)
        # Input(label_weights=...) seeds the weights, compile(loss_names, loss_weights) replaces
        # the named ones and an unknown label name is an error (update_label_weights,
        # R/HugeCTR/src/pybind/model_compile.cpp:748-765)
        self._loss_weights = dict(zip(self.input.label_names, self.input.label_weights))
        if loss_names is not None:
            ws = list(loss_weights) if loss_weights is not None else [1.0] * len(list(loss_names))
            if len(ws) != len(list(loss_names)):
                raise RuntimeError("compile: loss_names and loss_weights differ in length")
            for n, w in zip(loss_names, ws):
                if str(n) not in self.input.label_names:
                    raise RuntimeError(f"compile: '{n}' is not a label of this model "
                                       f"(labels: {self.input.label_names})")
                self._loss_weights[str(n)] = float(w)
        s = self.solver
        B, Be = s.batchsize, s.batchsize_eval
        self.bpg, self.bpg_eval = B // self.world, Be // self.world
        key_dtype = torch.int64 if s.i64_input_key else torch.uint32
        self.emb_dtype = torch.float16 if s.use_mixed_precision else torch.float32
        sp = {p.top_name: p for p in self.input.sparse_params}
        self._emb = {}
        self._shapes: Dict[str, tuple] = {self.input.dense_name: (self.input.dense_dim,)}
        for n, d in zip(self.input.label_names, self.input.label_dims):
            self._shapes[n] = (int(d),)
        for se in self.embeddings:
            p = sp[se.bottom_name]
            opt = self._emb_opt(se)
            ssa = se.slot_size_array or []
            if ssa:
                max_vocab = 0  # derived from the slot sizes by the library
            else:
                assert se.workspace_size_per_gpu_in_mb > 0, "workspace_size_per_gpu_in_mb or slot_size_array"
                max_vocab = _max_vocab_from_workspace(
                    se.workspace_size_per_gpu_in_mb,
                    se.optimizer if (se.optimizer is not None and se.optimizer.initialized)
                    else self.opt, se.embedding_vec_size)
            h = SparseEmbeddingHash(int(se.embedding_type), B, Be, max_vocab, se.embedding_vec_size,
                                    p.max_feature_num(), p.slot_num, se.combiner, opt,
                                    slot_size_array=ssa, key_dtype=key_dtype,
                                    out_dtype=self.emb_dtype, rank=self.rank, world=self.world,
                                    seed=s.seed, device=self.device)
            h.init_params()
            localized = se.embedding_type == Embedding_t.LocalizedSlotSparseEmbeddingHash
            ex = {}
            for mode, bb in (("train", B), ("eval", Be)):
                ex[mode] = (LocalizedExchange if localized else DistributedExchange)(
                    bb, p.slot_num, se.embedding_vec_size)
            self._emb[se.sparse_embedding_name] = (se, p, h, ex, localized)
            self._shapes[se.sparse_embedding_name] = (p.slot_num, se.embedding_vec_size)
        self._ebc = []
        self._ebc_stacked = {}  # id(config) -> ev of a list-form config that only optimizers split
        for cfg in self.ebc_configs:
            subs = self._split_by_ev_size(cfg)
            if len(subs) == 1:
                subs[0][0].top_name = cfg.top_name
            for sub, ids in subs:
                rt = self._compile_ebc(sub, sp, B, Be, declare_shapes=len(subs) == 1)
                rt.update(parent=cfg, ids=ids, whole=len(subs) == 1)
                self._ebc.append(rt)
            if len(subs) > 1:  # mixed vector sizes: outputs are concatenated in lookup order
                def width(t, bottom, c):  # a multi-hot concat lookup is max_hotness vectors wide
                    h = sp[bottom].max_nnz() if str(c).lower().endswith("concat") else 1
                    return t.ev_size * max(h, 1)
                if cfg.top_name and len(self._split_by_ev_size(cfg, by_optimizer=False)) == 1:
                    # only the tables' optimizers split this config: its output keeps the shape
                    # and type of the unsplit collection's, [batch, lookups, ev] in lookup order
                    ev = cfg.lookups[0][0].ev_size
                    self._ebc_stacked[id(cfg)] = ev
                    self._shapes[cfg.top_name] = (
                        sum(width(t, b, c) for t, b, _, c in cfg.lookups) // ev, ev)
                elif cfg.top_name:
                    self._shapes[cfg.top_name] = (sum(width(t, b, c) for t, b, _, c in cfg.lookups),)
                else:
                    for t, b, top, c in cfg.lookups:
                        self._shapes[top] = (width(t, b, c),)
        # dense modules
        self._mods = torch.nn.ModuleDict()
        self._loss_layer = None
        self._loss_layers = []
        for i, L in enumerate(self.layers):
            self._build_layer(i, L)
        self._mods.to(self.device)
        self._dense_params = [p for p in self._mods.parameters()]
        # solver.use_cuda_graph (graph_wrapper.cpp:30-41, default on): small batches are bound by
        # launch latency, not by kernels -- the dense tower's forward, loss(es), backward and
        # optimizer step are captured once into a HIP graph and replayed (one GPU; legacy
        # embeddings: at most 8192 samples per step -- measured: 1.13 -> 0.51 ms at 1024, no gain
        # at 16384 on DeepFM; models on an embedding_collection: whatever the batch, their towers
        # -- Wide & Deep, MMoE: tens of slices, gates and small MLPs per step -- are launch-bound
        # far beyond that; HCTR_HIP_GRAPH=0 keeps eager launches, =1 captures whatever the model)
        env = os.environ.get("HCTR_HIP_GRAPH", "auto")
        ebc_graph = bool(self.ebc_configs) and not self._emb and all(
            isinstance(rt["train"], EmbeddingCollection) for rt in self._ebc)
        self._graph_ok = (bool(s.use_cuda_graph) and env != "0" and self.world == 1 and
                          len(self._loss_layers) >= 1 and
                          ((not self.ebc_configs and len(self._loss_layers) == 1 and
                            (self.bpg <= 8192 or env == "1")) or
                           (ebc_graph and (self.bpg <= 32768 or env == "1"))))
        # dense Ftrl stays out of the captured step: the capture drops every parameter's .grad,
        # DenseFtrl's gradients live in persistent views (DESIGN.md "Dense-tower glue")
        if Optimizer_t(self.opt.optimizer_type) == Optimizer_t.Ftrl and self._dense_params:
            self._graph_ok = False
        self._graph, self._graph_wait = None, 0
        self._dense_opt = self._make_dense_opt()
        # Model.reader_override: anything with next_batch(train) / has_eval() handing out batches
        # in the readers' layout (data.py) -- bench.py serves batches resident in HBM this way
        self.reader = getattr(self, "reader_override", None) or _data.make_reader(
            self.reader_params, self.input, s, self.rank, self.world, self.device)
        self._gemm_selection = _use_gemm_selection(s)
        # readers that can (Raw) hand every collection its global CSR ready-made (data.RawReader)
        groups = [[p.top_name for p in rt["params"]] for rt in self._ebc]
        for j, rt in enumerate(self._ebc):
            rt["index"] = j
        for r in (getattr(self.reader, "train", None), getattr(self.reader, "evalr", None)):
            if r is not None and hasattr(r, "ebc_groups"):
                r.ebc_groups = groups
        self._plan_execution()
        # evaluation metrics as solver.metrics_spec names them (Model::create_metrics,
        # R/HugeCTR/src/pybind/model_compile.cpp:915-938); the device store is allocated by the
        # first eval()
        self._metrics = EvalMetrics(s.metrics_spec, self.input.label_dim, self.bpg_eval,
                                    s.max_eval_batches, num_loss_layers=len(self._loss_layers),
                                    world=self.world, device=self.device)
        self._compiled = True

    def _plan_execution(self):
        """what the training step may fuse and overlap, decided once from the graph:

        * dense SGD / Ftrl on flat buffers: when every trainable dense tensor lives in a 16-bit
          FusedMLP and the optimizer is SGD (the reference's DLRM configurations) or Ftrl (its
          samples/ftrl; there the finish launch always writes `flat_g` and `hctr_ftrl_shadow`
          takes the step per MLP, after the all-reduce on N > 1), the backward's
          kernels leave their partial sums and ONE launch per step (`hctr_dense_grad_finish`,
          `DenseGradFinish`) finishes every gradient of every MLP: on one GPU straight through the
          SGD step and the refresh of the 16-bit copies; on N > 1 into one flat gradient buffer
          per MLP, on which the data-parallel all-reduce runs as is, then `hctr_sgd_shadow`;
        * logit head: an MLP whose last layer (K -> 1, no activation) feeds only the
          BinaryCrossEntropyLoss computes that layer, the loss and both backward products in one
          pass (`hctr_logit_head`);
        * solver.train_intra_iteration_overlap (model_pipeline.cpp:299-346): on N > 1 GPUs the
          localized embedding's all-to-all is asynchronous -- dense layers that do not read the
          embedding are enqueued under it, the gradient all-to-all starts from inside backward as
          soon as dL/dE exists;
        * solver.train_inter_iteration_overlap: batch i + 1's index stage and exchange plan run on
          a side stream under batch i's dense tower (unique-row payload, `unique_exchange.py`);
        * the payload of the exchange (HCTR_EXCHANGE = rows | unique | unique16 | auto): rows = one
          pooled vector / gradient per (sample, slot), the reference's; unique = every distinct
          row once per destination + per-row gradient sums (one-hot sum lookups only); auto
          (default when both overlaps are on) times both over a few training steps and keeps the
          faster one -- the same decision on every rank."""
        s = self.solver
        consumers: Dict[str, list] = {}
        for i, L in enumerate(self.layers):
            for pos, b in enumerate(L.bottom_names):
                consumers.setdefault(b, []).append((i, pos))
        self._consumers = consumers
        fused_ok = os.environ.get("HCTR_MODEL_FUSED_DENSE", "1") != "0"
        # -- flat dense SGD -----------------------------------------------------------------------
        mlps = [m for m in self._mods.values() if isinstance(m, FusedMLP)]
        in_mlps = sum(sum(q.numel() for q in m.parameters()) for m in mlps)
        total = sum(q.numel() for q in self._dense_params)
        self._flat_mlps = []
        self._flat_ftrl = Optimizer_t(self.opt.optimizer_type) == Optimizer_t.Ftrl
        if (fused_ok and mlps and in_mlps == total and s.use_mixed_precision and
                Optimizer_t(self.opt.optimizer_type) in (Optimizer_t.SGD, Optimizer_t.Ftrl)):
            for m in mlps:
                m.flatten(ftrl_state=self._flat_ftrl)
            self._flat_mlps = mlps
            self._dense_opt = None
            for q in self._dense_params:  # (a DenseFtrl made before the plan left its views there)
                q.grad = None
            # every partial sum the backward's kernels leave is finished by one launch per step
            self._dense_finish = DenseGradFinish(mlps)
        # -- logit head -----------------------------------------------------------------------------
        self._head_layer = None
        if fused_ok and self._loss_layer is not None and s.use_mixed_precision:
            logit_name = self._loss_layer.bottom_names[0]
            for i, L in enumerate(self.layers):
                if (L.layer_type == Layer_t.MLP and L.top_names[0] == logit_name and
                        len(consumers.get(logit_name, [])) == 1 and
                        self._mods[f"l{i}"].can_fuse_bce_head()):
                    self._head_layer = i
        # -- exchange of the localized embeddings on N > 1 GPUs -----------------------------------
        self._intra = bool(s.train_intra_iteration_overlap) and self.world > 1
        self._inter = bool(s.train_inter_iteration_overlap) and self.world > 1
        # one GPU: what the flag still overlaps is the sparse update under the bottom MLP's backward
        self._upd_overlap = bool(s.train_intra_iteration_overlap) and self.world == 1
        # one GPU: the NEXT batch's index stage on a side stream (solver.train_inter_iteration_overlap)
        # HCTR_INDEX_AHEAD (default "0": the index stage stays at the step's start).  Measured on
        # MI355X, DLRM Criteo-1TB shape, round 4 (profiles/r4_index_ahead_ab.txt): "mlp" = under
        # this batch's top MLP: + 1 ms per step -- the probe kernel's waves keep the GEMMs' big
        # workgroups from being placed (the index stage itself 70 -> 260 us); "tail" = behind the
        # sparse update on its side stream, joined by the next step before its gather: 2.215 ->
        # 2.209 ms, inside the noise -- the side stream's chain ends when the next step needs it.
        self._idx_mode = os.environ.get("HCTR_INDEX_AHEAD", "0")
        self._idx_overlap = (bool(s.train_inter_iteration_overlap) and self.world == 1 and
                             self._idx_mode != "0")
        want = os.environ.get("HCTR_EXCHANGE", "auto" if (self._intra and self._inter) else "rows")
        if want not in ("rows", "unique", "unique16", "auto"):
            raise RuntimeError("HCTR_EXCHANGE must be rows, unique, unique16 or auto")
        self._xstate = {}
        for name, (se, p, h, ex, localized) in self._emb.items():
            st = {"mode": "rows", "ux": None, "select": None, "indexed": False, "timing_ms": None,
                  "fused_gather": False, "rows_indexed": False}
            one_hot = p.is_fixed_length and p.max_nnz() == 1
            cons = consumers.get(name, [])
            to_interaction = (len(cons) == 1 and cons[0][1] == 1 and
                              self.layers[cons[0][0]].layer_type == Layer_t.Interaction)
            # one GPU, one key per bucket, the Interaction layer the only reader: the gather rides
            # in the interaction kernel (no second trip of the pooled vectors through HBM)
            # N > 1, rows payload, Interaction the only reader: the interaction reads the
            # all-to-all receive buffer [peer][b][slot in peer][D] through the reorder map and
            # writes the embedding gradients straight in the send layout -- forward_reorder /
            # backward_reorder (a read + a write of the whole [B/N, S, D] tensor each) disappear
            n_ins = p.slot_num + 1
            st["rows_indexed"] = (self.world > 1 and localized and to_interaction and
                                  s.use_mixed_precision and self._intra and
                                  se.embedding_vec_size in (32, 64, 128) and n_ins <= 32 and
                                  (se.embedding_vec_size + n_ins * (n_ins - 1) // 2 + 1) % 8 == 0 and
                                  os.environ.get("HCTR_ROWS_INDEXED", "1") != "0")
            if st["rows_indexed"]:
                st["row_map"] = reorder_row_map(self.bpg, p.slot_num, self.world).to(
                    self.device).contiguous()
            st["fused_gather"] = (self.world == 1 and one_hot and se.combiner == 0 and
                                  to_interaction and s.use_mixed_precision and
                                  se.embedding_vec_size in (16, 32, 64, 128) and p.slot_num <= 31 and
                                  os.environ.get("HCTR_FUSED_GATHER", "1") != "0")
            if (self.world > 1 and localized and one_hot and se.combiner == 0 and
                    want != "rows" and self._intra and
                    (se.embedding_vec_size * (2 if s.use_mixed_precision else 4)) % 16 == 0):
                try:
                    from .unique_exchange import UniqueExchange
                    st["ux"] = UniqueExchange(h, self.bpg, p.slot_num, se.embedding_vec_size)
                except Exception as e:  # e.g. positions x peers beyond the 32-bit sort key
                    if self.rank == 0:
                        print(f"[HCTR][WARNING] unique-row exchange unavailable for {name}: {e!r}")
                if st["ux"] is not None:
                    st["indexed"] = to_interaction and s.use_mixed_precision
                    if want == "auto":
                        st["select"] = {"it": 0, "t0": 0.0, "t": {}}
                    else:
                        self._set_exchange(st, want)
            self._xstate[name] = st
        self._lookahead = None     # (batch i + 1) fetched early for the inter-iteration prefetch
        self._upd_stream = None    # one GPU: the sparse update under the bottom MLP's backward
        self._idx_stream = None    # one GPU: the next batch's index stage (inter-iteration overlap)
        self._idx_ahead = {}       # embedding name -> (the batch indexed ahead, its event)
        self._upd_timing = []      # (overlapped?, (start, end) events) of recent updates
        self._upd_overlap_on = True

    def _set_exchange(self, st, mode: str):
        st["mode"] = mode
        if st["ux"] is not None and mode != "rows":
            st["ux"].set_sum_dtype(self.emb_dtype if mode == "unique16" else torch.float32)

    # iterations of the exchange selection (HCTR_EXCHANGE=auto): the first ones insert most keys
    # (slow whatever the payload), then 3 timed steps of each payload after 2 untimed ones
    _SEL_WARM, _SEL_TIMED, _SEL_SWITCH = 8, 3, 2

    def _select_exchange(self, st):
        """called at the start of every train() while the selection of one embedding's payload is
        running; every step is a real training step (both payloads give the same model up to fp32
        rounding), only the clock reads add host synchronisations -- to 2 x 2 of the first 16"""
        sel = st["select"]
        W, T, S = self._SEL_WARM, self._SEL_TIMED, self._SEL_SWITCH
        it = sel["it"]
        sel["it"] += 1
        marks = {W: ("rows", None), W + T: ("unique", "rows"), W + T + S: ("unique", None),
                 W + 2 * T + S: (None, "unique")}
        if it not in marks:
            return
        nxt, done = marks[it]
        if done is not None or it in (W, W + T + S):
            if st["ux"] is not None:
                st["ux"].drain()
            torch.cuda.synchronize()
        if done is not None:
            sel["t"][done] = time.perf_counter() - sel["t0"]
        if it in (W, W + T + S):
            if dist.is_initialized():
                dist.barrier()
            sel["t0"] = time.perf_counter()
        if nxt is not None:
            self._set_exchange(st, nxt)
            return
        t = torch.tensor([sel["t"]["rows"], sel["t"]["unique"]], dtype=torch.float64)
        if dist.get_backend() != "gloo":
            t = t.to(self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)  # the slowest rank decides, the same on all
        t = t.cpu()
        st["timing_ms"] = {"rows": float(t[0]) / T * 1e3, "unique": float(t[1]) / T * 1e3}
        self._set_exchange(st, "rows" if float(t[0]) <= float(t[1]) else "unique")
        st["select"] = None

    def exchange_report(self) -> dict:
        """per localized embedding: the payload in use, the selection's timings and what this
        rank shipped in the last step (for bench.py's `config.exchange` / `per_rank`)"""
        out = {}
        for name, (se, p, h, ex, localized) in self._emb.items():
            st = self._xstate[name]
            esz = 2 if self.solver.use_mixed_precision else 4
            D = se.embedding_vec_size
            r = {"payload": st["mode"] if self.world > 1 else "none (1 GPU)",
                 "gather_fused_into_interaction": st["fused_gather"],
                 "selection_ms_per_step": st["timing_ms"],
                 "intra_iteration_overlap": self._intra, "inter_iteration_overlap": self._inter}
            if self.world > 1 and localized and st["mode"] == "rows":
                e = ex["train"]
                r["bytes_out_forward"] = (sum(e.send) - e.send[self.rank]) * esz
                r["bytes_out_backward"] = (sum(e.recv) - e.recv[self.rank]) * esz
            elif self.world > 1 and st["ux"] is not None and st["ux"].u_send is not None:
                ux = st["ux"]
                us, ur = ux.u_send, ux.u_recv
                gsz = 2 if st["mode"] == "unique16" else 4
                r.update(distinct_rows_out=sum(us) - us[self.rank], positions=ux.P,
                         bytes_out_forward=(sum(us) - us[self.rank]) * D * esz +
                         (ux.P - ux.P // self.world) * 8,
                         bytes_out_backward=(sum(ur) - ur[self.rank]) * D * gsz)
            out[name] = r
        # collections under CompressionStrategy.Unique: what this rank shipped in the last step
        for i, rt in enumerate(getattr(self, "_ebc", [])):
            e = rt["train"]
            if getattr(e, "_unique", False):
                r = {"payload": "unique rows", "tables": [t.name for t in e.tables]}
                r.update(e.last_exchange or {})
                out[f"embedding_collection{i}"] = r
        return out

    def _split_by_ev_size(self, cfg: EmbeddingCollectionConfig, by_optimizer: bool = True):
        """the runtime keeps one vector size per collection: lookups of a config that mixes sizes
        (wide 1 + deep 16 ...) run as one collection per size, each with the parent's placement.
        Likewise one optimizer per collection: tables whose resolved optimizers (their opt_params,
        else the model's) differ in type or in a hyper-parameter that type reads run as separate
        collections (embedding_collection.group_lookups_by_optimizer; the reference refuses such a
        group, embedding_table.cpp:40-45)."""
        opt_groups = group_lookups_by_optimizer(cfg.lookups, getattr(self, "opt", None)) \
            if by_optimizer else [(list(range(len(cfg.lookups))), None)]
        opt_of = {l: g for g, (ids, _) in enumerate(opt_groups) for l in ids}
        dp_names = set()
        if isinstance(cfg.shard_strategy, (list, tuple)):
            for kind, names in cfg.shard_strategy:
                if str(kind).lower() == "dp":
                    dp_names.update(str(n) for n in names)
        # dynamic tables cannot be replicated (they grow independently): keep them model parallel
        dp_names = {n for n in dp_names
                    if all(t.max_vocabulary_size >= 0 for t, _, _, _ in cfg.lookups if t.name == n)}
        sizes = sorted({t.ev_size for t, _, _, _ in cfg.lookups})
        # one collection is one model-parallel operator (one grouped_lookup_params entry of the
        # reference, R/HugeCTR/embedding/common.cpp:366-399): tables under
        # CompressionStrategy.Unique and under Reduction run as separate collections, and every
        # sub-config carries its tables' strategy
        # (one GPU: nothing travels, the direct path serves both, nothing is split)
        comp = (getattr(cfg, "compression", None) or {}) if self.world > 1 else {}
        strategies = sorted({comp.get(t.name, "reduction") for t, _, _, _ in cfg.lookups
                             if t.name not in dp_names})
        # one collection has one storage: hybrid tables (var_type="hybrid": bounded, LRU eviction,
        # optionally tiered to host memory) form sub-collections of their own; static and dynamic
        # tables are grouped as before -- a hybrid table does not turn its neighbours hybrid
        def kind(t):
            return "hybrid" if getattr(t, "var_type", None) == "hybrid" else "plain"
        kinds = sorted({kind(t) for t, _, _, _ in cfg.lookups if t.name not in dp_names})
        if len(sizes) == 1 and not dp_names and len(strategies) <= 1 and len(kinds) <= 1 and \
                len(opt_groups) == 1:
            return [(cfg, list(range(len(cfg.lookups))))]
        tables = []
        for t, _, _, _ in cfg.lookups:
            if t not in tables:
                tables.append(t)
        own = cfg.ownership(tables, self.world)
        out = []
        groups = range(len(opt_groups))
        # replicated ("dp") tables: one data-parallel collection per vector size (and optimizer)
        for ev, og in [(e, g) for e in sizes for g in groups]:
            ids = [l for l, (t, _, _, _) in enumerate(cfg.lookups)
                   if t.ev_size == ev and t.name in dp_names and opt_of[l] == og]
            if ids:
                sub = EmbeddingCollectionConfig()
                sub.lookups = [cfg.lookups[l] for l in ids]
                sub.shard_strategy = "dp"
                out.append((sub, ids))
        for ev, strategy, knd, og in [(e, k, q, g) for e in sizes for k in strategies
                                      for q in kinds for g in groups]:
            ids = [l for l, (t, _, _, _) in enumerate(cfg.lookups)
                   if t.ev_size == ev and t.name not in dp_names and opt_of[l] == og and
                   comp.get(t.name, "reduction") == strategy and kind(t) == knd]
            if not ids:
                continue
            sub = EmbeddingCollectionConfig()
            sub.lookups = [cfg.lookups[l] for l in ids]
            full = getattr(cfg, "compression", None) or {}
            sub.compression = {t.name: full[t.name] for t, _, _, _ in sub.lookups if t.name in full}
            sub_tables = []
            for t, _, _, _ in sub.lookups:
                if t not in sub_tables:
                    sub_tables.append(t)
            sub.shard_matrix = [[int(own[g][tables.index(t)]) for t in sub_tables]
                                for g in range(self.world)]
            if any(not any(row[c] for row in sub.shard_matrix) for c in range(len(sub_tables))):
                raise RuntimeError("embedding_collection: a table has no owner")
            out.append((sub, ids))
        return out

    def _compile_ebc(self, cfg: EmbeddingCollectionConfig, sp, B, Be, declare_shapes=True):
        """embedding_collection of the model (R/HugeCTR/src/pybind/add_embedding_collection.cpp):
        one runtime for the training batch, one for the evaluation batch, sharing the tables"""
        # (_split_by_ev_size: the tables of a sub-config resolve to one optimizer, checked by
        #  check_embedding_collection_config; the learning rate stays the model's)
        o, _ = resolve_table_optimizer(cfg.lookups[0][0], self.opt)
        # (the optimizer is one this kind of table runs: check_embedding_collection_config;
        #  Optimizer_t's values are the library's codes)
        code = int(o.optimizer_type)
        dynamic = any(tc.max_vocabulary_size < 0 for tc, _, _, _ in cfg.lookups)
        # (_split_by_ev_size: a sub-config is hybrid as a whole or not at all)
        hybrid = any(getattr(tc, "var_type", None) == "hybrid" for tc, _, _, _ in cfg.lookups)
        params, offsets = [], []
        slot0, slot_of_param = 0, {}
        for p in self.input.sparse_params:
            slot_of_param[p.top_name] = slot0
            slot0 += p.slot_num
        ssa = list(self.reader_params.slot_size_array or [])
        cum = np.concatenate([[0], np.cumsum(ssa)]).astype(np.int64) if ssa else None
        for _, bottom, _, _ in cfg.lookups:
            p = sp[bottom]
            if p.slot_num != 1:
                raise RuntimeError("embedding_collection inputs carry one slot per lookup "
                                   "(DataReaderSparseParam(name, hotness, fixed, 1))")
            params.append(p)
            # the readers add cumulative slot offsets for the legacy embeddings; tables of a
            # collection are indexed by the raw key
            offsets.append(int(cum[slot_of_param[bottom]]) if cum is not None else 0)
        hot = max(p.max_nnz() for p in params)
        kw = dict(lr=self._lr, optimizer=code, scaler=self.solver.scaler, epsilon=o.epsilon,
                  initial_accu_value=o.initial_accu_value, out_dtype=self.emb_dtype,
                  batch_major=True, max_hotness=hot, seed=self.solver.seed,
                  ftrl=(o.lambda1, o.lambda2, o.beta))
        ekw = dict(kw, hotness=[p.max_nnz() for p in params])  # multi-hot concat lookups
        if hybrid or dynamic:  # (capacity, tier and initializer travel in the table configs)
            # (CreateOptimizer has no argument of its own for RMSProp's beta: beta2 is passed)
            ekw.update(beta1=o.beta1, beta2=o.beta2, momentum_factor=o.momentum_factor,
                       rmsprop_beta=o.beta2)
        if cfg.shard_strategy == "dp":  # replicated tables: no all-to-all, gradient all-reduce
            dkw = {k: v for k, v in kw.items() if k != "batch_major"}
            train = DataParallelCollection(cfg, B, **dkw)
            ev = None
            if Be > 0:
                ev = train if Be == B else DataParallelCollection(cfg, Be, **dkw)
                ev.table, ev.accum, ev.ftrl_z = train.table, train.accum, train.ftrl_z
            L, evs = train.L, train.ev
            if declare_shapes:
                if cfg.top_name:
                    self._shapes[cfg.top_name] = (L, evs)
                else:
                    for _, _, top, _ in cfg.lookups:
                        self._shapes[top] = (evs,)
            return dict(cfg=cfg, train=train, eval=ev, params=params,
                        offsets=torch.tensor(offsets, dtype=torch.int64, device=self.device))
        train = EmbeddingCollection(cfg, B, **ekw)
        ev = None
        if Be > 0:
            # same tables, own per-batch scratch
            ev = train if (Be == B and not dynamic) else EmbeddingCollection(
                cfg, Be, tables_from=train, **ekw)
            if ev is not train and dynamic:
                # evaluation never inserts: unseen keys read as zeros (dynamic tables) or as the
                # initializer's value (hybrid tables)
                ev.training = False
        L, evs = train.L, train.ev  # (L counts a multi-hot concat lookup once per key slot)
        if declare_shapes:
            if cfg.top_name:
                self._shapes[cfg.top_name] = (L, evs)
            else:
                for (_, _, top, _), (_, reps) in zip(cfg.lookups, train.virt_span):
                    self._shapes[top] = (reps * evs,)
        return dict(cfg=cfg, train=train, eval=ev, params=params,
                    offsets=torch.tensor(offsets, dtype=torch.int64, device=self.device))

    def _ebc_forward(self, rt, batch, train: bool) -> torch.Tensor:
        """global feature-major CSR of the collection's lookups -> [batch/world, lookups, ev]"""
        e = rt["train"] if train else rt["eval"]
        pre = batch.get("ebc")
        if pre is not None:  # the reader built the collection's CSR (raw keys) on the host
            gk, gbr = pre[rt["index"]]
            if isinstance(e, DataParallelCollection):
                return e.forward(gk, gbr)
            return e.forward_global(gk, gbr)
        ros, keys = [], []
        for p in rt["params"]:
            ro, k = batch["sparse"][p.top_name]
            ros.append(ro.to(torch.int64))
            keys.append(k.to(torch.int64))
        ends = torch.stack([r[-1] for r in ros])
        base = torch.cumsum(ends, 0) - ends                      # first key of every lookup
        gbr = torch.cat([r[:-1] + base[l] for l, r in enumerate(ros)] + [ends.sum().view(1)])
        gk = torch.cat([k - rt["offsets"][l] for l, k in enumerate(keys)])
        if isinstance(e, DataParallelCollection):
            return e.forward(gk, gbr)
        return e.forward_global(gk, gbr)

    def _ebc_begin(self, rt, batch, train: bool, after):
        """starts the forward of one collection; returns a (memoising) function that hands out its
        output [batch/world, lookups, ev] -- for training a leaf whose gradient `after` consumes.
        N > 1 GPUs + train_intra_iteration_overlap: the all-to-all of the pooled vectors is
        asynchronous and waited for by the first dense layer that reads the output, the gradient
        all-to-all starts from inside backward."""
        e = rt["train"] if train else rt["eval"]
        box = {}
        use_async = (train and self._intra and isinstance(e, EmbeddingCollection) and
                     not e._direct and batch.get("ebc") is not None)
        if not use_async:
            E = self._ebc_forward(rt, batch, train)
            if train:
                E = E.detach().requires_grad_(True)

                def finish(E=E):
                    rt["train"].lr = self._lr
                    rt["train"].backward_and_update(E.grad.contiguous())
                after.append(finish)
            return lambda: E
        gk, gbr = batch["ebc"][rt["index"]]
        recv, work, keep = e.forward_global_begin(gk, gbr)

        def on_grad(g):
            box["back"] = e.backward_begin(g.contiguous())

        def get_E():
            if "E" not in box:
                box["E"] = e.forward_global_finish(recv, work).detach().requires_grad_(True)
                box["E"].register_hook(on_grad)
                box["keep"] = keep
            return box["E"]

        def finish():
            e.lr = self._lr
            if "back" not in box:  # the gradient hook never fired (output unused by the loss)
                box.clear()
                return
            top, w, _ = box.pop("back")
            e.backward_finish(top, w)
        after.append(finish)
        return get_E

    def _in_width(self, name):
        shp = self._shapes[name]
        n = 1
        for v in shp:
            n *= v
        return n

    def _build_layer(self, i, L: DenseLayer):
        t = L.layer_type
        key = f"l{i}"
        b0 = L.bottom_names[0]
        if t == Layer_t.InnerProduct:
            self._mods[key] = torch.nn.Linear(self._in_width(b0), L.num_output)
            self._shapes[L.top_names[0]] = (L.num_output,)
        elif t == Layer_t.MLP:
            dims = [self._in_width(b0)] + list(L.num_outputs)
            acts = L.activations or [L.act_type] * len(L.num_outputs)
            last_relu = acts[-1] == Activation_t.Relu
            self._mods[key] = FusedMLP(dims, last_relu,
                                       # use_mixed_precision = the reference's fp16 mode
                                       # (solver_wrapper.hpp:127-150: __half layers + loss scaler)
                                       dtype=torch.float16 if self.solver.use_mixed_precision
                                       else torch.float32)
            self._shapes[L.top_names[0]] = (dims[-1],)
        elif t in (Layer_t.ReLU, Layer_t.Sigmoid, Layer_t.Dropout, Layer_t.Softmax, Layer_t.ELU):
            self._shapes[L.top_names[0]] = self._shapes[b0]
        elif t == Layer_t.Concat:
            self._shapes[L.top_names[0]] = (sum(self._in_width(b) for b in L.bottom_names),)
        elif t == Layer_t.Reshape:
            if L.selected_slots:
                vec = self._shapes[b0][-1]
                self._shapes[L.top_names[0]] = (len(L.selected_slots) * vec,)
            elif L.shape:
                self._shapes[L.top_names[0]] = tuple(int(v) for v in L.shape[1:])
            else:
                self._shapes[L.top_names[0]] = (L.leading_dim,)
        elif t == Layer_t.Slice:
            for (a, b), top in zip(L.ranges, L.top_names):
                self._shapes[top] = (b - a,)
        elif t in (Layer_t.Add, Layer_t.ElementwiseMultiply, Layer_t.Sub):
            self._shapes[L.top_names[0]] = self._shapes[b0]
        elif t == Layer_t.FmOrder2:
            self._mods[key] = _FmOrder2(L.out_dim)
            self._shapes[L.top_names[0]] = (L.out_dim,)
        elif t == Layer_t.WeightMultiply:
            self._mods[key] = _WeightMultiply(int(L.weight_dims[0]), int(L.weight_dims[1]))
            self._shapes[L.top_names[0]] = (int(L.weight_dims[0]) * int(L.weight_dims[1]),)
        elif t == Layer_t.ReduceSum:
            self._shapes[L.top_names[0]] = (1,)
        elif t == Layer_t.MultiCross:
            w = self._in_width(b0)
            self._mods[key] = MultiCrossLayer(w, L.num_layers, L.projection_dim)
            self._shapes[L.top_names[0]] = (w,)
        elif t == Layer_t.Interaction:
            n_emb, W = self._shapes[L.bottom_names[1]]
            n_ins = n_emb + 1
            self._shapes[L.top_names[0]] = (W + n_ins * (n_ins - 1) // 2 + 1,)
        elif t == Layer_t.Scale:
            n = self._in_width(b0)
            self._shapes[L.top_names[0]] = (n * int(L.factor),)
        elif t == Layer_t.BinaryCrossEntropyLoss:
            self._loss_layer = L
            self._loss_layers = getattr(self, "_loss_layers", []) + [L]
        else:
            raise RuntimeError(f"Layer_t.{t.name} is outside the hot-path scope of hugectr_amd")

    def _make_dense_opt(self):
        o, lr = self.opt, self._lr
        t = Optimizer_t(o.optimizer_type)
        if not self._dense_params:
            return None
        if t == Optimizer_t.Adam:
            kw = dict(lr=lr, betas=(o.beta1, o.beta2), eps=o.epsilon,
                      capturable=bool(getattr(self, "_graph_ok", False)))
            # one multi-tensor launch for the whole step instead of ~ 25 (a small-batch step is a
            # chain of 5 us launches: BASELINE configs[0] spends 150 of its 510 us in them);
            # HCTR_FUSED_ADAM=0 keeps the per-operation form
            if os.environ.get("HCTR_FUSED_ADAM", "1") != "0":
                try:
                    return torch.optim.Adam(self._dense_params, fused=True, **kw)
                except (RuntimeError, TypeError, ValueError):
                    pass
            return torch.optim.Adam(self._dense_params, **kw)
        if t == Optimizer_t.AdaGrad:
            return torch.optim.Adagrad(self._dense_params, lr=lr,
                                       initial_accumulator_value=o.initial_accu_value, eps=o.epsilon)
        if t == Optimizer_t.MomentumSGD:
            return torch.optim.SGD(self._dense_params, lr=lr, momentum=o.momentum_factor)
        if t == Optimizer_t.Nesterov:
            return torch.optim.SGD(self._dense_params, lr=lr, momentum=max(o.momentum_factor, 1e-6),
                                   nesterov=True)
        if t == Optimizer_t.Ftrl:  # torch has none: this library's own (dense.DenseFtrl)
            return DenseFtrl(self._dense_params, lr=lr, beta=o.beta, lambda1=o.lambda1,
                             lambda2=o.lambda2, scaler=self.solver.scaler)
        return torch.optim.SGD(self._dense_params, lr=lr)

    # -- execution ---------------------------------------------------------------------------------
    def _forward_dense(self, tensors: Dict[str, torch.Tensor], train: bool, head=None):
        """the dense layers in graph order.  head = (label, grad_scale) lets the MLP that feeds
        only the loss run its logit layer + BinaryCrossEntropyLoss + their backward as one pass;
        returns (logit or None, fused loss or None)"""
        logit, fused_loss = None, None
        logits = tensors.setdefault("__logits__", [])
        for i, L in enumerate(self.layers):
            t, key = L.layer_type, f"l{i}"
            if t == Layer_t.BinaryCrossEntropyLoss and fused_loss is not None:
                continue  # (the logit never existed as a tensor)
            x = [tensors[b] for b in L.bottom_names]
            if t == Layer_t.MLP and head is not None and i == self._head_layer:
                fused_loss = self._mods[key].forward_bce(x[0].reshape(x[0].shape[0], -1), *head)
                continue
            if t == Layer_t.MultiCross and self._mods[key].projection_dim > 0:
                # v2 in the activations' own type: under use_mixed_precision the reference's
                # MultiCrossLayer<__half> runs its GEMMs in fp16 (multi_cross_layer.cu:1023-1114)
                y = self._mods[key](x[0].reshape(x[0].shape[0], -1))
            elif t in (Layer_t.InnerProduct, Layer_t.MLP, Layer_t.MultiCross, Layer_t.FmOrder2):
                y = self._mods[key](x[0].reshape(x[0].shape[0], -1).float()
                                    if t != Layer_t.MLP else x[0].reshape(x[0].shape[0], -1))
            elif t == Layer_t.WeightMultiply:
                y = self._mods[key](x[0].reshape(x[0].shape[0], -1).float())
            elif t == Layer_t.ReLU:
                y = torch.relu(x[0])
            elif t == Layer_t.Sigmoid:
                y = torch.sigmoid(x[0])
            elif t == Layer_t.Softmax:
                y = torch.softmax(x[0].float(), dim=-1)
            elif t == Layer_t.ELU:
                y = torch.nn.functional.elu(x[0], L.elu_alpha)
            elif t == Layer_t.Scale:
                y = _ScaleFn.apply(x[0].reshape(x[0].shape[0], -1), int(L.axis), int(L.factor))
            elif t == Layer_t.Dropout:
                y = torch.nn.functional.dropout(x[0], L.dropout_rate, training=train)
            elif t == Layer_t.Concat:
                # (inputs of one type keep it -- under use_mixed_precision the tower stays fp16
                #  between layers as the reference's __half layers do; mixed inputs: fp32)
                same = all(v.dtype == x[0].dtype for v in x)
                y = torch.cat([v.reshape(v.shape[0], -1) if same else
                               v.reshape(v.shape[0], -1).float() for v in x], dim=1)
            elif t == Layer_t.Reshape:
                if L.selected_slots:
                    y = x[0][:, list(L.selected_slots), :].reshape(x[0].shape[0], -1)
                elif L.shape:
                    y = x[0].reshape([x[0].shape[0]] + [int(v) for v in L.shape[1:]])
                else:
                    y = x[0].reshape(-1, L.leading_dim)
            elif t == Layer_t.Slice:
                for (a, b), top in zip(L.ranges, L.top_names):
                    tensors[top] = x[0][:, a:b]
                continue
            elif t == Layer_t.Add:
                y = sum(v.float() for v in x)
            elif t == Layer_t.Sub:
                y = x[0].float() - x[1].float()
            elif t == Layer_t.ElementwiseMultiply:
                y = x[0]
                for v in x[1:]:
                    y = y * v
            elif t == Layer_t.ReduceSum:
                y = x[0].sum(dim=L.axis, keepdim=True)
            elif t == Layer_t.Interaction:
                if isinstance(x[1], _GatherEmb):
                    e = x[1]
                    y = interaction_gather(x[0].to(e.emb.out_dtype).contiguous(), e.emb, e.train,
                                           on_emb_grad=e.on_grad, store_pooled=not regather_supported(
                                               e.emb.embedding_vec_size, e.emb.slot_num))
                    if e.after_forward is not None:
                        e.after_forward()
                elif isinstance(x[1], _IndexedEmb):
                    e = x[1]
                    y = interaction_indexed(x[0].to(e.rows.dtype).contiguous(), e.rows, e.row_of,
                                            on_emb_grad=e.on_grad, scatter_grad=e.scatter)
                else:
                    dt = x[1].dtype
                    y = interaction(x[0].to(dt).contiguous(), x[1].contiguous())
            elif t == Layer_t.BinaryCrossEntropyLoss:
                if fused_loss is None:
                    logit = x[0].float()
                    logits.append((L, x[0], x[1]))
                continue
            else:
                raise RuntimeError(t)
            tensors[L.top_names[0]] = y
        return logit, fused_loss

    def _overlap_update_now(self) -> bool:
        """one GPU: should this step's sparse update run under the bottom MLP's backward?  The two
        share the chip, which pays while the update is about as long as that backward (power-law
        keys: 0.27 ms next to 0.22 ms, - 65 us per step) and costs dearly when it is a long
        bandwidth-bound kernel (uniform keys over big tables: 2 GB of row read-modify-writes --
        the dense kernels beside it were measured at 10-16 x their own time, + 1.6 ms per step).
        auto: the update's own duration, taken with events two or more steps back (never waited
        for), switches the mode with hysteresis -- above 0.6 ms overlapped -> in line, below
        0.35 ms in line -> overlapped."""
        mode = os.environ.get("HCTR_UPDATE_OVERLAP", "auto")
        if mode == "0":
            return False
        if mode == "1":
            return True
        q = self._upd_timing
        while len(q) > 1 or (q and q[0][1][1].query()):
            was_overlapped, (e0, e1) = q.pop(0)
            if not e1.query():  # (older than the newest and still running: cannot be; skip)
                continue
            ms = e0.elapsed_time(e1)
            if was_overlapped and ms > 0.6:
                self._upd_overlap_on = False
            elif not was_overlapped and ms < 0.35:
                self._upd_overlap_on = True
        return self._upd_overlap_on

    def _emb_forward(self, name, batch, nxt, train: bool, tensors, leaves, after):
        """forward of one legacy embedding into `tensors[name]`; `after` collects what has to run
        once backward is through (wait for the gradient exchange, backward + sparse update)"""
        se, p, h, ex, localized = self._emb[name]
        st = self._xstate[name]
        mode = "train" if train else "eval"
        bpg = self.bpg if train else self.bpg_eval
        S, D, W = p.slot_num, se.embedding_vec_size, self.world
        ro, keys = batch["sparse"][se.bottom_name]
        if st["fused_gather"]:
            # (the fused kernel indexes value_index as [sample][slot]: one key per bucket, which the
            #  reader's static parameters promise -- a batch of another size is refused here)
            if keys.numel() != bpg * S or ro.numel() != bpg * S + 1:
                raise RuntimeError(
                    f"{name}: fixed-length one-hot input declared (is_fixed_length, max_nnz 1) but the "
                    f"batch holds {keys.numel()} keys for {bpg * S} buckets")
            ahead = self._idx_ahead.pop(name, None) if train else None
            if ahead is not None and ahead[0] is batch:
                # this batch's rows were resolved under the previous step's top MLP
                h.index_adopt()
                torch.cuda.current_stream().wait_event(ahead[1])
            else:
                if ahead is not None:  # (another batch than the one indexed ahead: drop that)
                    torch.cuda.current_stream().wait_event(ahead[1])
                h.index(train, ro, keys)
            launch_ahead = None
            if (train and self._idx_overlap and nxt is not None and
                    nxt["sparse"][se.bottom_name][1].numel() == bpg * S):
                def launch_ahead(nxt=nxt):
                    # behind this batch's index stage AND its gather (both memory-bound), under
                    # the top MLP's GEMMs; the hash table is the only state the two batches share
                    if self._idx_stream is None:
                        self._idx_stream = torch.cuda.Stream()
                    side = self._idx_stream
                    side.wait_stream(torch.cuda.current_stream())
                    nro, nkeys = nxt["sparse"][se.bottom_name]
                    with torch.cuda.stream(side):
                        h.index_ahead(nro, nkeys)
                        ev = torch.cuda.Event()
                        ev.record()
                    self._idx_ahead[name] = (nxt, ev)
            got = {}
            if train and self._upd_overlap and self._overlap_update_now():
                # The sparse update needs the embedding's top gradient only, and the Interaction
                # layer's backward hands that over BEFORE the bottom MLP's backward runs -- a chain
                # of small kernels that leaves most of the chip idle.  The update starts from the
                # gradient hook on a side stream (ordered behind the kernel that produced the
                # gradient) and the step joins it before the dense optimizer step
                # (solver.train_intra_iteration_overlap; HCTR_UPDATE_OVERLAP=0: in line, 1: always,
                # auto: see _overlap_update_now).
                if self._upd_stream is None:
                    self._upd_stream = torch.cuda.Stream()
                side = self._upd_stream
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

                tail = launch_ahead is not None and self._idx_mode == "tail"

                def on_grad(g):
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        ev[0].record()
                        h.backward(g)
                        h.update_params()
                        ev[1].record()
                        if tail:
                            # the next batch's index stage right behind the update: the step no
                            # longer joins the side stream at its end -- the next step waits for
                            # this event before it reads rows or table (adoption, _drain_prefetch)
                            nro, nkeys = nxt["sparse"][se.bottom_name]
                            h.index_ahead(nro, nkeys)
                            eva = torch.cuda.Event()
                            eva.record()
                            self._idx_ahead[name] = (nxt, eva)
                    got["g"] = g  # (alive until the join: the allocator cannot hand it out before)

                def finish():
                    ran = "g" in got
                    if tail and name in self._idx_ahead:
                        got["keep"] = got.pop("g", None)  # (until the next step has joined)
                        self._upd_keep = got
                    else:
                        got.clear()
                        torch.cuda.current_stream().wait_stream(side)
                    # (events of a step whose gradient hook never fired -- the embedding's output
                    #  does not reach the loss -- were never recorded: not a timing sample)
                    if ran:
                        self._upd_timing.append((True, ev))
                tensors[name] = _GatherEmb(h, train, on_grad,
                                           None if tail else launch_ahead)
                after.append(finish)
                return
            if train and self._upd_overlap:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

                def finish():
                    ev[0].record()
                    h.backward(got.pop("g"))
                    h.update_params()
                    ev[1].record()
                    self._upd_timing.append((False, ev))
                tensors[name] = _GatherEmb(h, train, lambda g: got.__setitem__("g", g),
                                           launch_ahead if self._idx_mode == "mlp" else None)
                after.append(finish)
                return
            tensors[name] = _GatherEmb(h, train, (lambda g: got.__setitem__("g", g)) if train
                                       else None, launch_ahead if self._idx_mode == "mlp" else None)
            if train:
                def finish():
                    h.backward(got.pop("g"))
                    h.update_params()
                after.append(finish)
            return
        if not train or W == 1 or not localized or not self._intra:
            # one GPU, evaluation, the distributed embedding, or no intra-iteration overlap asked
            # for: blocking collectives, in line
            pooled = h.forward(train, ro, keys)
            if localized:
                recv = ex[mode].forward(pooled)
                E = forward_reorder(recv, bpg, S, D, W) if W > 1 else pooled.view(bpg, S, D)
            else:
                # reduce-scatter of the partial sums, then the mean's division by the bucket's
                # key count over all GPUs (a no-op unless distributed + mean + world > 1)
                E = h.forward_scale(train, ex[mode].forward(pooled).contiguous())
            if train:
                E = E.detach().requires_grad_(True)
                leaves[name] = E

                def finish(E=E):
                    g = E.grad
                    if os.environ.get("HCTR_DEBUG_LOSS_CURVE"):
                        self._last_emb_grad = g.detach().clone()
                    if localized and W > 1:
                        g = backward_reorder(g.contiguous(), bpg, S, D, W)
                    top = ex["train"].backward(g.contiguous())
                    h.backward(top.contiguous())
                    h.update_params()
                after.append(finish)
            tensors[name] = E
            return
        if st["mode"] != "rows":
            # unique-row payload: every distinct row once per destination, per-row gradient sums
            # back; the next batch's index stage + plan + count exchange on a side stream
            ux = st["ux"]
            ux.forward_begin(ro, keys)
            nk = nxt["sparse"][se.bottom_name] if (nxt is not None and self._inter) else None

            def resolve():
                if st["indexed"]:
                    rows, row_of = ux.forward_finish(indexed=True)
                    E = _IndexedEmb(rows, row_of, ux.backward_begin)
                else:
                    E = ux.forward_finish().detach().requires_grad_(True)
                    E.register_hook(lambda g: ux.backward_begin(g))
                if nk is not None:  # after this batch's row all-to-all: the communicator serves
                    ux.prefetch(*nk)  # the critical-path transfer first
                return E
            tensors[name] = _Pending(resolve)
            after.append(ux.backward_finish)
            return
        # rows payload, asynchronous: the reference's all-to-all of pooled vectors / top gradients
        pooled = h.forward(True, ro, keys)
        e = ex["train"]
        recv, work = e.forward_async(pooled)
        top_grad = torch.empty_like(pooled)
        sent = {}

        def on_grad(g):
            # inside backward, right behind the consumer's backward kernel; must not keep `g`
            gsend = backward_reorder(g.contiguous(), bpg, S, D, W)
            sent["work"] = e.backward_async(gsend, top_grad.view(-1))
            sent["buf"] = gsend  # stays alive until the collective has read it

        def on_rows_grad(gsend):  # already in the send layout (scatter through the reorder map)
            sent["work"] = e.backward_async(gsend.view(-1), top_grad.view(-1))
            sent["buf"] = gsend

        def resolve():
            if work is not None:
                work.wait()
            if st["rows_indexed"]:
                return _IndexedEmb(recv.view(-1, D), st["row_map"], on_rows_grad, scatter=True)
            E = forward_reorder(recv, bpg, S, D, W).requires_grad_(True)
            E.register_hook(on_grad)
            return E

        def finish():
            if "work" not in sent:  # no gradient arrived (the output does not reach the loss):
                return              # nothing to exchange, nothing to update
            if sent.get("work") is not None:
                sent["work"].wait()
            sent.clear()
            h.backward(top_grad)
            h.update_params()
        tensors[name] = _Pending(resolve)
        after.append(finish)

    def _ebc_tensors(self, tensors, rt, get_E):
        """names the dense layers read -> (lazily resolved) pieces of one collection's output
        [batch, lookups, ev], handed out by get_E()"""
        cfg = rt["parent"]
        span = getattr(rt["train"], "virt_span", None)

        parts = {}  # E.unbind(1), taken once: ONE backward node (a stack) for all one-vector
                    # lookups instead of a zero-fill + add of the whole output per lookup

        def piece(v0, reps, as_float=False):
            def resolve():
                E = get_E()
                if reps == 1:
                    if "u" not in parts:
                        parts["u"] = E.unbind(1)
                    x = parts["u"][v0]
                else:
                    x = E[:, v0:v0 + reps, :].reshape(E.shape[0], -1)
                return x.float() if as_float else x
            return _Pending(resolve)
        if rt["whole"]:
            if cfg.top_name:
                tensors[cfg.top_name] = _Pending(get_E)
            else:
                for l, (_, _, top, _) in enumerate(cfg.lookups):
                    v0, reps = span[l] if span else (l, 1)
                    tensors[top] = piece(v0, reps)
        else:  # one of several collections of a mixed-size config
            for j, l in enumerate(rt["ids"]):
                v0, reps = span[j] if span else (j, 1)
                if cfg.top_name:
                    tensors[(id(cfg), l)] = piece(v0, reps,
                                                  as_float=id(cfg) not in self._ebc_stacked)
                else:
                    tensors[cfg.lookups[l][2]] = piece(v0, reps)

    def _ebc_concat_tops(self, tensors):
        for cfg in self.ebc_configs:
            if cfg.top_name and dict.__contains__(tensors, (id(cfg), 0)):
                n = len(cfg.lookups)
                ev = self._ebc_stacked.get(id(cfg))

                def resolve(cfg=cfg, n=n, ev=ev):
                    x = torch.cat([tensors[(id(cfg), l)] for l in range(n)], dim=1)
                    return x if ev is None else x.view(x.shape[0], -1, ev)
                tensors[cfg.top_name] = _Pending(resolve)

    def _multi_task_loss(self, tensors):
        """weighted sum of the tasks' losses + every task's scores side by side"""
        total, probs = None, []
        for L, lg, lab in tensors["__logits__"]:
            w = self._loss_weights.get(L.bottom_names[1], 1.0)
            li = torch.nn.functional.binary_cross_entropy_with_logits(lg.float(), lab.float())
            total = li * w if total is None else total + li * w
            probs.append(torch.sigmoid(lg.float()))
        return total, probs

    def _run_batch(self, batch, train: bool, nxt=None):
        tensors = _Tensors({self.input.dense_name: batch["dense"]})
        off = 0
        for n, d in zip(self.input.label_names, self.input.label_dims):
            tensors[n] = batch["label"] if len(self.input.label_names) == 1 else \
                batch["label"][:, off:off + d]
            off += d
        leaves, after = {}, []
        for name in self._emb:
            self._emb_forward(name, batch, nxt, train, tensors, leaves, after)
        for i, rt in enumerate(self._ebc):
            self._ebc_tensors(tensors, rt, self._ebc_begin(rt, batch, train, after))
        self._ebc_concat_tops(tensors)
        label = batch["label"].float()
        # the logit gradient is (sigmoid - y) * scaler / batch_per_gpu / total_gpu_count
        # (BinaryCrossEntropy_Kernel, R/HugeCTR/src/loss.cu:242-249): every gradient below --
        # the embeddings' top gradients included -- is a share of the GLOBAL-batch mean, and the
        # dense all-reduce is a plain sum
        gscale = self.solver.scaler / (max(self.bpg, 1) * self.world)
        head = (label, gscale) if (train and self._head_layer is not None and
                                   label.shape[1] == 1) else None
        multi = len(self._loss_layers) > 1
        if multi:
            head = None
        logit, loss = self._forward_dense(tensors, train, head)
        if multi:
            # weighted sum of the tasks' losses; evaluation scores = every task's, side by side
            total, probs = self._multi_task_loss(tensors)
            if not train:
                return total, torch.cat(probs, dim=1)
            (total * (self.solver.scaler / self.world)).backward()
            loss = total
        elif not train:
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, label)
            return loss, torch.sigmoid(logit)
        elif loss is not None:      # logit layer + loss + their backward already done in one pass
            loss.backward(self._unit_grad(loss))
        elif logit.is_cuda and label.shape == logit.shape:
            # fused BCE forward + logit gradient (two launches instead of ~20)
            lg = tensors[self._loss_layer.bottom_names[0]]
            loss, dlogit = bce_with_logits(lg, label, gscale)
            lg.backward(dlogit)
        else:
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, label)
            (loss * (self.solver.scaler / self.world)).backward()
        # the dense gradients' all-reduce (N > 1) runs on the communicator's stream under the
        # embeddings' backward + sparse update
        works = self._dense_reduce_begin()
        for fin in after:
            fin()
        self._dense_step(reduced=works)
        return loss.detach().reshape(()), None

    # -- HIP-graph replay of the dense tower (solver.use_cuda_graph) ---------------------------------
    def _graph_dense(self, G, skip_step: bool):
        """forward of the dense layers on the graph's static inputs, loss, backward, optimizer step"""
        tensors = _Tensors({self.input.dense_name: G["dense"]})
        off = 0
        for n, d in zip(self.input.label_names, self.input.label_dims):
            tensors[n] = G["label"] if len(self.input.label_names) == 1 else \
                G["label"][:, off:off + d]
            off += d
        for name, (se, p, h, ex, localized) in self._emb.items():
            if self._xstate[name]["fused_gather"]:
                tensors[name] = _GatherEmb(h, True, lambda g, n=name: G["grads"].__setitem__(n, g))
            else:
                tensors[name] = G["leaf"][name]
        for i, rt in enumerate(self._ebc):
            self._ebc_tensors(tensors, rt, lambda i=i: G["ebc_leaf"][i])
        self._ebc_concat_tops(tensors)
        gscale = self.solver.scaler / max(self.bpg, 1)
        multi = len(self._loss_layers) > 1
        head = (G["label"], gscale) if (self._head_layer is not None and not multi and
                                        G["label"].shape[1] == 1) else None
        logit, loss = self._forward_dense(tensors, True, head)
        if multi:
            loss, _ = self._multi_task_loss(tensors)
            (loss * self.solver.scaler).backward()
        elif loss is not None:
            loss.backward(self._unit_grad(loss))
        else:
            lg = tensors[self._loss_layer.bottom_names[0]]
            loss, dlogit = bce_with_logits(lg, G["label"], gscale)
            lg.backward(dlogit)
        for name, leaf in G["leaf"].items():
            G["grads"][name] = leaf.grad
        for i, leaf in enumerate(G["ebc_leaf"]):
            G["ebc_grads"][i] = leaf.grad
        self._dense_step(skip=skip_step)
        return loss.detach().reshape(())

    def _graph_capture(self, batch):
        B = self.bpg
        G = {"lr": self._lr, "leaf": {}, "pooled": {}, "grads": {}, "ebc_leaf": [], "ebc_grads": {},
             "dense": torch.empty_like(batch["dense"]),
             "label": torch.empty_like(batch["label"].float())}
        G["dense"].copy_(batch["dense"])
        G["label"].copy_(batch["label"].float())
        for rt in self._ebc:  # the collections' outputs: static leaves the replay reads
            E = self._ebc_forward(rt, batch, True)
            G["ebc_leaf"].append(E.detach().clone().requires_grad_(True))
        for name, (se, p, h, ex, localized) in self._emb.items():
            ro, keys = batch["sparse"][se.bottom_name]
            if self._xstate[name]["fused_gather"]:
                h.index(True, ro, keys)
                continue
            S = h.slots_on_rank if localized else p.slot_num
            G["pooled"][name] = torch.empty((self.solver.batchsize, S, se.embedding_vec_size),
                                            dtype=self.emb_dtype, device=self.device)
            h.forward(True, ro, keys, out=G["pooled"][name])
            G["leaf"][name] = G["pooled"][name].view(B, p.slot_num, se.embedding_vec_size) \
                .requires_grad_(True)
        # the kernels of this graph have all run eagerly in earlier iterations; two more passes on
        # a side stream settle the allocator, without optimizer steps
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._graph_dense(G, skip_step=True)
        torch.cuda.current_stream().wait_stream(side)
        for leaf in list(G["leaf"].values()) + G["ebc_leaf"]:
            leaf.grad = None
        for q in self._dense_params:
            q.grad = None
        G["graph"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(G["graph"]):
            G["loss"] = self._graph_dense(G, skip_step=False)
        return G

    def _graph_step(self, batch):
        """one training step with the dense tower replayed from its HIP graph: the embedding's index
        stage / gather in front of it and its backward + sparse update behind it stay eager launches
        on the same stream (their sizes follow the data)"""
        G = self._graph
        fresh = G is None or G["lr"] != self._lr
        if fresh:
            G = self._graph = self._graph_capture(batch)
        else:
            for name, (se, p, h, ex, localized) in self._emb.items():
                ro, keys = batch["sparse"][se.bottom_name]
                if self._xstate[name]["fused_gather"]:
                    h.index(True, ro, keys)
                else:
                    h.forward(True, ro, keys, out=G["pooled"][name])
            for i, rt in enumerate(self._ebc):
                with torch.no_grad():
                    G["ebc_leaf"][i].copy_(self._ebc_forward(rt, batch, True))
            G["dense"].copy_(batch["dense"])
            G["label"].copy_(batch["label"])
        G["graph"].replay()
        for i, rt in enumerate(self._ebc):
            g = G["ebc_grads"].get(i)
            if g is not None:  # (None: the losses do not depend on this collection's output)
                rt["train"].lr = self._lr
                rt["train"].backward_and_update(g.contiguous())
        for name, (se, p, h, ex, localized) in self._emb.items():
            g = G["grads"][name]
            if not self._xstate[name]["fused_gather"]:
                g = ex["train"].backward(g.contiguous())  # (one GPU: a view)
            h.backward(g.contiguous())
            h.update_params()
        return G["loss"]

    def _dense_reduce_begin(self):
        """N > 1: starts the data-parallel all-reduce of the dense gradients (shares of the
        global-batch mean: a plain sum) and returns the handles _dense_step waits on; None when
        there is nothing to reduce asynchronously (one GPU, frozen dense part, host-staged gloo)"""
        if self.world == 1 or getattr(self, "_dense_frozen", False) or not self._intra or \
                dist.get_backend() == "gloo":
            return None
        if self._flat_mlps:
            self._dense_finish.finish(sgd=False)  # the partial sums -> flat_g
        ts = [m.flat_g for m in self._flat_mlps] if self._flat_mlps else \
            [q.grad for q in self._dense_params if q.grad is not None]
        return [dist.all_reduce(t, async_op=True) for t in ts]

    def _unit_grad(self, loss):
        """the upstream gradient of `loss.backward()`, made once instead of filled every step"""
        g = getattr(self, "_unit_grad_t", None)
        if g is None or g.device != loss.device or g.dtype != loss.dtype or g.shape != loss.shape:
            g = self._unit_grad_t = torch.ones_like(loss)
        return g

    def _dense_step(self, skip: bool = False, reduced=None):
        frozen = getattr(self, "_dense_frozen", False) or skip
        if reduced is not None:
            for w in reduced:
                w.wait()
        if self._flat_mlps:
            # one GPU: the finish launch takes the partial sums through the SGD step; N > 1 (or no
            # step): it leaves the gradients in flat_g, the all-reduce and hctr_sgd_shadow follow
            # Ftrl: always gradients first, then (after the all-reduce: ONE step on the summed
            # gradient) hctr_ftrl_shadow per MLP
            one = self.world == 1 and not frozen and not self._flat_ftrl
            if reduced is None:
                self._dense_finish.finish(one, self._lr, 1.0 / self.solver.scaler)
            if frozen or one:
                return
            with self._dense_finish.one_transpose():  # (W^T of all modules: one launch)
                for m in self._flat_mlps:  # gradients are shares of the global-batch mean: plain sum
                    if reduced is None and self.world > 1:
                        _all_reduce(m.flat_g)
                    if self._flat_ftrl:
                        o = self.opt
                        m.ftrl_step(self._lr, o.beta, o.lambda1, o.lambda2, 1.0 / self.solver.scaler)
                    else:
                        m.sgd_step(self._lr, 1.0 / self.solver.scaler)
            return
        if self._dense_opt is None:
            return
        if frozen:
            self._dense_opt.zero_grad(set_to_none=True)
            return
        ftrl = isinstance(self._dense_opt, DenseFtrl)  # (divides by the scaler in its own launch)
        if self.world > 1 and reduced is None:
            for q in self._dense_params:
                if q.grad is not None:
                    _all_reduce(q.grad)
        if self.solver.scaler != 1.0 and not ftrl:  # one multi-tensor launch, not one per parameter
            grads = [q.grad for q in self._dense_params if q.grad is not None]
            if grads:
                torch._foreach_div_(grads, self.solver.scaler)
        self._dense_opt.step()
        self._dense_opt.zero_grad(set_to_none=True)
        for m in self._mods.values():
            if isinstance(m, FusedMLP):
                m.refresh_shadow()

    def check_overflow(self, blocking: bool = True):
        if blocking:
            self._drain_prefetch()
        return self._check_overflow(blocking)

    def _check_overflow(self, blocking: bool = True):
        """Model::check_overflow (R/HugeCTR/src/pybind/model.cpp:1088: called by every train()):
        raises when an embedding saw more distinct keys than max_vocabulary_size_per_gpu.  train()
        uses the non-blocking form (the flag of an earlier iteration, no host sync on the path);
        eval / fit's end / save use the blocking one."""
        for (_, _, h, _, _) in self._emb.values():
            h.check_overflow() if blocking else h.poll_overflow()

    def train(self) -> bool:
        assert self._compiled
        for st in self._xstate.values():
            if st["select"] is not None:
                self._select_exchange(st)
        batch, self._lookahead = self._lookahead, None
        if batch is None:
            batch = self.reader.next_batch(train=True)
        if batch is None:
            return False
        nxt = None
        if (self._inter and any(st["mode"] != "rows" for st in self._xstate.values())) or \
                (self._idx_overlap and any(st["fused_gather"] for st in self._xstate.values())):
            # inter-iteration overlap: the next batch's keys are needed a step early
            nxt = self._lookahead = self.reader.next_batch(train=True)
        self.check_overflow(blocking=False)
        loss = None
        if self._graph_ok and not getattr(self, "_dense_frozen", False):
            # three eager steps first (and after every change of the learning rate): lazy
            # initialisations -- optimizer state, GEMM selections, kernel modules -- happen there
            if getattr(self, "_graph_lr", None) != self._lr:
                self._graph_lr, self._graph_wait, self._graph = self._lr, 3, None
            if self._graph_wait > 0:
                self._graph_wait -= 1
            else:
                try:
                    loss = self._graph_step(batch)
                except Exception as e:  # capture is an optimisation: eager launches from here on
                    if self._graph is not None:
                        raise
                    print(f"[HCTR][WARNING] HIP-graph capture failed ({e!r}); eager launches")
                    self._graph_ok = False
                    for q in self._dense_params:
                        q.grad = None
        if loss is None:
            loss, _ = self._run_batch(batch, True, nxt)
        self._loss_t = loss.detach()
        self._iter += 1
        return True

    def _drain_prefetch(self):
        """an index stage running ahead on a side stream must be through before anything else
        touches the embedding (evaluation, checkpoints, overflow checks)"""
        for st in getattr(self, "_xstate", {}).values():
            if st["ux"] is not None:
                st["ux"].drain()
        for _, ev in getattr(self, "_idx_ahead", {}).values():
            torch.cuda.current_stream().wait_event(ev)

    @property
    def _eval_buf(self):
        """what eval() has accumulated since the last reset: the EvalMetrics object, falsy while it
        is empty.  Assigning anything (`model._eval_buf = []`) clears the store and the counters."""
        return getattr(self, "_metrics", None)

    @_eval_buf.setter
    def _eval_buf(self, _):
        m = getattr(self, "_metrics", None)
        if m is not None:
            m.reset()

    def eval(self) -> bool:
        batch = self.reader.next_batch(train=False)
        if batch is None:
            return False
        self._drain_prefetch()
        if not self._eval_buf:
            self.check_overflow()
        with torch.no_grad():
            loss, prob = self._run_batch(batch, False)
        # one launch files the scores away (hugectr_amd/metrics.py): no list, nothing waits
        self._metrics.add_batch(prob, batch["label"], loss)
        return True

    def get_current_loss(self) -> float:
        return float(self._loss_t)

    def get_eval_metrics(self):
        """one (name, value) pair per type of solver.metrics_spec in enum order, then
        ("AverageLoss", ...) unless the spec named it; over the samples of ALL GPUs.  Resets
        nothing."""
        return self._metrics.result()

    def set_learning_rate(self, lr: float):
        self._lr = lr
        for (_, _, h, _, _) in self._emb.values():
            h.set_learning_rate(lr)
        if self._dense_opt is not None:
            for g in self._dense_opt.param_groups:
                g["lr"] = lr

    def summary(self):
        if self.rank != 0:
            return
        print("=" * 67 + "Model Summary" + "=" * 67)
        print(f"{'Label':<40}{'Dense':<30}{'Sparse':<30}")
        print(f"{self.input.label_name:<40}{self.input.dense_name:<30}"
              f"{','.join(p.top_name for p in self.input.sparse_params):<30}")
        print(f"({self.bpg},{self.input.label_dim})".ljust(40) + f"({self.bpg},{self.input.dense_dim})")
        print("-" * 147)
        print(f"{'Layer Type':<40}{'Input Name':<30}{'Output Name':<30}{'Output Shape':<30}")
        for name, (se, p, h, _, _) in self._emb.items():
            print(f"{se.embedding_type.name:<40}{se.bottom_name:<30}{name:<30}"
                  f"({self.bpg},{p.slot_num},{se.embedding_vec_size})")
        for rt in self._ebc:
            cfg, e = rt["cfg"], rt["train"]
            print(f"{'EmbeddingCollection':<40}{','.join(b for _, b, _, _ in cfg.lookups)[:28]:<30}"
                  f"{(cfg.top_name or ','.join(t for _, _, t, _ in cfg.lookups))[:28]:<30}"
                  f"({self.bpg},{e.L},{e.ev})")
            for t in e.tables:  # each table's optimizer: its opt_params, else the model's
                src = "opt_params" if resolve_table_optimizer(t, self.opt)[1] == "table" \
                    else "model"
                print(f"{'  table ' + t.name:<40}{'optimizer':<30}"
                      f"{Optimizer_t(int(e.optimizer)).name + ' (' + src + ')':<30}")
        for L in self.layers:
            tops = ",".join(L.top_names)
            shp = self._shapes.get(L.top_names[0], ()) if L.top_names else ()
            print(f"{L.layer_type.name:<40}{','.join(L.bottom_names):<30}{tops:<30}"
                  f"({self.bpg},{','.join(str(v) for v in shp)})")
        print("-" * 147)

    def fit(self, num_epochs=0, max_iter=2000, display=200, eval_interval=1000, snapshot=10000,
            snapshot_prefix="", data_source_params=None):
        assert self._compiled, "call compile() first"
        s = self.solver
        if self.rank == 0:
            print(f"=====================================================Model Fit====================="
                  f"================================")
            print(f"[HCTR][INFO] Use non-epoch mode with number of iterations: {max_iter}"
                  if num_epochs <= 0 else f"[HCTR][INFO] Use epoch mode with number of epochs: {num_epochs}")
            print(f"[HCTR][INFO] Training batchsize: {s.batchsize}, evaluation batchsize: {s.batchsize_eval}")
        t0 = t_fit = time.time()
        it = 0
        hit_target = False
        limit = max_iter if num_epochs <= 0 else 10 ** 12
        self._eval_buf = []
        callbacks = list(getattr(s, "training_callbacks", None) or [])
        for tc in callbacks:  # model.cpp:869-872
            tc.on_training_start()
        stopped = False
        sch = self.get_learning_rate_scheduler()
        scheduled = s.warmup_steps > 1 or s.decay_start > 0
        while it < limit:
            if scheduled:
                self.set_learning_rate(sch.get_next())
            if not self.train():
                break
            it += 1
            if display > 0 and it % display == 0:
                torch.cuda.synchronize()
                if self.rank == 0:
                    print(f"[HCTR][INFO] Iter: {it} Time({display} iters): {time.time() - t0:.6f}s "
                          f"Loss: {self.get_current_loss():.6f} lr:{self._lr:.6f}")
                t0 = time.time()
            if eval_interval > 0 and it % eval_interval == 0 and s.batchsize_eval > 0 \
                    and self.reader.has_eval():
                self._eval_buf = []
                te = time.time()
                for tc in callbacks:  # model.cpp:921-924 (iter counts from 0 there)
                    tc.on_eval_start(it - 1)
                for _ in range(s.max_eval_batches):
                    if not self.eval():
                        break
                torch.cuda.synchronize()
                metrics = self.get_eval_metrics()
                early = False
                for tc in callbacks:  # model.cpp:935-943
                    early = bool(tc.on_eval_end(it - 1, dict(metrics))) or early
                if early:
                    for tc in callbacks:
                        tc.on_training_end(it - 1)
                    stopped = True
                    break
                for name, v in metrics:  # model.cpp:945-979
                    if self.rank == 0:
                        print(f"[HCTR][INFO] Evaluation, {name}: {v:.6f}")
                    if name != "AUC":
                        continue
                    per = self._metrics.per_class("AUC")
                    if self.rank == 0 and len(per) > 1:  # print_class_aucs, model.cpp:678-689
                        print("[HCTR][INFO] Evaluation, AUC: {" + ", ".join(f"{a:f}" for a in per) + "}")
                    target = self._metrics.targets.get("AUC")
                    if target is not None and v > target:
                        if self.rank == 0:
                            el = max(time.time() - t_fit, 1e-9)
                            print(f"[HCTR][INFO] Hit target accuracy AUC {target:.5f} at "
                                  f"{it - 1} / {max_iter} iterations with batchsize {s.batchsize} "
                                  f"in {el:.2f}s. Average speed "
                                  f"{float(it - 1) * s.batchsize / el:f} records/s.")
                        hit_target = True
                        break
                if hit_target:  # the reference returns here: no on_training_end, no summary line
                    break
                if self.rank == 0:
                    print(f"[HCTR][INFO] Eval Time for {s.max_eval_batches} iters: {time.time() - te:.6f}s")
            if snapshot > 0 and it % snapshot == 0 and snapshot_prefix:
                self.save_params_to_files(snapshot_prefix, it)
        if not stopped and not hit_target:
            for tc in callbacks:  # model.cpp:991-994
                tc.on_training_end(max(it - 1, 0))
        torch.cuda.synchronize()
        self.check_overflow()
        if self.rank == 0 and not hit_target:
            print(f"[HCTR][INFO] Finish {it} iterations with batchsize: {s.batchsize} in "
                  f"{time.time() - t0:.2f}s.")

    # -- checkpoints: directory layout of the reference (SURVEY §5 "Checkpoint / resume") ----------
    def save_params_to_files(self, prefix: str, iteration: int = 0):
        self._drain_prefetch()
        self.check_overflow()
        for i, (name, (se, p, h, _, localized)) in enumerate(self._emb.items()):
            keys, slot, vec = h.dump_parameters()
            # ONE directory <prefix><i>_sparse_<iter>.model with key / slot_id / emb_vector, the
            # ranks' rows one after another in rank order -- the merged layout the reference writes
            # (dump_parameters, localized_slot_sparse_embedding_hash.cu:1260-1340: every GPU's
            # offset is the sum of the counts before it), so that load_sparse_weights (which keeps
            # the keys / slots a rank owns) reads it back on any number of ranks
            d = f"{prefix}{i}_sparse_{iteration}.model"
            n, D = int(keys.numel()), se.embedding_vec_size
            counts = [n]
            if self.world > 1:
                counts = [None] * self.world
                dist.all_gather_object(counts, n)
            first, total = sum(counts[:self.rank]), sum(counts)
            files = [("key", "<i8", 1, keys)]
            if localized:
                files.append(("slot_id", "<u8", 1, slot))
            files.append(("emb_vector", "<f4", D, vec))
            if self.rank == 0:
                os.makedirs(d, exist_ok=True)
                for fn, dt, w, _ in files:
                    with open(os.path.join(d, fn), "wb") as f:
                        f.truncate(total * w * np.dtype(dt).itemsize)
            if self.world > 1:
                dist.barrier()
            for fn, dt, w, t in files:
                if n == 0:
                    continue
                mm = np.memmap(os.path.join(d, fn), dtype=dt, mode="r+", shape=(total * w,))
                mm[first * w:(first + n) * w] = t.cpu().numpy().astype(dt).reshape(-1)
                mm.flush()
                del mm
            if self.world > 1:
                dist.barrier()
            if h._opt_state_count():  # <prefix><i>_opt_sparse_<iter>.model (model.cpp:1244-1246)
                h.dump_opt_states(f"{prefix}{i}_opt_sparse_{iteration}.model")
        for i, rt in enumerate(self._ebc):
            d = f"{prefix}_ebc{i}_sparse_{iteration}.model"
            os.makedirs(d, exist_ok=True)
            e = rt["train"]
            if getattr(e, "hybrid", False):  # per local table shard: its stored keys and rows
                for t, tab in e.hyb.items():
                    k, v = tab.export()
                    k.cpu().numpy().astype("<i8").tofile(os.path.join(d, f"key.table{t}.rank{self.rank}"))
                    v.cpu().numpy().astype("<f4").tofile(
                        os.path.join(d, f"emb_vector.table{t}.rank{self.rank}"))
            elif getattr(e, "dynamic", False):  # per local table: the keys it holds and their vectors
                for t, c in e.class_of_table.items():
                    k, v = e.det.export(c)
                    k.cpu().numpy().astype("<i8").tofile(os.path.join(d, f"key.table{t}.rank{self.rank}"))
                    v.cpu().numpy().astype("<f4").tofile(
                        os.path.join(d, f"emb_vector.table{t}.rank{self.rank}"))
            else:  # one file per rank: its flat [rows][ev] shard table
                e.table.cpu().numpy().astype("<f4").tofile(
                    os.path.join(d, f"emb_vector.rank{self.rank}"))
        if self.rank == 0 and self._dense_opt is not None:
            torch.save(self._dense_opt.state_dict(), f"{prefix}_opt_dense_{iteration}.model")
        elif self.rank == 0 and self._flat_mlps and self._flat_ftrl:
            # the flat path has no optimizer object: z / n of the MLPs in DenseFtrl's layout
            torch.save(ftrl_state_dict(self._flat_ftrl_state()),
                       f"{prefix}_opt_dense_{iteration}.model")
        if self.rank == 0 and self._dense_params:
            blobs = [b.detach().float().contiguous().flatten() for b, _ in self._dense_blobs()]
            torch.cat(blobs).cpu().numpy().astype("<f4").tofile(f"{prefix}_dense_{iteration}.model")

    # -- embedding_collection checkpoints: the reference's embedding_dump / embedding_load
    #    (R/HugeCTR/include/pybind/model_wrapper.hpp:167-173, R/HugeCTR/src/pybind/model.cpp:521-665;
    #    bytes: hugectr_amd/embedding_io.py, deviations: INTEGRATION.md) -------------------------------
    def _ebc_io_plan(self, table_names):
        """per user config c (the order the configs were added): {table id: (name, runtime
        collection, position in its tables)} of the tables asked for.  A table's id is its
        position in the USER's config, in order of first appearance in config.lookups
        (emb_table_config_list_, embedding_collection.hpp:205-214) -- whatever runtime collections
        the config was split into (by ev_size, mp / dp placement, compression strategy)."""
        assert self._compiled, "call compile() first"
        wanted = [str(n) for n in (table_names or [])]
        plan, known = [], set()
        for cfg in self.ebc_configs:
            tables = []
            for t, _, _, _ in cfg.lookups:
                if t not in tables:
                    tables.append(t)
            entries = {}
            for rt in self._ebc:
                if rt["parent"] is not cfg:
                    continue
                e = rt["train"]
                for k, tc in enumerate(e.tables):
                    known.add(tc.name)
                    if not wanted or tc.name in wanted:
                        entries[tables.index(tc)] = (tc.name, e, k)
            plan.append(entries)
        unknown = [n for n in wanted if n not in known]
        if unknown:
            raise RuntimeError(f"embedding_dump / embedding_load: no embedding table named "
                               f"{unknown}; the model's tables are {sorted(known)}")
        return plan

    def embedding_dump(self, path: str, table_names: Sequence[str] = (),
                       optimizer_states: bool = False):
        """Model::embedding_dump: <path>/embedding_collection_<c>/{meta_data, key<i>, weight<i>}
        for every EmbeddingCollectionConfig c of the model, one key and one weight file per table,
        independent of the sharding and of how the config was split into runtime collections.
        table_names: EmbeddingTableConfig names (empty: every table).  optimizer_states=True also
        writes opt_state<i> (not in the reference).  Several ranks: rank 0 creates the files at full
        size, then every owner writes its portion at its offset (the scheme of
        save_params_to_files)."""
        from . import embedding_io
        self._drain_prefetch()
        self.check_overflow()
        plan = self._ebc_io_plan(table_names)
        if optimizer_states:  # refused before anything is written
            for entries in plan:
                for _, e, _ in entries.values():
                    e.io_check_optimizer_states()
        for c, entries in enumerate(plan):
            if not entries:
                continue
            ids = sorted(entries)
            mine = [entries[i][1].table_key_count(entries[i][2]) for i in ids]
            counts = [mine]
            if self.world > 1:
                counts = [None] * self.world
                dist.all_gather_object(counts, mine)
            e0 = entries[ids[0]][1]
            kd = "<i8" if getattr(e0, "key_dtype", torch.int64) == torch.int64 else "<u4"
            meta = embedding_io.MetaData(
                ids, {i: sum(r[j] for r in counts) for j, i in enumerate(ids)},
                {i: entries[i][1].ev for i in ids}, np.dtype(kd))
            # (per table: the config's tables may run different optimizers, opt_params)
            opt = {i: (entries[i][1].io_state_count(), int(entries[i][1].optimizer))
                   for i in ids} if optimizer_states else None
            if self.rank == 0:
                embedding_io.create_collection(path, c, meta, opt)
            if self.world > 1:
                dist.barrier()
            for j, i in enumerate(ids):
                name, e, k = entries[i]
                if mine[j] == 0:
                    continue
                with embedding_io.TableFiles(path, c, i, "r+", name=name) as f:
                    e.export_table(k, f, sum(r[j] for r in counts[:self.rank]), optimizer_states)
            torch.cuda.synchronize()
            if self.world > 1:
                dist.barrier()

    def embedding_load(self, path: str, table_names: Sequence[str] = ()):
        """Model::embedding_load: every rank keeps the keys it owns (key % num_shards ==
        shard_id; a replicated table loads whole on every rank).  The tables are written in place
        -- a captured graph stays valid -- and only after every table asked for has been
        validated.  Optimizer state is loaded where the dump holds it for that table's optimizer
        (its opt_params, else the model's); a state file of another optimizer is refused in the
        validation, before anything is written."""
        from . import embedding_io
        self._drain_prefetch()
        self.check_overflow()
        plan = self._ebc_io_plan(table_names)
        opened = []
        try:
            for c, entries in enumerate(plan):
                if not entries:
                    continue
                meta = embedding_io.read_meta(path, c)
                for i in sorted(entries):
                    name, e, k = entries[i]
                    opened.append((e, k, embedding_io.TableFiles(path, c, i, "r", meta, name)))
            for e, k, f in opened:
                e.validate_table(k, f)
            for e, k, f in opened:
                e.import_table(k, f, validated=True)
        finally:
            for _, _, f in opened:
                f.close()
        torch.cuda.synchronize()
        if self.world > 1:
            dist.barrier()

    def _dense_blobs(self):
        """the trainable dense tensors in the order and orientation of the reference's dense model
        file (what R/onnx_converter/hugectr2onnx/hugectr_loader.py:336-520 reads back): per layer
        in graph order -- InnerProduct / each MLP sub-layer: weight [in, out] then bias [out];
        MultiCross: per cross layer w[width], b[width] (v1) or U[width, p], V[p, width], b (v2,
        multi_cross_layer.cu:864-874); WeightMultiply: [slots, vec].  Yields (tensor in file
        orientation, setter taking a tensor of that shape)."""
        out = []

        def direct(q):
            return q, (lambda v, q=q: q.copy_(v.view_as(q)))

        def transposed(q):  # torch keeps [out, in]
            return q.t(), (lambda v, q=q: q.copy_(v.view(q.shape[1], q.shape[0]).t()))

        for i, L in enumerate(self.layers):
            m = self._mods[f"l{i}"] if f"l{i}" in self._mods else None
            t = L.layer_type
            if t == Layer_t.InnerProduct:
                out += [transposed(m.weight), direct(m.bias)]
            elif t == Layer_t.MLP:
                for w, b in zip(m.weights, m.biases):
                    out += [transposed(w), direct(b)]
            elif t == Layer_t.MultiCross:
                for l in range(m.num_layers):
                    if m.projection_dim == 0:
                        out += [direct(m.kernels[l]), direct(m.biases[l])]
                    else:
                        out += [direct(m.U[l]), direct(m.V[l]), direct(m.biases[l])]
            elif t == Layer_t.WeightMultiply:
                out += [direct(m.w)]
        return out

    def load_sparse_weights(self, paths: Sequence[str]):
        for path, (name, (se, p, h, _, localized)) in zip(paths, self._emb.items()):
            keys = np.fromfile(os.path.join(path, "key"), dtype="<i8")
            vec = np.fromfile(os.path.join(path, "emb_vector"), dtype="<f4").reshape(
                keys.size, se.embedding_vec_size)
            slot = None
            sp = os.path.join(path, "slot_id")
            if localized and os.path.exists(sp):
                slot = np.fromfile(sp, dtype="<u8").astype(np.int64)
                mine = slot % self.world == self.rank
            else:
                mine = keys % self.world == self.rank if self.world > 1 else np.ones(keys.size, bool)
            h.load_parameters(torch.from_numpy(keys[mine]),
                              torch.from_numpy(slot[mine]) if slot is not None else None,
                              torch.from_numpy(vec[mine]))

    def start_data_reading(self):
        """the low-level loop's first call (model.cpp start_data_reading): readers start lazily"""
        assert self._compiled, "call compile() first"

    def get_learning_rate_scheduler(self) -> LearningRateScheduler:
        if getattr(self, "_lr_sch", None) is None:
            s = self.solver
            self._lr_sch = LearningRateScheduler(s.lr, s.warmup_steps, s.decay_start, s.decay_steps,
                                                 s.decay_power, s.end_lr)
        return self._lr_sch

    def load_dense_optimizer_states(self, path: str):
        """state of the dense optimizer as save_params_to_files wrote it (<prefix>_opt_dense_<iter>
        .model, model.cpp:1238)"""
        if self._dense_opt is not None:  # (load_state_dict moves the state to the parameters)
            self._dense_opt.load_state_dict(torch.load(path, map_location="cpu"))
        elif self._flat_mlps and self._flat_ftrl:  # the same file, whichever path wrote it
            load_ftrl_state_dict(self._flat_ftrl_state(), torch.load(path, map_location="cpu"))

    def _flat_ftrl_state(self):
        """[(z, n)] per dense parameter of the flat Ftrl path, in the order of _dense_params (the
        order DenseFtrl holds them in when the same model runs unfused)"""
        by_param = {}
        for m in self._flat_mlps:
            for q, zn in zip(m.parameters(), m.ftrl_state()):
                by_param[id(q)] = zn
        return [by_param[id(q)] for q in self._dense_params]

    def load_sparse_optimizer_states(self, paths: Sequence[str]):
        for path, (name, (se, p, h, _, _)) in zip(paths, self._emb.items()):
            h.load_opt_states(path)

    # Model::freeze_embedding / unfreeze_embedding / freeze_dense / unfreeze_dense
    # (model_wrapper.hpp:147-156): a frozen part keeps computing, its weights stop moving
    def freeze_embedding(self, embedding_name: Optional[str] = None):
        for name, (se, p, h, _, _) in self._emb.items():
            if embedding_name is None or name == embedding_name:
                h.freeze()

    def unfreeze_embedding(self, embedding_name: Optional[str] = None):
        for name, (se, p, h, _, _) in self._emb.items():
            if embedding_name is None or name == embedding_name:
                h.unfreeze()

    def freeze_dense(self):
        self._dense_frozen = True

    def unfreeze_dense(self):
        self._dense_frozen = False

    def load_dense_weights(self, path: str):
        flat = torch.from_numpy(np.fromfile(path, dtype="<f4")).to(self.device)
        off = 0
        with torch.no_grad():
            for blob, put in self._dense_blobs():
                n = blob.numel()
                put(flat[off:off + n])
                off += n
        if off != flat.numel():
            raise RuntimeError(f"{path}: {flat.numel()} values, the model's dense layers hold {off}")
        for m in self._mods.values():
            if isinstance(m, FusedMLP):
                m.refresh_shadow()

    def graph_to_json(self, graph_config_file: str):
        """the reference's graph schema (save_graph_to_json,
        R/HugeCTR/src/pybind/add_dense_layer.cpp:65-460): single bottom / top names are strings,
        layer hyper-parameters sit under the reference's keys (fc_param, mlp_param, mc_param, ...)"""
        def one_or_list(names):
            return names[0] if len(names) == 1 else list(names)

        inp = self.input
        label = ({"top": inp.label_names[0], "label_dim": inp.label_dims[0]} if len(inp.label_names) == 1
                 else {"top": list(inp.label_names), "label_dim": list(inp.label_dims)})
        layers = [{"type": "Data", "label": label,
                   "dense": {"top": inp.dense_name, "dense_dim": inp.dense_dim},
                   "sparse": [{"top": p.top_name, "slot_num": p.slot_num,
                               "nnz_per_slot": (list(p.nnz_per_slot)
                                                if isinstance(p.nnz_per_slot, (list, tuple))
                                                else [int(p.nnz_per_slot)] * p.slot_num),
                               "is_fixed_length": p.is_fixed_length}
                              for p in inp.sparse_params]}]
        for se in self.embeddings:
            o = se.optimizer if (se.optimizer is not None and se.optimizer.initialized) else self.opt
            t = Optimizer_t(o.optimizer_type)
            hp = {Optimizer_t.Ftrl: ("ftrl_hparam", {"beta": o.beta, "lambda1": o.lambda1,
                                                      "lambda2": o.lambda2}),
                  Optimizer_t.Adam: ("adam_hparam", {"beta1": o.beta1, "beta2": o.beta2,
                                                      "epsilon": o.epsilon}),
                  Optimizer_t.AdaGrad: ("adagrad_hparam", {"initial_accu_value": o.initial_accu_value,
                                                            "epsilon": o.epsilon}),
                  Optimizer_t.MomentumSGD: ("momentum_sgd_hparam", {"momentum_factor": o.momentum_factor}),
                  Optimizer_t.Nesterov: ("nesterov_hparam", {"momentum_factor": o.momentum_factor}),
                  Optimizer_t.SGD: ("sgd_hparam", {"atomic_update": o.atomic_update})}.get(t)
            opt = {"update_type": Update_t(o.update_type).name, "type": t.name}
            if hp:
                opt[hp[0]] = hp[1]
            hparam = {"workspace_size_per_gpu_in_mb": se.workspace_size_per_gpu_in_mb,
                      "embedding_vec_size": se.embedding_vec_size,
                      "combiner": "sum" if se.combiner == 0 else "mean"}
            if self._compiled:  # max_vocabulary_size_per_gpu x GPUs (model_compile.cpp:200-201)
                h = self._emb[se.sparse_embedding_name][2]
                hparam["max_vocabulary_size_global"] = h.get_max_vocabulary_size() * self.world
            if se.slot_size_array:
                hparam["slot_size_array"] = list(se.slot_size_array)
            layers.append({"type": se.embedding_type.name, "bottom": se.bottom_name,
                           "top": se.sparse_embedding_name, "sparse_embedding_hparam": hparam,
                           "optimizer": opt})
        for cfg in self.ebc_configs:
            layers.append({"type": "EmbeddingCollection",
                           "lookups": [{"table": t.name, "max_vocabulary_size": t.max_vocabulary_size,
                                        "ev_size": t.ev_size, "bottom": b, "top": tp, "combiner": str(c)}
                                       for t, b, tp, c in cfg.lookups],
                           "shard_matrix": cfg.shard_matrix})
        for L in self.layers:
            t = L.layer_type
            d = {"type": t.name, "bottom": one_or_list(L.bottom_names), "top": one_or_list(L.top_names)}
            if t == Layer_t.Dropout:
                d["rate"] = L.dropout_rate
            elif t == Layer_t.ELU:
                d["elu_param"] = {"alpha": L.elu_alpha}
            elif t == Layer_t.MLP:
                mp = {"num_output": L.num_output, "num_outputs": list(L.num_outputs)}
                if L.biases:
                    mp["biases"] = list(L.biases)
                else:
                    mp["use_bias"] = L.use_bias
                if L.activations:
                    mp["activations"] = [_ACT_NAME[a] for a in L.activations]
                else:
                    mp["activation"] = _ACT_NAME[L.act_type]
                d["mlp_param"] = mp
            elif t == Layer_t.InnerProduct:
                d["fc_param"] = {"num_output": L.num_output}
            elif t == Layer_t.MultiCross:
                d["mc_param"] = {"num_layers": L.num_layers}
                if L.projection_dim:
                    d["mc_param"]["projection_dim"] = L.projection_dim
            elif t == Layer_t.Reshape:
                if L.selected_slots:
                    d["selected"] = list(L.selected_slots)
                else:
                    d["leading_dim"], d["time_step"] = L.leading_dim, L.time_step
            elif t == Layer_t.Concat:
                d["axis"] = L.axis
            elif t == Layer_t.Slice:
                d["ranges"] = [list(r) for r in L.ranges]
            elif t == Layer_t.WeightMultiply:
                d["weight_dims"] = [int(v) for v in L.weight_dims]
            elif t == Layer_t.FmOrder2:
                d["out_dim"] = L.out_dim
            elif t == Layer_t.ReduceSum:
                d["axis"] = L.axis
            elif t == Layer_t.Softmax:
                d["factor"] = L.factor
            layers.append(d)
        with open(graph_config_file, "w") as f:
            json.dump({"layers": layers}, f, indent=2)


# FC_ACTIVATION_TO_STRING (R/HugeCTR/include/pybind/model.hpp:132-133)
_ACT_NAME = {Activation_t.Relu: "Relu", Activation_t.Non: "None", Activation_t.Unspecified: "None"}


def _auc(p: torch.Tensor, y: torch.Tensor) -> float:
    """area under the ROC curve = Mann-Whitney U with tied scores sharing their average rank (a
    tie between a positive and a negative counts one half, the trapezoid rule of the reference's
    AUC metric, R/HugeCTR/src/metrics.cu)"""
    p, order = torch.sort(p.double())
    y = y[order].double()
    n_pos = float(y.sum())
    n_neg = float(y.numel() - n_pos)
    if n_pos == 0 or n_neg == 0:
        return 0.5
    _, inv, cnt = torch.unique_consecutive(p, return_inverse=True, return_counts=True)
    last = torch.cumsum(cnt, 0).double()               # 1-based rank of the last member of a tie
    avg = (last - (cnt.double() - 1) / 2)[inv]         # average rank of every member
    return float(((avg * y).sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))


class tools:  # hugectr.tools.* (R/HugeCTR/include/pybind/data_generator_wrapper.hpp:29-69)
    DataGeneratorParams = _data.DataGeneratorParams
    DataGenerator = _data.DataGenerator
