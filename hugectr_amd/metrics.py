"""Evaluation metrics of Model.eval / get_eval_metrics / fit (R/HugeCTR/src/metrics.cu): AUC,
AverageLoss, HitRate, NDCG, SMAPE as solver.metrics_spec names them.

eval() hands every batch to ONE hctr_metric_accumulate launch (csrc/metrics.hip): the scores go
into a class-major device store as order-preserving uint32 keys next to their labels, and a small
counter block collects HitRate's and SMAPE's sums -- no Python list of tensors, no host
synchronisation.  get_eval_metrics() finalises on the device (our radix sort + one tie-aware pass
per label column) and reads a handful of words back.

Deviations from the reference (INTEGRATION.md "Evaluation metrics"): AUC is the exact Mann-Whitney
statistic in integers instead of an fp32 trapezoid sum over a histogram-partitioned sort; HitRate
with nothing checked is 0.0 (the reference divides 0 by 0); a SMAPE term with p + l == 0 counts 0;
NaN scores tie with each other and rank last; with several GPUs every rank gathers the other ranks'
store slices and finalises the same arrays (no partitioned exchange).
"""
from __future__ import annotations

from ctypes import c_void_p

import numpy as np
import torch
import torch.distributed as dist

from . import _lib

_DTYPES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
# enum order of R/HugeCTR/include/metrics.hpp:36 (the reference keeps the spec in a std::map)
_ORDER = {"AUC": 0, "AverageLoss": 1, "HitRate": 2, "NDCG": 3, "SMAPE": 4}
_CT_CHECKED, _CT_HITS, _CT_SMAPE_CNT, _CT_SMAPE_SUM, _CT_BAD = 0, 1, 2, 3, 8


def _name(t) -> str:
    return t if isinstance(t, str) else t.name


def auc_from_words(two_u: int, pos: int, neg: int) -> float:
    """AUC = 2U / (2 P N) in fp64; 0.5 when one of the two classes is absent"""
    if pos == 0 or neg == 0:
        return 0.5
    return float(np.float64(two_u) / np.float64(2 * pos * neg))


class EvalMetrics:
    """accumulates the evaluation batches of one rank and finalises the metrics of metrics_spec"""

    def __init__(self, metrics_spec, label_dim: int, batch_per_gpu: int, max_eval_batches: int,
                 num_loss_layers: int = 1, world: int = 1, device=None):
        self.types = sorted({_name(t) for t in (metrics_spec or {})}, key=lambda s: _ORDER[s])
        self.targets = {_name(t): float(v) for t, v in (metrics_spec or {}).items()}
        if num_loss_layers > 1 and any(t != "AUC" for t in self.types):
            # R/HugeCTR/src/pybind/model_compile.cpp:929-932
            raise RuntimeError("Metrics besides AUC are not supported for multi-task models.")
        if not 1 <= int(label_dim) <= _lib.METRIC_MAX_CLASSES:
            raise RuntimeError(f"evaluation metrics support 1..{_lib.METRIC_MAX_CLASSES} label "
                               f"columns, not {label_dim}")
        self.C = int(label_dim)
        self.world = int(world)
        self.device = device
        self._cap0 = max(1, int(batch_per_gpu) * max(1, int(max_eval_batches)))
        self.cap = 0
        self.keys = self.labels = self.counters = self._acc_temp = self._loss = None
        self.n = 0          # samples stored per class
        self.batches = 0
        self._result = None
        self._per_class = {}

    # -- accumulation ------------------------------------------------------------------------------
    def __bool__(self):
        return self.n > 0 or self.batches > 0

    def reset(self):
        self.n = 0
        self.batches = 0
        self._result = None
        self._per_class = {}
        if self.counters is not None:
            self.counters.zero_()
            self._loss.zero_()

    def _reserve(self, need: int, device):
        if self.keys is None:
            self.device = device
            self.counters = torch.zeros(_lib.METRIC_COUNTER_WORDS, dtype=torch.int64, device=device)
            self._loss = torch.zeros(1, dtype=torch.float64, device=device)
            self._acc_temp = torch.empty(int(_lib.lib.hctr_metric_accumulate_temp_bytes()),
                                         dtype=torch.uint8, device=device)
        if need <= self.cap:
            return
        cap = max(need, self._cap0, 2 * self.cap)
        keys = torch.empty((self.C, cap), dtype=torch.int32, device=device)
        labels = torch.empty((self.C, cap), dtype=torch.float32, device=device)
        if self.n:
            keys[:, :self.n].copy_(self.keys[:, :self.n])
            labels[:, :self.n].copy_(self.labels[:, :self.n])
        self.keys, self.labels, self.cap = keys, labels, cap

    def add_batch(self, prob: torch.Tensor, label: torch.Tensor, loss: torch.Tensor):
        """scores [B, C] (fp32 / fp16 / bf16 as the network returns them), labels [B, C], the
        batch's loss: one launch and one add, nothing waits for the device"""
        label = label.detach().reshape(-1, self.C).float().contiguous()
        prob = prob.detach().reshape(-1, self.C)
        if prob.dtype not in _DTYPES:
            prob = prob.float()
        prob = prob.contiguous()
        B = int(label.shape[0])
        if int(prob.shape[0]) != B:
            raise RuntimeError(f"evaluation scores {tuple(prob.shape)} do not match the labels "
                               f"{tuple(label.shape)}")
        self._reserve(self.n + B, prob.device)
        _lib.check(_lib.lib.hctr_metric_accumulate(
            _lib.ptr(prob), _DTYPES[prob.dtype], _lib.ptr(label), B, self.C, _lib.ptr(self.keys),
            _lib.ptr(self.labels), self.cap, self.n, _lib.ptr(self.counters),
            _lib.ptr(self._acc_temp), self._acc_temp.numel(), _lib.stream_ptr()))
        self._loss.add_(loss.detach().reshape(()).double())
        self.n += B
        self.batches += 1
        self._result = None

    # -- finalise ----------------------------------------------------------------------------------
    def _gathered(self):
        """(keys [C, N], labels [C, N], counters, loss sum, batches) over the samples of ALL GPUs:
        every rank gathers the other ranks' store slices (8 B per sample and class), staged through
        the CPU under gloo"""
        keys, labels = self.keys[:, :self.n], self.labels[:, :self.n]
        counters, loss = self.counters.clone(), self._loss.clone()
        if self.world <= 1:
            return keys, labels, counters, loss, self.batches
        staged = dist.get_backend() == "gloo"
        dv = torch.device("cpu") if staged else self.device
        k, l = keys.contiguous().to(dv), labels.contiguous().to(dv)
        ks = [torch.empty_like(k) for _ in range(self.world)]
        ls = [torch.empty_like(l) for _ in range(self.world)]
        dist.all_gather(ks, k)
        dist.all_gather(ls, l)
        keys = torch.cat(ks, dim=1).to(self.device).contiguous()
        labels = torch.cat(ls, dim=1).to(self.device).contiguous()
        c = counters.to(dv)
        s = c[_CT_SMAPE_SUM:_CT_SMAPE_SUM + 1].view(torch.float64).clone()
        lo = loss.to(dv)
        dist.all_reduce(c)
        dist.all_reduce(s)
        dist.all_reduce(lo)
        c[_CT_SMAPE_SUM:_CT_SMAPE_SUM + 1] = s.view(torch.int64)
        return keys, labels, c.to(self.device), lo.to(self.device), self.batches * self.world

    def _finalise(self):
        L = _lib.lib
        keys, labels, counters, loss, batches = self._gathered()
        keys, labels = keys.contiguous(), labels.contiguous()
        N, C, dev = int(keys.shape[1]), self.C, self.device
        words = torch.zeros((C, 3), dtype=torch.int64, device=dev)
        dcg = torch.zeros((C, 2), dtype=torch.float64, device=dev)
        esz = 4
        if "AUC" in self.types:
            tb = int(L.hctr_metric_auc_temp_bytes(N))
            temp = torch.empty(tb, dtype=torch.uint8, device=dev)
            for c in range(C):
                _lib.check(L.hctr_metric_auc(
                    _lib.ptr(temp), tb, c_void_p(keys.data_ptr() + c * N * esz),
                    c_void_p(labels.data_ptr() + c * N * esz), N,
                    c_void_p(words.data_ptr() + c * 24), _lib.stream_ptr()))
        if "NDCG" in self.types:
            tb = int(L.hctr_metric_ndcg_temp_bytes(N))
            temp = torch.empty(tb, dtype=torch.uint8, device=dev)
            for c in range(C):
                _lib.check(L.hctr_metric_ndcg(
                    _lib.ptr(temp), tb, c_void_p(keys.data_ptr() + c * N * esz),
                    c_void_p(labels.data_ptr() + c * N * esz), N,
                    c_void_p(dcg.data_ptr() + c * 16), _lib.stream_ptr()))
        # the only wait: a few words come back in one copy each
        words = words.cpu().numpy()
        dcg = dcg.cpu().numpy()
        ct = counters.cpu().numpy()
        loss = float(loss.cpu()[0])
        values, per = {}, {}
        if "AUC" in self.types:
            bad = ct[_CT_BAD:_CT_BAD + C]
            if bad.any():
                raise RuntimeError(f"AUC needs labels that are 0 or 1: {int(bad.sum())} labels of "
                                   f"the evaluation set are neither")
            per["AUC"] = [auc_from_words(int(w[0]), int(w[1]), int(w[2])) for w in words]
            values["AUC"] = float(np.mean(np.array(per["AUC"], dtype=np.float64)))
        if "NDCG" in self.types:
            per["NDCG"] = [float(np.float64(d[0]) / np.float64(d[1])) if d[1] != 0 else 0.0
                           for d in dcg]
            values["NDCG"] = float(np.mean(np.array(per["NDCG"], dtype=np.float64)))
        checked, hits = int(ct[_CT_CHECKED]), int(ct[_CT_HITS])
        values["HitRate"] = hits / checked if checked else 0.0
        cnt = int(ct[_CT_SMAPE_CNT])
        ssum = float(ct[_CT_SMAPE_SUM:_CT_SMAPE_SUM + 1].view(np.float64)[0])
        values["SMAPE"] = ssum / cnt if cnt else 0.0
        values["AverageLoss"] = loss / batches if batches else 0.0
        return values, per

    def _values(self):
        """{metric name: value} of everything accumulated so far (overridden by the naming test)"""
        values, self._per_class = self._finalise()
        return values

    def result(self):
        """[(name, value)] for the spec's types in enum order; ("AverageLoss", ...) follows as the
        last entry when the spec did not name it.  Resets nothing: a second call repeats the
        first."""
        if not self:
            return []
        if self._result is None:
            v = self._values()
            out = [(t, v[t]) for t in self.types]
            if "AverageLoss" not in self.types:
                out.append(("AverageLoss", v["AverageLoss"]))
            self._result = out
        return list(self._result)

    def per_class(self, name: str = "AUC"):
        """the per-label-column values behind the last result() (AUC, NDCG)"""
        self.result()
        return list(self._per_class.get(name, []))
