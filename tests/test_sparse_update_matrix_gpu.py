"""Every dispatch branch of the sparse update (hugectr_amd/csrc/sparse_update.hip, su_segmented.hip,
the optimizer formulas of su_device.h) against plain numpy written in this file.

The two ideas the file rests on
  1. EXACT SUMS.  Every gradient is k * 2^-6 with an integer |k| <= 4 (exact in fp32, fp16 and
     bf16); mean-combiner buckets hold 1, 2 or 4 keys, so 1 / n and the product are exact too (the
     file counts in units of Q = 2^-8).  The longest run is about 2^17 positions: every partial sum,
     in any order and any tree, is a multiple of Q below 2^24 Q and therefore exact in fp32
     (_exact_sums asserts max_run * max|k| < 2^24 for every input it is given).  The reduce order no
     longer matters: the segmented kernels, the generic butterfly, hot chunks + joins, cold pieces of
     32 and the big-run chunks must all deliver THE SAME float, and one tight bound serves them all.
  2. ONE-STEP PARITY.  A case runs 3 or 4 steps (times = 1, 2, 3, ..).  Before every step the table
     and the state arrays are read back from the device and the reference computes that one step
     from those values, so a difference of one ulp never compounds.

The reference (_step / _apply) is written once over an arithmetic K and evaluated twice:
  * _F64: fp64 values that carry a running error bound (_V: every operation adds U |result| to the
    propagated bounds of its operands, U = 2^-24; the exact gradient sum enters with bound 0).  The
    assertion is |got - ref| <= bound, nothing added; "max err / bound" is printed per case.
  * _F32: a float32 numpy mirror of apply_opt, operation by operation.  The library is built with
    -ffp-contract=off (csrc/Makefile) and hipcc rounds fp32 divide and sqrt correctly unless told
    otherwise (the compile line carries neither -ffast-math nor
    -fno-hip-fp32-correctly-rounded-divide-sqrt), so every optimizer made of + - * / sqrt must be
    BIT-EQUAL to the mirror: everything but lazy Adam.  SGD (lr and scaler powers of two, table
    values multiples of 2^-11) is exact in fp32 from end to end and equals the fp64 result.
Lazy Adam calls powf.  ROCm's table of device math accuracy is not installed next to the compiler
here, so the lazy cases use the 1e-5 relative tolerance (atol 1e-6 table and m, 1e-7 v) of
test_embedding_gpu.py::test_train_steps_match_oracle as their bound.  prev_time is not exposed: the
reference tracks it (1 at the start, `times` where a row is touched) and step 2 leaves out rows that
steps 1 and 3 touch (skipped = 2).
fp16 state (fp16 embeddings): the stored value must be an fp16 number h with rn16(ref - b) <= h <=
rn16(ref + b); the weight of the same step uses the unrounded state (state_store, su_device.h).
Ftrl's soft threshold is continuous (1-Lipschitz in z), the reference bounds it as such: no element
is excluded anywhere in this file.

On every case: rows without a key keep their bits in the table and in every state (global update
types: the rows the sweep does not reach), GUARD rows behind the last row keep the poison, positions
whose index is all ones change nothing, nothing is NaN or Inf, the inputs come back unchanged and a
second run on a fresh handle gives the same bits.

What the entry points can reach.  hctr_updater_update is sum-only (it passes combiner 0), takes i64
offsets and fp32 state and has no prev_time: the mean combiner, u32 offsets, fp16 state and lazy Adam
are reached through SparseEmbeddingHash (part C), on the sorting path with HCTR_HOT_ROWS=0.

  kernel / branch                                  case that reaches it
  seg_reduce_kernel<LPR, i64, GradT, kFuseNone>    test_segmented[D-opt] for D = 4 .. 256 (LPR = 1 .. 64), every
                                                   optimizer but fused SGD / AdaGrad, f32 / f16 / bf16 inside
  seg_reduce_kernel<.., kFuseSgd / kFuseAdaGrad>   test_segmented[D-sgd], [D-adagrad]; the two-pass forms under
                                                   HCTR_SGD_FUSED=0: [D-sgd_unfused], [D-adagrad_unfused]
    run of 1, run inside a tile, run ending on a tile end, run the owner finishes alone (last position
    of tile t .. last of tile t + 1), overhang > kSegAhead, final partial tile, invalid tail (also as a
    long run: seg_combine_kernel drops it)         _seg_input(D, "classes"), offsets asserted by _seg_layout
  seg_apply_kernel<LPR, i64, kSgd = true / false>  [D-sgd_unfused] / every two-pass optimizer
  seg_combine_kernel: 2 head partials (the shortest long run), LPR - 1, LPR, LPR + 1 (the edges of a
    ballot round), the longest run it adds itself and the shortest it parks (below)   _seg_input(D, "classes")
  seg_combine_big_kernel: nch == 1 with 2048 head partials, nch == 2 with 2049 (last-arriver add);
    the shortest parked run also lands here (nch == 1)      test_segmented_big_runs[D], _seg_input(D, "big")
  update_segmented_u32 / fp16 state / lazy Adam / mean on the sorting path      test_hot_cold[..] with
                                                   HCTR_HOT_ROWS=0 (u32 keys, f16, adam_lazy, ragged batches)
  mean combiner, every LPR and every branch of the generic kernel             test_sorted_mean[D], D = 4 .. 256
                                                   and 1, 3, 6, 11, 20, 33, 100 (buckets of 0 / 1 / 2 / 4 keys)
  scale_row_offset (two ranks: divide by the global count), segmented / generic
                                                   test_distributed_mean_scale_row_offset[segmented / generic]
  run_count_kernel / run_write_kernel / update_rows_generic_kernel:
    D <= 32 and cnt > 64: butterfly, L == D (D = 1) and L > D (3, 6, 11, 20); cnt <= 64: plain sum;
    32 < D <= 64 (33) and the lane-stride loop (100); runs of 1, 64, 65, 1000     test_generic[D-opt]
    a16 == false (gradient base 4 bytes into a 16-byte line) at D = 16           test_generic_misaligned_grad
  sgd_atomic_kernel                                test_atomic_sgd[D-combiner], D = 4, 11, 32, 256
  adam / momentum / nesterov global sweeps         [D-adam_global] .. in every part; after a hot / cold
                                                   update in test_hot_cold; test_row_bound (rows below the bound)
  hot_sort / hot_reduce / hot_join / hot_apply     test_hot_cold: a hot row met once, a run inside one tile of
    32, a run across tile borders (hot_join_kernel), a row in both chunks of a stream and in several
    streams, a row absent from a batch (its loc entries stay kHotNone or the next batch would add a stale
    partial)
  cold_count / base / scatter / cold_reduce        test_hot_cold: runs of 1, 2, kShortMax = min(8 LPR, 32),
    kShortMax + 1, kColdLds = 2048 and 2049; batch 2 is ragged with nnz == buckets (the device flag sends
    every row through the cold chain, mean scaling included); batch 4 is ragged with nnz != buckets:
    both chains exit and the sorting path takes over on the same handle
  pairs_source: ext_rows (caller-presorted)        reached by hctr_updater_reduce_presorted only, which
                                                   test_ebc_matrix_gpu.py / test_ebc_unique_gpu.py cover;
    emb.update_rows (one entry per bucket)         test_update_rows
  apply_opt: every case of the switch              SGD, AdaGrad, Adam local / global, Momentum local / global,
                                                   Nesterov local / global, Ftrl (lambda1 = 0 and > 0) in parts
                                                   A and B; the nine embedding optimizers (lazy Adam among
                                                   them) in part C on the hot, cold and sorting paths

Long runs of seg_combine_kernel.  The loop that measures a run adds LPR head tiles per ballot round
and parks the run only after a FULL round that leaves n_heads > kCombBigTiles = 64: a run is parked
iff it has at least P = LPR * (64 / LPR + 1) head partials.  A run with h head partials that starts
at position p of its tile holds (32 - p) + 32 (h - 1) + (1 .. 32) positions (_run_len); the shortest
long run has two (a whole tile and one position).  Which of the two kernels adds a run cannot be
seen from outside -- with exact sums both deliver the same float -- so the cases pin the results on
both sides of the boundary, not the boundary itself.

  D     LPR   longest run it adds itself (P - 1 heads)   shortest it parks (P heads)
  4     1     64                                          65
  8     2     65                                          66
  16    4     67                                          68
  32    8     71                                          72
  64    16    79                                          80
  128   32    95                                          96
  256   64    127                                         128

Launch caps (grid-stride loops; kBlock = 256, kMaxGrid = 2048 unless named).  The cases marked grid
run two full passes and a partial third:
  seg_reduce_kernel     2^20 blocks x (256 / LPR) tiles of 32: not reachable below 2^24 sorted pairs
  seg_apply_kernel      2048 blocks x 256 positions = 524288      test_grid_seg_apply, D = 4, 1049600 positions
  seg_combine_kernel    1024 blocks x (256 / LPR) long runs; LPR = 64: 4096   test_grid_seg_combine, D = 256,
                        8200 long runs (LPR = 1 would need 2 x 262144 long runs of >= 34 positions: beyond
                        the 2^24 pairs of the radix sort, so D = 256 is the small shape here)
  seg_combine_big_kernel  256 blocks, one chunk each: 2 x 256 chunks need 2^25 positions, not reachable
  run_count / run_write 2048 blocks x kTile = 1024 positions = 2097152         test_grid_generic, D = 1,
  update_rows_generic_kernel  2048 blocks x 4 runs = 8192 runs                 4246000 positions

Under HCTR_EMU=1 (the host interpreter of tests/emu) the grid cases, the big runs and D > 64 are
dropped; part C runs there at D = 4 (the interpreter knows nothing of timing: of the two-stream
hot / cold fork it checks the logic, not the concurrency).  The arrays of part C belong to the
handle, so they have no guard rows; those of parts A and B do."""
import ctypes
import functools
import os

import numpy as np
import pytest

from util import DevIn as _In, DevOut as _Out, assert_bits as _assert_bits, lib_code as _code

pytestmark = pytest.mark.gpu

EMU = os.environ.get("HCTR_EMU") == "1"
SEED = int(os.environ.get("HCTR_TEST_SEED", "0"))  # (shared inputs; the rest draws from the fixture)
U = 2.0 ** -24  # unit roundoff of fp32
Q = 2.0 ** -8   # the unit gradients are counted in: k * 2^-6 = 4 k Q, divided by 1, 2 or 4
DTYPES = ["f32", "f16", "bf16"]
INVALID = np.uint64(2 ** 64 - 1)
SEG_TILE, COMB_BIG_TILES, COMB_BIG_CHUNK = 32, 64, 2048  # su_units.h, su_segmented.hip


def _grid(cases):
    return [] if EMU else cases


def _lib():
    from hugectr_amd import _lib
    return _lib


# ---- arithmetic: fp64 with a running error bound / the float32 mirror --------------------------------
class _V:
    """value and a bound of |computed - value| for the fp32 computation it stands for"""
    __slots__ = ("v", "b", "lo")

    def __init__(self, v, b=0.0, lo=None):
        self.v = np.asarray(v, np.float64)
        self.b = np.broadcast_to(np.asarray(b, np.float64), self.v.shape)
        # lo: the COMPUTED value is known to be >= lo >= 0 whatever the bound says (a square root, a
        # square root + epsilon: the divisors of AdaGrad and Adam, whose state may be tiny next to
        # its fp16 rounding)
        self.lo = lo

    @staticmethod
    def _of(x):
        return x if isinstance(x, _V) else _V(np.float64(x))

    @staticmethod
    def _rounded(v, b):
        return _V(v, b + U * (np.abs(v) + b))  # the computed result is rounded once more

    def __neg__(self):
        return _V(-self.v, self.b)

    def __add__(self, o):
        o = _V._of(o)
        r = _V._rounded(self.v + o.v, self.b + o.b)
        if self.lo is not None and (o.b == 0).all() and (o.v >= 0).all():
            r.lo = (self.lo + o.v) * (1 - U)
        return r

    def __sub__(self, o):
        o = _V._of(o)
        return _V._rounded(self.v - o.v, self.b + o.b)

    def __mul__(self, o):
        o = _V._of(o)
        return _V._rounded(self.v * o.v, np.abs(self.v) * o.b + np.abs(o.v) * self.b + self.b * o.b)

    def __truediv__(self, o):
        o = _V._of(o)
        den = np.abs(o.v) - o.b  # |computed divisor| >= den
        if o.lo is not None:
            den = np.maximum(den, o.lo)
        assert (den > 0).all(), "a divisor's interval holds zero"
        v = self.v / o.v
        return _V._rounded(v, (self.b + np.abs(v) * o.b) / den)

    def sqrt(self):
        assert (self.v >= 0).all()
        v = np.sqrt(self.v)
        lo, hi = np.sqrt(np.maximum(self.v - self.b, 0.0)), np.sqrt(self.v + self.b)
        r = _V._rounded(v, np.maximum(v - lo, hi - v))
        r.lo = np.zeros_like(v)
        return r

    def __getitem__(self, i):
        return _V(self.v[i], self.b[i])

    def copy(self):
        return _V(self.v.copy(), self.b.copy())

    def put(self, i, x):
        if not self.b.flags.writeable:
            self.b = self.b.copy()
        self.v[i], self.b[i] = x.v, x.b


class _F64:
    bits = False

    @staticmethod
    def c(x):
        return _V(np.float64(np.float32(x)))  # (constants are the floats the kernels hold)

    @staticmethod
    def arr(x):
        return _V(np.array(x, np.float64))

    @staticmethod
    def sqrt(x):
        return x.sqrt()

    @staticmethod
    def store16(x):
        # |rn16(y) - y| <= 2^-11 |y| (y normal in fp16) or 2^-25 (subnormal), y the computed fp32
        # value; a y that is known to be zero stays zero (the state of a row never handed out)
        top = np.abs(x.v) + x.b
        e = np.where(top >= 2.0 ** -14, 2.0 ** -11 * top, 2.0 ** -25)
        return _V(x.v, x.b + np.where(top == 0, 0.0, e))

    @staticmethod
    def ftrl_w(zi, l1, q):
        """w = p / q * [|z| > l1], p = sign(z) l1 - z: the soft threshold -sign(z) max(|z| - l1, 0) / q,
        1-Lipschitz in z -- on either side of |z| = l1 the computed p is within z's bound (+ its own
        rounding) of it"""
        s = -np.sign(zi.v) * np.maximum(np.abs(zi.v) - l1.v, 0.0)
        return _V(s, zi.b + U * (np.abs(s) + zi.b)) / q

    @staticmethod
    def put(a, i, x):
        a.put(i, x)


class _F32:
    bits = True

    @staticmethod
    def c(x):
        return np.float32(x)

    @staticmethod
    def arr(x):
        return np.array(x, np.float32)

    @staticmethod
    def sqrt(x):
        return np.sqrt(x)

    @staticmethod
    def store16(x):
        return x.astype(np.float16).astype(np.float32)

    @staticmethod
    def ftrl_w(zi, l1, q):
        one, two = np.float32(1), np.float32(2)
        p = (one - two * np.signbit(zi).astype(np.float32)) * l1 - zi
        return p / q * np.signbit(l1 - np.abs(zi)).astype(np.float32)

    @staticmethod
    def put(a, i, x):
        assert x.dtype == np.float32, "the mirror left float32"
        a[i] = x


# ---- the optimizers ------------------------------------------------------------------------------------
SGD, ADAGRAD, ADAM, MOMENTUM, NESTEROV, FTRL = "sgd", "adagrad", "adam", "momentum", "nesterov", "ftrl"
LOCAL, GLOBAL, LAZY = 0, 1, 2


class _Opt:
    def __init__(self, name, kind, ut=LOCAL, ns=0, lr=0.05, scaler=2.0, mf=0.0, ftrl=None, fused=True):
        self.name, self.kind, self.ut, self.ns, self.fused, self.ftrl = name, kind, ut, ns, fused, ftrl
        f = np.float32
        self.lr, self.scaler, self.mf = f(lr), f(scaler), f(mf)
        self.b1, self.b2, self.eps = f(0.9), f(0.999), f(1e-7)

    @property
    def code(self):
        L = _lib()
        return {SGD: L.OPT_SGD, ADAGRAD: L.OPT_ADAGRAD, ADAM: L.OPT_ADAM, MOMENTUM: L.OPT_MOMENTUM_SGD,
                NESTEROV: L.OPT_NESTEROV, FTRL: L.OPT_FTRL}[self.kind]

    # opt_const (su_device.h): host float arithmetic, restated in float32
    def alpha_t(self, times):
        # AdamOptHyperParams::bias() (optimizer.hpp:58-60): double pow, rounded to float, times lr
        b1, b2 = float(self.b1), float(self.b2)
        bias = np.float32(np.sqrt(1.0 - b2 ** float(times)) / (1.0 - b1 ** float(times)))
        return self.lr * bias

    def alpha_t_common(self):
        return self.lr / (np.float32(1) - self.b1)

    def ftrl_l2b(self):
        return np.float32(self.ftrl[1]) + np.float32(self.ftrl[2]) / self.lr


# SGD: lr / scaler = 2^-5 and table values multiples of 2^-11 keep every intermediate exact
_OPT_LIST = [
    _Opt("sgd", SGD, lr=0.125, scaler=4.0),
    _Opt("sgd_unfused", SGD, lr=0.125, scaler=4.0, fused=False),
    _Opt("adagrad", ADAGRAD, ns=1),
    _Opt("adagrad_unfused", ADAGRAD, ns=1, fused=False),
    _Opt("adam_local", ADAM, LOCAL, ns=2),
    _Opt("adam_global", ADAM, GLOBAL, ns=2),
    _Opt("momentum_local", MOMENTUM, LOCAL, ns=1, mf=0.9),
    _Opt("momentum_global", MOMENTUM, GLOBAL, ns=1, mf=0.9),
    _Opt("nesterov_local", NESTEROV, LOCAL, ns=1, mf=0.9),
    _Opt("nesterov_global", NESTEROV, GLOBAL, ns=1, mf=0.9),
    _Opt("ftrl_l1_0", FTRL, ns=2, ftrl=(0.0, 0.05, 0.3)),
    _Opt("ftrl", FTRL, ns=2, ftrl=(0.02, 0.05, 0.3)),
]
OPTS = {o.name: o for o in _OPT_LIST}
UPDATER_OPTS = list(OPTS)
# Lazy Adam's step is a m / (sqrt(v) + epsilon) with a ~ sqrt(1 - beta2^t): in fp32 that difference
# loses four digits (1 - 0.999 of a power rounded at 6e-8), so `a` carries a relative error of about
# 1.5e-5 whatever powf does, and the 1e-5 tolerance only holds while the step is small next to the
# weight.  It is, as long as v does not vanish next to m: v = 0.001 g^2 of the smallest gradient sum
# (2^-8 / scaler) must stay above fp16's subnormal quantum 2^-24, or fp16 state stores v = 0 and the
# step becomes a m / epsilon (weights move by 6 at scaler 2).  scaler = 2^-4: v >= 3.9e-6.
ADAM_LAZY = _Opt("adam_lazy", ADAM, LAZY, ns=2, scaler=0.0625)
# the nine optimizers of SparseEmbeddingHash (the reference's GPU update has no Ftrl: SURVEY q9)
EMB_OPTS = {n: OPTS[n] for n in ["sgd", "adagrad", "adam_local", "adam_global", "momentum_local",
                                 "momentum_global", "nesterov_local", "nesterov_global"]}
EMB_OPTS["adam_lazy"] = ADAM_LAZY


def _apply(K, o, times, gsum, w, s0, s1):
    """row_compute + apply_opt (su_device.h) on the touched rows, one operation per line of the source
    -> (w, s0, s1) with the states NOT yet rounded to the state type"""
    c, one = K.c, K.c(1.0)
    gi = gsum / c(o.scaler)
    lr, mf, b1, b2, eps = c(o.lr), c(o.mf), c(o.b1), c(o.b2), c(o.eps)
    if o.kind == SGD:  # opt_sgd_kernel, sparse_optimizer.cu:497-518
        return w + (-lr) * gi, None, None
    if o.kind == ADAGRAD:  # opt_adagrad_kernel :410-437
        accum = s0 + gi * gi
        return w + (-lr) * gi / (K.sqrt(accum) + eps), accum, None
    if o.kind == ADAM and o.ut == LOCAL:  # opt_adam_kernel :379-408
        mi = b1 * s0 + (one - b1) * gi
        vi = b2 * s1 + (one - b2) * gi * gi
        return w + (-c(o.alpha_t(times))) * mi / (K.sqrt(vi) + eps), mi, vi
    if o.kind == ADAM and o.ut == GLOBAL:  # opt_adam_kernel_global :241-265
        return w, s0 + (one - b1) * gi / b1, s1 + (one - b2) * gi * gi / b2
    if o.kind == MOMENTUM and o.ut == LOCAL:  # opt_momentum_sgd_kernel :440-465
        mo = mf * s0 - lr * gi
        return w + mo, mo, None
    if o.kind == MOMENTUM:  # opt_momentum_sgd_kernel_global :292-312
        return w, s0 - lr * gi / mf, None
    if o.kind == NESTEROV and o.ut == LOCAL:  # opt_nesterov_kernel :468-494
        new = mf * s0 - lr * gi
        return w + ((-mf) * s0 + (one + mf) * new), new, None
    if o.kind == NESTEROV:  # nesterov_local_update_kernel_global :352-375
        return w - (one + mf) * (lr * gi), s0 - lr * gi, None
    assert o.kind == FTRL  # FtrlOptimizer::update, ragged_static_embedding.cu:159-290 (s0 = n, s1 = z)
    e23 = c(1.1920929e-07)
    sq = K.sqrt(s0 + e23)
    ni = s0 + gi * gi
    sqn = K.sqrt(ni + e23)
    sigma = (sqn - sq) / lr
    zi = s1 + gi - sigma * w
    q = sqn / lr + c(o.ftrl_l2b())
    return K.ftrl_w(zi, c(o.ftrl[0]), q), ni, zi


def _step(K, o, times, rows, gsum, w, s0, s1, sweep, half):
    """one update of the whole table: the sweep of a global update type over the first `sweep` rows
    (before the rows of the batch: Nesterov; after them: Adam, momentum SGD), apply_opt on `rows`
    (ascending, unique) with the exact gradient sums gsum [len(rows), D].  States come back
    unrounded (fp16 state: the device stores rn16 of them); where a sweep reads a state the batch's
    rows wrote, it reads the rounded value."""
    W = K.arr(w)
    S = [K.arr(s) if s is not None else None for s in (s0, s1)]  # what device memory holds
    F = [K.arr(s) if s is not None else None for s in (s0, s1)]  # the last value written, unrounded
    st = K.store16 if half else (lambda x: x)

    def put_state(k, i, x):
        K.put(F[k], i, x)
        K.put(S[k], i, st(x))

    sw = slice(0, sweep)
    glob = o.ut == GLOBAL and o.kind in (ADAM, MOMENTUM, NESTEROV)
    if glob and o.kind == NESTEROV:  # nesterov_global_update_kernel_global :333-347
        a = S[0][sw] * K.c(o.mf)
        K.put(W, sw, W[sw] + a * K.c(o.mf))
        put_state(0, sw, a)
    if len(rows):
        nw, n0, n1 = _apply(K, o, times, K.arr(gsum), W[rows], S[0][rows] if S[0] is not None else None,
                            S[1][rows] if S[1] is not None else None)
        K.put(W, rows, nw)
        for k, n in enumerate((n0, n1)):
            if n is not None:
                put_state(k, rows, n)
    if glob and o.kind == ADAM:  # adam_update_kernel_global :269-288
        mi, vi = K.c(o.b1) * S[0][sw], K.c(o.b2) * S[1][sw]
        put_state(0, sw, mi)
        put_state(1, sw, vi)
        K.put(W, sw, W[sw] + (-K.c(o.alpha_t(times))) * mi / (K.sqrt(vi) + K.c(o.eps)))
    if glob and o.kind == MOMENTUM:  # momentum_sgd_update_kernel_global :316-329
        m = S[0][sw] * K.c(o.mf)
        K.put(W, sw, W[sw] + m)
        put_state(0, sw, m)
    return W, F[0], F[1]


def _step_lazy(o, times, rows, gsum, w, s0, s1, pt):
    """opt_adam_kernel_lazy :524-561 in fp64 with the bound of the module docstring (powf)"""
    b1, b2, eps = float(o.b1), float(o.b2), float(o.eps)
    omb1, omb2 = float(np.float32(1) - o.b1), float(np.float32(1) - o.b2)
    W, M, V = (_V(np.array(x, np.float64)) for x in (w, s0, s1))
    gi = gsum / float(o.scaler)
    p = pt[rows].astype(np.float64)[:, None]
    skipped = float(times) - p
    b1ps = b1 ** skipped
    a = float(o.alpha_t_common()) * np.sqrt(1.0 - b2 ** p) / (1.0 - b1 ** p) * (1.0 - b1ps)
    mi, vi = M.v[rows], V.v[rows]
    nw = W.v[rows] - a * mi / (np.sqrt(vi) + eps)
    nm = b1ps * mi + omb1 * gi
    nv = b2 ** skipped * vi + omb2 * gi * gi
    for A, x, atol in ((W, nw, 1e-6), (M, nm, 1e-6), (V, nv, 1e-7)):
        A.put(rows, _V(x, 1e-5 * np.abs(x) + atol))
    return W, M, V


# ---- checks ------------------------------------------------------------------------------------------
def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def _check(what, got, ref, half=False):
    """got (float32 view of what the device holds) against the bounded reference -> max err / bound"""
    assert np.isfinite(got).all(), f"{what}: NaN or Inf"
    g = got.astype(np.float64)
    err = np.abs(g - ref.v)
    if half:
        # an fp16 number between the roundings of the interval's ends
        lo = (ref.v - ref.b).astype(np.float16).astype(np.float64)
        hi = (ref.v + ref.b).astype(np.float16).astype(np.float64)
        bad = (g < lo) | (g > hi)
        r = _ratio(err, np.maximum(hi - ref.v, ref.v - lo))
    else:
        bad = err > ref.b
        r = _ratio(err, ref.b)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} elements outside the bound, first at "
                             f"{i}: got {got[i]!r}, want {ref.v[i]!r} +- {ref.b[i]:.3e}")
    return r


def _same_bits(what, got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    _assert_bits(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1]), what)


def _dyadic(shape, step, lo, hi):
    """multiples of `step` in (lo, hi), drawn from the generator the conftest fixture seeded"""
    k = np.random.randint(int(round(lo / step)) + 1, int(round(hi / step)), size=shape)
    return (k * step).astype(np.float32)


def _as_type(x, dt):
    """fp32 values exact in dt -> the host array whose bytes the device reads"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dt == "f32":
        return x
    if dt == "f16":
        y = x.astype(np.float16)
        assert (y.astype(np.float32) == x).all()
        return y
    assert (x.view(np.uint32) & 0xFFFF == 0).all()
    return (x.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def _exact_sums(rows, grow, scale4, kg):
    """per-row gradient sums, exact: rows[j] >= 0 the row of (valid) position j, grow[j] its gradient
    row, scale4[j] = 4 / (keys of its bucket: 1, 2, 4; sum combiner: 4), kg [.., D] the integers k of
    the gradients k * 2^-6 -> (unique rows ascending, sums as float64 [n, D], longest run).  Asserts
    the precondition under which every fp32 partial sum in any order is exact."""
    order = np.argsort(rows, kind="stable")
    urows, starts, counts = np.unique(rows[order], return_index=True, return_counts=True)
    max_run = int(counts.max()) if counts.size else 0
    assert max_run * int(np.abs(kg).max()) * 4 < 2 ** 24, "a partial sum could leave fp32's 24 bits"
    D = kg.shape[1]
    sums = np.zeros((urows.size, D), np.int64)
    step = max(1, (1 << 22) // D)  # positions gathered at a time
    run_of = np.repeat(np.arange(urows.size), counts)
    for a in range(0, order.size, step):
        j, ro = order[a:a + step], run_of[a:a + step]
        v = kg[grow[j]].astype(np.int32) * scale4[j][:, None].astype(np.int32)
        cut = np.flatnonzero(np.diff(ro, prepend=ro[0] - 1))  # (a run's pieces of several chunks add up)
        sums[ro[cut]] += np.add.reduceat(v, cut, axis=0, dtype=np.int64)
    return urows, sums.astype(np.float64) * Q, max_run


# ---- parts A and B: hctr_updater_update ------------------------------------------------------------------
def _run_len(phase, heads, last):
    """a run that starts at position `phase` of its tile and has `heads` head partials, the last of
    `last` positions: the rest of its own tile, heads - 1 whole tiles, `last` positions"""
    return (SEG_TILE - phase) + SEG_TILE * (heads - 1) + last


def _parked_from(lpr):
    return lpr * (COMB_BIG_TILES // lpr + 1)


def _seg_layout(D, kind):
    """[(phase, length)] of the run classes of the module docstring"""
    lpr = D // 4
    P = _parked_from(lpr)
    if kind == "big":
        return [(31, _run_len(31, COMB_BIG_CHUNK, 32)), (5, _run_len(5, COMB_BIG_CHUNK + 1, 1)), (9, 3)]
    runs = [(None, 1), (3, 10), (20, 12), (31, 33), (30, 50), (31, 34), (0, _run_len(0, 2, 5))]
    phases = [31, 0, 17]
    for i, h in enumerate(sorted({lpr - 1, lpr, lpr + 1, P - 1, P} - {0, 1})):
        runs.append((phases[i % 3], _run_len(phases[i % 3], h, [1, 32, 7][i % 3])))
    return runs


@functools.lru_cache(maxsize=None)
def _seg_input(D, kind):
    """the sorted list is fixed by row ids and counts (rows sort ascending, the sort is stable): the
    classes at their offsets, single rows in between, every second row id left out; "classes" ends
    with a partial tile and a tail of 100 invalid positions (a long run of its own), "big" with a
    partial tile of live rows.  The positions themselves are a random permutation in ragged buckets
    of 0 / 1 / 2 / 4 keys ("big": 300 buckets of hundreds)."""
    rng = np.random.default_rng(9100 + D + 7919 * SEED)
    rows, cur, row, where = [], 0, 0, []
    for phase, length in _seg_layout(D, kind):
        while phase is not None and cur % SEG_TILE != phase:
            rows.append(np.array([row], np.uint64))
            cur, row = cur + 1, row + 2
        where.append((cur, length, row))
        rows.append(np.full(length, row, np.uint64))
        cur, row = cur + length, row + 1 + (cur & 1)
    while cur % SEG_TILE != 5:
        rows.append(np.array([row], np.uint64))
        cur, row = cur + 1, row + 2
    n_rows = row + 3
    if kind == "classes":
        rows.append(np.full(100, INVALID, np.uint64))
    idx = np.concatenate(rows)
    # the layout the kernels will see, restated from the sorted list
    s = np.sort(idx)
    for off, length, r in where:
        assert (s[off:off + length] == r).all() and (off == 0 or s[off - 1] != r) and s[off + length] != r
    idx = idx[rng.permutation(idx.size)]
    nnz = idx.size
    assert nnz % SEG_TILE != 0
    if kind == "big":
        cuts = np.sort(rng.integers(0, nnz + 1, size=299))
        br = np.concatenate([[0], cuts, [nnz]]).astype(np.int64)
    else:
        lens = rng.choice([0, 1, 2, 4], size=nnz)
        br = np.concatenate([[0], np.cumsum(lens)])
        br = np.concatenate([br[br < nnz], [nnz]]).astype(np.int64)
    for a in (idx, br):
        a.setflags(write=False)
    return idx, br, n_rows


@functools.lru_cache(maxsize=None)
def _gen_input(D):
    """generic kernel: runs of 1, 64, 65 and 1000 (twice, other rows in between), single rows, a tail
    of invalid positions"""
    rng = np.random.default_rng(9200 + D + 7919 * SEED)
    rows, row = [], 0
    for length in [1, 64, 65, 1000, 2, 65, 64, 1000, 1, 1, 33]:
        rows.append(np.full(length, row, np.uint64))
        row += 2
    rows.append(np.full(7, INVALID, np.uint64))
    idx = np.concatenate(rows)
    idx = idx[rng.permutation(idx.size)]
    lens = rng.choice([0, 1, 2, 4], size=idx.size)
    br = np.concatenate([[0], np.cumsum(lens)])
    br = np.concatenate([br[br < idx.size], [idx.size]]).astype(np.int64)
    for a in (idx, br):
        a.setflags(write=False)
    return idx, br, row + 1


@functools.lru_cache(maxsize=None)
def _kgrad(nb, D, seed):
    """the integers k of nb gradient rows k * 2^-6, |k| <= 4 (shared, never written)"""
    k = np.random.default_rng(9300 + seed + 7919 * SEED).integers(-4, 5, size=(nb, D)).astype(np.int8)
    k.setflags(write=False)
    return k


class _Table:
    """table / state arrays of `rows` rows behind GUARD rows of poison, as fp32 or fp16"""

    def __init__(self, init, half=False):
        import torch
        self.rows, self.D = init.shape
        self.out = _Out(self.rows, self.D, "f16" if half else "f32")
        src = torch.from_numpy(np.ascontiguousarray(init, np.float16 if half else np.float32))
        self.out.t[:self.rows * self.D] = src.reshape(-1).to("cuda")

    @property
    def p(self):
        return self.out.p

    def read(self):
        return self.out.result().astype(np.float32)


def _updater_run(inp, D, dt, o, init, steps, row_bound=0, mis=0):
    """the steps of one case on a fresh handle -> [(before, after)] per step, each (w, s0, s1)"""
    import torch
    L = _lib()
    idx_h, br_h, n_rows = inp
    nb, nnz = br_h.size - 1, idx_h.size
    upd = ctypes.c_void_p()
    L.check(L.lib.hctr_updater_create(nnz, n_rows, D, ctypes.byref(upd)))
    try:
        if o.kind == FTRL:
            L.check(L.lib.hctr_updater_set_ftrl(upd, *[float(x) for x in o.ftrl]))
        if row_bound:
            L.check(L.lib.hctr_updater_set_row_bound(upd, row_bound))
        idx, br = _In(idx_h), _In(br_h)
        tabs = [_Table(init[0])] + [_Table(init[1 + k]) if k < o.ns else None for k in range(2)]
        trace = []
        for step in range(steps):
            grad = _In(_as_type(_kgrad(nb, D, step).astype(np.float32) * np.float32(2.0 ** -6), dt),
                       mis=mis)
            before = [t.read() if t else None for t in tabs]
            L.check(L.lib.hctr_updater_update(
                upd, nb, nnz, br.p, idx.p, grad.p, _code(dt), o.code, o.ut, float(o.lr), float(o.b1),
                float(o.b2), float(o.eps), float(o.mf), float(o.scaler), step + 1, tabs[0].p,
                tabs[1].p if tabs[1] else None, tabs[2].p if tabs[2] else None, L.stream_ptr()))
            torch.cuda.synchronize()
            trace.append((before, [t.read() if t else None for t in tabs]))
            for x, name in ((idx, "indices"), (br, "bucket_range"), (grad, "grad")):
                x.assert_unchanged(name)
        return trace
    finally:
        L.lib.hctr_updater_destroy(upd)


def _verify_step(tag, o, times, urows, gsum, before, after, sweep, half=False, pt=None):
    """one step against both references + the structural checks -> max err / bound"""
    names = ("table", "state0", "state1")
    before = (list(before) + [None, None])[:3]
    if o.ut == LAZY:
        ref = _step_lazy(o, times, urows, gsum, *before, pt)
        mirror = None
    else:
        ref = _step(_F64, o, times, urows, gsum, *before, sweep, half)
        mirror = _step(_F32, o, times, urows, gsum, *before, sweep, half)
    worst = 0.0
    frozen = np.ones(before[0].shape[0], bool)  # rows nothing may touch
    frozen[urows] = False
    if o.ut == GLOBAL and o.kind in (ADAM, MOMENTUM, NESTEROV):
        frozen[:sweep] = False
    for k in range(1 + o.ns):
        is_half = half and k > 0
        worst = max(worst, _check(f"{tag} {names[k]}", after[k], ref[k], is_half))
        _same_bits(f"{tag} {names[k]}: rows without a key", after[k][frozen], before[k][frozen])
        if mirror is not None:
            m = mirror[k]
            assert m.dtype == np.float32
            _same_bits(f"{tag} {names[k]} against the float32 mirror", after[k],
                       _F32.store16(m) if is_half else m)
    if o.kind == SGD:  # exact from end to end: the fp64 result itself
        assert (after[0].astype(np.float64) == ref[0].v).all(), f"{tag}: SGD is not exact"
    return worst


def _updater_case(inp, D, dt, o, monkeypatch, steps=3, row_bound=0, mis=0, init=None, verify=True):
    monkeypatch.setenv("HCTR_SGD_FUSED", "1" if o.fused else "0")
    idx_h, br_h, n_rows = inp
    nb = br_h.size - 1
    if init is None:
        init = [_dyadic((n_rows, D), 2.0 ** -11, -1, 1), _dyadic((n_rows, D), 2.0 ** -8, 0, 1),
                _dyadic((n_rows, D), 2.0 ** -8, 0, 1)]
    trace = _updater_run(inp, D, dt, o, init, steps, row_bound, mis)
    again = _updater_run(inp, D, dt, o, init, steps, row_bound, mis)
    for k in range(1 + o.ns):
        _same_bits(f"array {k} of a second run on a fresh handle", again[-1][1][k], trace[-1][1][k])
    if not verify:
        return trace
    live = idx_h != INVALID
    rows = idx_h[live].astype(np.int64)
    grow = np.repeat(np.arange(nb), np.diff(br_h))[live]
    worst = 0.0
    for step, (before, after) in enumerate(trace):
        urows, gsum, max_run = _exact_sums(rows, grow, np.full(rows.size, 4, np.int64),
                                           _kgrad(nb, D, step))
        worst = max(worst, _verify_step(f"{o.name} D={D} {dt} step {step + 1}", o, step + 1, urows, gsum,
                                        before[:1 + o.ns], after, row_bound or n_rows))
    print(f"sparse update {o.name} D={D} {dt} nnz={idx_h.size} longest run {max_run}: "
          f"max err / bound = {worst:.3f}")
    return trace


SEG_D = [4, 8, 16, 32, 64, 128, 256]


@pytest.mark.parametrize("name", UPDATER_OPTS)
@pytest.mark.parametrize("D", [d for d in SEG_D if not (EMU and d > 64)])
def test_segmented(D, name, monkeypatch):
    """part A: every LPR x gradient type x optimizer on the run classes of _seg_input"""
    for dt in DTYPES:
        _updater_case(_seg_input(D, "classes"), D, dt, OPTS[name], monkeypatch)


@pytest.mark.parametrize("D", _grid(SEG_D))
def test_segmented_big_runs(D, monkeypatch):
    """runs of 2048 head partials (one chunk of seg_combine_big_kernel) and 2049 (two chunks, the
    last arriver adds): SGD (exact) and a two-state optimizer, one gradient type per D"""
    dt = DTYPES[SEG_D.index(D) % 3]
    for name in ("sgd", "adam_local"):
        _updater_case(_seg_input(D, "big"), D, dt, OPTS[name], monkeypatch)


@pytest.mark.parametrize("name", ["adam_global", "momentum_global", "nesterov_global"])
def test_row_bound(name, monkeypatch):
    """hctr_updater_set_row_bound below max_rows: the sort covers fewer key bits and the sweep stops
    at the bound -- the rows behind it carry state and must keep it"""
    idx_h, br_h, n_rows = _seg_input(16, "classes")
    bound = int(idx_h[idx_h != INVALID].max()) + 2
    assert bound < n_rows
    inp = (idx_h, br_h, n_rows + 40)
    _updater_case(inp, 16, "f32", OPTS[name], monkeypatch, row_bound=bound)


GEN_D = [1, 3, 6, 11, 20, 33, 100]


@pytest.mark.parametrize("name", UPDATER_OPTS)
@pytest.mark.parametrize("D", GEN_D)
def test_generic(D, name, monkeypatch):
    """part B: update_rows_generic_kernel behind run_count / run_write"""
    for dt in DTYPES:
        _updater_case(_gen_input(D), D, dt, OPTS[name], monkeypatch)


@pytest.mark.parametrize("name", ["sgd", "adam_local"])
def test_generic_misaligned_grad(name, monkeypatch):
    """D = 16 with the gradient 4 bytes into a 16-byte line: update_typed's a16 test must send it to
    the generic kernel (the segmented one loads 16 bytes at a time), with the aligned run's bits"""
    inp, o = _seg_input(16, "classes"), OPTS[name]
    init = [_dyadic((inp[2], 16), 2.0 ** -11, -1, 1), _dyadic((inp[2], 16), 2.0 ** -8, 0, 1),
            _dyadic((inp[2], 16), 2.0 ** -8, 0, 1)]
    a = _updater_case(inp, 16, "f32", o, monkeypatch, init=init)
    b = _updater_case(inp, 16, "f32", o, monkeypatch, init=init, mis=1)
    for k in range(1 + o.ns):
        _same_bits("misaligned against aligned", b[-1][1][k], a[-1][1][k])


# ---- launch caps ---------------------------------------------------------------------------------------
def _many_runs_input(n_runs, run_len, singles, seed):
    rng = np.random.default_rng(9400 + seed + 7919 * SEED)
    idx = np.concatenate([np.repeat(np.arange(n_runs, dtype=np.uint64) * 2, run_len),
                          2 * n_runs + np.arange(singles, dtype=np.uint64)])
    idx = idx[rng.permutation(idx.size)]
    cuts = np.sort(rng.integers(0, idx.size + 1, size=255))
    br = np.concatenate([[0], cuts, [idx.size]]).astype(np.int64)
    return idx, br, 2 * n_runs + singles + 1


@pytest.mark.parametrize("name", _grid(["sgd_unfused", "momentum_local"]))
def test_grid_seg_apply(name, monkeypatch):
    """seg_apply_kernel, both kSgd forms: 2 x 524288 positions and a partial third pass"""
    inp = _many_runs_input(100, 40, 2 * 2048 * 256 + 1024 - 4000, 1)
    assert inp[0].size == 1049600 and inp[0].size > 2 * 2048 * 256
    _updater_case(inp, 4, "f32", OPTS[name], monkeypatch)


@pytest.mark.parametrize("name", _grid(["adam_local"]))
def test_grid_seg_combine(name, monkeypatch):
    """seg_combine_kernel at LPR = 64: 1024 blocks x 4 lane groups, 8200 long runs"""
    inp = _many_runs_input(8200, 65, 37, 2)
    assert 8200 > 2 * 1024 * (256 // 64)
    _updater_case(inp, 256, "bf16", OPTS[name], monkeypatch)


@pytest.mark.parametrize("name", _grid(["adagrad"]))
def test_grid_generic(name, monkeypatch):
    """run_count_kernel / run_write_kernel: 4147 tiles of 1024 positions; update_rows_generic_kernel:
    far more than 2 x 8192 runs"""
    inp = _many_runs_input(2000, 70, 4246000 - 140000, 3)
    assert inp[0].size == 4246000 and inp[0].size > 2 * 2048 * 1024
    _updater_case(inp, 1, "f16", OPTS[name], monkeypatch)


# ---- part C: the embedding handle -- hot / cold chains, u32, fp16 state, lazy Adam, mean ------------------
HC_B, HC_S, HC_H, HC_V = 4100, 4, 8, 2048  # samples, slots (= streams), hot rows, rows of the table
HOT_CHUNK, COLD_LDS = 4096, 2048           # kHotChunk, kColdLds (sparse_update.hip)
HOT0 = 1000                                 # keys HOT0 .. HOT0 + 7 become the hot rows 0 .. 7
COLD0 = 5000


def _short_max(D):
    return min(8 * (D // 4), 32)  # ColdShape<LPR>::kShortMax


@functools.lru_cache(maxsize=None)
def _hc_batches(sm):
    """the four batches of a hot / cold case (keys as int64, row offsets) for kShortMax = sm.
    Batch 1, one-hot, decides the rows: the table hands them out in first-occurrence order, and the
    first two samples hold the eight hot keys.
      hot: h0 once; h1 10 x in stream 1 (inside the first tile of 32 of its chunk); h2 100 x in stream 2
      (across tile borders: hot_join_kernel), h6 40 x behind it; h3 in streams 0, 1 and 3 and in both
      chunks of each (samples >= 4096); h7 33 x; h4 / h5 a few times
      cold: 300 rows met once, runs of 2, sm and sm + 1 (several each), 2048 and 2049, ~150 rows of
      dozens of positions (sorted inside LDS)
    Batch 2, ragged with as many keys as buckets (groups of four buckets holding 1111 / 2020 / 0211 /
    4000 / 0004 keys): the device flag sends every row through the cold chain; it leaves out h5 and
    a fifth of the cold keys (lazy Adam: skipped = 2 in batch 3) and brings new keys.
    Batch 3, one-hot again: batch 1 shuffled below the first two samples, WITHOUT h4 (its loc entries
    of batch 1 must have gone back to kHotNone) and h1.
    Batch 4, ragged with nnz != buckets (0 / 1 / 2 / 4 keys): both chains exit, the sorting path runs."""
    rng = np.random.default_rng(9500 + sm + 7919 * SEED)
    B, S = HC_B, HC_S
    K = np.full((B, S), -1, np.int64)
    h = HOT0 + np.arange(8)
    K[0], K[1] = h[:4], h[4:]
    K[2:11, 1] = h[1]                       # 10 with sample 0
    K[2:101, 2] = h[2]                      # 100
    K[101:140, 2] = h[6]                    # 40 with sample 1
    K[4090:4100, [0]] = h[3]
    K[4090:4100, [1]] = h[3]
    K[4090:4100, [3]] = h[3]
    K[200:261, 3] = h[3]
    K[200:261, 0] = h[3]
    K[300:332, 3] = h[7]                    # 33 with sample 1
    K[400:404, 0] = h[4]
    K[500:506, 1] = h[5]
    counts = [1] * 300 + [2] * 5 + [sm] * 3 + [sm + 1] * 3 + [COLD_LDS, COLD_LDS + 1] + [3, 5, 7]
    free = np.argwhere(K.reshape(-1) < 0).reshape(-1)
    rest = free.size - sum(counts)
    fill = rng.multinomial(rest, np.full(150, 1 / 150))
    counts = np.array(counts + list(fill[fill > 0]))
    cold = np.repeat(COLD0 + np.arange(counts.size), counts)
    K.reshape(-1)[free] = cold[rng.permutation(cold.size)]
    k1 = K.reshape(-1).copy()
    ro1 = np.arange(B * S + 1, dtype=np.int64)
    # batch 3: the rows below the first two samples shuffled, h4 and h1 replaced by a cold key
    K3 = K.copy()
    K3[2:] = K[2:][rng.permutation(B - 2)]
    K3[0, 1], K3[1, 0] = COLD0, COLD0 + 1
    K3[(K3 == h[4]) | (K3 == h[1])] = COLD0 + 2
    k3 = K3.reshape(-1).copy()
    assert (k3 != h[4]).all() and (k3 == h[5]).any() and (k3 == h[2]).sum() == 100
    # batch 2: nnz == buckets, ragged
    known = np.unique(k1)
    skip = np.concatenate([[h[5]], known[known >= COLD0][::5]])
    pool = np.concatenate([np.setdiff1d(known, skip), 9000 + np.arange(40)])
    pat = np.array([[1, 1, 1, 1], [2, 0, 2, 0], [0, 2, 1, 1], [4, 0, 0, 0], [0, 0, 0, 4]])
    lens2 = pat[rng.integers(0, len(pat), size=B * S // 4)].reshape(-1)
    ro2 = np.concatenate([[0], np.cumsum(lens2)]).astype(np.int64)
    assert ro2[-1] == B * S
    w = np.where(pool < COLD0, 40.0, 1.0)  # (the hot rows get long runs here too)
    k2 = pool[rng.choice(pool.size, size=B * S, p=w / w.sum())]
    assert not np.isin(k2, skip).any() and np.isin(k3, skip).any()
    # batch 4: nnz != buckets
    lens4 = rng.choice([0, 1, 2, 4], size=B * S)
    ro4 = np.concatenate([[0], np.cumsum(lens4)]).astype(np.int64)
    assert ro4[-1] != B * S and ro4[-1] <= B * S * 4
    k4 = np.concatenate([known, 9000 + np.arange(60)])[rng.integers(0, known.size + 60, size=ro4[-1])]
    out = [(ro1, k1), (ro2, k2), (ro1, k3), (ro4, k4)]
    for ro, k in out:
        ro.setflags(write=False)
        k.setflags(write=False)
    return out


def _torch_dt(dt):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]


def _emb_opt(o, atomic=False):
    import hugectr_amd as ha
    return ha.OptParams(optimizer=o.code, update_type=o.ut, lr=float(o.lr), beta1=float(o.b1),
                        beta2=float(o.b2), epsilon=float(o.eps), momentum_factor=float(o.mf),
                        atomic_update=atomic, scaler=float(o.scaler))


def _emb_states(emb, ns):
    return [emb.table().cpu().numpy().copy()] + [emb.opt_state(k).float().cpu().numpy().copy()
                                                 for k in range(ns)]


def _emb_run(batches, D, dt, kt, o, combiner, hot_rows, monkeypatch, init, V=HC_V, B=HC_B, S=HC_S,
             atomic=False, max_feature=16, world=1, rank=0):
    """the batches through one fresh SparseEmbeddingHash -> [(before, after, rows of the positions)]"""
    import torch
    import hugectr_amd as ha
    L = _lib()
    monkeypatch.setenv("HCTR_HOT_MIN", "0")
    monkeypatch.setenv("HCTR_HOT_ROWS", str(hot_rows))
    monkeypatch.setenv("HCTR_SGD_FUSED", "1")
    kdt = torch.int32 if kt == "u32" else torch.int64
    emb = ha.SparseEmbeddingHash(L.EMB_LOCALIZED if world == 1 else L.EMB_DISTRIBUTED, B, 0, V, D,
                                 max_feature, S, combiner, _emb_opt(o, atomic), key_dtype=kdt,
                                 out_dtype=_torch_dt(dt), rank=rank, world=world)
    emb.init_params()
    emb.table().copy_(torch.from_numpy(init).to("cuda"))
    torch.cuda.synchronize()
    trace = []
    for step, (ro_h, keys_h) in enumerate(batches):
        ro = torch.from_numpy(np.array(ro_h)).to("cuda").to(kdt)
        keys = torch.from_numpy(np.array(keys_h)).to("cuda").to(kdt)
        emb.forward(True, ro, keys)
        g = _kgrad(B * S, D, 10 + step).astype(np.float32) * np.float32(2.0 ** -6)
        top = torch.from_numpy(g).to("cuda").to(_torch_dt(dt)).view(B, S, D).contiguous()
        keep = (ro.clone(), keys.clone(), top.clone())
        emb.backward(top)
        torch.cuda.synchronize()
        mine = int((keys_h % world == rank).sum())  # (distributed: the keys this rank owns)
        vi = emb.value_index(mine).cpu().numpy().view(np.uint64).copy()
        before = _emb_states(emb, o.ns)
        emb.update_params()
        torch.cuda.synchronize()
        trace.append((before, _emb_states(emb, o.ns), vi))
        for a, b, name in zip((ro, keys, top), keep, ("row_offset", "keys", "top_grad")):
            assert torch.equal(a, b), f"the update changed its input {name}"
    del emb
    return trace


def _emb_verify(tag, trace, batches, D, o, combiner, half, V=HC_V, B=HC_B, S=HC_S, world=1, rank=0):
    pt = np.ones(V, np.uint64)
    worst = 0.0
    for step, ((before, after, vi), (ro_h, keys_h)) in enumerate(zip(trace, batches)):
        live = vi != INVALID
        assert live.all(), "the table is large enough for every key"
        lens = np.diff(ro_h)
        # the rank's keys in their order; a mean divides by the bucket's key count over ALL ranks
        grow = np.repeat(np.arange(B * S), lens)[keys_h % world == rank]
        scale4 = (4 // np.maximum(lens, 1))[grow] if combiner == 1 else np.full(grow.size, 4, np.int64)
        assert combiner == 0 or np.isin(lens, [0, 1, 2, 4]).all()
        urows, gsum, _ = _exact_sums(vi.astype(np.int64), grow, scale4.astype(np.int64),
                                     _kgrad(B * S, D, 10 + step))
        worst = max(worst, _verify_step(f"{tag} step {step + 1}", o, step + 1, urows, gsum, before, after,
                                        V, half, pt))
        pt[urows] = step + 1
    return worst


def _hc_classes(trace, batches, D):
    """the classes the docstring of _hc_batches promises, restated from the rows the table handed out"""
    sm = _short_max(D)
    vi1, k1 = trace[0][2].astype(np.int64), batches[0][1]
    hot_keys = HOT0 + np.arange(8)
    row_of = {int(k): int(vi1[np.flatnonzero(k1 == k)[0]]) for k in hot_keys}
    assert sorted(row_of.values()) == list(range(HC_H)), "the first eight keys took the hot rows"
    assert (vi1[~np.isin(k1, hot_keys)] >= HC_H).all()
    cnt = np.bincount(vi1, minlength=HC_V)
    cold = cnt[HC_H:]
    for c in (1, 2, sm, sm + 1, COLD_LDS, COLD_LDS + 1):
        assert (cold == c).any(), f"no cold run of {c}"
    assert cnt[row_of[HOT0]] == 1 and cnt[row_of[HOT0 + 1]] == 10 and cnt[row_of[HOT0 + 2]] == 100
    pos3 = np.flatnonzero(k1 == HOT0 + 3)
    assert len(set(pos3 % HC_S)) == 3 and (pos3 // HC_S >= HOT_CHUNK).any() and (pos3 // HC_S < HOT_CHUNK).any()
    vi3 = trace[2][2].astype(np.int64)
    assert not (vi3 == row_of[HOT0 + 4]).any() and (vi3 == row_of[HOT0 + 5]).any()
    assert not (trace[1][2].astype(np.int64) == row_of[HOT0 + 5]).any()


HC_CONFIGS = [("f32", "i64", 0), ("f32", "u32", 1), ("f16", "i64", 1), ("f16", "u32", 0), ("bf16", "i64", 0),
              ("bf16", "u32", 1)]
HC_CASES = [(D, n) for D in ([4] if EMU else [4, 16, 64, 256]) for n in EMB_OPTS] + \
    _grid([(D, n) for D in (8, 128) for n in ("sgd", "adam_lazy")])


@pytest.mark.parametrize("D,name", HC_CASES)
def test_hot_cold(D, name, monkeypatch):
    """part C: four batches on one handle with HCTR_HOT_ROWS = 8 (hot and cold chains, then the
    sorting path on the same handle) and with HCTR_HOT_ROWS = 0 (the sorting path throughout:
    update_segmented_u32, fp16 state with summed gradients, lazy Adam) -- both against the same
    reference, and with exact sums bit-equal to each other"""
    o = EMB_OPTS[name]
    batches = _hc_batches(_short_max(D))
    for i, (dt, kt, combiner) in enumerate(HC_CONFIGS):
        init = _dyadic((HC_V, D), 2.0 ** -11, -1, 1)
        half = dt == "f16"
        tag = f"{name} D={D} {dt} {kt} combiner={combiner}"
        hot = _emb_run(batches, D, dt, kt, o, combiner, HC_H, monkeypatch, init)
        _hc_classes(hot, batches, D)
        r_hot = _emb_verify(tag + " hot/cold", hot, batches, D, o, combiner, half)
        plain = _emb_run(batches, D, dt, kt, o, combiner, 0, monkeypatch, init)
        r_plain = _emb_verify(tag + " sorted", plain, batches, D, o, combiner, half)
        for k in range(1 + o.ns):
            _same_bits(f"{tag}: array {k}, hot / cold against the sorting path", hot[-1][1][k],
                       plain[-1][1][k])
        if i == 0:
            again = _emb_run(batches, D, dt, kt, o, combiner, HC_H, monkeypatch, init)
            for k in range(1 + o.ns):
                _same_bits(f"{tag}: array {k} of a second run on a fresh handle", again[-1][1][k],
                           hot[-1][1][k])
        print(f"sparse update {tag}: max err / bound = {r_hot:.3f} (hot / cold), {r_plain:.3f} (sorted)")


@functools.lru_cache(maxsize=None)
def _ragged_batch(B, S, V, seed, long_run=1000):
    """ragged buckets of 0 / 1 / 2 / 4 keys out of V - 8 keys, one of them met long_run times"""
    rng = np.random.default_rng(9600 + seed + 7919 * SEED)
    lens = rng.choice([0, 1, 2, 4], size=B * S)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keys = rng.integers(0, V - 8, size=ro[-1]).astype(np.int64)
    keys[rng.choice(keys.size, size=min(long_run, keys.size // 2), replace=False)] = 3
    ro.setflags(write=False)
    keys.setflags(write=False)
    return ro, keys


@pytest.mark.parametrize("combiner", [0, 1], ids=["sum", "mean"])
@pytest.mark.parametrize("D", [4, 11, 32, 256])
def test_atomic_sgd(D, combiner, monkeypatch):
    """sgd_atomic_kernel: lr / scaler = 2^-5, every addend a multiple of 2^-13 and every partial sum
    of the table below 2^11 -- the atomic adds are exact in any order: bit-equal to fp64"""
    B, S, V = 300, 4, 512
    o = OPTS["sgd"]
    batches = [_ragged_batch(B, S, V, s) for s in range(3)]
    for dt in DTYPES:
        init = _dyadic((V, D), 2.0 ** -11, -1, 1)
        trace = _emb_run(batches, D, dt, "i64", o, combiner, 0, monkeypatch, init, V=V, B=B, S=S,
                         atomic=True)
        again = _emb_run(batches, D, dt, "i64", o, combiner, 0, monkeypatch, init, V=V, B=B, S=S,
                         atomic=True)
        _same_bits("a second run on a fresh handle", again[-1][1][0], trace[-1][1][0])
        _emb_verify(f"atomic sgd D={D} {dt} combiner={combiner}", trace, batches, D, o, combiner, False,
                    V=V, B=B, S=S)


MEAN_D = SEG_D + GEN_D


@pytest.mark.parametrize("D", [d for d in MEAN_D if not (EMU and d > 64)])
def test_sorted_mean(D, monkeypatch):
    """the mean combiner (buckets of 0 / 1 / 2 / 4 keys, a run of 1000) on the sorting path for every
    LPR of the segmented kernels and every branch of the generic one, which hctr_updater_update
    cannot ask for: the nine embedding optimizers, one gradient type and key type per D"""
    B, S, V = 300, 4, 512
    i = MEAN_D.index(D)
    dt, kt = DTYPES[i % 3], ("i64", "u32")[i % 2]
    batches = [_ragged_batch(B, S, V, 10 + s) for s in range(3)]
    for name, o in EMB_OPTS.items():
        init = _dyadic((V, D), 2.0 ** -11, -1, 1)
        trace = _emb_run(batches, D, dt, kt, o, 1, 0, monkeypatch, init, V=V, B=B, S=S)
        r = _emb_verify(f"mean, sorted {name} D={D} {dt} {kt}", trace, batches, D, o, 1, dt == "f16", V=V, B=B,
                        S=S)
        print(f"sparse update mean, sorted {name} D={D} {dt} {kt}: max err / bound = {r:.3f}")


def test_update_rows(monkeypatch):
    """emb.update_rows: (row, gradient) entries, one per bucket, through the sort and the segmented
    kernels with a two-state optimizer; entries naming one row are summed"""
    import torch
    import hugectr_amd as ha
    L = _lib()
    D, V, n, o = 16, 600, 3000, OPTS["adam_local"]
    monkeypatch.setenv("HCTR_SGD_FUSED", "1")
    rng = np.random.default_rng(9700 + 7919 * SEED)
    rows_h = np.minimum(rng.pareto(0.8, size=n).astype(np.int64) * 2, V - 1)
    for dt in DTYPES:
        emb = ha.SparseEmbeddingHash(L.EMB_LOCALIZED, n, 0, V, D, 4, 1, 0, _emb_opt(o))
        emb.init_params()
        emb.table().copy_(torch.from_numpy(_dyadic((V, D), 2.0 ** -11, -1, 1)).to("cuda"))
        rows = torch.from_numpy(rows_h).to("cuda")
        ro = torch.arange(n + 1, dtype=torch.int64, device="cuda")
        for step in range(3):
            kg = _kgrad(n, D, 20 + step)
            g = torch.from_numpy(kg.astype(np.float32) * np.float32(2.0 ** -6)).to("cuda").to(_torch_dt(dt))
            keep = (rows.clone(), g.clone(), ro.clone())
            before = _emb_states(emb, o.ns)
            emb.update_rows(rows, g, ro)
            torch.cuda.synchronize()
            after = _emb_states(emb, o.ns)
            assert all(torch.equal(a, b) for a, b in zip((rows, g, ro), keep)), "inputs changed"
            urows, gsum, _ = _exact_sums(rows_h, np.arange(n), np.full(n, 4, np.int64), kg)
            r = _verify_step(f"update_rows {dt} step {step + 1}", o, step + 1, urows, gsum, before, after, V)
        print(f"sparse update update_rows adam_local D={D} {dt}: max err / bound = {r:.3f}")
        del emb


@functools.lru_cache(maxsize=None)
def _two_rank_batch(B, S, V, seed):
    """buckets of 0, 2 (one even key, one odd) and 4 keys (two even, two odd): over two ranks the
    global lengths are 2 and 4, each rank's own 1 and 2"""
    rng = np.random.default_rng(9800 + seed + 7919 * SEED)
    lens = rng.choice([0, 2, 4], size=B * S)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    half = rng.integers(0, (V - 8) // 2, size=ro[-1]) * 2
    half[rng.choice(half.size, size=200, replace=False)] = 6  # (a long run on either rank)
    keys = (half + np.arange(ro[-1]) % 2).astype(np.int64)   # even, odd, even, odd inside a bucket
    assert (ro % 2 == 0).all()
    ro.setflags(write=False)
    keys.setflags(write=False)
    return ro, keys


@pytest.mark.parametrize("name", ["sgd", "adagrad"])
@pytest.mark.parametrize("D", [16, 6], ids=["segmented", "generic"])
def test_distributed_mean_scale_row_offset(D, name, monkeypatch):
    """DistributedSlotSparseEmbeddingHash on two ranks, combiner mean: the update's scale_row_offset
    (the unfiltered offsets) makes the gradient of a key 1 / (keys of its bucket over both ranks),
    not 1 / (this rank's) -- on the segmented and on the generic kernel"""
    B, S, V, o = 64, 4, 512, OPTS[name]
    batches = [_two_rank_batch(B, S, V, s) for s in range(3)]
    for dt, kt in (("f32", "i64"), ("f16", "u32")):
        for rank in (0, 1):
            init = _dyadic((V, D), 2.0 ** -11, -1, 1)
            kw = dict(V=V, B=B, S=S, world=2, rank=rank)
            trace = _emb_run(batches, D, dt, kt, o, 1, 0, monkeypatch, init, **kw)
            r = _emb_verify(f"two ranks, rank {rank} D={D} {dt} {name}", trace, batches, D, o, 1, dt == "f16",
                            **kw)
            print(f"sparse update two ranks, rank {rank} {name} D={D} {dt} {kt}: max err / bound = {r:.3f}")
