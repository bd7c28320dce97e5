"""CPU restatement of the dynamic embedding table (TEST INFRASTRUCTURE ONLY, like everything under
oracle/): det::DynamicEmbeddingTable semantics
(R/third_party/dynamic_embedding_table/dynamic_embedding_table.cu:129-260,
cuCollections/include/cuco/detail/dynamic_map_kernels.cuh:100-260) and the optimizer formulas of
R/HugeCTR/embedding_storage/optimizers.cuh:29-233, as plain Python dicts + numpy float32.
The optimizer steps and the lookup / update flow are PINNED against the reference's own CPU mirror
of the table (R/HugeCTR/embedding_storage/dynamic_embedding_cpu.hpp + optimizers.hpp compiled into
oracle/_ref/libref_det.so; tests/test_ref_det_cpu.py).  The random initializer stays unpinned (the
reference seeds it from std::random_device); constant initializers are exact."""
import numpy as np

f32 = np.float32
FLT_EPSILON = f32(1.1920929e-07)

FTRL, ADAM, RMSPROP, ADAGRAD, NESTEROV, MOMENTUM, SGD = range(7)  # Optimizer_t values


class DetOracle:
    """dtype: the type the vectors are kept and summed in.  float32 (the default) is the reference's
    arithmetic; float64 evaluates the same operations on the same fp32 inputs without the rounding of
    the intermediate results (what the parity tests measure the fp32 evaluation's own error with)."""

    def __init__(self, dims, init_value, dtype=f32):
        self.dims = list(dims)
        self.dt = np.dtype(dtype).type
        self.init = f32(init_value)
        self.maps = [dict() for _ in dims]

    def _each(self, keys, id_spaces, offsets):
        for i, c in enumerate(id_spaces):
            for j in range(offsets[i], offsets[i + 1]):
                yield c, int(keys[j])

    def lookup(self, keys, id_spaces, offsets):
        out = []
        for c, k in self._each(keys, id_spaces, offsets):
            if k not in self.maps[c]:  # insert-if-missing with the initializer (lookup kernel)
                self.maps[c][k] = np.full(self.dims[c], self.init, dtype=self.dt)
            out.append(self.maps[c][k].copy())
        return np.concatenate(out) if out else np.zeros(0, dtype=self.dt)

    def scatter(self, keys, elements, id_spaces, offsets, add):
        off = 0
        for c, k in self._each(keys, id_spaces, offsets):
            d = self.dims[c]
            if k in self.maps[c]:  # missing keys are skipped
                if add:
                    self.maps[c][k] = (self.maps[c][k] + elements[off:off + d]).astype(self.dt)
                else:
                    self.maps[c][k] = elements[off:off + d].astype(self.dt).copy()
            off += d

    def remove(self, keys, id_spaces, offsets):
        for c, k in self._each(keys, id_spaces, offsets):
            self.maps[c].pop(k, None)

    def size_per_class(self):
        return [len(m) for m in self.maps]


def update(weights: DetOracle, states: DetOracle, opt, keys, id_spaces, offsets, ev_start, wgrad,
           lr, scaler=1.0, beta1=0.9, beta2=0.999, eps=1e-7, momentum=0.9, rms_beta=0.9,
           lambda1=0.0, lambda2=0.0, ftrl_beta=0.0, times=1, dtype=None):
    """dynamic_embedding.cu:176-330: state lookup (zeros), per-element formula, scatter_add.
    dtype (default: the weights oracle's, float32 unless it was created otherwise): the type of
    every intermediate result.  The inputs -- hyperparameters, gradients, initial values -- are the
    fp32 numbers the device gets in either case."""
    T = weights.dt if dtype is None else np.dtype(dtype).type
    lr, scaler = T(f32(lr)), T(f32(scaler))
    b1, b2, eps, mom, rb = (T(f32(x)) for x in (beta1, beta2, eps, momentum, rms_beta))
    lambda1, eps_ftrl, one, two = T(f32(lambda1)), T(FLT_EPSILON), T(1), T(2)
    # AdamOptHyperParams::bias() (optimizer.hpp:58-60): std::pow(float beta, uint64 times) promotes
    # the FLOAT beta to double -- 0.999f, not 0.999 (found by pinning against the reference build)
    bias = T(np.sqrt(1.0 - float(b2) ** times) / (1.0 - float(b1) ** times))
    lr_scaled_bias = lr * bias
    l2b = T(f32(lambda2)) + T(f32(ftrl_beta)) / lr
    pos = 0
    for i, c in enumerate(id_spaces):
        d = weights.dims[c]
        for j in range(offsets[i], offsets[i + 1]):
            k = int(keys[j])
            g = (wgrad[ev_start[pos]:ev_start[pos] + d].astype(T) / scaler).astype(T)
            pos += 1
            if opt != SGD:
                sd = states.dims[c]
                if k not in states.maps[c]:
                    states.maps[c][k] = np.zeros(sd, dtype=T)
                st = states.maps[c][k]
            if opt == FTRL and k not in weights.maps[c]:
                weights.maps[c][k] = np.full(d, weights.init, dtype=T)
            if opt == SGD:
                delta = (-lr * g).astype(T)
            elif opt == MOMENTUM:
                st[:] = (mom * st - lr * g).astype(T)
                delta = st.copy()
            elif opt == NESTEROV:
                prev = st.copy()
                st[:] = (mom * prev - lr * g).astype(T)
                delta = (st + mom * st - mom * prev).astype(T)
            elif opt == ADAGRAD:
                st[:] = (st + g * g).astype(T)
                delta = (-lr * g / (np.sqrt(st).astype(T) + eps)).astype(T)
            elif opt == RMSPROP:
                st[:] = (rb * st + (one - rb) * g * g).astype(T)
                delta = (-lr * g / (np.sqrt(st).astype(T) + eps)).astype(T)
            elif opt == ADAM:
                m, v = st[:d], st[d:]
                m[:] = (b1 * m + (one - b1) * g).astype(T)
                v[:] = (b2 * v + (one - b2) * g * g).astype(T)
                delta = (-lr_scaled_bias * m / (np.sqrt(v).astype(T) + eps)).astype(T)
            else:  # FTRL
                n, z = st[:d], st[d:]
                w = weights.maps[c][k]
                n_prev_sqrt = np.sqrt(n + eps_ftrl).astype(T)
                n[:] = (n + g * g).astype(T)
                n_sqrt = np.sqrt(n + eps_ftrl).astype(T)
                sigma = ((n_sqrt - n_prev_sqrt) / lr).astype(T)
                z[:] = (z + g - sigma * w).astype(T)
                p = ((one - two * np.signbit(z).astype(T)) * lambda1 - z).astype(T)
                q = (n_sqrt / lr + l2b).astype(T)
                delta = ((p / q) * np.signbit(lambda1 - np.abs(z)).astype(T) - w).astype(T)
            if k in weights.maps[c]:  # scatter_add skips missing keys
                weights.maps[c][k] = (weights.maps[c][k] + delta).astype(T)
