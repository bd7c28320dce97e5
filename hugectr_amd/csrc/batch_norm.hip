// batch_norm.hip -- BatchNormLayer<T> (R/HugeCTR/src/layers/batch_norm_layer.cu, cuDNN's
// per-activation mode) and PRelu_Dice_Layer<T> (R/HugeCTR/src/layers/prelu_dice_layer.cu), forward
// and backward, for gfx950 (wave 64).  Both are statistics of a COLUMN over the batch: of a
// row-major [rows][n] tensor, m = rows,
//   mean_c = sum_r x[r][c] / m,  var_c = sum_r (x[r][c] - mean_c)^2 / m (biased),
//   BatchNorm  rstd = 1 / sqrt(var + eps),  y = (x - mean) rstd gamma + beta
//              running_mean = (1 - f) running_mean + f mean,
//              running_var = (1 - f) running_var + f var m / max(m - 1, 1);  save = (mean, rstd)
//              inference: y = (x - running_mean) / sqrt(running_var + eps) gamma + beta
//              xh = (x - mean) rstd:  dbeta = sum_r dy,  dgamma = sum_r dy xh,
//              dx = gamma rstd (dy - dbeta / m - xh dgamma / m)
//   Dice       p = 1 / (1 + exp((mean - x) / sqrt(var + eps))),  y = p x + (1 - p) alpha x
//              backward, the reference's: the diagonal of the Jacobian (an element sees its own
//              1 / m share of mean and variance only).  r1 = r3 = 0 when var + eps < 1e-8, else
//              r1 = 1 / sqrt(var + eps), r3 = r1^3;  ys = (mean - x) r1,
//              ys_x = (1 / m - 1) r1 + (mean - x)^2 r3 / m,  p_x = -p (1 - p) ys_x,
//              dx = ((p_x x + p)(1 - alpha) + alpha) dy
// Activations fp32 / fp16 / bf16; everything per column (gamma, beta, their gradients, running and
// saved statistics, partials) and all arithmetic fp32.
//
// This is the transpose of what layer_norm.hip reduces, and HBM traffic and nothing else: there is
// no product here, so no matrix instructions -- plain C++, 16-byte vector loads and stores.  Two
// kernel bodies, each instantiated per (element type, lane group, what it computes):
//
// col_reduce_kernel, grid (column panels) x (row slabs).  A row is cut into 16-byte chunks (V = 4
// fp32 or 8 16-bit columns); G = 1, 2, 4 .. 64 lanes cover a panel of G V columns (the smallest G
// that covers n, 64 from n > 32 V on: a wavefront then reads 1 KiB of a row and n takes
// ceil(n / 64 V) panels), so a wavefront takes 64 / G rows a trip and the workgroup 256 / G.  A
// lane keeps the two accumulators of each of its V columns in registers while the workgroup walks
// its slab's rows, eight trips' loads in flight; no lane meets another inside the walk.  At the end
// the groups of a wavefront add theirs by a butterfly over the lanes G, 2 G .. 32 apart, the four
// wavefronts' sums meet in LDS and are added in wavefront order (as layer_norm.hip's backward
// ends), and the workgroup writes one fp32 pair per column to scratch [slab][2][n].  The body is
// instantiated for two accumulands:
//   StatAcc  sum(x - pivot), sum((x - pivot)^2), the pivot being the column's value in the slab's
//            own first row; the slab hands on (mean, M2 = sum (x - mean)^2) of its rows.  Never
//            E[x^2] - E[x]^2 of the raw values
//   GradAcc  sum(dy), sum(dy xh), with xh recomputed from x and the saved (mean, rstd)
// The slab count is a function of (rows, n, element type) alone (plan()): enough slabs for about
// 1024 workgroups, at most 64, none empty.
//
// col_apply_kernel, grid (column panels) x (row groups), same ownership of chunks.  Its prologue
// is per column (a thread a column): it merges the slabs' partials IN ASCENDING SLAB ORDER --
// (count, mean, M2) by the pairwise update, gradient sums by addition -- and folds the column's
// constants into at most four coefficients, which go through LDS to the lanes that own the column
// and stay in registers.  Only the workgroups of row group 0 write what is per column (save,
// running statistics, dgamma / dbeta, Dice's (mean, var)).  The row stream is then, an element,
//   BatchNorm forward  (x - mean) scale + beta        (scale = rstd gamma; one subtraction, one FMA)
//   BatchNorm dx       (x - mean) b + (dy a + c)      (a = gamma rstd, b = -a rstd dgamma / m,
//                                                      c = -a dbeta / m)
//   Dice forward / backward   one exp and a few FMAs
// mean is kept apart from the shift (x scale + shift would be one FMA) because a column that is
// far from zero with a small variance loses its y to the rounding of mean scale.  Inference and
// the Dice backward have no reduction: their prologue reads the statistics they are given.
//
// Launches: BatchNorm training forward 2, inference 1, backward 2; Dice forward 2, backward 1.  No
// finish launch, no memset, no atomics; per-lane, per-workgroup and per-slab orders are fixed, so two
// runs give the same bits.  A width that is no multiple of V (or a misaligned buffer) takes the same
// kernels with element accesses; chunk elements past the row's end read column 0 (in bounds) and
// are never written.
#include <cmath>
#include <type_traits>

#include "common.h"
#include "cvt16.h"

namespace hctr {
namespace bn {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxN = 65536;
constexpr int kMaxSlabs = 64;
constexpr int kReduceGrid = 1024;  // workgroups the reduction aims at: 4 a CU
constexpr int kApplyGrid = 2048;   // 8 a CU
constexpr int kUnroll = 4;         // trips whose loads are issued before the first is used (16-byte
constexpr int kReduceUnroll = 8;   // accesses only: element accesses walk a trip at a time)
constexpr int kMergeBatch = 8;     // slabs whose partials a consumer loads before it merges them

// V consecutive elements, 16-byte aligned: one or two 16-byte accesses
template <typename S, int V>
struct alignas(16) Pack {
  S e[V];
};

// how the lanes of a workgroup own a panel: G lanes a row, one chunk of V columns a lane
template <typename T, int G_>
struct Lanes {
  static constexpr int G = G_;
  static constexpr int V = 16 / (int)sizeof(T);
  static constexpr int kCols = G * V;        // columns of a panel
  static constexpr int kRows = kThreads / G;  // rows of one workgroup trip
  static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "G: 1, 2, 4 .. 64");
};

// the lane's chunk of a row as it lies in memory, c0 its first column; what lies past the row's end
// is column 0's value and never used for a column that exists
template <typename T, int V>
__device__ __forceinline__ Pack<T, V> load_chunk(const T* __restrict__ row, int c0, int n, bool vec) {
  if (vec) return *reinterpret_cast<const Pack<T, V>*>(row + (c0 < n ? c0 : 0));
  Pack<T, V> p;
#pragma unroll
  for (int e = 0; e < V; e++) p.e[e] = row[c0 + e < n ? c0 + e : 0];
  return p;
}

template <typename T, int V>
__device__ __forceinline__ void store_chunk(T* __restrict__ row, int c0, int n, bool vec,
                                            const float (&f)[V]) {
  if (vec) {
    Pack<T, V> p;
#pragma unroll
    for (int e = 0; e < V; e++) p.e[e] = from_f32<T>(f[e]);
    if (c0 < n) *reinterpret_cast<Pack<T, V>*>(row + c0) = p;
  } else {
#pragma unroll
    for (int e = 0; e < V; e++)
      if (c0 + e < n) row[c0 + e] = from_f32<T>(f[e]);
  }
}

// ================================================================================================
// The column reduction and its two accumulands
// ================================================================================================
// forward: sums of x - pivot and of its square, the pivot being the slab's first row
template <typename T>
struct StatAcc {
  static constexpr int V = 16 / (int)sizeof(T);
  const T* x;
  struct In {
    Pack<T, V> x;
  };
  struct Cols {
    float pivot[V];
  };
  __device__ __forceinline__ Cols prepare(size_t r0, int c0, int n, bool vec) const {
    const Pack<T, V> p = load_chunk<T, V>(x + r0 * n, c0, n, vec);
    Cols k;
#pragma unroll
    for (int e = 0; e < V; e++) k.pivot[e] = to_f32<T>(p.e[e]);
    return k;
  }
  __device__ __forceinline__ In load(size_t r, int c0, int n, bool vec) const {
    return In{load_chunk<T, V>(x + r * n, c0, n, vec)};
  }
  __device__ __forceinline__ void add(const In& in, const Cols& k, float (&a)[V], float (&b)[V]) const {
#pragma unroll
    for (int e = 0; e < V; e++) {
      const float d = to_f32<T>(in.x.e[e]) - k.pivot[e];
      a[e] += d;
      b[e] += d * d;
    }
  }
  // what the slab hands on for column c: (mean, M2) of its cnt rows
  __device__ __forceinline__ float2 finish(float s1, float s2, size_t r0, int c, int n, float cnt) const {
    const float pivot = to_f32<T>(x[r0 * n + c]);
    return make_float2(pivot + s1 / cnt, fmaxf(s2 - s1 * (s1 / cnt), 0.f));
  }
};

// BatchNorm backward: sums of dy and of dy xh, xh from x and the saved (mean, rstd)
template <typename T>
struct GradAcc {
  static constexpr int V = 16 / (int)sizeof(T);
  const T* x;
  const T* dy;
  const float* save;  // [2][n]
  struct In {
    Pack<T, V> x, dy;
  };
  struct Cols {
    float mean[V], rstd[V];
  };
  __device__ __forceinline__ Cols prepare(size_t, int c0, int n, bool) const {
    Cols k;
#pragma unroll
    for (int e = 0; e < V; e++) {
      const int c = c0 + e < n ? c0 + e : 0;
      k.mean[e] = save[c];
      k.rstd[e] = save[n + c];
    }
    return k;
  }
  __device__ __forceinline__ In load(size_t r, int c0, int n, bool vec) const {
    return In{load_chunk<T, V>(x + r * n, c0, n, vec), load_chunk<T, V>(dy + r * n, c0, n, vec)};
  }
  __device__ __forceinline__ void add(const In& in, const Cols& k, float (&a)[V], float (&b)[V]) const {
#pragma unroll
    for (int e = 0; e < V; e++) {
      const float d = to_f32<T>(in.dy.e[e]);
      a[e] += d;
      b[e] += d * ((to_f32<T>(in.x.e[e]) - k.mean[e]) * k.rstd[e]);
    }
  }
  __device__ __forceinline__ float2 finish(float s1, float s2, size_t, int, int, float) const {
    return make_float2(s1, s2);
  }
};

template <typename L, typename Acc>
__global__ __launch_bounds__(kThreads) void col_reduce_kernel(size_t rows, int n, size_t slab_rows,
                                                              Acc acc, float* __restrict__ partial,
                                                              bool vec) {
  constexpr int G = L::G, V = L::V;
  // the wavefronts' column sums, [accumulator][wavefront][element][lane]
  __shared__ float red[2 * kWaves * V * G];
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const int c0 = blockIdx.x * L::kCols + lane * V;
  const size_t r0 = (size_t)blockIdx.y * slab_rows;
  const size_t r1 = rows - r0 < slab_rows ? rows : r0 + slab_rows;
  const typename Acc::Cols cols = acc.prepare(r0, c0, n, vec);
  float a[V], b[V];
#pragma unroll
  for (int e = 0; e < V; e++) a[e] = b[e] = 0.f;
  size_t r = r0 + grp;
  if (vec)
    for (; r + (size_t)(kReduceUnroll - 1) * L::kRows < r1; r += (size_t)kReduceUnroll * L::kRows) {
      typename Acc::In in[kReduceUnroll];
#pragma unroll
      for (int u = 0; u < kReduceUnroll; u++) in[u] = acc.load(r + (size_t)u * L::kRows, c0, n, true);
#pragma unroll
      for (int u = 0; u < kReduceUnroll; u++) acc.add(in[u], cols, a, b);
    }
  for (; r < r1; r += L::kRows) acc.add(acc.load(r, c0, n, vec), cols, a, b);

  const int wave = threadIdx.x / 64;
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    float (&s)[V] = pass ? b : a;
#pragma unroll
    for (int e = 0; e < V; e++) {
      float v = s[e];  // over the wavefront's groups
#pragma unroll
      for (int dist = 32; dist >= G; dist >>= 1) v += __shfl_xor(v, dist, 64);
      if ((threadIdx.x & 63) < G) red[((pass * kWaves + wave) * V + e) * G + lane] = v;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < L::kCols; j += kThreads) {  // a thread a column of the panel
    const int c = blockIdx.x * L::kCols + j, at = (j % V) * G + j / V;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      s1 += red[w * V * G + at];
      s2 += red[(kWaves + w) * V * G + at];
    }
    if (c < n) {
      const float2 o = acc.finish(s1, s2, r0, c, n, (float)(r1 - r0));
      partial[((size_t)blockIdx.y * 2) * n + c] = o.x;
      partial[((size_t)blockIdx.y * 2 + 1) * n + c] = o.y;
    }
  }
}

// the slabs' partials of one reduction as a consumer sees them: [count][2][n], slab s = rows
// s slab_rows .. min(rows, (s + 1) slab_rows).  Merged in ascending slab order, always
struct Slabs {
  const float* partial;
  int count;
  size_t slab_rows, rows;
  __device__ __forceinline__ float rows_of(int s) const {
    const size_t r0 = (size_t)s * slab_rows;
    return (float)(rows - r0 < slab_rows ? rows - r0 : slab_rows);
  }
  // StatAcc's (mean, M2) pairs -> (mean, biased variance) of all rows, by the pairwise update
  // the pairs of slabs s0 .. s0 + kMergeBatch of column c, all loads issued before the first use (a
  // slab past the last reads the last again and is not merged)
  __device__ __forceinline__ void load_batch(int s0, int c, int n, float (&u)[kMergeBatch],
                                             float (&v)[kMergeBatch]) const {
#pragma unroll
    for (int i = 0; i < kMergeBatch; i++) {
      const size_t s = (size_t)(s0 + i < count ? s0 + i : count - 1);
      u[i] = partial[2 * s * n + c];
      v[i] = partial[(2 * s + 1) * n + c];
    }
  }
  // StatAcc's (mean, M2) pairs -> (mean, biased variance) of all rows, by the pairwise update
  // (from nothing: the first slab's pair comes through unchanged)
  __device__ __forceinline__ float2 mean_var(int c, int n) const {
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    for (int s0 = 0; s0 < count; s0 += kMergeBatch) {
      float mb[kMergeBatch], qb[kMergeBatch];
      load_batch(s0, c, n, mb, qb);
#pragma unroll
      for (int i = 0; i < kMergeBatch; i++) {
        if (s0 + i >= count) break;
        const float cb = rows_of(s0 + i), tot = cnt + cb;
        const float d = mb[i] - mean;
        mean += d * (cb / tot);
        m2 += qb[i] + d * d * (cnt * (cb / tot));
        cnt = tot;
      }
    }
    return make_float2(mean, m2 / cnt);
  }
  // GradAcc's sums
  __device__ __forceinline__ float2 sums(int c, int n) const {
    float a = 0.f, b = 0.f;
    for (int s0 = 0; s0 < count; s0 += kMergeBatch) {
      float ab[kMergeBatch], bb[kMergeBatch];
      load_batch(s0, c, n, ab, bb);
#pragma unroll
      for (int i = 0; i < kMergeBatch; i++) {
        if (s0 + i >= count) break;
        a += ab[i];
        b += bb[i];
      }
    }
    return make_float2(a, b);
  }
};

// ================================================================================================
// The streaming kernel and what it computes.  An Op: kCoef coefficients a column, kTwo when it reads
// dy next to x; column(c, n, first, k) is the prologue of column c (first: this workgroup writes the
// per-column outputs), elem(x, dy, k, e) the arithmetic of one element of the lane's column e
// ================================================================================================
template <typename T>
struct BnFwd {  // slabs.count = 0: inference from the running statistics
  static constexpr int kCoef = 3, V = 16 / (int)sizeof(T);
  static constexpr bool kTwo = false;
  const T* x;
  const T* dy;
  T* out;
  Slabs slabs;
  const float *gamma, *beta;
  float factor, eps;
  float *running_mean, *running_var, *save;
  __device__ __forceinline__ void column(int c, int n, bool first, float (&k)[kCoef]) const {
    const bool training = slabs.count > 0;
    const float2 mv = training ? slabs.mean_var(c, n) : make_float2(running_mean[c], running_var[c]);
    const float rstd = 1.f / sqrtf(mv.y + eps);
    k[0] = mv.x;
    k[1] = rstd * gamma[c];
    k[2] = beta[c];
    if (!(first && training)) return;
    if (save) {
      save[c] = mv.x;
      save[n + c] = rstd;
    }
    if (running_mean) {
      const float m = (float)slabs.rows;
      running_mean[c] = (1.f - factor) * running_mean[c] + factor * mv.x;
      running_var[c] = (1.f - factor) * running_var[c] + factor * (mv.y * (m / fmaxf(m - 1.f, 1.f)));
    }
  }
  __device__ __forceinline__ float elem(float x, float, const float (&k)[kCoef][V], int e) const {
    return fmaf(x - k[0][e], k[1][e], k[2][e]);
  }
};

template <typename T>
struct BnDx {
  static constexpr int kCoef = 4, V = 16 / (int)sizeof(T);
  static constexpr bool kTwo = true;
  const T* x;
  const T* dy;
  T* out;
  Slabs slabs;
  const float *gamma, *save;
  float *dgamma, *dbeta;
  __device__ __forceinline__ void column(int c, int n, bool first, float (&k)[kCoef]) const {
    const float2 s = slabs.sums(c, n);  // (dbeta, dgamma)
    const float m = (float)slabs.rows, rstd = save[n + c], a = gamma[c] * rstd;
    k[0] = save[c];
    k[1] = a;
    k[2] = -a * rstd * (s.y / m);
    k[3] = -a * (s.x / m);
    if (first) {
      dgamma[c] = s.y;
      dbeta[c] = s.x;
    }
  }
  __device__ __forceinline__ float elem(float x, float d, const float (&k)[kCoef][V], int e) const {
    return fmaf(x - k[0][e], k[2][e], fmaf(d, k[1][e], k[3][e]));
  }
};

template <typename T>
struct DiceFwd {
  static constexpr int kCoef = 2, V = 16 / (int)sizeof(T);
  static constexpr bool kTwo = false;
  const T* x;
  const T* dy;
  T* out;
  Slabs slabs;
  float alpha, eps;
  float* stats;  // [2][n] (mean, var) or NULL
  __device__ __forceinline__ void column(int c, int n, bool first, float (&k)[kCoef]) const {
    const float2 mv = slabs.mean_var(c, n);
    k[0] = mv.x;
    k[1] = 1.f / sqrtf(mv.y + eps);
    if (first && stats) {
      stats[c] = mv.x;
      stats[n + c] = mv.y;
    }
  }
  __device__ __forceinline__ float elem(float x, float, const float (&k)[kCoef][V], int e) const {
    const float p = 1.f / (1.f + __expf((k[0][e] - x) * k[1][e]));
    return x * fmaf(p, 1.f - alpha, alpha);  // p x + (1 - p) alpha x
  }
};

template <typename T>
struct DiceBwd {
  static constexpr int kCoef = 4, V = 16 / (int)sizeof(T);
  static constexpr bool kTwo = true;
  const T* x;
  const T* dy;
  T* out;
  const float* stats;
  float alpha, eps, inv_m;
  __device__ __forceinline__ void column(int c, int n, bool, float (&k)[kCoef]) const {
    const float t = stats[n + c] + eps;
    const float r1 = t < 1e-8f ? 0.f : 1.f / sqrtf(t);
    k[0] = stats[c];
    k[1] = r1;
    k[2] = (inv_m - 1.f) * r1;
    k[3] = r1 * r1 * r1 * inv_m;
  }
  __device__ __forceinline__ float elem(float x, float d, const float (&k)[kCoef][V], int e) const {
    const float t = k[0][e] - x;
    const float p = 1.f / (1.f + __expf(t * k[1][e]));
    const float p_x = -(p * (1.f - p)) * fmaf(t * t, k[3][e], k[2][e]);  // exp / (1 + exp)^2 = p (1 - p)
    return fmaf(fmaf(p_x, x, p), 1.f - alpha, alpha) * d;
  }
};

template <typename T, typename L, typename Op>
__global__ __launch_bounds__(kThreads) void col_apply_kernel(size_t rows, int n, Op op, bool vec) {
  constexpr int G = L::G, V = L::V, K = Op::kCoef;
  __shared__ float coef[K * L::kCols];
  for (int j = threadIdx.x; j < L::kCols; j += kThreads) {  // a thread a column of the panel
    const int c = blockIdx.x * L::kCols + j;
    float kc[K];
#pragma unroll
    for (int i = 0; i < K; i++) kc[i] = 0.f;
    if (c < n) op.column(c, n, blockIdx.y == 0, kc);
#pragma unroll
    for (int i = 0; i < K; i++) coef[i * L::kCols + j] = kc[i];
  }
  __syncthreads();
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const int c0 = blockIdx.x * L::kCols + lane * V;
  float k[K][V];
#pragma unroll
  for (int i = 0; i < K; i++)
#pragma unroll
    for (int e = 0; e < V; e++) k[i][e] = coef[i * L::kCols + lane * V + e];

  auto one = [&](size_t r, const Pack<T, V>& px, const Pack<T, V>& pd) {
    float o[V];
#pragma unroll
    for (int e = 0; e < V; e++)
      o[e] = op.elem(to_f32<T>(px.e[e]), Op::kTwo ? to_f32<T>(pd.e[e]) : 0.f, k, e);
    store_chunk<T, V>(op.out + r * n, c0, n, vec, o);
  };
  const size_t step = (size_t)gridDim.y * L::kRows;
  size_t r = (size_t)blockIdx.y * L::kRows + grp;
  if (vec)
    for (; r + (kUnroll - 1) * step < rows; r += kUnroll * step) {
      Pack<T, V> px[kUnroll], pd[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; u++) {
        px[u] = load_chunk<T, V>(op.x + (r + u * step) * n, c0, n, true);
        if (Op::kTwo) pd[u] = load_chunk<T, V>(op.dy + (r + u * step) * n, c0, n, true);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; u++) one(r + u * step, px[u], Op::kTwo ? pd[u] : px[u]);
    }
  for (; r < rows; r += step) {
    const Pack<T, V> px = load_chunk<T, V>(op.x + r * n, c0, n, vec);
    one(r, px, Op::kTwo ? load_chunk<T, V>(op.dy + r * n, c0, n, vec) : px);
  }
}

// dgamma = dbeta = 0 when there are no rows
__global__ void zero2_kernel(int n, float* __restrict__ a, float* __restrict__ b) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) a[c] = b[c] = 0.f;
}

// ================================================================================================
// Host side
// ================================================================================================
// what every entry point refuses, by name, before anything else
int check(const char* op, size_t rows, int n, int dtype) {
  const std::string who = std::string(op) + ": ";
  HCTR_REQUIRE(n >= 1 && n <= kMaxN, who + "n 1 .. 65536");
  HCTR_REQUIRE(rows <= (size_t)0x7FFFFFFF / (size_t)n, who + "rows * n < 2^31");
  HCTR_REQUIRE(dtype == HCTR_EMB_F32 || dtype == HCTR_EMB_F16 || dtype == HCTR_EMB_BF16,
               who + "dtype (f32 / f16 / bf16)");
  return HCTR_OK;
}

// (n, element type) -> f((T*)nullptr, Lanes): the one place where a shape picks its kernels
template <typename F>
int with_lanes(int dtype, int n, F&& f) {
  return with_dtype(dtype, [&](auto* t) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    constexpr int V = 16 / (int)sizeof(T);
    if (n <= V) return f(t, Lanes<T, 1>{});
    if (n <= 2 * V) return f(t, Lanes<T, 2>{});
    if (n <= 4 * V) return f(t, Lanes<T, 4>{});
    if (n <= 8 * V) return f(t, Lanes<T, 8>{});
    if (n <= 16 * V) return f(t, Lanes<T, 16>{});
    if (n <= 32 * V) return f(t, Lanes<T, 32>{});
    return f(t, Lanes<T, 64>{});
  });
}

// the slab rule: enough slabs for about kReduceGrid workgroups, at most kMaxSlabs, at most one a
// workgroup trip of rows, none empty.  A function of (rows, n, element type) alone
struct Plan {
  int panels, slabs;
  size_t slab_rows;
};
template <typename L>
Plan plan(size_t rows, int n) {
  Plan p;
  p.panels = ceil_div(n, L::kCols);
  size_t s = ceil_div<size_t>(rows, (size_t)L::kRows);
  const size_t want = (size_t)(kReduceGrid / p.panels > 1 ? kReduceGrid / p.panels : 1);
  s = s < want ? s : want;
  s = s < (size_t)kMaxSlabs ? s : (size_t)kMaxSlabs;
  p.slab_rows = ceil_div<size_t>(rows, s);
  p.slabs = (int)ceil_div<size_t>(rows, p.slab_rows);
  return p;
}

// no plan has more slabs, whatever the element type: 16-bit elements have the fewest panels, and no
// trip has fewer than kThreads / 64 rows
size_t scratch_bytes(size_t rows, int n) {
  if (n < 1 || n > kMaxN) return 0;
  const size_t panels = ceil_div<size_t>((size_t)n, 64 * 8);
  size_t s = ceil_div<size_t>(rows, (size_t)kWaves);
  const size_t want = (size_t)kReduceGrid / panels > 1 ? (size_t)kReduceGrid / panels : 1;
  s = s < want ? s : want;
  s = s < (size_t)kMaxSlabs ? s : (size_t)kMaxSlabs;
  return (s < 1 ? 1 : s) * 2 * (size_t)n * sizeof(float);
}

// 16-byte accesses need rows that start on 16-byte boundaries
template <typename... P>
bool vec_ok(int n, int V, const P*... p) {
  return n % V == 0 && ((reinterpret_cast<uintptr_t>(p) % 16 == 0) && ...);
}

template <typename L, typename Acc>
int reduce(const Plan& p, size_t rows, int n, const Acc& acc, void* scratch, bool vec, hipStream_t s) {
  hipLaunchKernelGGL((col_reduce_kernel<L, Acc>), dim3(p.panels, p.slabs), dim3(kThreads), 0, s, rows,
                     n, p.slab_rows, acc, (float*)scratch, vec);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

template <typename T, typename L, typename Op>
int apply(const Plan& p, size_t rows, int n, const Op& op, bool vec, hipStream_t s) {
  const size_t trips = ceil_div<size_t>(rows, (size_t)L::kRows);
  const size_t cap = (size_t)(kApplyGrid / p.panels > 1 ? kApplyGrid / p.panels : 1);
  hipLaunchKernelGGL((col_apply_kernel<T, L, Op>), dim3(p.panels, (int)(trips < cap ? trips : cap)),
                     dim3(kThreads), 0, s, rows, n, op, vec);
  HCTR_LAUNCH_CHECK();
  return HCTR_OK;
}

int bn_fwd(size_t rows, int n, const void* x, const float* gamma, const float* beta, float factor,
           float eps, float* running_mean, float* running_var, void* y, float* save, void* scratch,
           int training, int dtype, hctr_stream_t stream) {
  HCTR_TRY(check("batch_norm", rows, n, dtype));
  HCTR_REQUIRE(eps > 0.f, "batch_norm: eps > 0");
  HCTR_REQUIRE(factor >= 0.f && factor <= 1.f, "batch_norm: factor 0 .. 1");
  if (rows == 0) return HCTR_OK;
  HCTR_REQUIRE(x && gamma && beta && y, "null pointer");
  HCTR_REQUIRE(training ? scratch && !running_mean == !running_var : running_mean && running_var,
               "null pointer");
  return with_lanes(dtype, n, [&](auto* t, auto lanes) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    using L = decltype(lanes);
    const Plan p = plan<L>(rows, n);
    const bool vec = vec_ok(n, L::V, x, y);
    hipStream_t s = as_stream(stream);
    Slabs slabs{nullptr, 0, 0, rows};
    if (training) {
      HCTR_TRY(reduce<L>(p, rows, n, StatAcc<T>{(const T*)x}, scratch, vec, s));
      slabs = Slabs{(const float*)scratch, p.slabs, p.slab_rows, rows};
    }
    return apply<T, L>(p, rows, n,
                       BnFwd<T>{(const T*)x, nullptr, (T*)y, slabs, gamma, beta, factor, eps,
                                running_mean, running_var, training ? save : nullptr},
                       vec, s);
  });
}

int bn_bwd(size_t rows, int n, const void* x, const float* gamma, const float* save, const void* dy,
           void* dx, float* dgamma, float* dbeta, void* scratch, int dtype, hctr_stream_t stream) {
  HCTR_TRY(check("batch_norm", rows, n, dtype));
  if (rows == 0 && !(dgamma && dbeta)) return HCTR_OK;
  HCTR_REQUIRE(dgamma && dbeta, "null pointer");
  hipStream_t s = as_stream(stream);
  if (rows == 0) {  // no rows: the gradients of gamma and beta are zeros
    hipLaunchKernelGGL(zero2_kernel, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, s, n, dgamma,
                       dbeta);
    HCTR_LAUNCH_CHECK();
    return HCTR_OK;
  }
  HCTR_REQUIRE(x && gamma && save && dy && dx && scratch, "null pointer");
  return with_lanes(dtype, n, [&](auto* t, auto lanes) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    using L = decltype(lanes);
    const Plan p = plan<L>(rows, n);
    const bool vec = vec_ok(n, L::V, x, dy, dx);
    HCTR_TRY(reduce<L>(p, rows, n, GradAcc<T>{(const T*)x, (const T*)dy, save}, scratch, vec, s));
    return apply<T, L>(p, rows, n,
                       BnDx<T>{(const T*)x, (const T*)dy, (T*)dx,
                               Slabs{(const float*)scratch, p.slabs, p.slab_rows, rows}, gamma, save,
                               dgamma, dbeta},
                       vec, s);
  });
}

int dice_fwd(size_t rows, int n, const void* x, float alpha, float eps, void* y, float* stats,
             void* scratch, int dtype, hctr_stream_t stream) {
  HCTR_TRY(check("prelu_dice", rows, n, dtype));
  HCTR_REQUIRE(eps >= 0.f, "prelu_dice: eps >= 0");
  if (rows == 0) return HCTR_OK;
  HCTR_REQUIRE(x && y && scratch, "null pointer");
  return with_lanes(dtype, n, [&](auto* t, auto lanes) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    using L = decltype(lanes);
    const Plan p = plan<L>(rows, n);
    const bool vec = vec_ok(n, L::V, x, y);
    hipStream_t s = as_stream(stream);
    HCTR_TRY(reduce<L>(p, rows, n, StatAcc<T>{(const T*)x}, scratch, vec, s));
    return apply<T, L>(p, rows, n,
                       DiceFwd<T>{(const T*)x, nullptr, (T*)y,
                                  Slabs{(const float*)scratch, p.slabs, p.slab_rows, rows}, alpha, eps,
                                  stats},
                       vec, s);
  });
}

int dice_bwd(size_t rows, int n, const void* x, const float* stats, float alpha, float eps,
             const void* dy, void* dx, int dtype, hctr_stream_t stream) {
  HCTR_TRY(check("prelu_dice", rows, n, dtype));
  HCTR_REQUIRE(eps >= 0.f, "prelu_dice: eps >= 0");
  if (rows == 0) return HCTR_OK;
  HCTR_REQUIRE(x && stats && dy && dx, "null pointer");
  return with_lanes(dtype, n, [&](auto* t, auto lanes) -> int {
    using T = std::remove_pointer_t<decltype(t)>;
    using L = decltype(lanes);
    return apply<T, L>(plan<L>(rows, n), rows, n,
                       DiceBwd<T>{(const T*)x, (const T*)dy, (T*)dx, stats, alpha, eps,
                                  1.f / (float)rows},
                       vec_ok(n, L::V, x, dy, dx), as_stream(stream));
  });
}

}  // namespace
}  // namespace bn
}  // namespace hctr

extern "C" {

size_t hctr_col_stats_scratch_bytes(size_t rows, int n) { return hctr::bn::scratch_bytes(rows, n); }

int hctr_batch_norm_fwd(size_t rows, int n, const void* x, const float* gamma, const float* beta,
                        float factor, float eps, float* running_mean, float* running_var, void* y,
                        float* save, void* scratch, int training, int dtype, hctr_stream_t stream) {
  return hctr::bn::bn_fwd(rows, n, x, gamma, beta, factor, eps, running_mean, running_var, y, save,
                          scratch, training, dtype, stream);
}

int hctr_batch_norm_bwd(size_t rows, int n, const void* x, const float* gamma, const float* save,
                        const void* dy, void* dx, float* dgamma, float* dbeta, void* scratch,
                        int dtype, hctr_stream_t stream) {
  return hctr::bn::bn_bwd(rows, n, x, gamma, save, dy, dx, dgamma, dbeta, scratch, dtype, stream);
}

int hctr_prelu_dice_fwd(size_t rows, int n, const void* x, float alpha, float eps, void* y,
                        float* stats, void* scratch, int dtype, hctr_stream_t stream) {
  return hctr::bn::dice_fwd(rows, n, x, alpha, eps, y, stats, scratch, dtype, stream);
}

int hctr_prelu_dice_bwd(size_t rows, int n, const void* x, const float* stats, float alpha,
                        float eps, const void* dy, void* dx, int dtype, hctr_stream_t stream) {
  return hctr::bn::dice_bwd(rows, n, x, stats, alpha, eps, dy, dx, dtype, stream);
}

}  // extern "C"
